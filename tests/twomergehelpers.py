"""Machines, profiles, bounds and the device-against-restatement comparison of the two-profile sweeps against CTC-merged output
profiles (test_profile_two_merge_host.py, test_profile_two_merge_gpu.py; not a test module).  The bounds are those of
pairprofilehelpers / twoprofilehelpers: log values 1e-9 relative to max(1, |value|), -inf exact; counts >= 1e-3 at 1e-6 relative,
below 1e-9 + 1e-6 x count absolute; Viterbi scores 1e-12; paths, rows and input rows equal."""
import math

import numpy as np

from mergehelpers import merged_rows, quantised_rows
from prefixhelpers import machine_from_edges
from twoprofilehelpers import (HALF, HOST_SHAPES, chain_machine, counts_close, end_loop_variant, fixed_counts_close, logs_close,  # noqa: F401
                               machine_of, note, note_counts, one_hot, pair_machine, profile_of, soft_profile)


def merged_profile_of(em, B, colTok):
    """The Profile whose merged rows (Profile.mergeRows) against em are (B, colTok): column c headed by the symbol of colTok[c - 1]."""
    syms = em.outputTokenizer.tok2sym
    return profile_of([syms[int(t)] for t in colTok], B)


def merged_input(rng, em, nCols, K, L, pInf=0.1):
    """(A, B): an input profile of K rows, then merged output rows of L rows -- drawn in that order."""
    A = soft_profile(rng, K, em.nInTok, pInf)
    return A, merged_rows(rng, nCols, L, zeros=pInf)


# ---- the host grid (test_profile_two_merge_host.py): 2 x 2 x 3 machines, plain and end-loop, 3 column counts, 7 shapes = 504 ----------
HOST_STATES = (3, 5)
HOST_SEEDS = (0, 1, 2)
HOST_COLS = (1, 2, 4)


def host_cases():
    """(key, em, colTok, A, B): the inputs of one (S, seed, nCols) are drawn once and serve both level settings and both variants."""
    for S in HOST_STATES:
        for levels in (True, False):
            for seed in HOST_SEEDS:
                base = pair_machine(S, seed, levels, 2, 3)
                for variant, em in (("plain", base), ("endloop", end_loop_variant(base))):
                    for nCols in HOST_COLS:
                        rng = np.random.RandomState(7 * seed + nCols + 100 * S)
                        colTok = rng.randint(1, 4, nCols)
                        for K, L in HOST_SHAPES:
                            A = soft_profile(rng, K, em.nInTok, 0.1)
                            B = merged_rows(rng, nCols, L, zeros=0.1)
                            yield (S, levels, seed, variant, nCols, K, L), em, colTok, A, B


def rescore(em, A, B, colTok, edges, rows, ins):
    """The weight of a merged path with its blanks and repeats filled in: the edges' weights, the input rows (the token an edge read,
    the blank where none did) and the best reading of the output rows -- an emitting edge of token o at row r takes a column of o
    other than the last column taken, a row with no edge the blank or a repeat of the last column."""
    from mergehelpers import merged_path_weight
    w = merged_path_weight(em, B, colTok, edges, rows)
    usedA = {int(i) for e, i in zip(edges, ins) if em.inTok[e]}
    w += sum(A[i][em.inTok[e]] for e, i in zip(edges, ins) if em.inTok[e])
    return w + sum(A[i][0] for i in range(len(A)) if i not in usedA)


# ---- ties (host census and the GPU tie batch) --------------------------------------------------------------------------------------------
TIE_COLTOK = (1, 1, 1)                             # three columns of the one output token: planes that tie
TIE_KINDS = (("plane",), ("end",), ("blank",), ("repeat", "match"), ("match", "emit"), ("stay", "ins"), ("ins", "silent"), ("wait", "inblank"))


def tie_machine():
    from twoprofilehelpers import tie_machine as tm
    return tm()


def tie_pairs():
    """K, L in 1..4 with every weight 1, then quantised rows (1, 1/2, 1/4, some -inf) on both tapes."""
    out = [(np.zeros((K, 2)), np.zeros((L, 4))) for K in range(1, 5) for L in range(1, 5)]
    rng = np.random.RandomState(41)
    for K, L in ((2, 3), (3, 2), (3, 4), (4, 4)) * 3:
        out.append((quantised_rows(rng, 1, K, 0.1), quantised_rows(rng, 3, L, 0.1)))
    return out


def hand_tie_cases():
    """[(em, colTok, A, B, edges, rows, inRows)] worked by hand, every weight 1 (log 0), one column on the one output token.
    em2 at (1, 0): W[1][0][0][1] is attained by the input-only edge 0 -> 1 (edge 1) out of Z[0][0][0][0] and by the silent edge 0 -> 1
    (edge 2) out of W[1][0][0][0], which the input-only loop reached: the input-only edge comes first.  Z[1][0][0][1] is attained by
    that W and by the input blank out of Z[0][0][0][1]: W comes first.  The path is edge 1 alone, at output row 0 and input row 0.
    em3 at (1, 1): N[1][0] is -inf in every plane (nothing arrives at r = 0 past i = 0), so the repeat is dead and N[1][1][1][1] is
    attained by the match 0 -> 1 (edge 1) out of XZ[0][0][1][0] and by the output-only edge 0 -> 1 (edge 2) out of XW[1][0][1][0]:
    the match comes first.  The end Z[1][1][.][1] is attained by plane 1 alone (plane 0 holds state 1 only through the blank row,
    which needs N[1][0]).  The path is edge 1 alone."""
    em2 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 0, 0.0), (0, 1, 0, 0, 0.0)])
    em3 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 1, 0.0), (0, 1, 0, 1, 0.0)])
    return [(em2, (1,), np.zeros((1, 2)), np.zeros((0, 2)), [1], [0], [0]), (em3, (1,), np.zeros((1, 2)), np.zeros((1, 2)), [1], [0], [0])]


CHAIN_S = 5
CHAIN_SHAPES = ((3, 4), (0, 0), (4, 0), (0, 4), (1, 1), (3, 4))


def chain_case():
    """The chain machine against profiles without blanks on either tape and one column per token whose rows alternate between two
    columns (no repeat can stand in for an emission): every path has K + L + (K + L + 1)(S - 1) edges, the bound."""
    em = chain_machine(CHAIN_S)
    colTok = tuple(range(1, em.nOutTok + 1)) * 2
    pairs = []
    for k, (K, L) in enumerate(CHAIN_SHAPES):
        rng = np.random.RandomState(500 + k)
        A, B = merged_input(rng, em, len(colTok), K, L, pInf=0.0)
        A = A.copy(); B = B.copy(); A[:, 0] = -np.inf; B[:, 0] = -np.inf
        for r in range(L):                         # row r keeps the columns of one half of the map: the last column is never offered again
            half = slice(1, 1 + em.nOutTok) if r % 2 else slice(1 + em.nOutTok, 1 + 2 * em.nOutTok)
            B[r, half] = -np.inf
        pairs.append((A, B))
    return em, colTok, pairs


# ---- the GPU suite (held to its liveness conditions without a GPU by test_profile_two_merge_host.py::test_gpu_inputs_are_live) -----------
LANE_CASES = ((1, 1), (2, 1), (4, 13), (4, 65), (63, 2), (65, 2))           # (nCols, S)
LANE_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (5, 2), (9, 9))


def lane_case(nCols, S):
    """(colTok, [(em, A, B)]): the machine with silent levels (S >= 2) and without over alphabets (2, 3), each at every shape."""
    rng = np.random.RandomState(31 * nCols + S)
    colTok = rng.randint(1, 4, nCols)
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 300 + S, levels, 2, 3)
        for K, L in LANE_SHAPES:
            out.append((em,) + merged_input(np.random.RandomState(40000 + 1000 * S + 100 * nCols + 10 * K + L), em, nCols, K, L, pInf=0.05))
    return colTok, out


RING_S = 20
RING_COLS = 2                                      # a ring takes 24 (5 nCols + 3)(min(K, L) + 1) S = 6 240 (min(K, L) + 1) bytes
RING_LDS_MAX = 160 * 1024
RING_SHORT = (9, 10, 25, 26)                       # 62 400 / 68 640 bytes (64 KiB) and 162 240 / 168 480 bytes (160 KiB)
RING_LONG = 30
RING_SHAPES = tuple((m, RING_LONG) for m in RING_SHORT) + tuple((RING_LONG, m) for m in RING_SHORT)
MIXED_EXTRA = ((2, 3), (0, 40), (40, 0))
RING_COLTOK = (2, 3)


def ring_bytes(S, nCols, K, L, mat=False):
    return 24 * (2 * nCols if mat else 5 * nCols + 3) * (min(K, L) + 1) * S


def ring_pairs():
    """The eight ring pairs (found by i: K the short side; found by r: L the short side), then (2, 3), (0, 40), (40, 0) and a dead
    pair (a whole -inf row in B)."""
    em = pair_machine(RING_S, 40, True, 2, 3)
    pairs = [merged_input(np.random.RandomState(3000 + 100 * K + L), em, RING_COLS, K, L, pInf=0.0) for K, L in RING_SHAPES + MIXED_EXTRA]
    A, B = merged_input(np.random.RandomState(3999), em, RING_COLS, 5, 6, pInf=0.0)
    B = B.copy(); B[2] = -np.inf
    return em, pairs + [(A, B)]


PACKED_S = 140                                     # 6 240 * 4 * 140 / 20 = 174 720 bytes: past 160 KiB at K = L = 3
PACKED_SHAPES = ((3, 3), (3, 4), (4, 3), (2, 3)) * 6
PACKED_COLTOK = (1, 2)


def packed_case():
    """Twenty-four pairs on one levelled machine of 140 states, eighteen of them with rings in scratch (every fourth, (2, 3), has its
    ring in LDS): three workgroups to a die, so that rings which overlapped would meet in one cache."""
    em = pair_machine(PACKED_S, PACKED_S, True, 2, 2)
    return em, [merged_input(np.random.RandomState(5700 + k), em, 2, K, L, pInf=0.0) for k, (K, L) in enumerate(PACKED_SHAPES)]


COUNT_SHAPES = ((3, 4), (4, 3), (0, 3))
COUNT_COLTOK = (1, 3, 5, 3)


def big_counts_case():
    """11 204 transitions, past the 8 192 the counts kernel keeps in LDS: S = 700 with levels, (nIn, nOut) = (3, 5), four columns;
    three pairs and a dead pair (one row of B all -inf) to put beside them."""
    em = pair_machine(700, 700, True, 3, 5)
    pairs = [merged_input(np.random.RandomState(700 + k), em, 4, K, L, pInf=0.0) for k, (K, L) in enumerate(COUNT_SHAPES)]
    A, B = merged_input(np.random.RandomState(799), em, 4, 3, 4, pInf=0.0)
    B = B.copy(); B[2] = -np.inf
    return em, pairs, (A, B)


SEAM_PAIRS = 129
SEAM_DEAD = (63, 64, 128)                          # the last lane of block 0, the first of block 1, the only one of block 2
SEAM_SHAPES = LANE_SHAPES[:-1]
SEAM_COLTOK = (3, 1, 3)


def seam_case():
    """(em, pairs): 129 pairs on a levelled machine of 8 states, the shapes below (9, 9) in turn, a twentieth of the weights -inf;
    three dead pairs at the seams of the traceback's blocks of 64 lanes."""
    em = pair_machine(8, 108, True, 2, 3)
    pairs = []
    for k in range(SEAM_PAIRS):
        K, L = SEAM_SHAPES[k % len(SEAM_SHAPES)]
        pairs.append(merged_input(np.random.RandomState(9000 + k), em, 3, K, L, pInf=0.05))
    for k in SEAM_DEAD:
        A, B = merged_input(np.random.RandomState(9000 + k), em, 3, 3, 4, pInf=0.0)
        B = B.copy(); B[1] = -np.inf
        pairs[k] = (A, B)
    return em, pairs


def degenerate_cases():
    """(em, colTok, [(A, B)]) at (6, 7) on S = 40, three columns: all-blank rows on either tape, a whole -inf row on either tape, an
    eighth of the weights -inf."""
    em = pair_machine(40, 11, True, 2, 3)
    colTok = (1, 2, 3)
    rng = np.random.RandomState(11)
    A, B = merged_input(rng, em, 3, 6, 7, pInf=0.0)
    blankA = A.copy(); blankA[2, 1:] = -np.inf; blankA[4, 1:] = -np.inf
    blankB = B.copy(); blankB[3, 1:] = -np.inf
    allBlank = B.copy(); allBlank[:, 1:] = -np.inf
    deadA = A.copy(); deadA[3] = -np.inf
    deadB = B.copy(); deadB[5] = -np.inf
    return em, colTok, [(blankA, B), (A, blankB), (blankA, blankB), (A, allBlank), (deadA, B), (A, deadB)] + [merged_input(rng, em, 3, 6, 7, pInf=0.125) for _ in range(3)]


COLMAPS = ((1,), (2, 2, 2), (1, 4), (3, 1, 3))       # one column; all columns on one token; a token nothing emits (4); a doubled symbol


def column_map_cases():
    """(em, [(colTok, A, B)]): the machine emits tokens 1..3 of an output alphabet of 4, so token 4 heads a column nothing emits."""
    from prefixhelpers import machine_edges
    base = pair_machine(6, 21, True, 2, 3)
    em = machine_from_edges(base.nStates, 2, 4, machine_edges(base))
    out = []
    for k, ct in enumerate(COLMAPS):
        out.append((ct,) + merged_input(np.random.RandomState(600 + k), em, len(ct), 4, 5, pInf=0.05))
    return em, out


BUDGET_S = 65
BUDGET_SHAPES = ((5, 6), (2, 5), (0, 0), (6, 5), (0, 4), (4, 4), (6, 3), (4, 0))
BUDGET_COLTOK = (1, 2, 3)


def budget_case():
    em = pair_machine(BUDGET_S, 165, True, 2, 3)
    return em, [merged_input(np.random.RandomState(8000 + k), em, 3, K, L, pInf=0.0) for k, (K, L) in enumerate(BUDGET_SHAPES)]


def cell_bytes(S, nCols, K, L):
    return 8 * 3 * (nCols + 1) * S * (K + 1) * (L + 1)


# ---- the device against the restatement (the GPU module; the device is touched only when these are called) -------------------------------
WORST = {}


def reference(dp, A, B):
    ll, N, W, Z = dp.forward(A, B)
    _, NB, WB, ZB = dp.backward(A, B)
    v, VN, VW, VZ = dp.forward(A, B, "max")
    return dict(ll=ll, fwd=np.stack([N, W, Z], axis=2), bwd=np.stack([NB, WB, ZB], axis=2), v=v, vit=np.stack([VN, VW, VZ], axis=2),
                path=dp.viterbi(A, B)[1:], counts=dp.counts(A, B)[0])


def check_machine(em, colTok, pairs, fill=True, live=None, refs=None):
    """Everything the device computes for the pairs of one machine and one column map, in one batch, against the restatement."""
    from machineboss_amd import capi
    from machineboss_amd.profile import TwoMergedProfileDP
    dp = TwoMergedProfileDP(em, colTok)
    refs = [reference(dp, A, B) for A, B in pairs] if refs is None else refs
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs], colTok=colTok)
    try:
        want = np.array([r["ll"] for r in refs])
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        note("forward", fr, want, WORST)
        assert logs_close(fr, want) and logs_close(fm, want), (fr, fm, want)
        assert np.array_equal(fr, fm)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        v, off, edges, rows, ins = dev.viterbi()
        note("viterbi", v, wv, WORST)
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, r in enumerate(refs):
            sl = slice(off[k], off[k + 1])
            assert np.array_equal(edges[sl], r["path"][0]) and np.array_equal(rows[sl], r["path"][1]) and np.array_equal(ins[sl], r["path"][2]), k
        c, s, ll = dev.counts()
        wc = np.sum([r["counts"] for r in refs], axis=0)
        note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and (s == -math.inf if (want == -math.inf).any() else abs(s - want.sum()) <= 1e-9 * max(1.0, abs(want.sum())))
        if fill:
            for (A, B), r in zip(pairs, refs):
                for mode, key in ((capi.MB_FORWARD, "fwd"), (capi.MB_BACKWARD, "bwd")):
                    got = capi.profile_two_fill_merged(dm, mode, A, B, colTok)
                    note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key]), (mode, len(A), len(B))
                    if live is not None:
                        live["cells"] += int(np.isfinite(r[key]).sum()); live["all"] += r[key].size
                assert logs_close(capi.profile_two_fill_merged(dm, capi.MB_VITERBI, A, B, colTok), r["vit"], 1e-12), (len(A), len(B))
        if live is not None:
            live["ll"] += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
