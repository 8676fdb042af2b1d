"""Machines, inputs, bounds and the device-against-restatement comparison of the two-tape merged (CTC) profile tests
(test_profile_pair_merge_host.py, test_profile_pair_merge_gpu.py; not a test module).  Every builder is deterministic; the seeds were
searched on the CPU so that the conditions the GPU tests assert hold under the restatement, and
test_profile_pair_merge_host.py::test_edge_suite_inputs_are_live holds them to that without a GPU."""
import math

import numpy as np

from mergehelpers import greedy_chunks, merged_rows
from pairprofilehelpers import (HALF, chain_machine, counts_close, log_dev, logs_close, note, note_counts, pair_machine,
                                tie_machine)

LDS_MAX = 160 * 1024
SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (5, 2), (9, 9))
LANE_CASES = ((1, 1), (2, 1), (4, 13), (4, 65), (63, 2), (65, 2))


def ring_bytes(S, nCols, I, L, mat=False):
    """The ring of mb_profile_pair_merge.h: three diagonals of min(I, L) + 1 cells, each N, W (nCols + 1 planes) and X (nCols
    planes) rolling, X alone materialised."""
    return 8 * 3 * (nCols if mat else 3 * nCols + 2) * (min(I, L) + 1) * S


def merged_input(rng, em, nCols, I, L, zeros=0.2):
    """(x, P): I input tokens and L merged rows of nCols + 1 log weights, `zeros` of the column weights -inf, the blank positive."""
    x = rng.randint(1, em.nInTok + 1, size=I).astype(np.int32) if I else np.zeros(0, np.int32)
    P = merged_rows(rng, nCols, L, zeros)
    P[:, 0] = np.log(rng.uniform(0.02, 1.0, L))
    return x, P


def lane_case(nCols, S):
    """[(em, colTok, [(x, P)])]: the machine with silent levels (S >= 2) and without, each at every shape of SHAPES in one batch;
    the columns' tokens at random from 1..3."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 200 + S, levels, 2, 3)
        rng = np.random.RandomState(1000 * nCols + S)
        colTok = rng.randint(1, 4, nCols)
        out.append((em, colTok, [merged_input(rng, em, nCols, I, L) for I, L in SHAPES]))
    return out


# ---- rings: nCols = 4, S = 40: 336 (min(I, L) + 1) S bytes ---------------------------------------------------------------------------
RING_S, RING_COLTOK = 40, (1, 2, 3, 1)
RING_SHAPES = ((3, 30), (4, 30), (11, 30), (12, 30), (30, 12))
RAGGED_SHAPES = RING_SHAPES + ((2, 3), (0, 40), (40, 0))


def ring_machine():
    return pair_machine(RING_S, 340, True, 2, 3)


def ragged_case():
    """(em, colTok, pairs): the five ring shapes, (2, 3), (0, 40), (40, 0) and a dead pair (one row all -inf) last."""
    em = ring_machine()
    pairs = [merged_input(np.random.RandomState(4000 + 100 * I + L), em, 4, I, L, zeros=0.1) for I, L in RAGGED_SHAPES]
    x, P = merged_input(np.random.RandomState(4999), em, 4, 3, 4)
    P[2] = -np.inf
    return em, RING_COLTOK, pairs + [(x, P)]


RAGGED_BUDGET = 3 * 174720 // 2 + 4096           # one scratch ring (336 * 13 * 40 bytes) and a half: the two never share a chunk

PACKED_S = 200                                   # 336 * 4 * 200 = 268 800 bytes: a scratch ring at I = L = 3
PACKED_SHAPES = ((3, 3), (3, 4), (4, 3)) * 8


def packed_case():
    """Twenty-four pairs whose rings all lie in global scratch, in one launch."""
    em = pair_machine(PACKED_S, PACKED_S, True, 2, 3)
    return em, RING_COLTOK, [merged_input(np.random.RandomState(8000 + k), em, 4, I, L, zeros=0.0) for k, (I, L) in enumerate(PACKED_SHAPES)]


# ---- counts past the LDS table -------------------------------------------------------------------------------------------------------
COUNT_SHAPES = ((3, 4), (4, 3), (0, 3))          # see test_counts_past_the_lds_table on the fixed point
COUNT_COLTOK = (1, 2)


def big_counts_case():
    """11 204 transitions (S = 700 with levels, (nIn, nOut) = (3, 5)), two columns; three pairs and a dead one."""
    em = pair_machine(700, 700, True, 3, 5)
    pairs = [merged_input(np.random.RandomState(700 + k), em, 2, I, L, zeros=0.0) for k, (I, L) in enumerate(COUNT_SHAPES)]
    x, P = merged_input(np.random.RandomState(799), em, 2, 3, 4)
    P[1] = -np.inf
    return em, COUNT_COLTOK, pairs, (x, P)


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
TIE_KINDS = ("plane", "end", "stay", "repeat", "blank", "match", "emit", "input", "silent")
TIE_COLTOK = (1, 1)


def merged_tie_machine():
    """pairprofilehelpers.tie_machine with every edge twice: weights that are multiples of log 0.5, and two equal candidates of every
    kind, so that a tie can also be met by the second of two silent, two match or two output-only edges."""
    from prefixhelpers import machine_edges, machine_from_edges
    return machine_from_edges(4, 1, 1, machine_edges(tie_machine()) * 2)


def tie_pairs():
    """Sixteen pairs: the one input symbol I times against L quantised rows (weights 1, 1/2, 1/4 and 0) over the blank and two
    columns, both of the one output token; I, L in 1..4."""
    from mergehelpers import quantised_rows
    rng = np.random.RandomState(0)
    return [(np.ones(I, np.int32), quantised_rows(rng, 2, L, p_inf=0.15)) for I in range(1, 5) for L in range(1, 5)]


# ---- column maps and rows --------------------------------------------------------------------------------------------------------------
def column_map_cases():
    """{name: (em, colTok, pairs)} at S = 12: two columns on one token, every column on one token, a column whose token (3) nothing
    emits, one column."""
    import dataclasses
    from machineboss_amd.evalmachine import Tokenizer
    out = {}
    for name, colTok in (("two", [1, 2, 1]), ("same", [2, 2, 2]), ("unused", [1, 3, 2]), ("one", [2])):
        em = pair_machine(12, 40, True, 2, 2)
        if name == "unused":
            em = dataclasses.replace(em, outputTokenizer=Tokenizer(["a", "b", "c"]))
            assert em.nOutTok == 3 and not np.any(em.outTok == 3)
        rng = np.random.RandomState(41)
        out[name] = (em, colTok, [merged_input(rng, em, len(colTok), I, L, zeros=0.15) for I, L in ((0, 4), (3, 5), (5, 3), (4, 4))])
    return out


def row_cases():
    """{name: (em, colTok, pairs)}: rows whose columns are all -inf (only blanks); a whole row -inf in one pair of a batch; a machine
    with an eighth of its weights -inf."""
    out = {}
    colTok = [1, 2, 3, 1]
    em = pair_machine(20, 50, True, 2, 3)
    rng = np.random.RandomState(51)
    pairs = [merged_input(rng, em, 4, I, L) for I, L in ((3, 6), (0, 5), (4, 2))]
    for _, P in pairs:
        P[:, 1:] = -np.inf
    out["allblank"] = (em, colTok, pairs)
    pairs = [merged_input(rng, em, 4, I, L) for I, L in ((3, 6), (2, 5), (4, 2), (5, 5))]
    pairs[1][1][3] = -np.inf
    out["infrow"] = (em, colTok, pairs)
    lw = em.logWeight.copy()
    lw[np.random.RandomState(52).choice(len(lw), len(lw) // 8, replace=False)] = -np.inf
    out["infweights"] = (em.withLogWeights(lw), colTok, [merged_input(rng, em, 4, I, L, zeros=0.1) for I, L in ((3, 6), (2, 5), (4, 2), (5, 5))])
    return out


CHAIN_S = 5
CHAIN_SHAPES = ((3, 4), (0, 0), (4, 0), (0, 4), (1, 1))


def chain_case():
    """The chain machine against merged profiles without blanks and with one column per token at weight 1 in alternating columns, so
    that every row must be emitted and no row can repeat: every path has I + L + (I + L + 1)(S - 1) edges, the bound."""
    em = chain_machine(CHAIN_S)
    pairs = []
    for k, (I, L) in enumerate(CHAIN_SHAPES):
        x = np.random.RandomState(500 + k).randint(1, 3, size=I).astype(np.int32)
        P = np.full((L, 4), -np.inf)
        P[np.arange(L), 1 + np.arange(L) % 3] = 0.0
        pairs.append((x, P))
    return em, (1, 2, 3), pairs


# ---- the device against the restatement ------------------------------------------------------------------------------------------------
WORST = {}


def reference(dp, x, P):
    ll, N, W = dp.forward(x, P)
    _, NB, WB = dp.backward(x, P)
    v, VN, VW = dp.forward(x, P, "max")
    return dict(ll=ll, fwd=np.stack([N, W], axis=2), bwd=np.stack([NB, WB], axis=2), v=v, vit=np.stack([VN, VW], axis=2),
                path=dp.viterbi(x, P)[1:], counts=dp.counts(x, P)[0])


def check_machine(em, colTok, pairs, fill=True, live=None):
    """Everything the device computes for the pairs of one machine, in one batch, against PairMergedProfileDP: rolling and
    materialised Forward (and the same bits from both), Viterbi with and without paths, counts, and every pair's three lattices."""
    from machineboss_amd import capi
    from machineboss_amd.profile import PairMergedProfileDP
    dp = PairMergedProfileDP(em, colTok)
    refs = [reference(dp, x, P) for x, P in pairs]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs], colTok)
    try:
        want = np.array([r["ll"] for r in refs])
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        note("forward", fr, want, WORST)
        assert logs_close(fr, want), (fr, want)
        assert np.array_equal(fr, fm), (fr, fm)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        v, off, edges, rows = dev.viterbi()
        note("viterbi", v, wv, WORST)
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, r in enumerate(refs):
            assert np.array_equal(edges[off[k]:off[k + 1]], r["path"][0]) and np.array_equal(rows[off[k]:off[k + 1]], r["path"][1]), k
        c, s, ll = dev.counts()
        wc = np.sum([r["counts"] for r in refs], axis=0)
        note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and (s == -math.inf if (want == -math.inf).any() else abs(s - want.sum()) <= 1e-9 * max(1.0, abs(want.sum())))
        if fill:
            for (x, P), r in zip(pairs, refs):
                for mode, key in ((capi.MB_FORWARD, "fwd"), (capi.MB_BACKWARD, "bwd")):
                    got = capi.profile_pair_fill_merged(dm, mode, x, P, colTok)
                    note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key]), (mode, len(x), len(P))
                assert logs_close(capi.profile_pair_fill_merged(dm, capi.MB_VITERBI, x, P, colTok), r["vit"], 1e-12), (len(x), len(P))
        if live is not None:
            live += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs


# ---- the traceback past one block of 64 lanes (test_profile_pair_mixed_gpu.py) -------------------------------------------------------------
SEAM_PAIRS = 129
SEAM_DEAD = (63, 64, 128)                        # the last lane of block 0, the first of block 1, the only one of block 2
SEAM_COLTOK = (1, 2)
SEAM_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 3), (3, 2), (3, 3))


def seam_case():
    """(em, colTok, pairs): 129 pairs at S = 8 with levels against merged profiles of two columns, the shapes in turn; three dead
    pairs (a row all -inf) at the seams of k_profile_pair_merge_traceback's blocks."""
    em = pair_machine(8, 208, True, 2, 3)
    pairs = []
    for k in range(SEAM_PAIRS):
        I, L = (3, 3) if k in SEAM_DEAD else SEAM_SHAPES[k % len(SEAM_SHAPES)]
        x, P = merged_input(np.random.RandomState(9200 + k), em, 2, I, L, zeros=0.1)
        if k in SEAM_DEAD:
            P[1] = -np.inf
        pairs.append((x, P))
    return em, SEAM_COLTOK, pairs
