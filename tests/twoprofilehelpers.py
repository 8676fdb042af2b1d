"""Machines, profiles, bounds and the device-against-restatement comparison of the two-profile tests (test_profile_two_host.py,
test_profile_two_gpu.py, test_profile_two_edges_gpu.py; not a test module).  The bounds are those of pairprofilehelpers."""
import math

import numpy as np

from pairprofilehelpers import (HALF, chain_machine, counts_close, log_dev, logs_close, note, note_counts, pair_machine)  # noqa: F401
from prefixhelpers import machine_from_edges
from machineboss_amd.machine import Machine, MachineState, MachineTransition
from machineboss_amd.profile import Profile


def soft_profile(rng, rows, nTok, pInf=0.15):
    """[rows, nTok + 1] log weights: uniform(0.05, 1), every entry -- the blank too -- -inf with chance ``pInf``."""
    w = rng.uniform(0.05, 1.0, (rows, nTok + 1))
    with np.errstate(divide="ignore"):
        return np.log(np.where(rng.rand(rows, nTok + 1) < pInf, 0.0, w))


def two_input(rng, em, K, L, pInf=0.15):
    """(A, B): an input profile of K rows and an output profile of L rows."""
    return soft_profile(rng, K, em.nInTok, pInf), soft_profile(rng, L, em.nOutTok, pInf)


def one_hot(x, nIn):
    """The token string x as an input profile: 0 on its token per row, -inf elsewhere, the blank -inf."""
    A = np.full((len(x), nIn + 1), -np.inf)
    A[np.arange(len(x)), np.asarray(x, np.int64)] = 0.0
    return A


def machine_of(em):
    """An EvaluatedMachine as a Machine with numeric weights, transitions in global-id order."""
    m = Machine()
    for _ in range(em.nStates):
        m.state.append(MachineState())
    isym, osym = em.inputTokenizer.tok2sym, em.outputTokenizer.tok2sym
    for e in range(em.nTransitions):
        m.state[int(em.src[e])].trans.append(MachineTransition(dest=int(em.dst[e]), inp=isym[em.inTok[e]] if em.inTok[e] else "",
                                                                out=osym[em.outTok[e]] if em.outTok[e] else "", weight=float(np.exp(em.logWeight[e]))))
    return m


def profile_of(syms, P):
    """The Profile whose log rows against the alphabet ``syms`` (tok2sym[1:]) are P: the symbols head the columns, the blank last."""
    return Profile(list(syms), [list(np.exp(row[1:])) + [float(np.exp(row[0]))] for row in P])


def end_loop_variant(em):
    """``em`` with the end state stripped of its input-reading edges and given one output-only self-loop (the case a mask on the
    input blank would get wrong, docs/profile_tapes.md "Pairs of profiles")."""
    from prefixhelpers import machine_edges
    S = em.nStates
    edges = [e for e in machine_edges(em) if not (e[0] == S - 1 and e[2] > 0)]
    return machine_from_edges(S, em.nInTok, em.nOutTok, edges + [(S - 1, S - 1, 0, 1, float(np.log(0.3)))])


def transposed(em):
    from prefixhelpers import machine_edges
    return machine_from_edges(em.nStates, em.nOutTok, em.nInTok, [(s, d, o, a, w) for s, d, a, o, w in machine_edges(em)])


# ---- the host grid (test_profile_two_host.py) --------------------------------------------------------------------------------------
HOST_STATES = (3, 5, 8)
HOST_SEEDS = (0, 1, 2)
HOST_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 4), (4, 2), (3, 3))


def host_cases():
    for S in HOST_STATES:
        for levels in (True, False):
            for seed in HOST_SEEDS:
                em = pair_machine(S, seed, levels, 2, 3)
                for K, L in HOST_SHAPES:
                    yield (S, levels, seed, K, L), em, two_input(np.random.RandomState(97 * seed + 10 * K + L + 1000 * S), em, K, L)


# ---- the GPU suite (test_profile_two_gpu.py; held to its liveness conditions without a GPU by
# test_profile_two_host.py::test_two_suite_inputs_are_live) -------------------------------------------------------------------------
SUITE_STATES = (1, 2, 8, 65)
SUITE_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (5, 2), (9, 9))
SUITE_ALPHABETS = ((1, 1), (2, 3), (3, 4))
SUITE_CASES = [(S, nIn, nOut) for S in SUITE_STATES for nIn, nOut in SUITE_ALPHABETS]


def suite_case(S, nIn, nOut):
    """[(em, A, B)] of one case: the machine with silent levels (S >= 2) and without, each at every shape of SUITE_SHAPES; a tenth of
    the weights of either profile -inf (the seeds are chosen so that nine in ten likelihoods are finite all the same)."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 100 + S, levels, nIn, nOut)
        for K, L in SUITE_SHAPES:
            out.append((em,) + two_input(np.random.RandomState(200000 + 1000 * S + 10 * K + L), em, K, L, pInf=0.1))
    return out


RING_S = 40                                       # a ring takes 72 * (min(K, L) + 1) * S bytes
RING_LDS_MAX = 160 * 1024
RING_SHORT = (21, 22, 55, 56)                     # min(K, L): rings of 63 360 / 66 240 (64 KiB) and 161 280 / 164 160 bytes (160 KiB)
RING_LONG = 60
RING_SHAPES = tuple((m, RING_LONG) for m in RING_SHORT) + tuple((RING_LONG, m) for m in RING_SHORT)
MIXED_EXTRA = ((2, 3), (0, 40), (40, 0))


def ring_bytes(S, K, L):
    return 72 * (min(K, L) + 1) * S


def ring_machine():
    return pair_machine(RING_S, 40, True, 2, 3)


def ring_pairs():
    """The eight ring pairs (found by i: K the short side; found by r: L the short side), then (2, 3), (0, 40), (40, 0) and a dead
    pair (a whole -inf row in B)."""
    em = ring_machine()
    pairs = [two_input(np.random.RandomState(3000 + 100 * K + L), em, K, L, pInf=0.0) for K, L in RING_SHAPES + MIXED_EXTRA]
    A, B = two_input(np.random.RandomState(3999), em, 5, 6, pInf=0.0)
    B = B.copy(); B[2] = -np.inf
    return em, pairs + [(A, B)]


PACKED_S = 570                                    # 72 * 4 * 570 = 164 160 bytes: past 160 KiB at K = L = 3
PACKED_SHAPES = ((3, 3), (3, 4), (4, 3), (2, 3)) * 6


def packed_case():
    """Twenty-four pairs on one levelled machine of 570 states, eighteen of them with rings in scratch (every fourth, (2, 3), has its
    ring in LDS): three workgroups to a die, so that rings which overlapped would meet in one cache."""
    em = pair_machine(PACKED_S, PACKED_S, True, 2, 2)
    return em, [two_input(np.random.RandomState(5700 + k), em, K, L, pInf=0.0) for k, (K, L) in enumerate(PACKED_SHAPES)]


COUNT_SHAPES = ((3, 4), (4, 3), (0, 3))


def big_counts_case():
    """11 204 transitions, past the 8 192 the counts kernel keeps in LDS: S = 700 with levels, (nIn, nOut) = (3, 5); three pairs and a
    dead pair (one row of B all -inf) to put beside them."""
    em = pair_machine(700, 700, True, 3, 5)
    pairs = [two_input(np.random.RandomState(700 + k), em, K, L, pInf=0.0) for k, (K, L) in enumerate(COUNT_SHAPES)]
    A, B = two_input(np.random.RandomState(799), em, 3, 4, pInf=0.0)
    B = B.copy(); B[2] = -np.inf
    return em, pairs, (A, B)


def special_profiles():
    """(em, [(A, B)]) at (6, 7) on S = 40: all-blank rows on either tape, a whole -inf row on either tape, an eighth of the weights
    -inf."""
    em = pair_machine(40, 11, True, 2, 3)
    rng = np.random.RandomState(11)
    A, B = two_input(rng, em, 6, 7, pInf=0.0)
    blankA = A.copy(); blankA[2, 1:] = -np.inf; blankA[4, 1:] = -np.inf
    blankB = B.copy(); blankB[3, 1:] = -np.inf
    deadA = A.copy(); deadA[3] = -np.inf
    deadB = B.copy(); deadB[5] = -np.inf
    return em, [(blankA, B), (A, blankB), (blankA, blankB), (deadA, B), (A, deadB)] + [two_input(rng, em, 6, 7, pInf=0.125) for _ in range(3)]


FAR_SHIFT = -700.0


def far_case():
    """(em, A, B, A + FAR_SHIFT, B + FAR_SHIFT) at (9, 9): every entry of both profiles 700 lower."""
    em = pair_machine(65, 9, True, 2, 3)
    A, B = two_input(np.random.RandomState(99), em, 9, 9, pInf=0.0)
    return em, A, B, A + FAR_SHIFT, B + FAR_SHIFT


def tie_machine():
    """Weights that are multiples of log 0.5 on one input and one output symbol: every state loops on a match, an output-only and
    an input-only edge at weight 1, and the silent edges 0 -> 1 -> 2 -> 3 stand beside input-only edges of the same weight."""
    edges = [(0, 0, 1, 1, 0.0), (0, 0, 0, 1, 0.0), (0, 0, 1, 0, 0.0), (0, 1, 1, 0, HALF), (0, 1, 0, 0, HALF), (1, 1, 1, 1, 0.0),
             (1, 1, 0, 1, 0.0), (1, 1, 1, 0, 0.0), (1, 2, 0, 0, HALF), (1, 2, 1, 0, HALF), (2, 3, 0, 0, 0.0), (2, 2, 1, 1, 0.0),
             (2, 2, 0, 1, 0.0), (2, 2, 1, 0, 0.0), (3, 3, 1, 0, 0.0), (3, 3, 1, 1, 0.0), (3, 3, 0, 1, 0.0)]
    return machine_from_edges(4, 1, 1, edges)


def tie_pairs():
    """K, L in 1..4: blank and symbol weigh 1 in every row of both profiles."""
    return [(np.zeros((K, 2)), np.zeros((L, 2))) for K in range(1, 5) for L in range(1, 5)]


TIE_KINDS = (("blank", "match"), ("match", "emit"), ("stay", "ins"), ("ins", "silent"), ("wait", "inblank"))


def hand_tie_cases():
    """[(em, A, B, edges, rows, inRows)] worked by hand, every weight 1 (log 0).
    em2 at (1, 0): W[1][0][1] is attained by the input-only edge 0 -> 1 (edge 1) out of Z[0][0][0] and by the silent edge 0 -> 1
    (edge 2) out of W[1][0][0], which the input-only loop reached: the input-only edge comes first.  Z[1][0][1] is attained by that
    W and by the input blank out of Z[0][0][1]: W comes first.  The path is edge 1 alone, at output row 0 and input row 0.
    em3 at (1, 1): N[1][0] is -inf (nothing arrives at r = 0 past i = 0), so N[1][1][1] is attained by the match 0 -> 1 (edge 1) out
    of Z[0][0][0] and by the output-only edge 0 -> 1 (edge 2) out of W[1][0][0]: the match comes first.  The path is edge 1 alone."""
    em2 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 0, 0.0), (0, 1, 0, 0, 0.0)])
    em3 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 1, 0.0), (0, 1, 0, 1, 0.0)])
    return [(em2, np.zeros((1, 2)), np.zeros((0, 2)), [1], [0], [0]), (em3, np.zeros((1, 2)), np.zeros((1, 2)), [1], [0], [0])]


CHAIN_S = 5
CHAIN_SHAPES = ((3, 4), (0, 0), (4, 0), (0, 4), (1, 1), (3, 4))


def chain_case():
    """The chain machine against profiles without blanks on either tape: every path has K + L + (K + L + 1)(S - 1) edges, the bound."""
    em = chain_machine(CHAIN_S)
    pairs = []
    for k, (K, L) in enumerate(CHAIN_SHAPES):
        A, B = two_input(np.random.RandomState(500 + k), em, K, L, pInf=0.0)
        A = A.copy(); B = B.copy(); A[:, 0] = -np.inf; B[:, 0] = -np.inf
        pairs.append((A, B))
    return em, pairs


# ---- where the host splits a call (test_profile_two_edges_gpu.py; held to its liveness conditions without a GPU by
# test_profile_two_host.py::test_two_edge_inputs_are_live) ---------------------------------------------------------------------------
COUNT_GROUP_ITEMS = 2048                          # (cell, state) items of the largest lattice per count workgroup of a pair
COUNT_GROUPS_MAX = 256


def count_groups(S, shapes):
    """Workgroups per pair of one counts launch, as mb_profile_twos_counts has it: one per 2 048 items of the largest lattice of
    the launch, an item a state of a cell -- S (K + 1)(L + 1) of them --, at least one and at most 256."""
    items = max(S * (K + 1) * (L + 1) for K, L in shapes)
    return min(COUNT_GROUPS_MAX, max(1, -(-items // COUNT_GROUP_ITEMS)))


def lattice_chunks(sizes, budget):
    """[(p0, p1)]: lattice_chunks of mb_profile_api.hip restated -- chunks of at most ``budget`` bytes, evened out to within a twentieth."""
    total = float(sum(sizes))
    n = max(1.0, math.ceil(total / budget))
    share = min(float(budget), total / n * 1.05)
    out, p0, acc = [], 0, 0.0
    for k, b in enumerate(sizes):
        if k > p0 and (acc + b > budget or (acc >= share and acc + b > share)):
            out.append((p0, k)); p0, acc = k, 0.0
        acc += b
    return out + ([(p0, len(sizes))] if len(sizes) > p0 else [])


def dead_pair(rng, em, K, L, row):
    """A pair whose output profile has one row all -inf: likelihood -inf, an empty path, no counts."""
    A, B = two_input(rng, em, K, L, pInf=0.0)
    B = B.copy(); B[row] = -np.inf
    return A, B


GROUP_S = 5
# 2 040 items: one group (409 cells, the last count below 2 048 / 5, is prime); 2 050: two, the short side found by i and by r;
# 4 205: three, and the sixth stride of 768 stops at item 365 -- group 0 whole, group 1 in part, group 2 not at all; then
# 10 240 = 5 x 2 048 against 10 400: the last lattice of five groups and the first of six, by i and by r; 20 800: eleven
GROUP_SHAPES = ((23, 16), (9, 40), (40, 9), (28, 28), (31, 63), (31, 64), (64, 31), (63, 64))
GROUP_COUNTS = (1, 2, 2, 3, 5, 6, 6, 11)
GROUP_RAGGED = ((63, 64), (2, 3), (0, 0), (0, 5), (5, 0))


def group_machine():
    return pair_machine(GROUP_S, 5, True, 2, 3)


def group_pair(em, K, L):
    return two_input(np.random.RandomState(7000 + 100 * K + L), em, K, L, pInf=0.0)


def group_case():
    """(em, one pair per shape of GROUP_SHAPES, the ragged batch, a dead pair): an odd S, so that a stride of 256 lanes does not end
    on a cell; the first pair of the ragged batch is the last of the shapes."""
    em = group_machine()
    return em, [group_pair(em, K, L) for K, L in GROUP_SHAPES], [group_pair(em, K, L) for K, L in GROUP_RAGGED], dead_pair(np.random.RandomState(7999), em, 5, 6, 2)


def fixed_counts_close(got, want, cells):
    """counts_close with the error of MB_DETERMINISTIC's fixed point added: ``cells`` adds to a transition at most, each rounded to
    the nearest 2^-36."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.where(want >= 1e-3, 0.0, 1e-9) + 1e-6 * want + cells * 2.0 ** -37))


SPLIT_S = 8
SPLIT_SHAPES = ((9, 9), (2, 5), (0, 0), (7, 9), (0, 4), (6, 7), (9, 6), (4, 0), (5, 2), (9, 9))
SPLIT_DEAD = 5                                     # the (6, 7) pair


def split_machine():
    return pair_machine(SPLIT_S, 108, True, 2, 3)


def split_case():
    """(em, pairs): ten ragged pairs on the levelled machine of 8 states, the fifth of them dead."""
    em = split_machine()
    pairs = [two_input(np.random.RandomState(8000 + 100 * k + 10 * K + L), em, K, L, pInf=0.0) for k, (K, L) in enumerate(SPLIT_SHAPES)]
    pairs[SPLIT_DEAD] = dead_pair(np.random.RandomState(8999), em, *SPLIT_SHAPES[SPLIT_DEAD], 3)
    return em, pairs


def count_bytes(S, K, L):
    """What lattice_chunks is told a pair costs mb_profile_twos_counts: the Forward and the Backward lattice."""
    return 2 * 8 * 3 * S * (K + 1) * (L + 1)


def path_bytes(S, K, L, bound):
    """And mb_profile_twos_viterbi: the max lattice and a traceback slot of ``bound`` entries in three arrays of four bytes."""
    return 8 * 3 * S * (K + 1) * (L + 1) + 12 * bound


def path_bound(nLevels, K, L):
    """The size of a traceback slot: K + L edges that read or write, and between them runs of at most ``nLevels`` silent ones."""
    return K + L + (K + L + 1) * nLevels


SEAM_PAIRS = 129
SEAM_DEAD = (63, 64, 128)                          # the last lane of block 0, the first of block 1, the only one of block 2
SEAM_SHAPES = SUITE_SHAPES[:-1]


def seam_case():
    """(em, pairs): 129 pairs on the machine of split_case, the shapes of the suite below (9, 9) in turn, a tenth of the weights
    -inf; three dead pairs at the seams of the traceback's blocks of 64 lanes."""
    em = split_machine()
    pairs = []
    for k in range(SEAM_PAIRS):
        K, L = SEAM_SHAPES[k % len(SEAM_SHAPES)]
        pairs.append(two_input(np.random.RandomState(9000 + k), em, K, L, pInf=0.1))
    for k in SEAM_DEAD:
        pairs[k] = dead_pair(np.random.RandomState(9000 + k), em, 3, 4, 1)
    return em, pairs


def rescore(em, A, B, edges, rows, ins):
    """The weight of a path with its blanks filled in: the rows of either tape that no edge consumed took the blank."""
    w = sum(float(em.logWeight[e]) for e in edges)
    usedB = {int(r) for e, r in zip(edges, rows) if em.outTok[e]}
    usedA = {int(i) for e, i in zip(edges, ins) if em.inTok[e]}
    w += sum(B[r][em.outTok[e]] for e, r in zip(edges, rows) if em.outTok[e]) + sum(A[i][em.inTok[e]] for e, i in zip(edges, ins) if em.inTok[e])
    return w + sum(B[r][0] for r in range(len(B)) if r not in usedB) + sum(A[i][0] for i in range(len(A)) if i not in usedA)


# ---- the device against the restatement (the GPU module; the device is touched only when these are called) -------------------------
WORST = {}


def reference(dp, A, B):
    ll, N, W, Z = dp.forward(A, B)
    _, NB, WB, ZB = dp.backward(A, B)
    v, VN, VW, VZ = dp.forward(A, B, "max")
    return dict(ll=ll, fwd=np.stack([N, W, Z], axis=2), bwd=np.stack([NB, WB, ZB], axis=2), v=v, vit=np.stack([VN, VW, VZ], axis=2),
                path=dp.viterbi(A, B)[1:], counts=dp.counts(A, B)[0])


def check_machine(em, pairs, fill=True, live=None, refs=None):
    """Everything the device computes for the pairs of one machine, in one batch, against the restatement."""
    from machineboss_amd import capi
    from machineboss_amd.profile import TwoProfileDP
    dp = TwoProfileDP(em)
    refs = [reference(dp, A, B) for A, B in pairs] if refs is None else refs
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs])
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
                    got = capi.profile_two_fill(dm, mode, A, B)
                    note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key]), (mode, len(A), len(B))
                    if live is not None:
                        live["cells"] += int(np.isfinite(r[key]).sum()); live["all"] += r[key].size
                assert logs_close(capi.profile_two_fill(dm, capi.MB_VITERBI, A, B), r["vit"], 1e-12), (len(A), len(B))
        if live is not None:
            live["ll"] += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
