"""Machines, inputs, bounds and the device-against-restatement comparison of the two-tape profile tests (test_profile_pair_host.py,
test_profile_pair_gpu.py, test_profile_pair_edges_gpu.py; not a test module)."""
import math

import numpy as np

from prefixhelpers import machine_edges, machine_from_edges, populated_machine, twin_machine
from profileprefixhelpers import random_profile

LOG_TOL = 1e-9          # log values: relative to max(1, |value|), -inf matching exactly
COUNT_REL = 1e-6        # counts >= 1e-3: relative
COUNT_ABS = 1e-9        # counts below 1e-3: COUNT_ABS + COUNT_REL * count, absolute


def pair_machine(S, seed, levels, nIn, nOut):
    """populated_machine(S, seed, levels, nIn, nOut) plus, on each of start -> start, start -> end and end -> end, one input-only
    edge per input symbol, one output-only edge per output symbol and one matching edge per input symbol.  populated_machine alone
    sends its edges to random states, so a lattice of a handful of cells -- (I, L) = (3, 0), (1, 1), (7, 2) -- cannot reach the end
    state of a machine without silent levels and scores -inf whatever the seed; with these edges every shape but (0, 0) without
    levels (where nothing can move at all) has a finite likelihood, and the liveness conditions of the suites can hold.  No silent
    edge is added: a machine without levels stays without."""
    em = populated_machine(S, seed, levels, nIn, nOut)
    lw = float(np.log(0.15))
    extra = []
    for s, d in sorted({(0, 0), (0, S - 1), (S - 1, S - 1)}):
        extra += [(s, d, a, 0, lw) for a in range(1, nIn + 1)]
        extra += [(s, d, 0, o, lw) for o in range(1, nOut + 1)]
        extra += [(s, d, a, a % nOut + 1, lw) for a in range(1, nIn + 1)]
    return machine_from_edges(S, nIn, nOut, machine_edges(em) + extra)


def pair_input(rng, em, I, L, pZero=0.2):
    """(x, P): I input tokens and a random profile of L rows with a positive blank."""
    x = rng.randint(1, em.nInTok + 1, size=I).astype(np.int32) if I else np.zeros(0, np.int32)
    return x, random_profile(rng, L, em.nOutTok, pZero)


def logs_close(got, want, tol=LOG_TOL):
    """Every entry within tol * max(1, |want|), -inf (and only -inf) matching -inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or np.isnan(got).any():
        return False
    dead = want == -math.inf
    if not np.array_equal(got == -math.inf, dead):
        return False
    return bool(np.all(np.abs(got[~dead] - want[~dead]) <= tol * np.maximum(1.0, np.abs(want[~dead]))))


def log_dev(got, want):
    """The worst deviation relative to max(1, |want|) over the finite entries."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    fin = want > -math.inf
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])), initial=0.0))


def counts_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    big = want >= 1e-3
    return bool(np.all(np.abs(got[big] - want[big]) <= COUNT_REL * want[big]) and
                np.all(np.abs(got[~big] - want[~big]) <= COUNT_ABS + COUNT_REL * want[~big]))


# ---- the GPU suite (test_profile_pair_gpu.py; held to its liveness conditions without a GPU by
# test_profile_pair_host.py::test_pair_suite_inputs_are_live) ---------------------------------------------------------------------
SUITE_STATES = (1, 2, 8, 65, 300)
SUITE_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 7), (7, 2), (9, 9))
SUITE_ALPHABETS = ((1, 1), (2, 3), (3, 2))
SUITE_CASES = [(S, nIn, nOut) for S in SUITE_STATES for nIn, nOut in SUITE_ALPHABETS]


def suite_case(S, nIn, nOut):
    """[(em, x, P)] of one case: the machine with silent levels (S >= 2) and without, each at every shape of SUITE_SHAPES."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 100 + S, levels, nIn, nOut)
        for I, L in SUITE_SHAPES:
            out.append((em,) + pair_input(np.random.RandomState(1000 * S + 10 * I + L), em, I, L))
    return out


def wide_case():
    """A diagonal with more items than lanes and a ring that wraps many times: S = 40, I = L = 40."""
    em = pair_machine(40, 41, True, 2, 3)
    return (em,) + pair_input(np.random.RandomState(41), em, 40, 40)


RING_BYTES_PER_STATE = 48 * 4      # 3 diagonals x 2 layers x (min(I, L) + 1 = 4) cells x 8 bytes, at I = L = 3
# the largest S whose ring fits the LDS limit and the first beyond it (LDS, then global scratch), around 160 KiB and around the
# 64 KiB from which the kernel has to be told; and the same marks for a ring of 24 * 4 * S bytes, a single layer
LDS_STATES = sorted({lim // per + k for lim in (160 * 1024, 64 * 1024) for per in (RING_BYTES_PER_STATE, 24 * 4) for k in (0, 1)})


def lds_case(S):
    em = pair_machine(S, S, False, 2, 2)
    return (em,) + pair_input(np.random.RandomState(S), em, 3, 3, pZero=0.0)


def ragged_case():
    """Ten pairs with I = 0..9 and L = 9..0 on one machine: S = 40 with levels."""
    em = pair_machine(40, 7, True, 3, 5)
    return em, [pair_input(np.random.RandomState(50 + I), em, I, 9 - I) for I in range(10)]


CHUNK_SHAPE = (300, 24, 12, 12)      # S, pairs, I, L


def chunk_case():
    S, n, I, L = CHUNK_SHAPE
    em = pair_machine(S, 300, True, 2, 3)
    return em, [pair_input(np.random.RandomState(70 + k), em, I, L) for k in range(n)]


def chained_case():
    """S = 65, (nIn, nOut) = (3, 2), I = 5, L = 9, four pairs: against the chained prefix fills."""
    em = pair_machine(65, 165, True, 3, 2)
    return em, [pair_input(np.random.RandomState(90 + k), em, 5, 9) for k in range(4)]


def sparse_case():
    """A third of the profile's weights -inf, blanks included."""
    em = pair_machine(40, 11, True, 2, 3)
    rng = np.random.RandomState(11)
    pairs = []
    for k in range(6):
        x = rng.randint(1, 3, size=6).astype(np.int32)
        w = rng.uniform(0.05, 1.0, (8, 4))
        with np.errstate(divide="ignore"):
            pairs.append((x, np.log(np.where(rng.rand(8, 4) < 1.0 / 3.0, 0.0, w))))
    return em, pairs


# ---- the device against the restatement (the GPU modules; the device is touched only when these are called) ----------------------
WORST = {}


def note(what, got, want, worst=None):
    worst = WORST if worst is None else worst
    worst[what] = max(worst.get(what, 0.0), log_dev(got, want))
    print("worst deviation so far, %s: %.3g" % (what, worst[what]))


def note_counts(c, wc, worst=None, what="counts"):
    worst = WORST if worst is None else worst
    big = wc >= 1e-3
    worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(c[big] - wc[big]) / wc[big], initial=0.0)))
    worst["small " + what] = max(worst.get("small " + what, 0.0), float(np.max(np.abs(c[~big] - wc[~big]), initial=0.0)))
    print("worst deviation so far, %s: %.3g relative, %.3g absolute below 1e-3" % (what, worst[what], worst["small " + what]))


def reference(dp, x, P):
    ll, N, W = dp.forward(x, P)
    _, NB, WB = dp.backward(x, P)
    v, VN, VW = dp.forward(x, P, "max")
    return dict(ll=ll, fwd=np.stack([N, W], axis=2), bwd=np.stack([NB, WB], axis=2), v=v, vit=np.stack([VN, VW], axis=2),
                path=dp.viterbi(x, P)[1:], counts=dp.counts(x, P)[0])


def check_machine(em, pairs, fill=True, live=None, worst=None):
    """Everything the device computes for the pairs of one machine, in one batch, against the restatement."""
    from machineboss_amd import capi
    from machineboss_amd.profile import PairProfileDP
    dp = PairProfileDP(em)
    refs = [reference(dp, x, P) for x, P in pairs]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        want = np.array([r["ll"] for r in refs])
        for flags in (capi.MB_ROLLING, capi.MB_MATERIALISE):
            got = dev.forward(flags)
            note("forward", got, want, worst)
            assert logs_close(got, want), (flags, got, want)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        v, off, edges, rows = dev.viterbi()
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, r in enumerate(refs):
            assert np.array_equal(edges[off[k]:off[k + 1]], r["path"][0]) and np.array_equal(rows[off[k]:off[k + 1]], r["path"][1]), k
        c, s, ll = dev.counts()
        wc = np.sum([r["counts"] for r in refs], axis=0)
        note_counts(c, wc, worst)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and (s == -math.inf if (want == -math.inf).any() else abs(s - want.sum()) <= 1e-9 * max(1.0, abs(want.sum())))
        if fill:
            for (x, P), r in zip(pairs, refs):
                for mode, key in ((capi.MB_FORWARD, "fwd"), (capi.MB_BACKWARD, "bwd")):
                    got = capi.profile_pair_fill(dm, mode, x, P)
                    note("cells", got, r[key], worst)
                    assert logs_close(got, r[key]), (mode, len(x), len(P))
                    if live is not None:
                        live["cells"] += int(np.isfinite(r[key]).sum()); live["all"] += r[key].size
                assert logs_close(capi.profile_pair_fill(dm, capi.MB_VITERBI, x, P), r["vit"], 1e-12), (len(x), len(P))
        if live is not None:
            live["ll"] += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs


def assert_live(live):
    assert np.mean(live["ll"]) >= 0.9, np.mean(live["ll"])
    assert live["all"] == 0 or live["cells"] >= 0.5 * live["all"], (live["cells"], live["all"])


# ---- the edge suite (test_profile_pair_edges_gpu.py; held to its liveness conditions without a GPU by
# test_profile_pair_host.py::test_pair_edge_suite_inputs_are_live) -----------------------------------------------------------------
HALF = math.log(0.5)
RING_S = 300                                      # a ring takes 48 * (min(I, L) + 1) * S bytes
RING_LDS_MAX = 160 * 1024
# 158 400 bytes: the last ring in LDS (past 64 KiB, so the limit is raised); 172 800: global scratch, found by i; by r
RING_SHAPES = ((10, 30), (11, 30), (30, 11))
MIXED_SHAPES = ((10, 30), (11, 30), (30, 11), (2, 3), (11, 11), (0, 40), (40, 0), (11, 30))


def ring_bytes(S, I, L):
    return 48 * (min(I, L) + 1) * S


def ring_machine(levels):
    return pair_machine(RING_S, 300, levels, 2, 3)


def ring_case(I, L, levels):
    em = ring_machine(levels)
    return (em,) + pair_input(np.random.RandomState(3000 + 100 * I + L + (0 if levels else 7)), em, I, L)


def mixed_case():
    """Eight pairs on the levelled ring machine: rings in LDS below and above 64 KiB and in global scratch, found by i and by r,
    square, without input and without rows; (11, 30) twice with different data.  The first three are the pairs of ring_case."""
    em = ring_machine(True)
    pairs = [ring_case(I, L, True)[1:] for I, L in MIXED_SHAPES[:3]]
    return em, pairs + [pair_input(np.random.RandomState(3100 + k), em, I, L) for k, (I, L) in enumerate(MIXED_SHAPES) if k >= 3]


PACKED_S = 854                                   # 48 * 4 * 854 = 163 968 bytes: the first ring past 160 KiB at I = L = 3 (LDS_STATES)
PACKED_SHAPES = ((3, 3), (3, 4), (4, 3), (2, 3)) * 6


def packed_case():
    """Twenty-four pairs on one levelled machine of 854 states, eighteen of them with rings in scratch (every fourth, (2, 3), has its
    ring in LDS): more workgroups than the device has dies, so that rings which overlapped would meet in one cache."""
    em = pair_machine(PACKED_S, PACKED_S, True, 2, 2)
    return em, [pair_input(np.random.RandomState(8540 + k), em, I, L, pZero=0.0) for k, (I, L) in enumerate(PACKED_SHAPES)]


COUNT_SHAPES = ((5, 6), (6, 5), (0, 3))          # (I + 1)(L + 1) <= 45: see test_counts_past_the_lds_table on the fixed point


def big_counts_case():
    """11 204 transitions, past the 8 192 the counts kernel keeps in LDS: S = 700 with levels, (nIn, nOut) = (3, 5); three pairs, one
    much shorter than the others; and a dead pair (one profile row all -inf) to put beside them."""
    em = pair_machine(700, 700, True, 3, 5)
    pairs = [pair_input(np.random.RandomState(700 + k), em, I, L) for k, (I, L) in enumerate(COUNT_SHAPES)]
    x, P = pair_input(np.random.RandomState(799), em, 5, 6)
    P = P.copy(); P[2] = -np.inf
    return em, pairs, (x, P)


def flat_counts_case():
    """8 634 transitions without silent levels: S = 1 200, (nIn, nOut) = (2, 2), one pair at (5, 6)."""
    em = pair_machine(1200, 1200, False, 2, 2)
    return em, [pair_input(np.random.RandomState(1200), em, 5, 6)]


def tie_machine():
    """Weights that are multiples of log 0.5.  Two routes 0 -> 3 tie at every step:
    N ties: the blank against a match (0 -> 0 reading a, emitting A, at weight 1 beside a blank of weight 1 ... see the census);
    W ties: staying against an input-only self-loop, an input-only edge against a silent one."""
    edges = [(0, 0, 1, 1, 0.0), (0, 0, 0, 1, 0.0), (0, 0, 1, 0, 0.0), (0, 1, 1, 0, HALF), (0, 1, 0, 0, HALF), (1, 1, 1, 1, 0.0),
             (1, 1, 0, 1, 0.0), (1, 1, 1, 0, 0.0), (1, 2, 0, 0, HALF), (1, 2, 1, 0, HALF), (2, 3, 0, 0, 0.0), (2, 2, 1, 1, 0.0),
             (2, 2, 0, 1, 0.0), (2, 2, 1, 0, 0.0), (3, 3, 1, 0, 0.0), (3, 3, 1, 1, 0.0), (3, 3, 0, 1, 0.0)]
    return machine_from_edges(4, 1, 1, edges)


def tie_pairs():
    """I, L in 1..4: the one input symbol I times against L rows whose blank and symbol both weigh 1."""
    return [(np.ones(I, np.int32), np.zeros((L, 2))) for I in range(1, 5) for L in range(1, 5)]


def hand_tie_cases():
    """[(em, x, P)]: the two machines of test_tie_census worked by hand.  em2: W[1][0][1] is attained by the input-only edge 0 -> 1
    and by the loop and then the silent edge; em3: N[1][1][1] by the match and by the loop and then the output-only edge."""
    em2 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 0, 0.0), (0, 1, 0, 0, 0.0)])
    em3 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 1, 0.0), (0, 1, 0, 1, 0.0)])
    return [(em2, np.array([1], np.int32), np.zeros((0, 2))), (em3, np.array([1], np.int32), np.zeros((1, 2)))]


TWIN_INPUTS = ((1, 2, 3), (2, 1, 3))


def twin_case():
    """(em, [(x, P)]): the quantised twin machine (symbols 1 and 2 read the same edges at the same weights) at (3, 3), against one
    profile of multiples of log 0.5, on two inputs that differ only in which twin stands where."""
    em = twin_machine(5, 1, quantised=True)
    P = HALF * np.random.RandomState(5).randint(0, 3, size=(3, 3)).astype(np.float64)
    return em, [(np.array(x, np.int32), P) for x in TWIN_INPUTS]


CHAIN_S = 5
CHAIN_SHAPES = ((3, 4), (0, 0), (4, 0), (0, 4), (1, 1), (3, 4))


def chain_machine(S, nIn=2, nOut=3):
    """Silent edges s -> s+1 for every s; from S-1 back to 0 one input-only edge per input symbol and one output-only edge per output
    symbol; no match edge; every weight log 0.5.  nLevF = S, and against a profile without blanks every path has
    I + L + (I + L + 1)(S - 1) edges: the traceback's bound."""
    edges = [(s, s + 1, 0, 0, HALF) for s in range(S - 1)]
    edges += [(S - 1, 0, a, 0, HALF) for a in range(1, nIn + 1)] + [(S - 1, 0, 0, o, HALF) for o in range(1, nOut + 1)]
    return machine_from_edges(S, nIn, nOut, edges)


def chain_case():
    em = chain_machine(CHAIN_S)
    pairs = []
    for k, (I, L) in enumerate(CHAIN_SHAPES):
        x, P = pair_input(np.random.RandomState(500 + k), em, I, L, pZero=0.0)
        P = P.copy(); P[:, 0] = -np.inf
        pairs.append((x, P))
    return em, pairs


FLAT_SHAPES = ((5, 60), (60, 5))


def flat_diagonals_case(I, L):
    """S = 300 at (5, 60) or (60, 5): six cells of 300 states on every one of 55 diagonals in a row, 1 800 items against 1 024 lanes;
    at (60, 5) the first cell of each of them is past i = 0."""
    em = pair_machine(300, 302, True, 3, 2)
    return em, [pair_input(np.random.RandomState(302 + I), em, I, L)]


SMALL_SHAPES = ((4, 6), (6, 4))
SMALL_ALPHABETS = ((1, 4), (4, 1), (5, 3))


def alphabet_case(nIn, nOut):
    """[(em, pairs)]: S = 65 with silent levels and without, each at (4, 6) and (6, 4)."""
    out = []
    for levels in (True, False):
        em = pair_machine(65, 65 + 10 * nIn + nOut, levels, nIn, nOut)
        out.append((em, [pair_input(np.random.RandomState(650 + 10 * nIn + nOut + I), em, I, L) for I, L in SMALL_SHAPES]))
    return out


def pair_self_loop_case():
    """The machine of prefixhelpers.self_loop_case with pair_machine's edges: a silent self-loop on the start state, the last edge."""
    em = pair_machine(8, 3, True, 3, 5)
    em = machine_from_edges(8, 3, 5, machine_edges(em) + [(0, 0, 0, 0, float(np.log(0.1)))])
    return em, [pair_input(np.random.RandomState(80 + I), em, I, L) for I, L in SMALL_SHAPES]


def self_loop_edge(em):
    return int(np.nonzero((em.src == 0) & (em.dst == 0) & (em.inTok == 0) & (em.outTok == 0))[0][0])


FAR_SHIFT = -700.0


def far_case():
    """(em, x, P, P + FAR_SHIFT) at (9, 9): every entry of the profile 700 lower, a lattice whose cells run down to about -6 300."""
    em = pair_machine(65, 9, True, 2, 3)
    x, P = pair_input(np.random.RandomState(99), em, 9, 9)
    return em, x, P, P + FAR_SHIFT
