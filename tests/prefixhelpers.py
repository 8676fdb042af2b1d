"""Machines and node families for the prefix-search tests (not a test module)."""
import numpy as np

from machineboss_amd.evalmachine import EvaluatedMachine, Tokenizer


def populated_machine(S, seed, levels, nIn=2, nOut=2):
    """A random transducer whose prefix-search lattices are well populated, with or without silent levels.

    Every state has two input-free emitting edges per output symbol and one matching edge per input symbol, all to random states,
    one inserting edge (input, no output) and now and then an emitting edge to the end state; with ``levels`` also a silent
    backbone s -> s+1 (chance 0.7) and one silent edge further on.  The output-less weights out of a state (inserting and silent
    edges) are scaled to sum to at most 0.8, so that (I - N)^-1 is a convergent sum and the prefix layer is a real probability
    mass: a child's prefix probability cannot exceed its parent's."""
    rng = np.random.RandomState(seed)
    w = lambda lo, hi: float(np.log(rng.uniform(lo, hi)))
    edges = []
    for s in range(S):
        for o in range(1, nOut + 1):
            for _ in range(2):
                edges.append((s, rng.randint(0, S), 0, o, w(0.1, 0.5)))
        for a in range(1, nIn + 1):
            edges.append((s, rng.randint(0, S), a, rng.randint(1, nOut + 1), w(0.1, 0.9)))
        edges.append((s, rng.randint(0, S), rng.randint(1, nIn + 1), 0, w(0.05, 0.4)))
        if rng.rand() < 0.2:
            edges.append((s, S - 1, 0, rng.randint(1, nOut + 1), w(0.1, 0.5)))
        if levels and s + 1 < S:
            if rng.rand() < 0.7:
                edges.append((s, s + 1, 0, 0, w(0.2, 0.6)))
            edges.append((s, rng.randint(s + 1, S), 0, 0, w(0.05, 0.3)))
    edges.sort(key=lambda e: e[0])
    n = len(edges)
    src = np.array([e[0] for e in edges], np.uint32); dst = np.array([e[1] for e in edges], np.uint32)
    it = np.array([e[2] for e in edges], np.uint16); ot = np.array([e[3] for e in edges], np.uint16)
    lw = np.array([e[4] for e in edges], np.float64)
    mass = np.zeros(S)
    np.add.at(mass, src[ot == 0].astype(np.int64), np.exp(lw[ot == 0]))
    scale = np.where(mass > 0.8, 0.8 / np.maximum(mass, 1e-300), 1.0)
    lw = np.where(ot == 0, lw + np.log(scale[src.astype(np.int64)]), lw)
    off = np.zeros(S + 1, np.int64)
    np.add.at(off, src.astype(np.int64) + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(n) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, Tokenizer([chr(65 + k) for k in range(nIn)]), Tokenizer([chr(97 + k) for k in range(nOut)]),
                            src, dst, it, ot, tidx, lw, off, [None] * S)


def family_paths(nIn):
    """The root, its children and one grandchild of each (the grandchild's token differs from child to child)."""
    toks = list(range(1, nIn + 1))
    return [()] + [(t,) for t in toks] + [(t, toks[t % nIn]) for t in toks]


# ---- the edge suite of the token and profile fills (test_prefix_edges_gpu.py; held to its liveness conditions without a GPU by
# test_prefix_host.py::test_edge_suite_inputs_are_live) -----------------------------------------------------------------------------
EDGE_L = 33
EDGE_ALPHABETS = [(1, 1), (1, 4), (3, 5), (5, 3)]
# (S, nIn, nOut, levels).  One live lane of 64 (S = 1, which has no silent level), 63/64/65 around a wavefront, 1024/1025 around
# the first state a lane meets on its second stride.  Up to 65 the whole cross product; from 1024 on, where the numpy yardstick
# takes seconds, every alphabet once and both settings of the levels twice.
EDGE_CASES = [(S, nIn, nOut, lv) for S in (1, 2, 63, 64, 65) for nIn, nOut in EDGE_ALPHABETS for lv in (True, False) if S > 1 or not lv]
EDGE_CASES += [(1024, 1, 4, True), (1024, 1, 4, False), (1025, 1, 1, True), (1025, 1, 4, False), (1025, 3, 5, True), (1025, 5, 3, False)]
WITNESS_CASES = [(65, 3, 5, True), (65, 3, 5, False), (65, 5, 3, True), (65, 5, 3, False)]


def edge_case(S, nIn, nOut, levels, L=EDGE_L):
    """(em, y): the machine and the output string of one case of EDGE_CASES (the profile of the same case: edge_profile)."""
    em = populated_machine(S, 100 + S, levels, nIn, nOut)
    return em, np.random.RandomState(S + L).randint(1, nOut + 1, size=L).astype(np.int32)


def machine_from_edges(S, nIn, nOut, edges):
    """EvaluatedMachine of (src, dst, inTok, outTok, logWeight) tuples; edges of one source keep their order."""
    edges = sorted(edges, key=lambda e: e[0])
    src = np.array([e[0] for e in edges], np.uint32); dst = np.array([e[1] for e in edges], np.uint32)
    it = np.array([e[2] for e in edges], np.uint16); ot = np.array([e[3] for e in edges], np.uint16)
    lw = np.array([e[4] for e in edges], np.float64)
    off = np.zeros(S + 1, np.int64)
    np.add.at(off, src.astype(np.int64) + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(len(edges)) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, Tokenizer([chr(65 + k) for k in range(nIn)]), Tokenizer([chr(97 + k) for k in range(nOut)]),
                            src, dst, it, ot, tidx, lw, off, [None] * S)


def machine_edges(em):
    return [(int(s), int(d), int(i), int(o), float(w)) for s, d, i, o, w in zip(em.src, em.dst, em.inTok, em.outTok, em.logWeight)]


def banded_R(S):
    """A stand-in for log((I - N)^-1) that costs no inversion: 0 on the diagonal, -1 one state on, -2 at (7 i + 3) mod S.  The
    kernels and the yardsticks take R as data, so the same matrix goes to both."""
    R = np.full((S, S), -np.inf)
    i = np.arange(S)
    R[i, (7 * i + 3) % S] = -2.0
    R[i, (i + 1) % S] = -1.0
    R[i, i] = 0.0
    return R


LDS_TOKEN_STATES = (8192, 8193)          # 64 KiB of doubles: the last machine below the opt-in for more dynamic LDS, the first above
LDS_L = 4


def lds_machine(S, nOut=2):
    """A machine for the LDS marks: no silent levels (they are deep at this size and are not what the marks are about), and on top of
    populated_machine an input-free emitting edge from the start state to the end state per output symbol, so that two rows
    already carry mass to the end."""
    em = populated_machine(S, S, False, 2, nOut)
    extra = [(0, S - 1, 0, o, float(np.log(0.3))) for o in range(1, nOut + 1)] + [(S - 1, S - 1, 0, o, float(np.log(0.3))) for o in range(1, nOut + 1)]
    return machine_from_edges(S, 2, nOut, machine_edges(em) + extra)


def lds_token_case(S):
    """(em, R, y) for the root and the child by symbol 1."""
    em = lds_machine(S)
    return em, banded_R(S), np.random.RandomState(S).randint(1, em.nOutTok + 1, size=LDS_L).astype(np.int32)


BATCH_LENGTHS = tuple(range(10))


def batch_case():
    """(em, [y of length 0..9]): S = 40, silent levels, nIn = 3, nOut = 5."""
    em = populated_machine(40, 7, True, 3, 5)
    return em, [np.random.RandomState(20 + L).randint(1, 6, size=L).astype(np.int32) for L in BATCH_LENGTHS]


COLUMN_STATE = 3          # the column of the V product that only far-down terms feed
COLUMN_FED = 4            # the state whose prefix cell in the next row is fed through that column alone


def far_column_case():
    """(em, R, y): five states, y = (a, b).  Row 1 of every node's prefix layer holds cells near 0 in the states 1 and 2; R (built by
    hand) lets them into column 3 at -850 and -900 only, next to diagonal terms near 0, and state 4 (the end state) is entered
    from state 3 alone, on b.  A linear product under the row's one maximum would lose V[1][3], then prefix[2][4], then the node's
    logPrefixProb, which reads nothing else."""
    lg = lambda x: float(np.log(x))
    edges = [(0, 1, 0, 1, lg(0.5)), (0, 2, 1, 1, lg(0.3)), (0, 1, 2, 1, lg(0.2)), (0, 0, 1, 0, lg(0.2)), (0, 0, 2, 0, lg(0.1)),
             (1, 1, 0, 2, lg(0.4)), (1, 2, 1, 2, lg(0.3)), (2, 1, 2, 2, lg(0.25)), (2, 2, 0, 1, lg(0.1)),
             (3, 4, 0, 2, lg(0.4)), (1, 3, 0, 0, lg(0.05))]
    R = np.full((5, 5), -np.inf)
    R[np.arange(5), np.arange(5)] = 0.0
    R[0, 0] = lg(1.0 / 0.7)
    R[1, 2] = -1.0
    R[1, 3], R[2, 3] = -850.0, -900.0
    return machine_from_edges(5, 2, 2, edges), R, np.array([1, 2], np.int32)


def twin_machine(S, seed, quantised=False):
    """Three input symbols of which 1 and 2 are twins: every edge that reads 1 is followed at once by the same edge reading 2, so
    the two have the same edges, weights and order; symbol 3 has edges of its own, a quarter as heavy.  Every output needs an input symbol (no
    input-free emitting edge), so a search has to choose among them.  A silent backbone gives levels.  ``quantised``: every weight
    is a multiple of log 0.5, so that different paths tie exactly."""
    rng = np.random.RandomState(seed)
    half = float(np.log(0.5))
    w = (lambda lo, hi: half * rng.randint(1, 4)) if quantised else (lambda lo, hi: float(np.log(rng.uniform(lo, hi))))
    weak = half * 2 if quantised else float(np.log(0.25))          # symbol 3 is the less likely reading of any output
    edges = []
    for s in range(S):
        for a in (1, 3):
            mine = [(s, rng.randint(0, S), a, o, w(0.1, 0.5) + (weak if a == 3 else 0.0)) for o in (1, 2)]
            mine.append((s, rng.randint(0, S), a, rng.randint(1, 3), w(0.1, 0.5) + (weak if a == 3 else 0.0)))
            if rng.rand() < 0.3:
                mine.append((s, rng.randint(0, S), a, 0, w(0.05, 0.2)))
            for e in mine:
                edges.append(e)
                if a == 1:
                    edges.append(e[:2] + (2,) + e[3:])
        if s + 1 < S:
            edges.append((s, s + 1, 0, 0, w(0.2, 0.4)))
    return machine_from_edges(S, 3, 2, edges)


def twin_outputs(em, n, L, seed):
    """n output strings of L symbols."""
    rng = np.random.RandomState(seed)
    return [[em.outputTokenizer.tok2sym[t] for t in rng.randint(1, em.nOutTok + 1, size=L)] for _ in range(n)]


def self_loop_case():
    """(em, y): a small levelled machine with a silent self-loop on the start state, the only place where the machine compiler
    lets one through.  The fills skip it."""
    em = populated_machine(8, 3, True, 3, 5)
    em = machine_from_edges(8, 3, 5, machine_edges(em) + [(0, 0, 0, 0, float(np.log(0.1)))])
    return em, np.random.RandomState(8).randint(1, 6, size=12).astype(np.int32)


TWIN_STATES, TWIN_SEED, TWIN_L, TWIN_SEARCHES = 5, 1, 3, 4
