"""GPU tests of what the token batch Viterbi asks of ``pathCap`` (mb_api.hip: mb_batch_viterbi and the path tail its routes share).
The Python wrapper always passes the sum of the path bounds, so the C function is called directly here with a cap of the test's own,
as tests/test_profile_pathcap_gpu.py does for the profile families.

No route checks the cap up front: it has to hold the paths themselves, chunk by chunk.  With the cap equal to the sum of the true
path lengths the call succeeds; one entry less fails with "pathCap too small for the Viterbi paths of this batch" in the chunk whose
paths no longer fit, the offsets of the chunks before it written and the later ones untouched.  A pair without a finite path (its
output holds a symbol no transition emits) scores -inf and has an empty path.  All routes behave alike here: the generic fp64
walker (set_kernel 1), the small family (2), the tiled family's traceback bytes (3) and, on the one-tape machine, the default's
traceback codes.

Both machines have four states and weights that are powers of 1/2 with parallel edges, so Viterbi candidates tie; the expected
scores and paths come from the CPU oracle (oracle/mb_oracle.c: the fill and DPMatrix::traceBack with selectMaxTrans, the rule
machineboss_amd/dp.py restates -- dp.py's own matrices are filled on the device, so they are not the reference here).

Every budget is worked out from the cell counts so that no two pairs share a chunk (five chunks); the same calls under a budget
of 1 GiB run in one chunk and return the same."""
import ctypes as C
import math

import numpy as np
import pytest

from machineboss_amd import capi
from machineboss_amd.evalmachine import EvaluatedMachine, Tokenizer
from oracle import oracle

pytestmark = pytest.mark.gpu

S = 4
H = math.log(0.5)
Q = math.log(0.25)
# (src, dst, inTok, outTok, log weight); output token 3 is in the alphabet and on no transition
TWO_TAPE = [(0, 1, 0, 0, 0.0), (0, 2, 0, 0, H),
            (1, 1, 1, 1, H), (1, 1, 1, 1, H), (1, 2, 2, 0, H), (1, 1, 0, 2, H), (1, 2, 1, 2, Q), (1, 3, 0, 0, H),
            (2, 1, 1, 2, H), (2, 2, 0, 1, Q), (2, 2, 2, 1, H), (2, 1, 2, 0, Q), (2, 2, 1, 0, Q), (2, 3, 0, 0, H)]
ONE_TAPE = [(0, 1, 0, 0, 0.0), (0, 2, 0, 0, H),
            (1, 1, 0, 1, H), (1, 1, 0, 1, H), (1, 2, 0, 2, H), (1, 2, 0, 1, Q), (1, 3, 0, 0, H),
            (2, 1, 0, 2, H), (2, 2, 0, 1, Q), (2, 1, 0, 1, Q), (2, 3, 0, 0, H)]
N_PAIRS, PATHLESS = 5, 2
BIG = 1 << 30
SENTINEL = -7
CAP_ERROR = "pathCap too small for the Viterbi paths of this batch"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    capi.set_option("MB_WIDE_MIN_STATES", "1")      # the four-state one-tape machine goes to the one-tape family
    yield
    capi.set_option("MB_WIDE_MIN_STATES", None)
    capi.set_kernel(0)
    capi.set_memory_budget(0)


def _machine(edges, nIn, nOut):
    edges = sorted(edges, key=lambda e: e[0])
    src = np.array([e[0] for e in edges], np.uint32); dst = np.array([e[1] for e in edges], np.uint32)
    it = np.array([e[2] for e in edges], np.uint16); ot = np.array([e[3] for e in edges], np.uint16)
    lw = np.array([e[4] for e in edges], np.float64)
    off = np.zeros(S + 1, np.int64)
    for s in src:
        off[s + 1] += 1
    off = np.cumsum(off)
    tidx = (np.arange(len(edges)) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, Tokenizer([chr(65 + k) for k in range(nIn)]), Tokenizer([chr(97 + k) for k in range(nOut)]),
                            src, dst, it, ot, tidx, lw, off, [None] * S)


def _case(tape):
    """(machine, pairs): sequences of 4..6 tokens, so that the lattices of any two pairs outgrow the largest one."""
    two = tape == "two"
    em = _machine(TWO_TAPE if two else ONE_TAPE, 2 if two else 0, 3)
    rng = np.random.RandomState(5 if two else 6)
    pairs = []
    for k in range(N_PAIRS):
        x = rng.randint(1, 3, size=rng.randint(4, 7)).astype(np.int32) if two else np.zeros(0, np.int32)
        y = rng.randint(1, 3, size=rng.randint(4, 7)).astype(np.int32)
        if k == PATHLESS:
            y[len(y) // 2] = 3
        pairs.append((x, y))
    return em, pairs


_REF = {}


def _reference(tape):
    """The oracle's scores and paths of the case, computed once."""
    if tape not in _REF:
        em, pairs = _case(tape)
        oracle.build()
        om = oracle.OracleMachine(em)
        lls, paths = [], []
        for x, y in pairs:
            V = om.viterbi(x, y)
            lls.append(float(V[-1, -1, -1]))
            paths.append(om.traceback(x, y, V) if lls[-1] > -np.inf else np.zeros(0, np.uint32))
        _REF[tape] = (em, pairs, np.array(lls), paths)
    return _REF[tape]


def _cells(pairs):
    return [(len(x) + 1) * (len(y) + 1) * S for x, y in pairs]


def _budget(route, pairs):
    """Bytes that hold the largest pair of the batch and no two pairs, by the planner of the route (mb_api.hip)."""
    cells = _cells(pairs)
    if route == "small":
        # small_chunks_plan: traceback bytes (one strip of even(outLen + 65) steps x 64 lanes x 4) + 16, a halo row of at most S doubles
        # per output position, a boundary record of at most 2 S doubles for each of 64 lanes
        tb = [((len(y) + 65) & ~1) * 64 * 4 + 16 for _, y in pairs]
        lo, hi = min(tb), max(tb) + max(len(y) + 1 for _, y in pairs) * S * 8 + 64 * 2 * S * 8
    else:
        # plan_chunks: 8 bytes per cell of the fp64 matrix; traceback bytes (tiled: 16 per supercell of four states) and traceback
        # codes (one-tape: 4 per column) are planned at stride / S + 0.01 bytes per cell
        per = {"fp64": 8.0, "bytes": 16 / S + 0.01, "codes": 4 / S + 0.01}[route]
        lo, hi = int(min(cells) * per), int(math.ceil(max(cells) * per))
        assert int(hi / per) >= max(cells)
    assert hi < 2 * lo, (lo, hi)
    return hi


def _call(b, cap):
    """mb_batch_viterbi on buffers of ``cap`` entries and a pre-filled offset array: (rc, error, loglike, off, edges)."""
    L = capi.load()
    ll = np.full(b.nPairs, np.nan, np.float64)
    off = np.full(b.nPairs + 1, SENTINEL, np.int64)
    edges = np.zeros(max(cap, 1), np.uint32)
    rc = L.mb_batch_viterbi(b.h, ll.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)),
                            edges.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
    return rc, L.mb_last_error().decode() if rc else "", ll, off, edges


ROUTES = [("two", 1, "fp64", "k_generic_fill_fwd<1>"), ("two", 2, "small", "k_small_tb"), ("two", 3, "bytes", "k_medium_jit"),
          ("one", 0, "codes", "codes"), ("one", 1, "fp64", "k_generic_fill_fwd<1>")]


def test_the_cases_have_ties_and_one_pathless_pair():
    for tape in ("two", "one"):
        em, pairs, lls, paths = _reference(tape)
        assert [v > -np.inf for v in lls] == [k != PATHLESS for k in range(N_PAIRS)]
        assert all(len(p) > 0 for k, p in enumerate(paths) if k != PATHLESS) and len(paths[PATHLESS]) == 0
        assert all(max(len(x), len(y)) <= 6 for x, y in pairs)
        dup = int(np.flatnonzero((em.src == 1) & (em.dst == 1) & (em.outTok == 1))[0])      # the first of two parallel edges of equal weight
        assert any(dup in p for p in paths), "no path takes the tied parallel edges"


@pytest.mark.parametrize("tape,kernel,route,name", ROUTES, ids=["%s-kernel%d" % (r[0], r[1]) for r in ROUTES])
def test_cap_holds_the_paths_chunk_by_chunk(tape, kernel, route, name):
    em, pairs, lls, paths = _reference(tape)
    lens = [len(p) for p in paths]
    want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(want_off[-1])
    want_edges = np.concatenate(paths).astype(np.uint32)
    dm = capi.DeviceMachine(em)
    b = capi.DeviceBatch.from_pairs(dm, pairs)
    capi.set_kernel(kernel)
    try:
        assert total < sum(dm.path_bound(len(x), len(y)) for x, y in pairs)
        # the failing chunk of a cap one short of the total is the last one that has a path: one chunk per pair, so the last pair's
        last = max(k for k in range(N_PAIRS) if lens[k])
        for budget, written in ((_budget(route, pairs), last), (BIG, 0)):
            capi.set_memory_budget(budget)
            rc, err, ll, off, edges = _call(b, total)
            assert rc == 0, err
            k = capi.last_kernel_name()
            print("%s machine, set_kernel(%d), budget %d: %s" % (tape, kernel, budget, k))
            assert (name in k) if route == "codes" else (k == name), k
            assert np.array_equal(ll, lls), (ll, lls)                           # the max semiring is exact; the pathless pair: -inf
            assert np.array_equal(off, want_off) and off[PATHLESS + 1] == off[PATHLESS]
            assert np.array_equal(edges[:total], want_edges)
            rc, err, ll, off, edges = _call(b, total - 1)
            assert rc != 0 and err == CAP_ERROR, (rc, err)
            assert np.array_equal(off[:written + 1], want_off[:written + 1]), (off, want_off)
            assert np.all(off[written + 1:] == SENTINEL), off
            assert np.array_equal(edges[:want_off[written]], want_edges[:want_off[written]])
    finally:
        capi.set_kernel(0)
        capi.set_memory_budget(0)
        b.close(); dm.close()


@pytest.mark.parametrize("tape,kernel,route,name", ROUTES, ids=["%s-kernel%d" % (r[0], r[1]) for r in ROUTES])
def test_scores_without_paths_need_no_cap(tape, kernel, route, name):
    """pathOff / pathEdges null: the scores alone, chunked or not (the traceback bytes and codes are kept for paths only on the
    one-tape machine: its score-only call takes the fp64 sweep)."""
    em, pairs, lls, _ = _reference(tape)
    dm = capi.DeviceMachine(em)
    b = capi.DeviceBatch.from_pairs(dm, pairs)
    capi.set_kernel(kernel)
    try:
        for budget in (_budget("fp64" if route == "codes" else route, pairs), BIG):
            capi.set_memory_budget(budget)
            ll, off, edges = b.viterbi(paths=False)
            assert off is None and edges is None and np.array_equal(ll, lls), (ll, lls)
    finally:
        capi.set_kernel(0)
        capi.set_memory_budget(0)
        b.close(); dm.close()
