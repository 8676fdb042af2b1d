"""GPU tests of what the three profile families ask of ``pathCap`` (mb_profile_api.hip: mb_profiles_viterbi, mb_profile_pairs_viterbi,
mb_profile_twos_viterbi, unpack_paths).  The Python wrappers always pass the sum of the path bounds, so the C functions are called
directly here with a cap of the test's own.

One-tape profiles, plain and CTC-merged, have no check up front: the cap has to hold the paths themselves, and a call whose cap is
below the bound sum but not below the real total succeeds.  One entry less fails with the plain "pathCap too small" while the
paths are copied, the earlier items' paths and offsets already written.  Pairs and two-profile pairs refuse up front any cap below
the sum of the path bounds, and say so.

The machine is a chain of three states (silent 0 -> 1 -> 2, emitting 2 -> 0); each profile has a dead row that only its blank
passes, so every Viterbi path is finite and shorter than its bound: both are checked against the restatement on the CPU."""
import ctypes as C

import numpy as np
import pytest

import pairprofilehelpers as ph
from machineboss_amd import capi
from machineboss_amd.profile import MergedProfileDP, PairProfileDP, ProfileDP, TwoProfileDP

pytestmark = pytest.mark.gpu

S, N_IN, N_OUT = 3, 2, 3
ROWS = (2, 3)          # rows of the two profiles; the pair families' inputs have as many tokens (rows)
COL_TOK = (1, 3, 1)    # merged profiles: three CSV columns on two tokens


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)


def _rows(rng, n, width):
    """n rows of ``width`` + 1 log weights that must emit (blank -inf), but row 1: dead, only its blank passes."""
    P = np.log(rng.uniform(0.05, 1.0, (n, width + 1)))
    P[:, 0] = -np.inf
    P[1, :] = -np.inf
    P[1, 0] = 0.0
    return P


def _call(fn, handle, n, cap, third=False):
    """fn(handle, loglike, pathOff, pathEdges, pathRow[, pathInRow], cap) on buffers of ``cap`` entries: (rc, error, off, arrays)."""
    ll = np.empty(n, np.float64)
    off = np.full(n + 1, -7, np.int64)
    arrays = [np.zeros(max(cap, 1), np.uint32)] + [np.zeros(max(cap, 1), np.int32) for _ in range(2 if third else 1)]
    ptrs = [a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_int32)) for a in arrays]
    rc = fn(handle, ll.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)), *ptrs, cap)
    return rc, capi.load().mb_last_error().decode() if rc else "", off, arrays


@pytest.mark.parametrize("merged", [False, True], ids=["plain", "merged"])
def test_one_tape_cap_holds_the_paths_not_the_bounds(merged):
    em = ph.chain_machine(S, nIn=0, nOut=N_OUT)
    rng = np.random.RandomState(11 + merged)
    profs = [_rows(rng, n, len(COL_TOK) if merged else N_OUT) for n in ROWS]
    dp = MergedProfileDP(em, COL_TOK) if merged else ProfileDP(em)
    want = [dp.viterbi(P) for P in profs]
    lens = [len(e) for _, e, _ in want]
    assert all(v > -np.inf for v, _, _ in want) and all(lens)
    L = capi.load()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs, colTok=COL_TOK if merged else None)
    try:
        boundSum = sum(L.mb_profile_path_bound(dm.h, n) for n in ROWS)
        total = sum(lens)
        assert total < boundSum, (total, boundSum)
        _, off, edges, rows = dev.viterbi()                      # the wrapper: the full cap
        assert list(off) == [0, lens[0], total]
        assert np.array_equal(edges, np.concatenate([e for _, e, _ in want])) and np.array_equal(rows, np.concatenate([r for _, _, r in want]))
        rc, err, off1, (e1, r1) = _call(L.mb_profiles_viterbi, dev.h, 2, total)
        assert rc == 0, err
        assert np.array_equal(off1, off) and np.array_equal(e1[:total], edges) and np.array_equal(r1[:total], rows)
        rc, err, off2, (e2, r2) = _call(L.mb_profiles_viterbi, dev.h, 2, total - 1)
        assert rc != 0 and err == "pathCap too small for the Viterbi paths", err
        assert off2[0] == 0 and off2[1] == lens[0]
        assert np.array_equal(e2[:lens[0]], edges[:lens[0]]) and np.array_equal(r2[:lens[0]], rows[:lens[0]])
    finally:
        dev.close(); dm.close()


def _refused_below_the_bound_sum(fn, dev, dm, shapes, third):
    L = capi.load()
    boundSum = sum(L.mb_profile_pair_path_bound(dm.h, i, r) for i, r in shapes)
    assert boundSum == dev.path_cap() and boundSum > 0
    rc, err, _, _ = _call(fn, dev.h, len(shapes), boundSum - 1, third)
    assert rc != 0 and err.startswith("pathCap too small for the Viterbi paths: %d entries" % (boundSum - 1)), err
    assert err.endswith("the path bounds of the pairs sum to %d" % boundSum), err
    rc, err, off, arrays = _call(fn, dev.h, len(shapes), boundSum, third)
    assert rc == 0, err
    return boundSum, off, arrays


def test_pairs_refuse_a_cap_below_the_bound_sum():
    em = ph.chain_machine(S, nIn=N_IN, nOut=N_OUT)
    rng = np.random.RandomState(21)
    pairs = [(rng.randint(1, N_IN + 1, size=n).astype(np.int32), _rows(rng, n, N_OUT)) for n in ROWS]
    dp = PairProfileDP(em)
    want = [dp.viterbi(x, P) for x, P in pairs]
    assert all(v > -np.inf and len(e) for v, e, _ in want)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        boundSum, off, (edges, rows) = _refused_below_the_bound_sum(capi.load().mb_profile_pairs_viterbi, dev, dm, [(n, n) for n in ROWS], False)
        total = sum(len(e) for _, e, _ in want)
        assert total < boundSum and list(off) == [0, len(want[0][1]), total]
        assert np.array_equal(edges[:total], np.concatenate([e for _, e, _ in want])) and np.array_equal(rows[:total], np.concatenate([r for _, _, r in want]))
    finally:
        dev.close(); dm.close()


def test_twos_refuse_a_cap_below_the_bound_sum():
    em = ph.chain_machine(S, nIn=N_IN, nOut=N_OUT)
    rng = np.random.RandomState(31)
    pairs = [(_rows(rng, n, N_IN), _rows(rng, n, N_OUT)) for n in ROWS]
    dp = TwoProfileDP(em)
    want = [dp.viterbi(A, B) for A, B in pairs]
    assert all(w[0] > -np.inf and len(w[1]) for w in want)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs])
    try:
        boundSum, off, (edges, rows, ins) = _refused_below_the_bound_sum(capi.load().mb_profile_twos_viterbi, dev, dm, [(n, n) for n in ROWS], True)
        total = sum(len(w[1]) for w in want)
        assert total < boundSum and list(off) == [0, len(want[0][1]), total]
        for got, j in ((edges, 1), (rows, 2), (ins, 3)):
            assert np.array_equal(got[:total], np.concatenate([w[j] for w in want]))
    finally:
        dev.close(); dm.close()
