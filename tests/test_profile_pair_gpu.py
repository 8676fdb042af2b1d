"""GPU tests of the two-tape profile sweeps (mb_profile_pair.hip through capi.DeviceProfilePairs, capi.profile_pair_fill and
`boss --recognize-csv` beside input data): every case compares the device against the numpy restatement profile.PairProfileDP.
Bounds (docs/profile_tapes.md): log values 1e-9 relative to max(1, |value|) with -inf matching exactly; counts >= 1e-3 at 1e-6
relative, smaller ones at 1e-9 + 1e-6 x count absolute; Viterbi scores at 1e-12, paths and rows equal.  Every case but the dead-input
ones asserts that half of the cells and nine in ten of the likelihoods it compares are finite
(test_profile_pair_host.py::test_pair_suite_inputs_are_live holds the same inputs to that on the CPU)."""
import io
import json
import math

import numpy as np
import pytest

import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, log_dev, logs_close, pair_input, pair_machine
from prefixhelpers import banded_R
from profileprefixhelpers import random_profile
from randmachine import random_machine
from machineboss_amd import boss, capi
from machineboss_amd.profile import PairProfileDP, ProfileDP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


WORST = ph.WORST
_note, _check_machine, _assert_live = ph.note, ph.check_machine, ph.assert_live      # (shared with test_profile_pair_edges_gpu.py)


@pytest.mark.parametrize("S,nIn,nOut", ph.SUITE_CASES)
def test_every_cell_against_restatement(S, nIn, nOut):
    """S = 65 crosses a wavefront; (0, L) and (I, 0) degenerate to one row or one column; (2, 7) and (7, 2) size the ring by the
    short side.  With silent levels and without (S >= 2)."""
    live = dict(ll=[], cells=0, all=0)
    cases = ph.suite_case(S, nIn, nOut)
    for em in list(dict.fromkeys(id(c[0]) for c in cases)):
        mine = [c for c in cases if id(c[0]) == em]
        _check_machine(mine[0][0], [(x, P) for _, x, P in mine], live=live)
    _assert_live(live)


def test_diagonal_wider_than_the_workgroup():
    """S = 40, I = L = 40: 41 x 40 items on the longest diagonal against 1 024 lanes, and a ring that wraps 27 times."""
    em, x, P = ph.wide_case()
    live = dict(ll=[], cells=0, all=0)
    _check_machine(em, [(x, P)], live=live)
    _assert_live(live)


@pytest.mark.parametrize("S", ph.LDS_STATES)
def test_ring_on_both_sides_of_the_lds_limits(S):
    """I = L = 3: a ring of 48 * 4 * S bytes.  853 / 854 states: the last ring in LDS and the first in global scratch; 341 / 342: the
    last under 64 KiB of dynamic LDS and the first for which the limit is raised.  (682 / 683 and 1 706 / 1 707 are those marks for a
    ring of 24 * 4 * S bytes, one layer: all four on the side of their neighbours here.)  Rolling Forward and Viterbi score."""
    em, x, P = ph.lds_case(S)
    dp = PairProfileDP(em)
    want, wv = dp.forward(x, P)[0], dp.forward(x, P, "max")[0]
    assert want > -math.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x], [P])
    try:
        got = dev.forward(capi.MB_ROLLING)
        _note("forward", got, [want])
        assert logs_close(got, [want]), (got, want)
        assert logs_close(dev.viterbi(paths=False)[0], [wv], 1e-12)
    finally:
        dev.close(); dm.close()


def _all(dev):
    return dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi()


def test_ragged_batch_is_bit_identical_to_single_pairs():
    em, pairs = ph.ragged_case()
    live = dict(ll=[], cells=0, all=0)
    _check_machine(em, pairs, fill=False, live=live)
    _assert_live(live)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        r0, m0, (v0, o0, e0, w0) = _all(dev)
        r1, m1, (v1, o1, e1, w1) = _all(dev)
        assert np.array_equal(r0, r1) and np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(e0, e1) and np.array_equal(w0, w1)
        for k, (x, P) in enumerate(pairs):
            one = capi.DeviceProfilePairs(dm, [x], [P])
            r, m, (v, o, e, w) = _all(one)
            one.close()
            assert r[0] == r0[k] and m[0] == m0[k] and v[0] == v0[k], k
            assert np.array_equal(e, e0[o0[k]:o0[k + 1]]) and np.array_equal(w, w0[o0[k]:o0[k + 1]]), k
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            c1 = dev.counts()[0]; c2 = dev.counts()[0]
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        assert np.array_equal(c1, c2) and c1.any()
        assert counts_close(c1, dev.counts()[0]) or np.allclose(c1, dev.counts()[0], rtol=1e-6, atol=1e-9)     # fixed point at 2^-36
    finally:
        dev.close(); dm.close()


def test_chunking():
    em, pairs = ph.chunk_case()
    S, n, I, L = ph.CHUNK_SHAPE
    dp = PairProfileDP(em)
    want = np.array([dp.forward(x, P)[0] for x, P in pairs[:4]])
    assert (want > -math.inf).all()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        f0, (v0, o0, e0, r0), c0 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()[0]
        assert logs_close(f0[:4], want)
        capi.set_memory_budget((n // 3) * (I + 1) * (L + 1) * 2 * S * 8 + 4096)       # a third of the lattices: three chunks or more
        try:
            f1, (v1, o1, e1, r1), c1 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()[0]
            assert capi.last_launch_count() >= 3
        finally:
            capi.set_memory_budget(0)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1) and np.array_equal(o0, o1) and np.array_equal(e0, e1) and np.array_equal(r0, r1)
        assert counts_close(c1, c0)
    finally:
        dev.close(); dm.close()


def test_no_input_equals_device_profiles():
    em = random_machine(40, 0, 3, 31)
    profs = [random_profile(np.random.RandomState(31 + L), L, 3) for L in (0, 1, 9, 23)]
    dm = capi.DeviceMachine(em)
    a = capi.DeviceProfilePairs(dm, [[] for _ in profs], profs)
    b = capi.DeviceProfiles(dm, profs)
    try:
        want = b.forward()
        assert (want > -math.inf).mean() >= 0.9
        assert logs_close(a.forward(), want, 1e-12) and logs_close(a.forward(capi.MB_MATERIALISE), want, 1e-12)
        va, oa, ea, ra = a.viterbi(); vb, ob, eb, rb = b.viterbi()
        assert logs_close(va, vb, 1e-12) and np.array_equal(oa, ob) and np.array_equal(ea, eb) and np.array_equal(ra, rb)
        assert np.allclose(a.counts()[0], b.counts()[0], rtol=1e-9, atol=1e-12)
    finally:
        a.close(); b.close(); dm.close()


def test_likelihood_equals_chained_prefix_fills():
    """logSeqProb of I chained k_prefix_fill_profile fills (layer 0 of the node of x) is the Forward likelihood of (x, profile)."""
    em, pairs = ph.chained_case()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    px = capi.DevicePrefix(dm, None, banded_R(em.nStates), 8 * len(pairs), profiles=[P for _, P in pairs])
    try:
        got = dev.forward()
        want = []
        for k, (x, P) in enumerate(pairs):
            node, sp, _ = px.root(k)
            for a in x:
                nodes, sps, _ = px.extend([k], [node], [int(a)])
                node, sp = int(nodes[0]), float(sps[0])
            want.append(sp)
        assert (np.array(want) > -math.inf).mean() >= 0.9
        _note("forward against chained fills", got, want)
        assert logs_close(got, want), (got, want)
    finally:
        px.close(); dev.close(); dm.close()


def test_dead_inputs():
    em = pair_machine(40, 5, True, 2, 3)
    dp = PairProfileDP(em)
    rng = np.random.RandomState(5)
    x, P = pair_input(rng, em, 6, 8, pZero=0.0)
    dead = P.copy(); dead[3] = -np.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x, x], [dead, P])
    try:
        assert dp.forward(x, dead)[0] == -math.inf
        for ll in (dev.forward(), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]):
            assert ll[0] == -math.inf and ll[1] > -math.inf
        v, off, edges, rows = dev.viterbi()
        assert v[0] == -math.inf and off[0] == off[1] == 0 and off[2] > 0
        one = capi.DeviceProfilePairs(dm, [x], [dead])
        c, s, ll = one.counts()
        one.close()
        assert not c.any() and ll[0] == -math.inf
        c2 = dev.counts()[0]
        assert counts_close(c2, dp.counts(x, P)[0])            # the dead pair adds nothing
    finally:
        dev.close()
    # a third of the weights -inf
    em2, pairs = ph.sparse_case()
    _check_machine(em2, pairs)
    dm.close()
    # an x the machine cannot read: only symbol 1 has edges; symbol 2 is in the alphabet and leads nowhere
    from prefixhelpers import machine_edges, machine_from_edges
    em3 = pair_machine(8, 3, True, 1, 2)
    em3 = machine_from_edges(8, 2, 2, machine_edges(em3))
    dm3 = capi.DeviceMachine(em3)
    P3 = random_profile(np.random.RandomState(3), 4, 2, pZero=0.0)
    dev = capi.DeviceProfilePairs(dm3, [[1, 2, 1], [1, 1, 1]], [P3, P3])
    try:
        ll = dev.forward()
        assert ll[0] == -math.inf and logs_close(ll, [PairProfileDP(em3).forward(x_, P3)[0] for x_ in ([1, 2, 1], [1, 1, 1])]) and ll[1] > -math.inf
        assert dev.viterbi()[0][0] == -math.inf
    finally:
        dev.close(); dm3.close()


def test_errors():
    em = pair_machine(8, 1, True, 2, 3)
    dm = capi.DeviceMachine(em)
    P = random_profile(np.random.RandomState(1), 5, 3)

    def works():
        dev = capi.DeviceProfilePairs(dm, [[1, 2]], [P])
        ll = dev.forward()
        dev.close()
        assert ll[0] > -math.inf and logs_close(ll, [PairProfileDP(em).forward([1, 2], P)[0]])
    for bad in ([0], [3], [1, 2, 3]):
        with pytest.raises(capi.MbError, match="outside 1..nInTok"):
            capi.DeviceProfilePairs(dm, [bad], [P])
        works()
    with pytest.raises(capi.MbError, match="outside 1..nInTok"):
        capi.profile_pair_fill(dm, capi.MB_FORWARD, [3], P)
    nan = P.copy(); nan[2, 1] = np.nan
    with pytest.raises(capi.MbError, match="NaN"):
        capi.DeviceProfilePairs(dm, [[1]], [nan])
    works()
    inf = P.copy(); inf[0, 0] = np.inf
    with pytest.raises(capi.MbError, match="infinity"):
        capi.DeviceProfilePairs(dm, [[1]], [inf])
    works()
    dev = capi.DeviceProfilePairs(dm, [[1, 2], [2]], [P, P])
    with pytest.raises(capi.MbError, match="pathCap too small"):
        dev.viterbi(cap=dev.path_cap() - 1)
    v, off, edges, rows = dev.viterbi()
    assert (v > -math.inf).all() and off[-1] == len(edges)
    dev.close()
    capi.set_memory_budget(1024)
    try:
        dev = capi.DeviceProfilePairs(dm, [[1, 2]], [P])
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.forward(capi.MB_MATERIALISE)
        dev.close()
    finally:
        capi.set_memory_budget(0)
    works()
    dm.close()
    gen = random_machine(8, 0, 2, 41)                      # a generator: any input token is outside its (empty) alphabet
    dg = capi.DeviceMachine(gen)
    with pytest.raises(capi.MbError, match="outside 1..nInTok"):
        capi.DeviceProfilePairs(dg, [[1]], [random_profile(np.random.RandomState(2), 3, 2)])
    ok = capi.DeviceProfilePairs(dg, [[]], [random_profile(np.random.RandomState(2), 3, 2)])
    assert ok.forward().shape == (1,)
    ok.close(); dg.close()


def _boss(*args):
    """boss.run in this process (the device is open already; a child process per call would cost seconds each)."""
    out = io.StringIO()
    assert boss.run(list(args), out) == 0
    return json.loads(out.getvalue())


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return abs(a - b) <= 1e-9 * max(1.0, abs(b))
    return a == b


def test_cli_on_the_device(tmp_path):
    """`dnastore4 --use-defaults --input-chars <x> --recognize-csv tiny_uc.csv` with -L, -V and -C: the device's output is the numpy
    backend's.  dnastore4's input symbols have three characters, so --input-chars spells the empty sequence; --input-json gives it
    a sequence to read, and bitnoise (one-character symbols, parameters) one through --input-chars."""
    (tmp_path / "x.json").write_text(json.dumps({"name": "x1", "sequence": ["0_3", "2_3", "1_3"]}))
    base = ["tests/golden/machine/dnastore4.json", "--use-defaults", "--recognize-csv", "tests/golden/csv/tiny_uc.csv"]
    bit = ["tests/golden/machine/bitnoise.json", "-P", "tests/golden/io/params.json", "--recognize-csv", "tests/golden/csv/prof001.csv"]
    for args in (base + ["--input-chars", ""], base + ["--input-chars", "", "--input-json", str(tmp_path / "x.json")], bit + ["--input-chars", "101"]):
        for flag in ("-L", "-V", "-C"):
            got, want = _boss(*args, flag), _boss(*args, flag, "--decode-backend", "numpy")
            assert _same(got, want), (args, flag, got, want)
            if flag != "-C":
                assert all(isinstance(g[2], float) for g in got), got
