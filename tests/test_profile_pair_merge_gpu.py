"""GPU tests of the two-tape merged (CTC) profile sweeps (mb_profile_pair_merge.hip) against profile.PairMergedProfileDP under the
bounds of test_profile_pair_gpu.py (pairprofilehelpers: log values 1e-9 relative to max(1, |value|) with -inf exact; counts >= 1e-3
at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x count absolute; Viterbi scores and cells at 1e-12, paths and rows equal).  The
builders are pairmergehelpers'; test_profile_pair_merge_host.py::test_edge_suite_inputs_are_live holds them to the conditions
asserted here on the CPU."""
import math

import numpy as np
import pytest

import pairmergehelpers as pm
from pairprofilehelpers import counts_close, logs_close, note, note_counts
from machineboss_amd import algebra, boss, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine
from machineboss_amd.profile import PairMergedProfileDP, Profile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    print("worst deviations:", pm.WORST)


def _pairs(dm, pairs, colTok):
    return capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs], colTok)


# ---- 1. lane grouping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", pm.LANE_CASES)
def test_lane_grouping(nCols, S):
    """(planes, states) from one item per diagonal to more items than lanes, at lattices from (0, 0) to (9, 9), with silent levels and
    without: everything the device computes, in one batch per machine."""
    live = []
    for em, colTok, pairs in pm.lane_case(nCols, S):
        pm.check_machine(em, colTok, pairs, live=live)
    assert np.mean(live) >= 0.9


# ---- 2. where the ring lives ----------------------------------------------------------------------------------------------------------
def _rolling(dev):
    return dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]


@pytest.fixture(scope="module")
def ragged():
    em, colTok, pairs = pm.ragged_case()
    dp = PairMergedProfileDP(em, colTok)
    return em, colTok, pairs, np.array([dp.forward(x, P)[0] for x, P in pairs]), np.array([dp.forward(x, P, "max")[0] for x, P in pairs])


def test_ragged_launch_of_lds_and_scratch_rings(ragged):
    """nCols = 4, S = 40: a ring of 336 (min(I, L) + 1) S bytes.  (3, 30) below 64 KiB, (4, 30) above it, (11, 30) the last in LDS,
    (12, 30) in global scratch found by i, (30, 12) by r; beside (2, 3), (0, 40), (40, 0) and a dead pair, in one launch.  Rolling
    has the bits of materialised; a second call, every pair alone on the workspace the batch left behind, and the batch cut into
    chunks under a lowered budget return the same bits."""
    em, colTok, pairs, want, wv = ragged
    assert (want[:-1] > -math.inf).all() and want[-1] == -math.inf
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    try:
        f0, v0 = _rolling(dev)
        note("forward", f0, want, pm.WORST)
        assert logs_close(f0, want), (f0, want)
        assert logs_close(v0, wv, 1e-12), (v0, wv)
        assert capi.last_launch_count() == 1
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), f0)
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        order = sorted(range(len(pairs)), key=lambda k: -pm.ring_bytes(pm.RING_S, 4, len(pairs[k][0]), len(pairs[k][1])))
        for k in order:
            one = _pairs(dm, pairs[k:k + 1], colTok)
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
        capi.set_memory_budget(pm.RAGGED_BUDGET)
        try:
            f2 = dev.forward(capi.MB_ROLLING)
            n2 = capi.last_launch_count()
            v2 = dev.viterbi(paths=False)[0]
        finally:
            capi.set_memory_budget(0)
        assert n2 >= 2 and np.array_equal(f0, f2) and np.array_equal(v0, v2), (n2, f0, f2)
    finally:
        dev.close(); dm.close()


def test_chunked_lattices_return_the_bits_of_unchunked():
    """nCols = 4, S = 65 at the seven lattices up to (9, 9): materialised Forward, Viterbi with paths and counts under budgets of 1.2
    times what the largest pair needs on its own -- its lattice (twice for the counts) and its path slot; the X ring of 62 400 bytes
    is in LDS -- which the seven pairs together pass: two chunks or more each.  Likelihoods, scores, paths and rows are the bits of
    the unchunked calls; the counts too under MB_DETERMINISTIC=1 (fixed point: the chunks' sums add exactly)."""
    em, colTok, pairs = pm.lane_case(4, 65)[0]
    assert pm.ring_bytes(65, 4, 9, 9, mat=True) <= pm.LDS_MAX
    lattice = [8 * (len(x) + 1) * (len(P) + 1) * 2 * 5 * 65 for x, P in pairs]
    assert sum(lattice) > 1.2 * max(lattice) + 8 * 4096
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        f0, v0, c0 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()
        assert capi.last_launch_count() == 1 and (f0 > -math.inf).sum() >= 6 and c0[0].any()
        capi.set_memory_budget(int(1.2 * max(lattice)) + 8 * 4096)
        f1 = dev.forward(capi.MB_MATERIALISE); nf = capi.last_launch_count()
        v1 = dev.viterbi(); nv = capi.last_launch_count()
        capi.set_memory_budget(int(2.4 * max(lattice)))
        c1 = dev.counts(); nc = capi.last_launch_count()
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()
    assert min(nf, nv, nc) >= 2, (nf, nv, nc)
    assert np.array_equal(f0, f1) and all(np.array_equal(a, b) for a, b in zip(v0, v1))
    assert np.array_equal(c0[0], c1[0]) and np.array_equal(c0[2], c1[2]) and c0[1] == c1[1]


def test_ragged_launch_everything(ragged):
    """The ragged batch through every entry point (paths, counts, the lattices of the two scratch-ring pairs)."""
    em, colTok, pairs, _, _ = ragged
    pm.check_machine(em, colTok, pairs, fill=False)
    pm.check_machine(em, colTok, pairs[3:5])


def test_many_scratch_rings_packed_in_one_launch():
    """Twenty-four workgroups, each with a ring of its own in the scratch buffer: several per die, so that rings which overlapped
    would meet in one cache.  Against the restatement, and every third pair alone returns the bits it had in the batch."""
    em, colTok, pairs = pm.packed_case()
    dp = PairMergedProfileDP(em, colTok)
    want = np.array([dp.forward(x, P)[0] for x, P in pairs])
    assert np.mean(want > -math.inf) >= 0.9
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    try:
        f0, v0 = _rolling(dev)
        assert capi.last_launch_count() == 1
        note("forward", f0, want, pm.WORST)
        assert logs_close(f0, want), (f0, want)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), f0)
        for k in range(0, len(pairs), 3):
            one = _pairs(dm, pairs[k:k + 1], colTok)
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], k
    finally:
        dev.close(); dm.close()


# ---- 3. counts ------------------------------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table():
    """11 204 transitions: beyond 8 192 every posterior goes into the global table with an atomic of its own.  With
    MB_DETERMINISTIC=1 the adds are 64-bit fixed point at 2^-36, each rounded to the nearest; a transition receives at most
    nCols + 1 = 3 adds per cell, 44 cells in all: 132 x 2^-37 = 9.6e-10, under the 1e-9 floor of counts_close.  A dead pair adds
    nothing in either mode, and the fixed point returns the same bits twice."""
    em, colTok, pairs, dead = pm.big_counts_case()
    dp = PairMergedProfileDP(em, colTok)
    refs = [dp.counts(x, P) for x, P in pairs]
    wc, want = np.sum([r[0] for r in refs], axis=0), np.array([r[1] for r in refs])
    assert em.nTransitions > 8192 and (want > -math.inf).all()
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    both = _pairs(dm, pairs[:1] + [dead] + pairs[1:], colTok)
    try:
        c, s, ll = dev.counts()
        note_counts(c, wc, pm.WORST)
        assert counts_close(c, wc) and logs_close(ll, want)
        c, s, ll = both.counts()
        assert counts_close(c, wc) and ll[1] == -math.inf and s == -math.inf and logs_close(np.delete(ll, 1), want)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            d1 = dev.counts(); d2 = dev.counts(); d3 = both.counts()
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        note_counts(d1[0], wc, pm.WORST, "fixed-point counts")
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and counts_close(d1[0], wc) and np.array_equal(d3[0], d1[0])
    finally:
        both.close(); dev.close(); dm.close()


def test_counts_same_bits_twice_through_the_lds_table():
    em, colTok, pairs = pm.lane_case(4, 13)[0]
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        a, b = dev.counts(), dev.counts()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()
    assert em.nTransitions <= 8192 and a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------------
def test_ties_are_decided_by_candidate_order():
    """The doubled tie machine against sixteen quantised pairs in one batch: every sum is exact, so equal candidates are equal on the
    device too; the census of what is compared holds every kind of tie, so equal paths mean the device took the first candidate."""
    em = pm.merged_tie_machine()
    dp = PairMergedProfileDP(em, pm.TIE_COLTOK)
    pairs, census = pm.tie_pairs(), {}
    refs = [dp.viterbi(x, P, census) for x, P in pairs]
    assert len(pairs) == 16 and all(census.get(k, 0) >= 1 for k in pm.TIE_KINDS), census
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, pm.TIE_COLTOK)
    try:
        v, off, edges, rows = dev.viterbi()
        assert np.array_equal(dev.viterbi(paths=False)[0], v)
        for k, ((x, P), (wv, we, wr)) in enumerate(zip(pairs, refs)):
            assert wv > -math.inf and v[k] == wv, (k, v[k], wv)
            assert np.array_equal(edges[off[k]:off[k + 1]], we) and np.array_equal(rows[off[k]:off[k + 1]], wr), k
            _, N, W = dp.forward(x, P, "max")
            assert np.array_equal(capi.profile_pair_fill_merged(dm, capi.MB_VITERBI, x, P, pm.TIE_COLTOK), np.stack([N, W], axis=2)), k
    finally:
        dev.close(); dm.close()


# ---- 5. cross-checks without the restatement --------------------------------------------------------------------------------------------
def test_no_input_equals_device_profiles():
    """I = 0 against the one-tape merged sweeps, DeviceProfiles(dm, profiles, colTok): scores, paths and counts."""
    em, colTok, pairs = pm.lane_case(4, 13)[0]
    profs = [P for _, P in pairs] + [pm.merged_input(np.random.RandomState(5), em, 4, 0, 17)[1]]
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfilePairs(dm, [[] for _ in profs], profs, colTok)
    one = capi.DeviceProfiles(dm, profs, colTok)
    try:
        f2, f1 = two.forward(), one.forward()
        assert (f1 > -math.inf).any() and logs_close(f2, f1)
        v2, v1 = two.viterbi(), one.viterbi()
        assert logs_close(v2[0], v1[0], 1e-12) and all(np.array_equal(a, b) for a, b in zip(v2[1:], v1[1:]))
        assert counts_close(two.counts()[0], one.counts()[0])
    finally:
        two.close(); one.close(); dm.close()


def test_equals_token_kernels_on_the_composite():
    """S = 8, nCols = 2, I = 3, L = 6 against the existing two-tape token kernels on algebra.compose(M, merging recogniser): the
    materialised fill of the generic family, whose sums are the exact fp64 log-sum-exp as this family's are (test_gpu_parity.py holds
    it to 1e-11 of the oracle), so the 1e-9 of the likelihoods holds between them.  (The tiled token families add their correction
    terms in fp32, about 1e-7 per cell, and would need a bound of their own.)"""
    from pairprofilehelpers import pair_machine
    from profhelpers import _machine_of
    em = pair_machine(8, 3, True, 2, 3)
    colTok = [2, 1]
    x, P = pm.merged_input(np.random.RandomState(8), em, 2, 3, 6, zeros=0.1)
    prof = Profile([em.outputTokenizer.tok2sym[t] for t in colTok], [list(np.exp(r[1:])) + [float(np.exp(r[0]))] for r in P])
    ec = EvaluatedMachine.fromMachine(algebra.compose(_machine_of(em), prof.mergingRecogniserMachine(), True, False), {}, useDefaults=True)
    xs = ec.inputTokenizer.tokenize([em.inputTokenizer.tok2sym[t] for t in x])
    dc = capi.DeviceMachine(ec)
    capi.set_kernel(1)                                               # the generic family
    try:
        want = dc.fill(capi.MB_FORWARD, xs, np.zeros(0, np.int32))[0, -1, -1]
        assert "generic" in capi.last_kernel_name()
    finally:
        capi.set_kernel(capi.KERNEL_AUTO)
        dc.close()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x], [P], colTok)
    try:
        got = dev.forward()
    finally:
        dev.close(); dm.close()
    assert want > -math.inf and logs_close(got, [want]), (got, want)


# ---- 6. column maps and rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("two", "same", "unused", "one"))
def test_column_maps(name):
    em, colTok, pairs = pm.column_map_cases()[name]
    pm.check_machine(em, colTok, pairs)


@pytest.mark.parametrize("name", ("allblank", "infrow", "infweights"))
def test_rows(name):
    em, colTok, pairs = pm.row_cases()[name]
    refs = pm.check_machine(em, colTok, pairs)
    if name == "infrow":
        assert refs[1]["ll"] == -math.inf and refs[0]["ll"] > -math.inf


# ---- 7. errors and bounds ---------------------------------------------------------------------------------------------------------------
def test_errors():
    from pairprofilehelpers import pair_machine
    em = pair_machine(8, 1, True, 2, 3)
    dm = capi.DeviceMachine(em)
    colTok = [1, 3]
    P = pm.merged_input(np.random.RandomState(1), em, 2, 0, 5)[1]
    want = PairMergedProfileDP(em, colTok).forward([1, 2], P)[0]

    def works():
        dev = capi.DeviceProfilePairs(dm, [[1, 2]], [P], colTok)
        ll = dev.forward()
        dev.close()
        assert ll[0] > -math.inf and logs_close(ll, [want])
    with pytest.raises(capi.MbError, match="columns"):
        capi.DeviceProfilePairs(dm, [[1]], [np.zeros((2, 1))], [])
    works()
    for bad in ([0, 1], [1, 4]):
        with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
            capi.DeviceProfilePairs(dm, [[1]], [P], bad)
        works()
    with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
        capi.profile_pair_fill_merged(dm, capi.MB_FORWARD, [1], P, [4, 1])
    for bad in ([0], [3], [1, 2, 3]):
        with pytest.raises(capi.MbError, match="outside 1..nInTok"):
            capi.DeviceProfilePairs(dm, [bad], [P], colTok)
        works()
    with pytest.raises(capi.MbError, match="outside 1..nInTok"):
        capi.profile_pair_fill_merged(dm, capi.MB_FORWARD, [3], P, colTok)
    nan = P.copy(); nan[2, 1] = np.nan
    with pytest.raises(capi.MbError, match="NaN"):
        capi.DeviceProfilePairs(dm, [[1]], [nan], colTok)
    works()
    inf = P.copy(); inf[0, 0] = np.inf
    with pytest.raises(capi.MbError, match="infinity"):
        capi.DeviceProfilePairs(dm, [[1]], [inf], colTok)
    works()
    dev = capi.DeviceProfilePairs(dm, [[1, 2], [2]], [P, P], colTok)
    with pytest.raises(capi.MbError, match="pathCap too small"):
        dev.viterbi(cap=dev.path_cap() - 1)
    v, off, edges, rows = dev.viterbi()
    assert (v > -math.inf).all() and off[-1] == len(edges)
    capi.set_memory_budget(1024)
    try:
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.forward(capi.MB_MATERIALISE)
    finally:
        capi.set_memory_budget(0)
    dev.close()
    works()
    dm.close()


def test_full_traceback_slots():
    """The chain machine against merged profiles that force an emission at every row: every path has exactly
    I + L + (I + L + 1)(nLevF - 1) edges, the size of its slot."""
    em, colTok, pairs = pm.chain_case()
    dp = PairMergedProfileDP(em, colTok)
    refs = [dp.viterbi(x, P) for x, P in pairs]
    bounds = [len(x) + len(P) + (len(x) + len(P) + 1) * (pm.CHAIN_S - 1) for x, P in pairs]
    assert [len(r[1]) for r in refs] == bounds and bounds[0] == 39
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, pairs, colTok)
    try:
        assert dev.path_cap() == sum(bounds)
        v, off, edges, rows = dev.viterbi(cap=dev.path_cap())
        assert list(np.diff(off)) == bounds
        for k, (wv, we, wr) in enumerate(refs):
            assert abs(v[k] - wv) <= 1e-12 * max(1.0, abs(wv)), (k, v[k], wv)
            assert np.array_equal(edges[off[k]:off[k + 1]], we) and np.array_equal(rows[off[k]:off[k + 1]], wr), k
        with pytest.raises(capi.MbError, match="pathCap too small"):
            dev.viterbi(cap=dev.path_cap() - 1)
    finally:
        dev.close(); dm.close()


# ---- 8. the Python entry point ----------------------------------------------------------------------------------------------------------
def test_score_profile_pairs_device_equals_numpy():
    m = Machine.fromFile("tests/golden/machine/dnastore4.json")
    par = m.getParamDefs(True)
    prof = Profile.fromCsv("tests/golden/csv/tiny_uc.csv")
    seqs = [[], ["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"]]
    kw = dict(params=par, merge=True, loglike=True, viterbi=True, counts=True)
    (sd, cd), (sn, cn) = boss.scoreProfilePairs(m, seqs, prof, backend="device", **kw), boss.scoreProfilePairs(m, seqs, prof, backend="numpy", **kw)
    assert logs_close(sd["loglike"], sn["loglike"]) and logs_close(sd["viterbi"], sn["viterbi"], 1e-12)
    assert np.isfinite(sn["loglike"]).sum() >= 2 and sn["loglike"][2] == -math.inf
    assert cd.keys() == cn.keys()          # (dnastore4 has no parameters)
    # a machine with parameters: bitnoise against three rows that merge to "01"; the counts under the bounds of the table
    import json
    mb = Machine.fromFile("tests/golden/machine/bitnoise.json")
    kw["params"] = json.load(open("tests/golden/io/params.json"))
    prof = Profile.fromCsv("tests/golden/csv/prof001.csv")
    seqs = [list("01"), list("10"), list("0z"), list("00"), list("11")]
    (sd, cd), (sn, cn) = boss.scoreProfilePairs(mb, seqs, prof, backend="device", **kw), boss.scoreProfilePairs(mb, seqs, prof, backend="numpy", **kw)
    assert logs_close(sd["loglike"], sn["loglike"]) and logs_close(sd["viterbi"], sn["viterbi"], 1e-12)
    assert np.isfinite(sn["loglike"]).sum() == 4 and sn["loglike"][2] == -math.inf
    keys = sorted(cn)
    got, want = np.array([cd[k] for k in keys]), np.array([cn[k] for k in keys])
    note_counts(got, want, pm.WORST, "parameter counts")
    assert sorted(cd) == keys and len(keys) == 2 and (want > 1.0).all() and counts_close(got, want), (cd, cn)
