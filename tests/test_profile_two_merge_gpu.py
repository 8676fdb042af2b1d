"""GPU tests of the two-profile sweeps against CTC-merged output profiles (mb_profile_two_merge.hip, mb_profile_api.hip;
docs/profile_tapes.md, "Pairs of profiles against a merged profile"): the device against profile.TwoMergedProfileDP.  Bounds
(twomergehelpers, those of the pair and two-profile families, unchanged): log values 1e-9 relative to max(1, |value|) with -inf
exact; counts >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x count absolute; fixed-point counts by fixed_counts_close with
cells x planes; Viterbi scores at 1e-12; paths, output rows and input rows equal.
test_profile_two_merge_host.py::test_gpu_inputs_are_live holds the builders to their liveness conditions without a GPU."""
import math

import numpy as np
import pytest

import twomergehelpers as tm
import twoprofilehelpers as th
from twomergehelpers import counts_close, logs_close, note, note_counts
from machineboss_amd import algebra, boss, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import Profile, TwoMergedProfileDP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    print("worst deviations of the module:", tm.WORST)


def _twos(dm, pairs, colTok):
    return capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs], colTok=colTok)


def _rolling(dev):
    return dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]


def _cell_planes(pairs, colTok):
    return sum((len(A) + 1) * (len(B) + 1) for A, B in pairs) * (len(colTok) + 1)


# ---- 1. lane grouping -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", tm.LANE_CASES)
def test_lane_grouping(nCols, S):
    """Every cell of the three fills, rolling and materialised Forward (the same bits), Viterbi with paths and counts, with silent
    levels and without, at the seven shapes."""
    colTok, cases = tm.lane_case(nCols, S)
    live = dict(ll=[], cells=0, all=0)
    for em in dict.fromkeys(id(c[0]) for c in cases):
        group = [c for c in cases if id(c[0]) == em]
        tm.check_machine(group[0][0], colTok, [(A, B) for _, A, B in group], live=live)
    assert np.mean(live["ll"]) >= 0.9 and live["cells"] > 0.5 * live["all"], (np.mean(live["ll"]), live["cells"], live["all"])
    assert capi.last_kernel_name().startswith("k_profile_two_merge_")


# ---- 2. rings ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    em, pairs = tm.ring_pairs()
    dp = TwoMergedProfileDP(em, tm.RING_COLTOK)
    return em, pairs, np.array([dp.forward(A, B)[0] for A, B in pairs]), np.array([dp.forward(A, B, "max")[0] for A, B in pairs])


def test_ragged_launch_of_lds_and_scratch_rings(ragged):
    """nCols = 2, S = 20: a ring of 6 240 (min(K, L) + 1) bytes.  Short sides 9 / 10 around 64 KiB and 25 / 26 around 160 KiB, found
    by i and by r, beside (2, 3), (0, 40), (40, 0) and a dead pair, in one launch.  Rolling has the bits of materialised; every pair
    alone on the workspace the batch left behind, and the batch cut into chunks of one scratch ring each, return the same bits."""
    em, pairs, want, wv = ragged
    colTok = tm.RING_COLTOK
    assert (want[:-1] > -math.inf).all() and want[-1] == -math.inf
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs, colTok)
    try:
        f0, v0 = _rolling(dev)
        assert capi.last_kernel_name() == "k_profile_two_merge_fwd<max,rolling>"
        note("forward", f0, want, tm.WORST)
        assert logs_close(f0, want), (f0, want)
        assert logs_close(v0, wv, 1e-12), (v0, wv)
        assert capi.last_launch_count() == 1
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), f0)
        assert capi.last_kernel_name() == "k_profile_two_merge_fwd<sum,mat>"
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        order = sorted(range(len(pairs)), key=lambda k: -tm.ring_bytes(tm.RING_S, 2, len(pairs[k][0]), len(pairs[k][1])))
        for k in order:
            one = _twos(dm, pairs[k:k + 1], colTok)
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
        capi.set_memory_budget(tm.ring_bytes(tm.RING_S, 2, 26, 30) + 1024)
        try:
            f2 = dev.forward(capi.MB_ROLLING)
            n2 = capi.last_launch_count()
            v2 = dev.viterbi(paths=False)[0]
        finally:
            capi.set_memory_budget(0)
        assert n2 >= 2 and np.array_equal(f0, f2) and np.array_equal(v0, v2), (n2, f0, f2)
    finally:
        dev.close(); dm.close()


def test_ragged_launch_everything(ragged):
    """The small pairs of the ragged batch and two ring pairs through every entry point (paths, counts, lattices)."""
    em, pairs, _, _ = ragged
    tm.check_machine(em, tm.RING_COLTOK, [pairs[0], pairs[4]] + pairs[8:], fill=False)
    tm.check_machine(em, tm.RING_COLTOK, pairs[8:9] + pairs[11:])


def test_many_scratch_rings_packed_in_one_launch():
    """Twenty-four workgroups, eighteen with a ring of their own in the scratch buffer: several per die, so that rings which
    overlapped would meet in one cache.  Against the restatement, and every third pair alone returns the bits it had in the batch."""
    em, pairs = tm.packed_case()
    colTok = tm.PACKED_COLTOK
    dp = TwoMergedProfileDP(em, colTok)
    want = np.array([dp.forward(A, B)[0] for A, B in pairs])
    assert np.mean(want > -math.inf) >= 0.9
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs, colTok)
    try:
        f0, v0 = _rolling(dev)
        assert capi.last_launch_count() == 1
        note("forward", f0, want, tm.WORST)
        assert logs_close(f0, want), (f0, want)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), f0)
        for k in range(0, len(pairs), 3):
            one = _twos(dm, pairs[k:k + 1], colTok)
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], k
    finally:
        dev.close(); dm.close()


# ---- 3. counts --------------------------------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table():
    """11 204 transitions: beyond 8 192 every posterior goes into the global table with an atomic of its own.  A dead pair adds
    nothing in either mode, and the fixed point returns the same bits twice."""
    em, pairs, dead = tm.big_counts_case()
    colTok = tm.COUNT_COLTOK
    dp = TwoMergedProfileDP(em, colTok)
    refs = [dp.counts(A, B) for A, B in pairs]
    wc, want = np.sum([r[0] for r in refs], axis=0), np.array([r[1] for r in refs])
    assert em.nTransitions > 8192 and (want > -math.inf).all()
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs, colTok)
    both = _twos(dm, pairs[:1] + [dead] + pairs[1:], colTok)
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_merge_counts"
        note_counts(c, wc, tm.WORST)
        assert counts_close(c, wc) and logs_close(ll, want)
        c, s, ll = both.counts()
        assert counts_close(c, wc) and ll[1] == -math.inf and s == -math.inf and logs_close(np.delete(ll, 1), want)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            d1 = dev.counts(); d2 = dev.counts(); d3 = both.counts()
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        note_counts(d1[0], wc, tm.WORST, "fixed-point counts")
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d3[0], d1[0])
        assert tm.fixed_counts_close(d1[0], wc, _cell_planes(pairs, colTok)), np.abs(d1[0] - wc).max()
    finally:
        both.close(); dev.close(); dm.close()


# ---- 4. the traceback past one block ----------------------------------------------------------------------------------------------------
def test_traceback_past_one_block():
    """129 pairs of tiny shapes with dead pairs at slots 63, 64 and 128: against the restatement, and the first 64 and 65 pairs as
    objects of their own return the batch's bits."""
    em, pairs = tm.seam_case()
    colTok = tm.SEAM_COLTOK
    dp = TwoMergedProfileDP(em, colTok)
    refs = [dp.viterbi(A, B) for A, B in pairs]
    assert all(refs[k][0] == -math.inf and len(refs[k][1]) == 0 for k in tm.SEAM_DEAD)
    assert np.mean([r[0] > -math.inf for r in refs]) >= 0.8
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs, colTok)
    try:
        v, off, edges, rows, ins = dev.viterbi()
        assert capi.last_kernel_name() == "k_profile_two_merge_fwd<max,mat>" and capi.last_launch_count() == 1
        note("viterbi", v, [r[0] for r in refs], tm.WORST)
        assert logs_close(v, [r[0] for r in refs], 1e-12)
        for k, r in enumerate(refs):
            sl = slice(off[k], off[k + 1])
            assert np.array_equal(edges[sl], r[1]) and np.array_equal(rows[sl], r[2]) and np.array_equal(ins[sl], r[3]), k
        for n in (64, 65):
            part = _twos(dm, pairs[:n], colTok)
            try:
                pv, poff, pe, pr, pi = part.viterbi()
            finally:
                part.close()
            assert np.array_equal(pv, v[:n]) and np.array_equal(poff, off[:n + 1])
            assert np.array_equal(pe, edges[:off[n]]) and np.array_equal(pr, rows[:off[n]]) and np.array_equal(pi, ins[:off[n]])
    finally:
        dev.close(); dm.close()


# ---- 5. ties and the path bound ---------------------------------------------------------------------------------------------------------
def test_ties_are_decided_by_candidate_order():
    em = tm.tie_machine()
    pairs = tm.tie_pairs()
    census = {}
    dp = TwoMergedProfileDP(em, tm.TIE_COLTOK)
    for A, B in pairs:
        dp.viterbi(A, B, census)
    assert all(any(k[0] in c and k[-1] in c for c in census) for k in tm.TIE_KINDS), census
    tm.check_machine(em, tm.TIE_COLTOK, pairs)
    for em, colTok, A, B, edges, rows, ins in tm.hand_tie_cases():
        dm = capi.DeviceMachine(em)
        dev = _twos(dm, [(A, B)], colTok)
        try:
            v, off, e, r, i = dev.viterbi()
        finally:
            dev.close(); dm.close()
        assert v[0] == 0.0 and list(e) == edges and list(r) == rows and list(i) == ins


def test_full_traceback_slots():
    """The chain machine against profiles that force an emission at every row: every path has exactly
    K + L + (K + L + 1)(nLevF - 1) edges, the size of its slot."""
    em, colTok, pairs = tm.chain_case()
    refs = tm.check_machine(em, colTok, pairs, fill=False)
    nLev = len(TwoMergedProfileDP(em, colTok).fLevels)
    assert nLev == tm.CHAIN_S - 1
    for (A, B), r in zip(pairs, refs):
        assert r["v"] > -math.inf and len(r["path"][0]) == th.path_bound(nLev, len(A), len(B))


# ---- 6. reductions on the device --------------------------------------------------------------------------------------------------------
def test_device_reductions():
    """A one-hot A against merged DeviceProfilePairs on its tokens, K = 0 against merged DeviceProfiles: likelihoods at the log
    bound, Viterbi scores at 1e-12, paths equal."""
    em = th.pair_machine(8, 3, True, 2, 3)
    colTok = [3, 1, 3, 2]
    rng = np.random.RandomState(8)
    Bs = [tm.merged_rows(rng, 4, L, zeros=0.1) for L in (4, 6, 0)]
    xs = [rng.randint(1, 3, size=n) for n in (3, 5, 2)]
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [th.one_hot(x, 2) for x in xs], Bs, colTok=colTok)
    pair = capi.DeviceProfilePairs(dm, xs, Bs, colTok)
    none = capi.DeviceProfileTwos(dm, [np.zeros((0, 3))] * 2, Bs[:2], colTok=colTok)
    prof = capi.DeviceProfiles(dm, Bs[:2], colTok)
    try:
        f, g = two.forward(), pair.forward()
        assert (g[:2] > -math.inf).all() and logs_close(f, g), (f, g)
        tv, toff, te, tr, ti = two.viterbi()
        pv, poff, pe, pr = pair.viterbi()
        assert logs_close(tv, pv, 1e-12) and np.array_equal(toff, poff) and np.array_equal(te, pe) and np.array_equal(tr, pr)
        assert counts_close(two.counts()[0], pair.counts()[0])
        f, g = none.forward(), prof.forward()
        assert (g > -math.inf).all() and logs_close(f, g), (f, g)
        assert logs_close(none.viterbi(paths=False)[0], prof.viterbi(paths=False)[0], 1e-12)
        assert counts_close(none.counts()[0], prof.counts()[0])
    finally:
        prof.close(); none.close(); pair.close(); two.close(); dm.close()


def test_equals_token_kernels_on_the_composite():
    """S = 5, nCols = 2, K = 2, L = 3 against the generic token family on compose(A.machine(), compose(M, merging recogniser)) with
    both tapes empty: its sums are the exact fp64 log-sum-exp as this family's are, so the 1e-9 of the likelihoods holds between
    them."""
    em = th.pair_machine(5, 3, True, 2, 3)
    colTok = [2, 1]
    A, B = tm.merged_input(np.random.RandomState(8), em, 2, 2, 3, pInf=0.1)
    gen = th.profile_of(em.inputTokenizer.tok2sym[1:], A).machine()
    rec = tm.merged_profile_of(em, B, colTok).mergingRecogniserMachine()
    ec = EvaluatedMachine.fromMachine(algebra.compose(gen, algebra.compose(th.machine_of(em), rec, True, False), True, False), {}, useDefaults=True)
    dc = capi.DeviceMachine(ec)
    capi.set_kernel(1)                                               # the generic family
    try:
        want = dc.fill(capi.MB_FORWARD, np.zeros(0, np.int32), np.zeros(0, np.int32))[-1, -1, -1]
        assert "generic" in capi.last_kernel_name()
    finally:
        capi.set_kernel(capi.KERNEL_AUTO)
        dc.close()
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, [(A, B)], colTok)
    try:
        got = dev.forward()
    finally:
        dev.close(); dm.close()
    assert want > -math.inf and logs_close(got, [want]), (got, want)


# ---- 7. rows and column maps ------------------------------------------------------------------------------------------------------------
def test_degenerate_rows():
    """All-blank rows on either tape, a whole -inf row on either tape, an eighth of the weights -inf."""
    em, colTok, pairs = tm.degenerate_cases()
    refs = tm.check_machine(em, colTok, pairs)
    assert refs[3]["ll"] > -math.inf and refs[4]["ll"] == -math.inf and refs[5]["ll"] == -math.inf and refs[0]["ll"] > -math.inf


@pytest.mark.parametrize("which", range(len(tm.COLMAPS)))
def test_column_maps(which):
    """One column; every column on one token; a token nothing emits; a doubled symbol."""
    em, cases = tm.column_map_cases()
    colTok, A, B = cases[which]
    refs = tm.check_machine(em, colTok, [(A, B), (A[:2], B[:3]), (A[:0], B)])
    assert refs[0]["ll"] > -math.inf


def test_set_rows():
    """New rows on either tape or both; a refused table leaves both old tables in effect."""
    em = th.pair_machine(8, 2, True, 2, 3)
    colTok = (1, 3, 2)
    dp = TwoMergedProfileDP(em, colTok)
    rng = np.random.RandomState(2)
    old = [tm.merged_input(rng, em, 3, K, L, pInf=0.0) for K, L in ((3, 4), (0, 2), (4, 3))]
    new = [tm.merged_input(rng, em, 3, len(A), len(B), pInf=0.0) for A, B in old]
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, old, colTok)
    try:
        assert logs_close(dev.forward(), [dp.forward(A, B)[0] for A, B in old])
        dev.set_profiles(outProfiles=[B for _, B in new])
        assert logs_close(dev.forward(), [dp.forward(A, B)[0] for (A, _), (_, B) in zip(old, new)])
        bad = [B.copy() for _, B in old]; bad[0][1, 2] = np.nan
        with pytest.raises(capi.MbError, match="NaN"):
            dev.set_profiles(inProfiles=[A for A, _ in old], outProfiles=bad)
        assert logs_close(dev.forward(), [dp.forward(A, B)[0] for (A, _), (_, B) in zip(old, new)])
        dev.set_profiles(inProfiles=[A for A, _ in new])
        want = [dp.counts(A, B) for A, B in new]
        c, _, ll = dev.counts()
        assert logs_close(ll, [w[1] for w in want]) and counts_close(c, np.sum([w[0] for w in want], axis=0))
        with pytest.raises(ValueError):
            dev.set_profiles(outProfiles=[B[:1] for _, B in new])
    finally:
        dev.close(); dm.close()


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors():
    em = th.pair_machine(8, 1, True, 2, 3)
    dm = capi.DeviceMachine(em)
    colTok = [1, 3]
    A, B = tm.merged_input(np.random.RandomState(1), em, 2, 2, 5, pInf=0.0)
    want = TwoMergedProfileDP(em, colTok).forward(A, B)[0]

    def works():
        dev = _twos(dm, [(A, B)], colTok)
        ll = dev.forward()
        dev.close()
        assert ll[0] > -math.inf and logs_close(ll, [want])
    with pytest.raises(capi.MbError, match="columns"):
        capi.DeviceProfileTwos(dm, [A], [np.zeros((2, 1))], colTok=[])
    works()
    for bad in ([0, 1], [1, 4]):
        with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
            capi.DeviceProfileTwos(dm, [A], [B], colTok=bad)
        works()
    with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
        capi.profile_two_fill_merged(dm, capi.MB_FORWARD, A, B, [4, 1])
    with pytest.raises(capi.MbError, match="unknown fill mode"):
        capi.profile_two_fill_merged(dm, 77, A, B, colTok)
    nan = B.copy(); nan[2, 1] = np.nan
    with pytest.raises(capi.MbError, match="NaN"):
        capi.DeviceProfileTwos(dm, [A], [nan], colTok=colTok)
    inf = A.copy(); inf[0, 0] = np.inf
    with pytest.raises(capi.MbError, match="infinity"):
        capi.DeviceProfileTwos(dm, [inf], [B], colTok=colTok)
    works()
    with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
        capi.DeviceProfileTwos(dm, [A], [B], envs=[None], colTok=colTok)
    dev = _twos(dm, [(A, B), (A[:1], B)], colTok)
    with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
        dev.envelopes([([0] * 6, [3] * 6), None])
    dev.envelopes(None)
    with pytest.raises(capi.MbError, match="row posteriors take plain profiles"):
        dev.row_posteriors()
    with pytest.raises(capi.MbError, match="pathCap too small"):
        dev.viterbi(cap=dev.path_cap() - 1)
    with pytest.raises(capi.MbError, match="unknown flags"):
        dev.forward(77)
    v, off, edges, rows, ins = dev.viterbi()
    assert (v > -math.inf).all() and off[-1] == len(edges) == len(ins)
    assert dev.cells() == sum(3 * 3 * 8 * (len(a) + 1) * 6 for a in (A, A[:1]))
    capi.set_memory_budget(1024)
    try:
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.forward(capi.MB_MATERIALISE)
    finally:
        capi.set_memory_budget(0)
    dev.close()
    from prefixhelpers import machine_from_edges
    dn = capi.DeviceMachine(machine_from_edges(2, 0, 2, [(0, 1, 0, 1, -0.5), (0, 1, 0, 2, -1.0)]))
    with pytest.raises(capi.MbError, match="two-profile sweeps need a machine with an input alphabet"):
        capi.DeviceProfileTwos(dn, [np.zeros((0, 1))], [np.zeros((1, 2))], colTok=[1])
    dn.close()
    works()
    dm.close()


# ---- 9. chunks under a budget -----------------------------------------------------------------------------------------------------------
def test_chunked_lattices_return_the_bits_of_unchunked():
    """S = 65, nCols = 3: materialised Forward, Viterbi with paths and counts under a budget of two of the largest count footprints
    (the Forward and the Backward lattice; every X / T ring is in LDS): three chunks or more for the counts, two or more for the
    others under half of it.  Likelihoods, scores, paths and rows are the bits of the unchunked calls; the counts too under
    MB_DETERMINISTIC=1 (fixed point: the chunks' sums add exactly)."""
    em, pairs = tm.budget_case()
    colTok = tm.BUDGET_COLTOK
    sizes = [2 * tm.cell_bytes(tm.BUDGET_S, 3, len(A), len(B)) for A, B in pairs]
    budget = 2 * max(sizes) + 4096
    assert len(th.lattice_chunks(sizes, budget)) >= 3
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs, colTok)
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        f0, v0, c0 = dev.forward(capi.MB_MATERIALISE), dev.viterbi(), dev.counts()
        assert capi.last_launch_count() == 1 and (f0 > -math.inf).all() and c0[0].any()
        capi.set_memory_budget(budget // 2)
        f1 = dev.forward(capi.MB_MATERIALISE); nf = capi.last_launch_count()
        v1 = dev.viterbi(); nv = capi.last_launch_count()
        capi.set_memory_budget(budget)
        c1 = dev.counts(); nc = capi.last_launch_count()
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()
    assert min(nf, nv) >= 2 and nc >= 3, (nf, nv, nc)
    assert np.array_equal(f0, f1) and all(np.array_equal(a, b) for a, b in zip(v0, v1))
    assert np.array_equal(c0[0], c1[0]) and np.array_equal(c0[2], c1[2]) and c0[1] == c1[1]
    dp = TwoMergedProfileDP(em, colTok)
    assert logs_close(f0, [dp.forward(A, B)[0] for A, B in pairs])


# ---- 10. the Python entry ---------------------------------------------------------------------------------------------------------------
def test_score_two_profiles_merge_device_equals_numpy(tmp_path):
    m = Machine.fromFile("tests/golden/machine/dnastore4.json")
    par = m.getParamDefs(True)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    pa, pb = Profile.fromCsv(str(a)), Profile.fromCsv("tests/golden/csv/tiny_uc.csv")
    short = Profile(pa.header, pa.row[:1])
    dev, dc = boss.scoreTwoProfiles(m, [pa, short], pb, params=par, loglike=True, viterbi=True, counts=True, merge=True)
    assert capi.last_kernel_name().startswith("k_profile_two_merge_")
    ref, rc = boss.scoreTwoProfiles(m, [pa, short], pb, backend="numpy", params=par, loglike=True, viterbi=True, counts=True, merge=True)
    assert ref["loglike"][0] > -math.inf
    assert logs_close(dev["loglike"], ref["loglike"]) and logs_close(dev["viterbi"], ref["viterbi"], 1e-12) and dc == rc
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, params=par, merge=True, posteriors=True)
    with pytest.raises(MachineError, match="envelopes take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, params=par, merge=True, band=2)
