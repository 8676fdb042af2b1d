"""GPU tests of the two-profile sweeps against CTC-merged output profiles under an envelope (k_profile_two_merge_env_* in
mb_profile_two_merge.hip; docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope").  The reference is
profile.TwoMergedProfileDP(env=...) called per pair; the bounds are the family's (twomergeenvhelpers): log values 1e-9 relative to
max(1, |value|) with -inf exact; counts and posteriors >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x value; row sums 1e-6;
Viterbi scores at 1e-12 with equal paths, rows and input rows; fixed-point counts under fixed_counts_close; "the same bits" is ==.
test_profile_two_merge_env_host.py holds the builders to their conditions on the CPU."""
import functools
import math

import numpy as np
import pytest

import twomergeenvhelpers as tv
import twomergehelpers as tm
import twomergeposthelpers as tq
import twoprofilehelpers as th
from pairenvhelpers import diag_max, full, n_cells
from pairprofilehelpers import counts_close, logs_close, note, note_counts
from machineboss_amd import capi
from machineboss_amd.profile import MergedProfileDP, TwoMergedProfileDP
from machineboss_amd.seqpair import Envelope

pytestmark = pytest.mark.gpu

WORST = tv.WORST
ENV_FWD = "k_profile_two_merge_env_fwd<%s>"
FULL_FWD = "k_profile_two_merge_fwd<%s>"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the merged two-profile sweeps under an envelope:", WORST)


def _everything(dev):
    """cells() and, bit for bit comparable (call under MB_DETERMINISTIC=1), rolling and materialised Forward, Viterbi scores, paths,
    rows and input rows, counts and both posterior tables."""
    out = [np.array([dev.cells()]), dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]]
    out += list(dev.viterbi())
    c, s, ll = dev.counts()
    out += [c, np.array([s]), ll]
    out += list(dev.merged_row_posteriors())
    return out


def _same(a, b, what=None):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(u, v), (what, u, v)


def _per_pair(dev):
    """What a pair of a batch can be compared by, bit for bit: Forward both ways, the Viterbi score, its path, its posterior rows."""
    fr, fm, v = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]
    vv, off, e, r, i = dev.viterbi()
    pa, pb, pl = dev.merged_row_posteriors()
    sa, sb = tq.split(dev, pa, pb)
    return [[fr[k:k + 1], fm[k:k + 1], v[k:k + 1], vv[k:k + 1], e[off[k]:off[k + 1]], r[off[k]:off[k + 1]], i[off[k]:off[k + 1]], sa[k], sb[k], pl[k:k + 1]]
            for k in range(dev.nPairs)]


# ---- 1. the lane cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", tv.LANE_CASES)
def test_every_cell_under_every_envelope(nCols, S):
    """With and without silent levels, the seven lattices under the full envelope, band(0), band(1), a path envelope and a
    staircase: every cell of the Forward, max and Backward fills, all layers and planes exactly -inf outside; scores, paths, counts
    and both posterior tables.  At least half of the case's likelihoods are finite."""
    live = []
    for em, colTok, quads in tv.lane_case(nCols, S):
        tv.check_env_batch(em, colTok, [(A, B, env) for A, B, _, env in quads], fill=True, live=live)
    assert np.mean(live) >= 0.5, np.mean(live)


def test_lane_likelihoods_are_live_on_the_device():
    """Three in four of all likelihoods of the lane suite are finite, and half under every envelope kind."""
    by_kind = {}
    for nCols, S in tv.LANE_CASES:
        for em, colTok, quads in tv.lane_case(nCols, S):
            dm, dev = tv.open_twos(em, colTok, [(A, B, env) for A, B, _, env in quads])
            try:
                for (_, _, kind, _), ll in zip(quads, dev.forward(capi.MB_ROLLING)):
                    by_kind.setdefault(kind, []).append(ll > -math.inf)
            finally:
                dev.close(); dm.close()
    assert set(by_kind) == set(tv.ENV_KINDS) and all(np.mean(v) >= 0.5 for v in by_kind.values())
    assert np.mean(np.concatenate(list(by_kind.values()))) >= 0.75


# ---- 2. the ring marks -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mark_ref(M):
    dp = TwoMergedProfileDP(tv.mark_machine(), tv.MARK_COLTOK)
    A, B, env = tv.mark_case(M)
    return dp.forward(A, B, env=env)[0], dp.forward(A, B, "max", env=env)[0], dp.backward(A, B, env=env)[0]


@pytest.mark.parametrize("M", tv.MARK_M)
def test_rings_either_side_of_the_marks(M):
    """nCols = 4, S = 80, K = L = 40 under band(M - 1): the rolling ring takes 44 160 M bytes (M = 1 | 2 either side of 64 KiB, 3 | 4
    of 160 KiB), the X ring of the materialised Forward and the T ring of the Backward 15 360 M (4 | 5 and 10 | 11).  The rolling
    Forward, the materialised Forward with the same bits, the rolling Viterbi score and the Backward's likelihood: the pair alone, in
    one ragged launch beside a None pair, a (0, 0) pair and a dead pair, and alone again -- its bits of the batch."""
    em = tv.mark_machine()
    A, B, env = tv.mark_case(M)
    assert diag_max(env) == M
    ll, v, bl = _mark_ref(M)
    assert ll > -math.inf and v > -math.inf
    extras = list(tv.mark_extras())

    def alone():
        dm, dev = tv.open_twos(em, tv.MARK_COLTOK, [(A, B, env)])
        try:
            fr, fm, vr = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]
            assert capi.last_kernel_name() == ENV_FWD % "max,rolling" and capi.last_launch_count() == 1
            nb = capi.profile_two_fill_merged(dm, capi.MB_BACKWARD, A, B, tv.MARK_COLTOK, env)
            assert capi.last_kernel_name() == "k_profile_two_merge_env_bwd"
            pa, pb, pl = dev.merged_row_posteriors()
            return [fr, fm, vr, nb[0, 0, 0, 0, :1], pa, pb, pl]
        finally:
            dev.close(); dm.close()
    first = alone()
    note("forward at the marks", first[0], [ll], WORST)
    assert logs_close(first[0], [ll]) and np.array_equal(first[0], first[1])
    assert logs_close(first[2], [v], 1e-12)
    note("backward at the marks", first[3], [bl], WORST)
    assert logs_close(first[3], [bl]) and logs_close(first[6], [ll])
    assert np.abs(first[4].sum(axis=1) - 1.0).max() <= 1e-6 and np.abs(first[5].sum(axis=1) - 1.0).max() <= 1e-6
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        one = alone()
        dm, dev = tv.open_twos(em, tv.MARK_COLTOK, extras[:2] + [(A, B, env)] + extras[2:])
        try:
            fr, fm, vr = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]
            assert capi.last_kernel_name() == ENV_FWD % "max,rolling" and capi.last_launch_count() == 1
            pa, pb, pl = dev.merged_row_posteriors()
            sa, sb = tq.split(dev, pa, pb)
            assert fr[3] == fm[3] == -math.inf and not sa[3].any() and not sb[3].any()      # (the dead pair)
            assert np.all(fr[:3] > -math.inf)
            _same([fr[2:3], fm[2:3], vr[2:3], sa[2], sb[2], pl[2:3]], [one[0], one[1], one[2], one[4], one[5], one[6]], "the pair of the batch")
        finally:
            dev.close(); dm.close()
        _same(alone(), one, "alone again")
    finally:
        capi.set_option("MB_DETERMINISTIC", None)


# ---- 3. scratch rings in one launch ----------------------------------------------------------------------------------------------------------
def test_scratch_rings_of_one_launch_do_not_meet():
    """Twenty-four pairs at S = 140, nCols = 2, eighteen of them with rolling rings of 174 720 bytes in the scratch buffer, in one
    launch: every likelihood and Viterbi score against the yardstick, and three pairs alone with their bits of the batch."""
    em, triples = tv.packed_case()
    dp = TwoMergedProfileDP(em, tv.PACKED_COLTOK)
    want = np.array([dp.forward(A, B)[0] for A, B, _ in triples])
    wv = np.array([dp.forward(A, B, "max")[0] for A, B, _ in triples])
    dm, dev = tv.open_twos(em, tv.PACKED_COLTOK, triples)
    try:
        fr = dev.forward(capi.MB_ROLLING)
        assert capi.last_kernel_name() == ENV_FWD % "sum,rolling" and capi.last_launch_count() == 1
        note("forward, rings in scratch", fr, want, WORST)
        assert logs_close(fr, want) and np.all(want > -math.inf)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), fr)
        vr = dev.viterbi(paths=False)[0]
        assert logs_close(vr, wv, 1e-12)
    finally:
        dev.close()
    try:
        for k in (0, 1, 23):
            A, B, _ = triples[k]
            one = capi.DeviceProfileTwos(dm, [A], [B], colTok=tv.PACKED_COLTOK, mergedEnvs=[full(len(A), len(B))])
            try:
                assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.viterbi(paths=False)[0][0] == vr[k], k
            finally:
                one.close()
    finally:
        dm.close()


# ---- 4. the full envelope against none -------------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope_on_the_device():
    """The ragged batch without envelopes, with the full envelope on every pair, and with it on one pair alone (the others then get
    theirs from the host): Forward in both modes, Viterbi with paths, fixed-point counts and both posterior tables, the same bits;
    and one pair of the batch alone."""
    em, colTok, pairs = tv.ragged_case()
    plain = [(A, B, None) for A, B in pairs]
    whole = [(A, B, full(len(A), len(B))) for A, B in pairs]
    one = [(A, B, full(len(A), len(B)) if k == 4 else None) for k, (A, B) in enumerate(pairs)]
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        dm, dev = tv.open_twos(em, colTok, plain)
        try:
            want = _everything(dev)
            assert capi.last_kernel_name() == "k_profile_two_merge_rowpost" and capi.last_launch_count() == 1
            each = _per_pair(dev)
            dev.merged_envelopes([t[2] for t in whole])
            _same(_everything(dev), want, "the full envelope on every pair")
            assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost" and capi.last_launch_count() == 1
            dev.merged_envelopes([t[2] for t in one])
            _same(_everything(dev), want, "the full envelope on one pair")
            assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost"
        finally:
            dev.close(); dm.close()
        k = len(pairs) - 3
        dm, dev = tv.open_twos(em, colTok, whole[k:k + 1])
        try:
            _same(_per_pair(dev)[0], each[k], "one pair alone")
        finally:
            dev.close(); dm.close()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)


# ---- 5. counts past the LDS table ------------------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table_under_a_band():
    """11 204 transitions under band(2) beside a dead pair: floating point against the yardstick; fixed point the same bits twice
    and the sum of the pairs run alone."""
    em, colTok, triples = tv.big_counts_env_case()
    dp = TwoMergedProfileDP(em, colTok)
    want = np.sum([dp.counts(A, B, env=env)[0] for A, B, env in triples[:-1]], axis=0)
    cells = sum(n_cells(env) for _, _, env in triples) * (len(colTok) + 1)
    dm, dev = tv.open_twos(em, colTok, triples)
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_merge_env_counts" and capi.last_launch_count() == 1
        note_counts(c, want, WORST, "counts past the table")
        assert counts_close(c, want), np.abs(c - want).max()
        assert ll[-1] == -math.inf and np.all(ll[:-1] > -math.inf) and s == -math.inf
        capi.set_option("MB_DETERMINISTIC", "1")
        f1, f2 = dev.counts()[0], dev.counts()[0]
        assert np.array_equal(f1, f2) and th.fixed_counts_close(f1, want, cells)
        alone = np.zeros(em.nTransitions)
        for t in triples:
            one = capi.DeviceProfileTwos(dm, [t[0]], [t[1]], colTok=colTok, mergedEnvs=[t[2]])
            try:
                alone = alone + one.counts()[0]
            finally:
                one.close()
        assert np.array_equal(f1, alone)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 6. the axis-1 traversal -------------------------------------------------------------------------------------------------------------------
def test_columns_of_many_two_and_one_cell():
    em, colTok, A, B, env = tv.post_stairs_case()
    tv.check_env_batch(em, colTok, [(A, B, env), (A, B, None)], fill=True)


@functools.lru_cache(maxsize=None)
def _long_refs(K, L):
    em, colTok, triples = tv.long_case(K, L)
    dp = TwoMergedProfileDP(em, colTok)
    return em, colTok, triples, [dp.mergedRowPosteriors(A, B, env=env) for A, B, env in triples]


@pytest.mark.parametrize("K,L", tv.LONG_SHAPES)
def test_row_posteriors_past_the_table_and_past_1024_lines(K, L):
    """S = 2 at (1, 1 100) and (1 100, 1) under the staircase, with MB_ROWPOST_TABLE at 4 (one line a block on the input axis, no
    line of the five output bins), at 2 (global bins on both axes) and the default: the yardstick's tables, row sums 1, column sums
    the counts() of the same object, the dead pair's rows exactly zero."""
    em, colTok, triples, refs = _long_refs(K, L)
    dm, dev = tv.open_twos(em, colTok, triples)
    try:
        c = dev.counts()[0]
        ga, gb = tq.grouped(em, colTok, c)
        rep = []      # (the repeat part of the live pair's output table, which the device does not hand back on its own)
        TwoMergedProfileDP(em, colTok).mergedRowPosteriors(*triples[0][:2], rep, env=triples[0][2])
        for table in tv.LONG_TABLES:
            capi.set_option("MB_ROWPOST_TABLE", table)
            pa, pb, pl = dev.merged_row_posteriors()
            assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost" and capi.last_launch_count() == 1
            sa, sb = tq.split(dev, pa, pb)
            tq.compare(em, colTok, sa, sb, pl, refs, "posteriors, long lines")
            assert pl[0] > -math.inf and pl[1] == -math.inf and not sa[1].any() and not sb[1].any()
            assert np.abs(sa[0].sum(axis=1) - 1.0).max() <= 1e-6 and np.abs(sb[0].sum(axis=1) - 1.0).max() <= 1e-6
            assert counts_close(pa[:, 1:].sum(axis=0), ga), table
            assert counts_close(tq.by_token(em, colTok, (sb[0] - rep[0])[:, 1:].sum(axis=0)), gb), table
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        dev.close(); dm.close()


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------------------
def test_compact_lattices_under_a_budget_below_one_rectangle():
    """S = 65, nCols = 3, K = L = 60 under band(4), the budget a third of one rectangle: three pairs make three chunks, and the
    chunked fixed-point counts and posteriors are the unchunked bits; a budget below one compact lattice is the existing error."""
    em, colTok, pairs, env = tv.chunk_case()
    triples = [(A, B, env) for A, B in pairs]
    dm, dev = tv.open_twos(em, colTok, triples)
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        assert 8 * dev.cells() == 3 * tv.chunk_pair_bytes("forward")
        c0 = dev.counts()
        assert capi.last_launch_count() == 1
        p0 = dev.merged_row_posteriors()
        assert capi.last_launch_count() == 1 and np.all(p0[2] > -math.inf)
        capi.set_memory_budget(tv.chunk_budget())
        c1 = dev.counts()
        assert capi.last_launch_count() == 3 and capi.last_kernel_name() == "k_profile_two_merge_env_counts"
        _same([c1[0], np.array([c1[1]]), c1[2]], [c0[0], np.array([c0[1]]), c0[2]], "chunked counts")
        p1 = dev.merged_row_posteriors()
        assert capi.last_launch_count() == 3
        _same(p1, p0, "chunked posteriors")
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), c0[2])
        capi.set_memory_budget(tv.chunk_pair_bytes("forward") // 2)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.forward(capi.MB_MATERIALISE)
        assert np.array_equal(dev.forward(capi.MB_ROLLING), c0[2])      # (the rolling sweep keeps no lattice)
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 8. ties, traceback blocks, envelope changes ---------------------------------------------------------------------------------------------
def test_ties_under_a_band():
    """The tie machine under band(1): scores at 1e-12 and the yardstick's paths, rows and input rows, where a repeat, an output-only,
    an input-only and an input-blank candidate each lose by lying outside (the CPU census asserts that they do)."""
    em = tm.tie_machine()
    triples = tv.tie_env_pairs()
    dp = TwoMergedProfileDP(em, tm.TIE_COLTOK)
    refs = [dict(v=dp.forward(A, B, "max", env=env)[0], path=dp.viterbi(A, B, env=env)[1:]) for A, B, env in triples]
    dm, dev = tv.open_twos(em, tm.TIE_COLTOK, triples)
    try:
        tv.check_paths(*dev.viterbi(), refs, "viterbi, ties")
        assert capi.last_kernel_name() == ENV_FWD % "max,mat" and all(r["v"] > -math.inf for r in refs)
    finally:
        dev.close(); dm.close()


def test_traceback_past_one_block():
    """129 pairs with dead pairs at slots 63, 64 and 128, each under an envelope of its shape."""
    em, triples = tv.seam_case()
    dp = TwoMergedProfileDP(em, tv.SEAM_COLTOK)
    refs = [dict(v=dp.forward(A, B, "max", env=env)[0], path=dp.viterbi(A, B, env=env)[1:]) for A, B, env in triples]
    dm, dev = tv.open_twos(em, tv.SEAM_COLTOK, triples)
    try:
        v, off, e, r, i = dev.viterbi()
        assert capi.last_launch_count() == 1
        tv.check_paths(v, off, e, r, i, refs, "viterbi, 129 pairs")
        for k in tv.SEAM_DEAD:
            assert v[k] == -math.inf and off[k] == off[k + 1]
    finally:
        dev.close(); dm.close()


def test_envelopes_set_changed_and_cleared_on_one_object():
    """Envelopes set, changed, cleared, and the profiles replaced in between: every state gives the bits of a fresh object."""
    em, colTok, pairs = tv.ragged_case()
    pairs = pairs[:8]
    rng = np.random.RandomState(77)
    bands = [tv.band_or_full(len(A), len(B), 2) for A, B in pairs]
    stairs = [tv.staircase(len(A), len(B)) for A, B in pairs]
    other = [tm.merged_input(rng, em, len(colTok), len(A), len(B), pInf=0.0) for A, B in pairs]
    capi.set_option("MB_DETERMINISTIC", "1")
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs], colTok=colTok)
    try:
        def fresh(ps, envs):
            one = capi.DeviceProfileTwos(dm, [A for A, _ in ps], [B for _, B in ps], colTok=colTok, mergedEnvs=envs)
            try:
                return _everything(one)
            finally:
                one.close()
        _same(_everything(dev), fresh(pairs, None), "new")
        dev.merged_envelopes(bands)
        _same(_everything(dev), fresh(pairs, bands), "bands")
        assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost"
        dev.set_profiles([A for A, _ in other], [B for _, B in other])
        _same(_everything(dev), fresh(other, bands), "new profiles keep the envelopes")
        dev.merged_envelopes(stairs)
        _same(_everything(dev), fresh(other, stairs), "staircases")
        dev.merged_envelopes(None)
        _same(_everything(dev), fresh(other, None), "cleared")
        assert capi.last_kernel_name() == "k_profile_two_merge_rowpost"
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 9. reductions on the device -------------------------------------------------------------------------------------------------------------
def test_one_hot_input_is_the_merged_pair_sweep_on_the_device():
    """A one-hot A under band(3) against a merged DeviceProfilePairs under the same envelope: likelihood, Viterbi score, counts and
    the output-row posteriors within the family's bounds."""
    em, colTok, x, A, B, env = tv.onehot_case()
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [A], [B], colTok=colTok, mergedEnvs=[env])
    pair = capi.DeviceProfilePairs(dm, [x], [B], colTok)
    try:
        pair.set_merged_envelopes([env])
        assert logs_close(two.forward(capi.MB_ROLLING), pair.forward(capi.MB_ROLLING)) and two.forward()[0] > -math.inf
        assert logs_close(two.viterbi(paths=False)[0], pair.viterbi(paths=False)[0], 1e-12)
        v2, o2, e2, r2, _ = two.viterbi()
        v1, o1, e1, r1 = pair.viterbi()
        assert np.array_equal(e2, e1) and np.array_equal(r2, r1)
        assert counts_close(two.counts()[0], pair.counts()[0])
        pa, pb, _ = two.merged_row_posteriors()
        assert counts_close(pb, pair.merged_row_posteriors()[0])
        assert np.allclose(pa[np.arange(len(x)), x], 1.0, rtol=0, atol=1e-9)
    finally:
        two.close(); pair.close(); dm.close()


def test_no_input_under_its_only_envelope_is_the_one_tape_sweep():
    em, colTok, Bs = tv.no_input_case()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [np.zeros((0, em.nInTok + 1))] * len(Bs), Bs, colTok=colTok, mergedEnvs=[full(0, len(B)) for B in Bs])
    one = capi.DeviceProfiles(dm, Bs, colTok)
    try:
        got = dev.forward(capi.MB_ROLLING)
        assert capi.last_kernel_name() == ENV_FWD % "sum,rolling"
        want = one.forward()
        note("no input", got, want, WORST)
        assert logs_close(got, want) and np.all(want > -math.inf), (got, want)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), got) and capi.last_kernel_name() == ENV_FWD % "sum,mat"
        dp = MergedProfileDP(em, colTok)
        assert logs_close(got, [dp.forward(B)[0] for B in Bs])
    finally:
        dev.close(); one.close(); dm.close()


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------------------
BAD_ENVELOPES = (([0, 0], [4, 4], "Envelope/sequence mismatch"), ([0, 0, 0], [4, 4, 5], "Envelope/sequence mismatch"),
                 ([0, 2, 3], [1, 3, 4], "Envelope is not connected"), ([0, 1, 0], [4, 4, 4], "Envelope is not monotone"))


def test_errors_leave_the_object_usable_and_launch_nothing():
    em = th.pair_machine(3, 0, True, 2, 3)
    colTok = (1, 2)
    A, B = tm.merged_input(np.random.RandomState(0), em, 2, 3, 2, pInf=0.0)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfileTwos(dm, [A], [B], colTok=colTok)
    plain = capi.DeviceProfileTwos(dm, [A], [np.zeros((2, em.nOutTok + 1))])
    try:
        want = dev.forward(capi.MB_MATERIALISE)
        assert capi.last_kernel_name() == FULL_FWD % "sum,mat" and capi.last_launch_count() == 1
        rect = dev.cells()
        for st, en, msg in BAD_ENVELOPES:
            dev.merged_envelopes([Envelope.band(3, 2, 1)])
            assert dev.cells() < rect
            launches = capi.last_launch_count()
            with pytest.raises(capi.MbError, match=msg):
                dev.merged_envelopes([(st, en)])
            assert capi.last_launch_count() == launches
            assert dev.cells() == rect and np.array_equal(dev.forward(capi.MB_MATERIALISE), want)      # (a rejected call leaves no envelopes)
            assert capi.last_kernel_name() == FULL_FWD % "sum,mat"
            with pytest.raises(capi.MbError, match=msg):
                capi.profile_two_fill_merged(dm, capi.MB_FORWARD, A, B, colTok, (st, en))
            # (rows that do not match are refused before the call; the call clears the count of the last one and launches nothing)
            assert capi.last_launch_count() == (1 if len(st) != len(B) + 1 else 0)
        dev.forward(capi.MB_MATERIALISE)
        launches = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="merged envelopes take merged profiles"):
            plain.merged_envelopes([Envelope.band(3, 2, 1)])
        with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
            dev.envelopes([Envelope.band(3, 2, 1)])
        with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
            capi.DeviceProfileTwos(dm, [A], [B], envs=[Envelope.band(3, 2, 1)], colTok=colTok)
        with pytest.raises(capi.MbError, match="row posteriors take plain profiles"):
            dev.row_posteriors()
        assert capi.last_launch_count() == launches
        dev.merged_envelopes([Envelope.band(3, 2, 1)])
        got = dev.forward(capi.MB_MATERIALISE)
        assert capi.last_kernel_name() == ENV_FWD % "sum,mat" and got[0] < want[0]
        for call, name in ((lambda: dev.forward(capi.MB_ROLLING), ENV_FWD % "sum,rolling"), (lambda: dev.viterbi(paths=False), ENV_FWD % "max,rolling"),
                           (dev.viterbi, ENV_FWD % "max,mat"), (dev.counts, "k_profile_two_merge_env_counts"),
                           (dev.merged_row_posteriors, "k_profile_two_merge_env_rowpost"),
                           (lambda: capi.profile_two_fill_merged(dm, capi.MB_BACKWARD, A, B, colTok, Envelope.band(3, 2, 1)), "k_profile_two_merge_env_bwd")):
            call()
            assert capi.last_kernel_name() == name
        assert plain.forward(capi.MB_ROLLING)[0] > -math.inf
    finally:
        dev.close(); plain.close(); dm.close()


# ---- 11. the layers above --------------------------------------------------------------------------------------------------------------------
def test_score_merged_twos_on_the_device(tmp_path):
    import os
    from machineboss_amd import boss
    from machineboss_amd.machine import Machine
    from machineboss_amd.profile import Profile
    here = os.path.dirname(os.path.abspath(__file__))
    m = Machine.fromFile(os.path.join(here, "golden", "machine", "dnastore4.json"))
    par = m.getParamDefs(True)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    pa, pb = Profile.fromCsv(str(a)), Profile.fromCsv(os.path.join(here, "golden", "csv", "tiny_uc.csv"))
    rows = [list(r) for r in pa.row]
    profs = [pa, Profile(pa.header, rows[:1]), Profile(pa.header, rows[1:]), Profile(pa.header, [[0.0] * len(pa.header)] + rows[1:])]
    kw = dict(params=par, loglike=True, viterbi=True, counts=True, posteriors=True, band=2)
    sd, cd = boss.scoreMergedTwos(m, profs, pb, "device", **kw)
    assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost"
    sn, cn = boss.scoreMergedTwos(m, profs, pb, "numpy", **kw)
    assert logs_close(sd["loglike"], sn["loglike"]) and logs_close(sd["viterbi"], sn["viterbi"], 1e-12)
    assert [l > -math.inf for l in sn["loglike"]] == [True, True, True, False]
    for (ga, gb), (wa, wb) in zip(sd["posteriors"], sn["posteriors"]):
        assert counts_close(ga, wa) and counts_close(gb, wb)
    assert sorted(cd) == sorted(cn)
    for k in cd:
        assert counts_close(np.array([cd[k]]), np.array([cn[k]])), (k, cd[k], cn[k])
    pd, ld = boss.mergedTwoPosteriors(m, profs, pb, "device", params=par, band=2)
    pn, ln = boss.mergedTwoPosteriors(m, profs, pb, "numpy", params=par, band=2)
    assert logs_close(ld, ln) and logs_close(ld, sn["loglike"])
    for (ga, gb), (wa, wb) in zip(pd, pn):
        assert counts_close(ga, wa) and counts_close(gb, wb)


def test_merged_two_profile_loglike_on_the_device():
    import torch
    from machineboss_amd.torchprofile import merged_two_profile_loglike
    em, colTok, A0, B0 = tq.fd_case()
    A1, B1 = tm.merged_input(np.random.RandomState(4), em, 3, 2, 2, pInf=0.0)
    A, B, inOff, rowOff = np.concatenate([A0, A1]), np.concatenate([B0, B1]), [0, 3, 5], [0, 3, 5]
    envs = [Envelope.band(3, 3, 1), None]
    weights = torch.tensor([1.0, -2.5], dtype=torch.float64)
    out = {}
    for backend in ("numpy", "device"):
        logA = torch.tensor(A, dtype=torch.float64, requires_grad=True)
        logB = torch.tensor(B, dtype=torch.float64, requires_grad=True)
        ll = merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, envs=envs, backend=backend)
        (ll * weights).sum().backward()
        out[backend] = (ll.detach().numpy(), logA.grad.numpy(), logB.grad.numpy())
    assert capi.last_kernel_name() == "k_profile_two_merge_env_rowpost"
    assert logs_close(out["device"][0], out["numpy"][0]) and np.isfinite(out["numpy"][0]).all()
    for g, w in zip(out["device"][1:], out["numpy"][1:]):
        assert counts_close(np.abs(g), np.abs(w)) and np.array_equal(np.sign(g), np.sign(w))
    # a one-hot input and the echo transducer: CTC under the full envelope, never above it under a band
    echo = capi.DeviceMachine(tq.echo_machine())
    K = len(tq.CTC_X)
    logA = torch.tensor(th.one_hot(tq.CTC_X, 3), dtype=torch.float64)
    try:
        for T in tq.CTC_T:
            lp = tq.ctc_frames(T, True)
            loss, grad = tq.ctc_reference(lp)
            t = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
            ll = merged_two_profile_loglike(echo, logA, [0, K], t, [0, T], tq.CTC_COLTOK, envs=[full(K, T)])
            if not math.isfinite(loss):
                assert ll.item() == -math.inf
                continue
            ll.sum().backward()
            assert logs_close([-ll.item()], [loss]), (T, ll.item(), loss)
            assert counts_close(t.grad.numpy(), np.exp(lp) - grad), np.abs(t.grad.numpy() - (np.exp(lp) - grad)).max()
            for w in range(0, 4):
                try:
                    env = Envelope.band(K, T, w)
                except Exception:
                    continue
                b = merged_two_profile_loglike(echo, logA, [0, K], torch.tensor(lp), [0, T], tq.CTC_COLTOK, envs=[env]).item()
                assert b <= ll.item() + 1e-9 * max(1.0, abs(ll.item())), (T, w, b, ll.item())
    finally:
        echo.close()
