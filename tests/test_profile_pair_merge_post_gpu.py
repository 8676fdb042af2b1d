"""GPU tests of the row posteriors of pairs against CTC-merged profiles (k_profile_pair_merge_rowpost in mb_profile_pair_merge.hip;
docs/profile_tapes.md, "Row posteriors of pairs against a merged profile"): capi.DeviceProfilePairs.merged_row_posteriors() against
profile.PairMergedProfileDP.rowPosteriors at the places where the kernel changes form -- one wavefront of many cells and planes
(S = 1), wavefronts that hold exactly one (cell, plane) (S = 64) and one lane more (S = 65), more bins than a wavefront has lanes,
more row blocks than a pair has groups, a table too small for a row, chunks -- and against the device itself: grouped counts(), the
one-tape merged sweeps at I = 0, central differences of forward(), the CTC loss.  Inputs and bounds: pairmergeposthelpers; what the
tests assume of the inputs is held to the yardstick by test_profile_pair_merge_post_host.py::test_gpu_suite_inputs_are_live."""
import math

import numpy as np
import pytest
import torch

import pairmergehelpers as mh
import pairmergeposthelpers as pp
from pairmergeposthelpers import compare, yardstick
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import capi
from machineboss_amd.profile import PairMergedProfileDP
from machineboss_amd.torchprofile import pair_profile_loglike

pytestmark = pytest.mark.gpu
KERNEL = "k_profile_pair_merge_rowpost"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the merged pair posteriors:", pp.WORST)


def _open(em, colTok, pairs):
    dm = capi.DeviceMachine(em)
    return dm, capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs], colTok)


def _split(dev, post):
    return [post[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)]


def _check(em, colTok, pairs, launches=None, refs=None):
    refs = yardstick(em, colTok, pairs) if refs is None else refs
    dm, dev = _open(em, colTok, pairs)
    try:
        post, ll = dev.merged_row_posteriors()
        assert capi.last_kernel_name() == KERNEL
        if launches is not None:
            assert capi.last_launch_count() == launches
        assert post.shape == (dev.rowOff[-1], len(colTok) + 1)
        got = _split(dev, post)
        compare(got, ll, refs)
    finally:
        dev.close(); dm.close()
    return got, ll, refs


# ---- 1. the suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", pp.LANE_CASES)
def test_lane_cases_against_the_yardstick(nCols, S):
    """The seven SHAPES on the machine with silent levels and without, each machine's pairs in one batch: L = 0 gives an empty
    result, I = 0 a single cell a row; (1, 1) and (2, 1) put many cells and planes in a wavefront, (4, 65) one lane more than a
    wavefront a plane, (63, 2) and (65, 2) rows of 64 and 66 bins."""
    live = []
    for em, colTok, pairs in pp.lane_case(nCols, S):
        got, ll, _ = _check(em, colTok, pairs, launches=1)
        assert [g.shape[0] for g in got] == [L for _, L in pp.SHAPES]
        live += list(ll > -math.inf)
    assert np.mean(live) >= 0.85, np.mean(live)


def test_wavefronts_of_one_cell_and_plane():
    em, colTok, pairs = pp.wave_case()
    _, ll, _ = _check(em, colTok, pairs, launches=1)
    assert (ll > -math.inf).all()


@pytest.fixture(scope="module")
def wrap():
    em, colTok, pairs = pp.wrap_case()
    return em, colTok, pairs, yardstick(em, colTok, pairs)


@pytest.mark.parametrize("table", ("5", "2", None))
def test_more_row_blocks_than_groups(wrap, table):
    """(1, 1 100) at S = 2 beside a dead pair of the same shape.  A table of 5 doubles: one row a block, 1 100 blocks for 1 024
    groups, so 76 groups take a second block and must clear the table between them; 2: the global bins; the default: three blocks."""
    em, colTok, pairs, refs = wrap
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        got, ll, _ = _check(em, colTok, pairs, launches=1, refs=refs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert ll[0] > -math.inf and ll[1] == -math.inf and not got[1].any() and got[1].shape == (1100, 5) and (got[0][1024:] > 0).any()


@pytest.mark.parametrize("table", (None, "16"))
def test_more_bins_than_lanes(table):
    """nCols = 65 at S = 2: 66 bins a row, in the full table and, with a table of 16 doubles, in their global bins."""
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        for em, colTok, pairs in pp.wide_case():
            got, ll, _ = _check(em, colTok, pairs, launches=1)
            assert (ll > -math.inf).sum() >= 6 and got[-1].shape == (9, 66)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)


def test_ragged_batch_with_a_dead_pair():
    """The ring shapes of pairmergehelpers (X / T rings in LDS and in global scratch), an empty input, an empty profile, a dead pair."""
    em, colTok, pairs = pp.ragged_post_case()
    got, ll, _ = _check(em, colTok, pairs, launches=1)
    assert ll[-1] == -math.inf and not got[-1].any() and got[-1].shape == (4, 5) and (ll[:-1] > -math.inf).all()
    assert got[mh.RAGGED_SHAPES.index((40, 0))].shape == (0, 5)


def test_infinite_weights_give_exact_zeros():
    em, colTok, pairs = pp.third_inf_case()
    got, ll, _ = _check(em, colTok, pairs, launches=1)
    assert (ll > -math.inf).sum() >= 3
    for g, (_, P) in zip(got, pairs):
        assert (P == -math.inf).any() and not g[P == -math.inf].any()


@pytest.mark.parametrize("name", ("allblank", "infrow", "infweights"))
def test_rows_of_blanks_and_a_row_of_nothing(name):
    em, colTok, pairs = mh.row_cases()[name]
    got, ll, _ = _check(em, colTok, pairs, launches=1)
    if name == "allblank":
        assert (ll > -math.inf).all() and not any(g[:, 1:].any() for g in got)
    if name == "infrow":
        assert ll[1] == -math.inf and not got[1].any()


def test_lattice_far_below_zero():
    em, colTok, pairs = pp.far_case()
    got, ll, _ = _check(em, colTok, pairs, launches=1)
    assert ll[0] > -math.inf and ll[1] < -6000 and np.abs(got[1].sum(axis=1) - 1.0).max() <= pp.ROW_TOL
    assert counts_close(got[1], got[0])


@pytest.mark.parametrize("name", ("two", "same", "unused", "one"))
def test_column_maps(name):
    em, colTok, pairs = mh.column_map_cases()[name]
    got, ll, _ = _check(em, colTok, pairs, launches=1)
    assert (ll > -math.inf).sum() >= len(pairs) - 1
    if name == "unused":
        assert not any(g[:, 2].any() for g in got)      # nothing emits token 3: its column is never taken


# ---- 2. chunks and the fixed point ------------------------------------------------------------------------------------------------------
def test_chunking_and_the_same_bits():
    em, colTok, pairs = pp.chunk_case()
    refs = yardstick(em, colTok, pairs)
    dm, dev = _open(em, colTok, pairs)
    budget = pp.chunk_budget()
    try:
        p0, l0 = dev.merged_row_posteriors()
        assert capi.last_launch_count() == 1
        compare(_split(dev, p0), l0, refs)
        capi.set_memory_budget(budget)
        p1, l1 = dev.merged_row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert np.array_equal(l0, l1)
        compare(_split(dev, p1), l1, refs)
        capi.set_option("MB_DETERMINISTIC", "1")
        d0, _ = dev.merged_row_posteriors()
        d0b, _ = dev.merged_row_posteriors()
        capi.set_memory_budget(budget)
        d1, _ = dev.merged_row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert np.array_equal(d0, d0b) and np.array_equal(d0, d1)
        compare(_split(dev, d0), l0, refs, "fixed point")
        for table in ("5", "3", "40"):      # a row a block, global bins, eight rows a block
            capi.set_option("MB_ROWPOST_TABLE", table)
            assert np.array_equal(dev.merged_row_posteriors()[0], d0), table
        capi.set_option("MB_ROWPOST_TABLE", None)
        for k in (0, 1, 4):
            _, one = _open(em, colTok, pairs[k:k + 1])
            try:
                assert np.array_equal(one.merged_row_posteriors()[0], d0[dev.rowOff[k]:dev.rowOff[k + 1]]), k
            finally:
                one.close()
        capi.set_memory_budget(1024)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.merged_row_posteriors()
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        capi.set_option("MB_ROWPOST_TABLE", None)
        dev.close(); dm.close()


# ---- 3. the device against itself -------------------------------------------------------------------------------------------------------
def test_fresh_column_sums_are_the_grouped_counts():
    """sum_r (post - repeats)[r][c] over the columns of a token against counts() of the same object added up by token: the repeats
    are the yardstick's (they are not edges), and the same call's likelihoods are the bits of counts()'."""
    em, colTok, pairs = pp.ragged_post_case()
    dp = PairMergedProfileDP(em, colTok)
    rep = []
    for x, P in pairs:
        dp.rowPosteriors(x, P, repeats=rep)
    dm, dev = _open(em, colTok, pairs)
    try:
        post, ll = dev.merged_row_posteriors()
        c, _, ll2 = dev.counts()
        assert np.array_equal(ll, ll2)
        got, want = pp.by_token(em, colTok, (post - np.concatenate(rep)).sum(axis=0)[1:]), pp.grouped(em, colTok, c)
        # the entries of post are within 1e-6 relative, so the difference is within 1e-6 of the sums it was taken from, on top of the counts' own bound
        bound = 1e-6 * pp.by_token(em, colTok, post.sum(axis=0)[1:]) + 1e-9 + 1e-6 * want
        pp.WORST["grouped counts"] = float(np.abs(got - want).max())
        assert (np.abs(got - want) <= bound).all() and want.any(), (got, want)
    finally:
        dev.close(); dm.close()


def test_no_input_equals_device_profiles():
    """A generator (no input alphabet) against merged profiles of 0, 1, 9 and 23 rows: the pairs with I = 0 against
    capi.DeviceProfiles(dm, profiles, colTok).row_posteriors()."""
    from randmachine import random_machine
    em = random_machine(40, 0, 3, 31)
    profs = [mh.merged_input(np.random.RandomState(31 + L), em, 4, 0, L)[1] for L in (0, 1, 9, 23)]
    dm = capi.DeviceMachine(em)
    a = capi.DeviceProfilePairs(dm, [[]] * len(profs), profs, pp.WAVE_COLTOK)
    b = capi.DeviceProfiles(dm, profs, pp.WAVE_COLTOK)
    try:
        pa, la = a.merged_row_posteriors()
        pb, lb = b.row_posteriors()
        assert logs_close(la, lb, 1e-12) and (la > -math.inf).any()
        assert counts_close(pa, pb) and not pa[pb == 0.0].any(), np.abs(pa - pb).max()
    finally:
        a.close(); b.close(); dm.close()


def test_finite_differences_of_the_device_forward():
    """All 2 L (nCols + 1) perturbed profiles of one (3, 3) pair at S = 8 as one batch, one launch of the rolling Forward."""
    em, colTok, x, P = pp.fd_case()
    L, C = P.shape
    profs = []
    for r in range(L):
        for c in range(C):
            for sgn in (1.0, -1.0):
                Q = P.copy(); Q[r, c] += sgn * pp.FD_H
                profs.append(Q)
    dm = capi.DeviceMachine(em)
    many = capi.DeviceProfilePairs(dm, [x] * len(profs), profs, colTok)
    one = capi.DeviceProfilePairs(dm, [x], [P], colTok)
    try:
        f = many.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and len(f) == 2 * L * C
        post, ll = one.merged_row_posteriors()
        assert abs(ll[0]) < 100
        fd = ((f[0::2] - f[1::2]) / (2 * pp.FD_H)).reshape(L, C)
        pp.WORST["finite differences"] = float(np.abs(fd - post).max())
        print("central differences of the device Forward off by at most %.3g" % pp.WORST["finite differences"])
        assert np.abs(fd - post).max() <= pp.FD_TOL, (fd, post)
    finally:
        many.close(); one.close(); dm.close()


@pytest.mark.parametrize("normalised", (True, False))
def test_ctc_loss_through_the_autograd_function(normalised):
    """The echo transducer on x = 1 2 2 3 against T = 3, 4, 7, 12 frames in one batch: -inf and zero gradients below five frames,
    -ctc_loss and exp(lp) - d ctc_loss / d lp from seven up."""
    frames = [pp.ctc_frames(T, normalised) for T in pp.CTC_T]
    rowOff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    logP = torch.tensor(np.concatenate(frames), dtype=torch.float64, requires_grad=True)
    ll = pair_profile_loglike(pp.echo_machine(), [pp.CTC_X] * len(frames), logP, rowOff, backend="device", colTok=pp.CTC_COLTOK)
    assert capi.last_kernel_name() == KERNEL
    ll[2:].sum().backward()
    grad, ll = logP.grad.numpy(), ll.detach().numpy()
    for k, lp in enumerate(frames):
        loss, g = pp.ctc_reference(lp)
        mine = grad[rowOff[k]:rowOff[k + 1]]
        if len(lp) < 5:
            assert float(ll[k]) == -math.inf and loss == math.inf and not mine.any()
            continue
        assert abs(float(ll[k]) + loss) <= 1e-9 * max(1.0, abs(loss)), (float(ll[k]), loss)
        assert counts_close(mine, np.exp(lp) - g), np.abs(mine - (np.exp(lp) - g)).max()


def test_the_other_calls_keep_their_bits():
    """Forward, Viterbi with paths and counts of one object before and after a merged_row_posteriors() call."""
    em, colTok, pairs = pp.chunk_case()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = _open(em, colTok, pairs)
    try:
        def everything():
            return [dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)] + list(dev.viterbi()) + list(dev.counts())
        before = everything()
        dev.merged_row_posteriors()
        after = everything()
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(before, after))
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_merged_pair_posteriors_on_the_device():
    """boss.mergedPairPosteriors on dnastore4 against the merged tiny profile: the device against the numpy backend, with an input
    that cannot be tokenised (zeros, -inf) and an empty one."""
    from machineboss_amd import boss
    from machineboss_amd.machine import Machine
    from machineboss_amd.profile import Profile
    m = Machine.fromFile("tests/golden/machine/dnastore4.json")
    par, prof = m.getParamDefs(True), Profile.fromCsv("tests/golden/csv/tiny_uc.csv")
    seqs = [["0_3", "2_3", "1_3"], ["nonsense"], [], ["1_3", "1_3"]]
    want, wl = boss.mergedPairPosteriors(m, seqs, prof, backend="numpy", params=par)
    got, ll = boss.mergedPairPosteriors(m, seqs, prof, backend="device", params=par)
    assert capi.last_kernel_name() == KERNEL and ll[1] == -math.inf and not got[1].any() and sum(v > -math.inf for v in wl) >= 2
    compare(got, np.array(ll), list(zip(want, wl)))


# ---- 4. new rows and refusals -----------------------------------------------------------------------------------------------------------
def test_set_merged_profiles():
    em, colTok, old = pp.chunk_case()
    rng = np.random.RandomState(77)
    new = [(x, mh.merged_input(rng, em, 4, len(x), len(P))[1]) for x, P in old]
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = _open(em, colTok, old)
    _, fresh = _open(em, colTok, new)
    try:
        p_old, _ = dev.merged_row_posteriors()
        dev.set_merged_profiles([P for _, P in new])
        p_new, l_new = dev.merged_row_posteriors()
        want, wl = fresh.merged_row_posteriors()
        assert np.array_equal(p_new, want) and np.array_equal(l_new, wl) and not np.array_equal(p_new, p_old)
        assert np.array_equal(dev.forward(), fresh.forward()) and np.array_equal(dev.counts()[0], fresh.counts()[0])
        compare(_split(dev, p_new), l_new, yardstick(em, colTok, new), "fixed point")
        bad = [P.copy() for _, P in old]
        bad[2][1, 1] = np.nan
        dev.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="NaN"):
            dev.set_merged_profiles(bad)
        bad[2][1, 1] = np.inf
        with pytest.raises(capi.MbError, match="infinity"):
            dev.set_merged_profiles(bad)
        assert capi.last_launch_count() == n
        with pytest.raises(ValueError):
            dev.set_merged_profiles([P for _, P in old][:2])
        assert np.array_equal(dev.merged_row_posteriors()[0], want)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); fresh.close(); dm.close()


def test_plain_objects_are_refused():
    from pairprofilehelpers import pair_input, pair_machine
    em = pair_machine(8, 108, True, 2, 3)
    x, P = pair_input(np.random.RandomState(8), em, 2, 4)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x], [P])
    try:
        dev.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="merged row posteriors take merged profiles"):
            dev.merged_row_posteriors()
        with pytest.raises(capi.MbError, match="merged row posteriors take merged profiles"):
            dev.set_merged_profiles([P])
        assert capi.last_launch_count() == n
    finally:
        dev.close(); dm.close()
