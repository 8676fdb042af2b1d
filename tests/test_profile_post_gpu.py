"""GPU tests of the row posteriors of the one-tape profile sweeps (k_profile_rowpost<MERGED> in mb_profile_post.hip;
docs/profile_tapes.md, "Row posteriors of one-tape profiles"): capi.DeviceProfiles.row_posteriors() against the yardsticks
profile.ProfileDP.rowPosteriors and profile.MergedProfileDP.rowPosteriors over the inputs of profileposthelpers, at the places where
the kernel changes form -- many rows in one wavefront (S = 1), one wavefront per row and one lane either side (S = 63, 64, 65),
several row blocks, more blocks than groups, a table too small for a row, more columns than lanes, planes on either side of a
wavefront -- in batches, chunks and under MB_DETERMINISTIC, and against the device itself: grouped counts(), finite differences of
forward(), the pair sweep at an empty input, torch's CTC loss.

Bounds (pairprofilehelpers): entries as counts, 1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; likelihoods 1e-9 relative
to max(1, |value|); -inf entries and dead profiles exactly 0; row sums 1e-6; central differences at h = 1e-6 within 1e-7 absolute
(truncation about h^2, rounding about 2 ulp(LL) / 2h < 1e-8)."""
import math

import numpy as np
import pytest
import torch

import pairprofilehelpers as ph
import profileposthelpers as h
from pairprofilehelpers import counts_close, logs_close
from profileposthelpers import FD_H, FD_TOL, ROW_TOL
from machineboss_amd import capi
from machineboss_amd.torchprofile import profile_loglike

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the one-tape row posteriors:", WORST)


def _open(em, colTok, profs):
    dm = capi.DeviceMachine(em)
    return dm, capi.DeviceProfiles(dm, profs, colTok)


def _split(dev, post):
    return [post[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nProfiles)]


def _yardstick(em, colTok, profs):
    dp = h.yardstick(em, colTok)
    return [dp.rowPosteriors(P) for P in profs]


def _name(colTok):
    return "k_profile_rowpost" if colTok is None else "k_profile_merge_rowpost"


def _compare(got, ll, refs, what="posteriors"):
    """The device's per-profile posteriors and likelihoods against the yardstick's: entries, exact zeros, row sums."""
    want = np.array([r[1] for r in refs])
    ph.note("loglike", ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    for k, (g, (w, wl)) in enumerate(zip(got, refs)):
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if not g.size:
            continue
        ph.note_counts(g.ravel(), w.ravel(), WORST, what)
        assert counts_close(g, w), (k, np.abs(g - w).max())
        assert not g[w == 0.0].any() and (g >= 0.0).all(), k
        if wl > -math.inf:
            WORST["row sums"] = max(WORST.get("row sums", 0.0), float(np.abs(g.sum(axis=1) - 1.0).max()))
            assert np.abs(g.sum(axis=1) - 1.0).max() <= ROW_TOL, (k, g.sum(axis=1))
        else:
            assert not g.any(), k


def _check(em, colTok, profs, launches=1, what="posteriors"):
    refs = _yardstick(em, colTok, profs)
    dm, dev = _open(em, colTok, profs)
    try:
        post, ll = dev.row_posteriors()
        assert capi.last_kernel_name() == _name(colTok)
        if launches is not None:
            assert capi.last_launch_count() == launches
        assert post.shape == (dev.rowOff[-1], em.nOutTok + 1 if colTok is None else len(colTok) + 1)
        got = _split(dev, post)
        _compare(got, ll, refs, what)
        for g, P in zip(got, profs):
            assert not g[P == -math.inf].any()
    finally:
        dev.close(); dm.close()
    return got, ll, refs


# ---- 1. plain profiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,silent", [(S, v) for S in h.GPU_STATES for v in ((True, False) if S >= 2 else (False,))])
def test_plain_suite_against_the_yardstick(S, silent):
    """L = 0, 1, 2, 9 in one batch.  S = 1 and 2 put many rows in a wavefront, 63, 64 and 65 lie around one wavefront per row, 300
    takes five wavefronts a row with a seam in the last."""
    em, profs = h.gpu_plain_case(S, silent)
    got, ll, _ = _check(em, None, profs)
    assert [len(g) for g in got] == list(h.GPU_LENGTHS) and np.mean(ll > -math.inf) >= 0.75


def test_every_lane_its_own_row():
    em, profs = h.one_lane_rows_case()
    got, ll, _ = _check(em, None, profs)
    assert em.nStates == 1 and got[0].shape == (200, 4) and ll[0] > -math.inf


def test_several_row_blocks():
    em, profs = h.row_blocks_case()
    got, ll, _ = _check(em, None, profs)
    assert em.nStates == 40 and got[0].shape == (300, 4) and ll[0] > -math.inf


# ---- 2. merged profiles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", h.GPU_MERGED)
def test_merged_suite_against_the_yardstick(nCols, S):
    """One column; two; planes x states below, at and above a wavefront; 64 and 66 planes of two states."""
    em, colTok, profs = h.gpu_merged_case(nCols, S)
    assert em.nStates == S and len(colTok) == nCols and max(len(P) for P in profs) == 9
    got, ll, _ = _check(em, colTok, profs)
    assert np.mean(ll > -math.inf) >= 0.5


# ---- 3. the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
def test_one_row_a_block_and_more_blocks_than_groups(merged):
    """S = 2 at L = 1 100 with four columns: a table of 4 doubles holds one row, so the profile has 1 100 blocks for its 1 024 groups
    and the first 76 groups take a second one; the full table gives the same posteriors."""
    em, colTok, profs = h.many_blocks_case(merged)
    full, ll, _ = _check(em, colTok, profs)
    capi.set_option("MB_ROWPOST_TABLE", "4")
    try:
        got, _, _ = _check(em, colTok, profs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert ll[0] > -math.inf and got[0].shape == (1100, 4) and counts_close(got[0], full[0])


@pytest.mark.parametrize("merged", (False, True))
def test_rows_wider_than_the_table_are_summed_in_global_bins(merged):
    """A table of 2 doubles is narrower than a row of 4 or 5 columns: the owning workgroup clears the row's global bins and adds
    into them.  The ragged batch: ten profiles, one of no rows, one dead."""
    em, colTok, profs = h.ragged_case(merged)
    capi.set_option("MB_ROWPOST_TABLE", "2")
    try:
        got, ll, _ = _check(em, colTok, profs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert ll[5] == -math.inf and not got[5].any() and got[2].shape[0] == 0


@pytest.mark.parametrize("table", (None, "16"))
def test_more_columns_than_lanes(table):
    """71 columns at S = 2: with the full table 57 rows a block, with one of 16 doubles the global bins."""
    em, profs = h.wide_alphabet_case()
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        got, ll, _ = _check(em, None, profs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert (ll > -math.inf).all() and got[0].shape == (5, 71)


# ---- 4. batches, chunks, fixed point ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
def test_ragged_batch_chunks_and_the_same_bits(merged):
    """Ten profiles, the third empty and the sixth dead, in one launch; then under a budget of 1.8 x the largest profile's bytes in
    several, and under MB_DETERMINISTIC=1 the same bits chunked or not, from call to call, alone or in the batch, with any table."""
    em, colTok, profs = h.ragged_case(merged)
    got, ll, refs = _check(em, colTok, profs)
    assert ll[5] == -math.inf and ll[2] == -math.inf and not got[5].any() and got[5].shape[0] == 6 and np.sum(ll > -math.inf) == 8
    budget = int(1.8 * max(h.post_bytes(em, colTok, P) for P in profs))
    dm, dev = _open(em, colTok, profs)
    try:
        p0, l0 = dev.row_posteriors()
        capi.set_memory_budget(budget)
        p1, l1 = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert np.array_equal(l0, l1) and counts_close(p1, p0)
        capi.set_option("MB_DETERMINISTIC", "1")
        d0, dl = dev.row_posteriors()
        d0b, _ = dev.row_posteriors()
        capi.set_memory_budget(budget)
        d1, _ = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        capi.set_option("MB_ROWPOST_TABLE", "8")
        d2, _ = dev.row_posteriors()
        capi.set_option("MB_ROWPOST_TABLE", "2")
        d3, _ = dev.row_posteriors()
        capi.set_option("MB_ROWPOST_TABLE", None)
        assert np.array_equal(d0, d0b) and np.array_equal(d0, d1) and np.array_equal(d0, d2) and np.array_equal(d0, d3)
        assert np.array_equal(dl, l0)
        _compare(_split(dev, d0), dl, refs, "fixed point")
        for k in (0, 3, 5):
            one = capi.DeviceProfiles(dm, [profs[k]], colTok)
            try:
                p, l = one.row_posteriors()
            finally:
                one.close()
            assert np.array_equal(p, d0[dev.rowOff[k]:dev.rowOff[k + 1]]) and l[0] == dl[k], k
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        capi.set_option("MB_ROWPOST_TABLE", None)
        dev.close(); dm.close()


def test_a_profile_beyond_the_budget_is_refused_before_any_launch():
    em, _, profs = h.ragged_case(False)
    dm, dev = _open(em, None, profs)
    try:
        dev.forward()
        n = capi.last_launch_count()
        capi.set_memory_budget(h.post_bytes(em, None, profs[3]) - 8)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.row_posteriors()
        assert capi.last_launch_count() == 0 and n == 1
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


@pytest.mark.parametrize("merged", (False, True))
def test_set_profiles(merged):
    em, colTok, old = h.ragged_case(merged)
    rng = np.random.RandomState(77)
    new = [h.long_rows(rng, P.shape[1], len(P)) for P in old]
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = _open(em, colTok, old)
    fresh = capi.DeviceProfiles(dm, new, colTok)
    try:
        p_old, _ = dev.row_posteriors()
        dev.set_profiles(new)
        p_new, l_new = dev.row_posteriors()
        want, wl = fresh.row_posteriors()
        assert np.array_equal(p_new, want) and np.array_equal(l_new, wl) and not np.array_equal(p_new, p_old)
        assert np.array_equal(dev.forward(), fresh.forward()) and np.array_equal(dev.counts()[0], fresh.counts()[0])
        _compare(_split(dev, p_new), l_new, _yardstick(em, colTok, new), "fixed point")
        bad = [P.copy() for P in old]
        bad[3][1, 1] = np.nan
        dev.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="NaN"):
            dev.set_profiles(bad)
        assert capi.last_launch_count() == n
        with pytest.raises(ValueError):
            dev.set_profiles(old[:2])
        assert np.array_equal(dev.row_posteriors()[0], want)      # the refused table left the rows in effect
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        fresh.close(); dev.close(); dm.close()


# ---- 5. hard weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(h.hard_cases()))
def test_hard_weights(name):
    """A third of the weights -inf; a row all -inf; rows of the blank alone; every entry 700 lower."""
    em, colTok, profs = h.hard_cases()[name]
    got, ll, _ = _check(em, colTok, profs)
    if name.startswith("infrow"):
        assert ll[1] == -math.inf and not got[1].any() and ll[0] > -math.inf
    if name.startswith("allblank"):
        assert ll[0] > -math.inf and np.abs(got[0][:, 0] - 1.0).max() <= ROW_TOL and not got[0][:, 1:].any()
    if name.startswith("far"):
        assert ll[1] < -6000 and np.abs(got[1].sum(axis=1) - 1.0).max() <= ROW_TOL and counts_close(got[1], got[0])


# ---- 6. the device against itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
def test_column_sums_are_the_grouped_counts_of_the_same_object(merged):
    """sum_r post[r][o] over the batch against counts() added up by output token; merged: the fresh-emission part, the repeat part
    being the yardstick's (the device returns the sum of both)."""
    em, colTok, profs = h.ragged_case(merged)
    dm, dev = _open(em, colTok, profs)
    try:
        post, ll = dev.row_posteriors()
        c, _, ll2 = dev.counts()
        assert np.array_equal(ll, ll2)
        if merged:
            dp = h.yardstick(em, colTok)
            rep = []
            for P in profs:
                dp.rowPosteriors(P, rep)
            cols = h.by_token(em, colTok, (post - np.concatenate(rep)).sum(axis=0))
        else:
            cols = post.sum(axis=0)[1:]
        assert counts_close(cols, h.grouped(em, c)), (cols, h.grouped(em, c))
    finally:
        dev.close(); dm.close()


@pytest.mark.parametrize("merged", (False, True))
def test_finite_differences_of_the_device_forward(merged):
    """All 2 L C perturbed profiles of one profile of three rows at S = 8 as one batch, one launch of the rolling Forward."""
    em = h.post_machine(8, 3, True, 708)
    colTok = [1, 2, 3, 1] if merged else None
    P = h.long_rows(np.random.RandomState(3 + merged), 5 if merged else 4, 3)
    L, C = P.shape
    profs = []
    for r in range(L):
        for o in range(C):
            for sgn in (1.0, -1.0):
                Q = P.copy(); Q[r, o] += sgn * FD_H
                profs.append(Q)
    dm = capi.DeviceMachine(em)
    many = capi.DeviceProfiles(dm, profs, colTok)
    one = capi.DeviceProfiles(dm, [P], colTok)
    try:
        f = many.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and len(f) == 2 * L * C
        post, ll = one.row_posteriors()
        assert abs(ll[0]) < 100
        fd = ((f[0::2] - f[1::2]) / (2 * FD_H)).reshape(L, C)
        WORST["finite differences"] = max(WORST.get("finite differences", 0.0), float(np.abs(fd - post).max()))
        print("central differences of the device Forward off by at most %.3g" % WORST["finite differences"])
        assert np.abs(fd - post).max() <= FD_TOL, (fd, post)
    finally:
        many.close(); one.close(); dm.close()


def test_plain_posteriors_equal_the_pair_sweep_at_an_empty_input():
    em, _, profs = h.ragged_case(False)
    dm, dev = _open(em, None, profs)
    pairs = capi.DeviceProfilePairs(dm, [[]] * len(profs), profs)
    try:
        post, ll = dev.row_posteriors()
        want, wl = pairs.row_posteriors()
        assert capi.last_kernel_name() == "k_profile_pair_rowpost"
        assert logs_close(ll, wl, 1e-12) and counts_close(post, want) and not post[want == 0.0].any()
    finally:
        pairs.close(); dev.close(); dm.close()


# ---- 7. CTC ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalised", (True, False))
def test_ctc_loss_and_gradient_on_the_device(normalised):
    """The chain generator of y = [1, 2, 2, 3] against frames of T = 3, 4, 7, 12 in one batch through profile_loglike: -ctc_loss per
    profile and, after backward(), exp(lp) - d ctc_loss / d lp of torch's CPU loss; the infeasible T = 3 and 4 score -inf with
    zeros."""
    em = h.ctc_machine()
    frames = [h.ctc_frames(T, normalised) for T in h.CTC_FRAMES]
    refs = [h.ctc_reference(lp) for lp in frames]
    rowOff = np.concatenate([[0], np.cumsum(h.CTC_FRAMES)])
    logP = torch.cat(frames).clone().requires_grad_(True)
    ll = profile_loglike(em, logP, rowOff, h.CTC_COLTOK, backend="device")
    assert capi.last_kernel_name() == "k_profile_merge_rowpost"
    mask = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64)      # (-inf times 0 is NaN: sum the finite ones)
    (torch.where(mask > 0, ll, torch.zeros_like(ll))).sum().backward()
    got = logP.grad.numpy()
    want = np.array([r[0] for r in refs])
    ph.note("ctc loglike", ll.detach().numpy(), want, WORST)
    assert logs_close(ll.detach().numpy(), want) and list(want[:2]) == [-math.inf, -math.inf] and np.isfinite(want[2:]).all()
    for k, (_, w) in enumerate(refs):
        g = got[rowOff[k]:rowOff[k + 1]]
        if k < 2:
            assert not g.any()
        else:
            ph.note_counts(g.ravel(), w.ravel(), WORST, "ctc gradient")
            assert counts_close(g, w), (k, np.abs(g - w).max())
    dm = capi.DeviceMachine(em)
    try:
        l2 = profile_loglike(dm, logP.detach(), rowOff, h.CTC_COLTOK)
        assert np.array_equal(l2.numpy(), ll.detach().numpy())
    finally:
        dm.close()


# ---- 8. the existing calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
def test_existing_sweeps_keep_their_bits_around_the_new_call(merged):
    """forward (rolling and materialised), viterbi with paths and counts of one object before and after row_posteriors(), which
    shares the workspace with them."""
    em, colTok, profs = h.ragged_case(merged)
    dm, dev = _open(em, colTok, profs)

    def sweeps():
        v = dev.viterbi()
        c = dev.counts()
        return [dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), v[0], v[1], v[2], v[3], c[0], np.array([c[1]]), c[2]]
    try:
        before = sweeps()
        post, ll = dev.row_posteriors()
        after = sweeps()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert np.array_equal(ll, before[1]) and np.array_equal(dev.row_posteriors()[1], ll)
    finally:
        dev.close(); dm.close()
