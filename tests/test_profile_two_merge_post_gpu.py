"""GPU tests of the row posteriors of the two-profile sweeps against CTC-merged output profiles (k_profile_two_merge_rowpost in
mb_profile_two_merge.hip; docs/profile_tapes.md, "Row posteriors of pairs of profiles against a merged profile"):
capi.DeviceProfileTwos.merged_row_posteriors() against profile.TwoMergedProfileDP.mergedRowPosteriors at the smallest shapes at which
each path of the kernel can go wrong -- lanes that share a wavefront with other cells, planes and lines, wavefronts of exactly one
(cell, plane), more blocks than a pair has workgroups, lines wider than a wavefront and wider than the table, a ragged batch whose
X / T scratch lies in LDS and in global memory, chunks -- and against the device itself: grouped counts(), the pair sweep under a
one-hot input, the one-tape sweep at K = 0, finite differences of forward().  The inputs are those of twomergeposthelpers, held to
their conditions without a GPU by test_profile_two_merge_post_host.py::test_gpu_inputs_are_live.

Bounds (twomergeposthelpers): entries as counts, 1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; likelihoods 1e-9 relative
to max(1, |value|); row sums 1e-6; -inf weights and dead pairs exactly 0; central differences at h = 1e-6 within 1e-7 absolute.  In
fixed point a lane sum is rounded once to the nearest 2^-36, so a bin fed by n items -- (K + 1)(nCols + 1) S for an output row,
(L + 1)(nCols + 1) S for an input row -- may be off by n 2^-37 more, and a row sum by that of its bins."""
import math

import numpy as np
import pytest
import torch

import twomergehelpers as tm
import twomergeposthelpers as tq
import twoprofilehelpers as th
from pairprofilehelpers import counts_close, logs_close
from twomergeposthelpers import FD_H, FD_TOL, ROW_TOL, WORST, check, compare, open_pairs, split, yardstick
from machineboss_amd import boss, capi
from machineboss_amd.torchprofile import merged_two_profile_loglike

pytestmark = pytest.mark.gpu
KERNEL = "k_profile_two_merge_rowpost"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the merged two-profile row posteriors:", WORST)


# ---- 1. lanes, wavefronts, blocks, wide lines -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", tm.LANE_CASES)
def test_lane_cases_against_the_yardstick(nCols, S):
    """The seven lattices on the machine with silent levels and without, each machine's pairs in one batch.  K = 0 and L = 0 give
    empty tables; at S = 1 and 2 a wavefront holds many cells and planes, at 13 and 65 planes and cells end inside a wavefront, at 63
    and 65 columns a line has a bin per lane and one more."""
    colTok, cases = tq.lane_case(nCols, S)
    live = []
    for em in {id(c[0]): c[0] for c in cases}.values():
        pairs = [(A, B) for e, A, B in cases if e is em]
        gotA, gotB, ll, _ = check(em, colTok, pairs, launches=1)
        assert [(len(a), len(b)) for a, b in zip(gotA, gotB)] == list(tq.SHAPES)
        live += list(ll > -math.inf)
    assert np.mean(live) >= 0.8, np.mean(live)


def test_whole_wavefronts():
    """nCols = 4, S = 64 at (2, 5) and (5, 2): every wavefront is one (cell, plane) of one line, the butterfly on every item."""
    em, colTok, pairs = tq.wave_case()
    gotA, gotB, ll, refs = check(em, colTok, pairs, launches=1)
    assert (ll > -math.inf).all()
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        check(em, colTok, pairs, launches=1, refs=refs, what="fixed point", fixed=True)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)


@pytest.mark.parametrize("K,L", tq.LONG_SHAPES)
def test_more_blocks_than_a_pair_has_workgroups(K, L):
    """nCols = 4, S = 2 at (1, 1 100) and (1 100, 1) beside a dead pair of the same shape.  Under a table of one line (5 doubles on
    axis 0, 3 on axis 1) the long axis has 1 100 blocks for the 1 024 workgroups a pair gets, so 76 of them take a second block and
    clear the table between; under 2 doubles every line is summed in its global bins; then the default."""
    em, colTok, pairs, refs = tq.long_refs(K, L)
    for table in tq.long_tables(K, L):
        capi.set_option("MB_ROWPOST_TABLE", table)
        try:
            gotA, gotB, ll, _ = check(em, colTok, pairs, launches=1, refs=refs, what="posteriors, table %s" % table)
        finally:
            capi.set_option("MB_ROWPOST_TABLE", None)
        assert ll[0] > -math.inf and ll[1] == -math.inf and not gotA[1].any() and not gotB[1].any()
        long = gotA[0] if K > L else gotB[0]
        assert long.shape[0] == tq.LONG and (long[tq.ROWPOST_GROUPS_MAX:] > 0).any()


@pytest.mark.parametrize("table", (None, "16"))
@pytest.mark.parametrize("which", tq.WIDE_AXES)
def test_lines_wider_than_a_wavefront(which, table):
    """66 bins a line on axis 0 (nCols = 65), then 71 on axis 1 (nIn = 70), at S = 2.  With a table of 16 doubles that line does not
    fit it and is summed in its global bins, while the other axis takes several lines a block."""
    em, colTok, pairs = tq.wide_case(which)
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        gotA, gotB, ll, _ = check(em, colTok, pairs, launches=1)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert (ll > -math.inf).all() and gotA[0].shape == (4, em.nInTok + 1) and gotB[0].shape == (5, len(colTok) + 1)


# ---- 2. the ragged batch, scratch, chunks ---------------------------------------------------------------------------------------------
def test_ragged_batch_alone_and_in_chunks():
    """(0, 0), (0, 5), (5, 0), the ring marks at nCols = 2, S = 20 (short sides 9 / 10 and 25 / 26, found by i and by r), (2, 3),
    (0, 40), (40, 0) and a dead pair in one launch; then every pair alone, and the batch in chunks under about 1.8 times the largest
    pair's bytes: floating point against the yardstick, the fixed point the same bits all three ways."""
    em, colTok, pairs, refs = tq.ragged_refs()
    budget = tq.ragged_budget(em, pairs)
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        a0, b0, l0 = dev.merged_row_posteriors()
        assert capi.last_launch_count() == 1 and capi.last_kernel_name() == KERNEL
        gotA, gotB = split(dev, a0, b0)
        compare(em, colTok, gotA, gotB, l0, refs)
        assert l0[-1] == -math.inf and (l0[:-1] > -math.inf).all() and not gotA[-1].any() and not gotB[-1].any()
        assert gotA[0].shape == (0, 3) and gotB[0].shape == (0, 3) and gotA[1].shape == (0, 3) and gotB[2].shape == (0, 3)
        capi.set_memory_budget(budget)
        a1, b1, l1 = dev.merged_row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        compare(em, colTok, *split(dev, a1, b1), l1, refs, "posteriors, chunked")
        assert np.array_equal(l0, l1)
        capi.set_option("MB_DETERMINISTIC", "1")
        d0 = dev.merged_row_posteriors()
        compare(em, colTok, *split(dev, d0[0], d0[1]), d0[2], refs, "fixed point", fixed=True)
        again = dev.merged_row_posteriors()
        assert all(np.array_equal(x, y) for x, y in zip(d0, again))
        capi.set_memory_budget(budget)
        d1 = dev.merged_row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert all(np.array_equal(x, y) for x, y in zip(d0, d1))
        for k, pair in enumerate(pairs):
            _, one = open_pairs(em, colTok, [pair])
            try:
                a, b, l = one.merged_row_posteriors()
            finally:
                one.close()
            assert np.array_equal(a, d0[0][dev.inOff[k]:dev.inOff[k + 1]]) and np.array_equal(b, d0[1][dev.rowOff[k]:dev.rowOff[k + 1]]) and l[0] == d0[2][k], k
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_scratch_rings_of_the_materialised_sweeps():
    """nCols = 4, S = 65 at (13, 14) and (14, 13): the X / T ring of either is past 160 KiB and lies in the scratch buffer the call
    hands to both fills, with (2, 3) between them in LDS; a pair whose lattices exceed the budget alone is the error of counts()."""
    em, colTok, pairs = tq.scratch_case()
    gotA, gotB, ll, _ = check(em, colTok, pairs, launches=1)
    assert (ll > -math.inf).all()
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        dev.forward()
        n = capi.last_launch_count()
        capi.set_memory_budget(tq.pair_bytes(em.nStates, 4, 13, 14, em.nInTok) // 2)
        with pytest.raises(capi.MbError) as post:
            dev.merged_row_posteriors()
        with pytest.raises(capi.MbError) as counts:
            dev.counts()
        words = lambda e: (str(e.value).split("(")[0], str(e.value).split(")")[-1])      # (the bytes between differ by the bins)
        assert "exceeds the device memory budget" in str(post.value) and words(post) == words(counts), (str(post.value), str(counts.value))
        assert capi.last_launch_count() in (0, n)
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


# ---- 3. dead weights and column maps ----------------------------------------------------------------------------------------------------
def test_dead_weights_give_exact_zeros():
    """A third of the weights of either table -inf; all-blank rows and whole -inf rows on either tape; both profiles 700 lower."""
    live = []
    for name, em, colTok, pairs in tq.dead_weight_cases():
        gotA, gotB, ll, refs = check(em, colTok, pairs, launches=1, what="posteriors, " + name)
        live += list(ll > -math.inf)
        for ga, gb, (A, B) in zip(gotA, gotB, pairs):
            assert not ga[A == -math.inf].any() and not gb[B == -math.inf].any()
        if name == "third":
            assert all((A == -math.inf).any() and (B == -math.inf).any() for A, B in pairs)
        if name == "degenerate":
            assert list(ll[:6] > -math.inf) == [True, True, True, True, False, False]
            assert not gotB[3][:, 1:].any() and np.abs(gotB[3][:, 0] - 1.0).max() <= ROW_TOL        # all-blank rows: the blank takes every row
        if name == "far":
            assert ll[0] > -math.inf and ll[1] < -12000 and counts_close(gotA[1], gotA[0]) and counts_close(gotB[1], gotB[0])
    assert np.mean(live) >= 0.8


@pytest.mark.parametrize("which", range(len(tm.COLMAPS)))
def test_column_maps(which):
    """One column; every column on one token; a token nothing emits (its column stays 0 but for repeats of nothing); a doubled symbol."""
    em, cases = tq.column_map_cases()
    colTok, A, B = cases[which]
    gotA, gotB, ll, _ = check(em, colTok, [(A, B), (A[:2], B[:3]), (A[:0], B)], launches=1)
    assert ll[0] > -math.inf
    for c, t in enumerate(colTok):
        if t == 4:
            assert not any(g[:, c + 1].any() for g in gotB)


# ---- 4. the device against itself -------------------------------------------------------------------------------------------------------
def test_column_sums_are_the_grouped_counts():
    """The column sums of postA over all pairs against counts() of the same object added up by input token; the columns of postB
    added up by token are at least the counts of the transitions that write it (the rest are the repeats), and the blank column,
    the repeats and the emissions together are the rows."""
    em, colTok, pairs, _ = tq.ragged_refs()
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        postA, postB, ll = dev.merged_row_posteriors()
        c, _, ll2 = dev.counts()
        assert np.array_equal(ll, ll2)
        byIn, byOut = tq.grouped(em, colTok, c)
        assert counts_close(postA.sum(axis=0)[1:], byIn), (postA.sum(axis=0)[1:], byIn)
        cols = tq.by_token(em, colTok, postB.sum(axis=0)[1:])
        rows = sum(len(B) for (_, B), l in zip(pairs, ll) if l > -math.inf)
        assert (cols >= byOut * (1 - 1e-6)).all() and abs(postB.sum() - rows) <= 1e-6 * rows
        # a map of distinct tokens on rows without a repeat to take: emissions alone
        em1, colTok1, pairs1 = tm.chain_case()
        dm1, dev1 = open_pairs(em1, colTok1, pairs1)
        try:
            pa, pb, l1 = dev1.merged_row_posteriors()
            c1 = dev1.counts()[0]
            byIn1, byOut1 = tq.grouped(em1, colTok1, c1)
            assert (l1 > -math.inf).any() and counts_close(pa.sum(axis=0)[1:], byIn1) and counts_close(tq.by_token(em1, colTok1, pb.sum(axis=0)[1:]), byOut1)
        finally:
            dev1.close(); dm1.close()
    finally:
        dev.close(); dm.close()


def test_one_hot_input_equals_the_merged_pair_sweep():
    """A one-hot A against DeviceProfilePairs(..., colTok).merged_row_posteriors() on the token strings, at 1e-12; postA comes back as
    the one-hot rows."""
    em, colTok, xs, Bs = tq.one_hot_case()
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [th.one_hot(x, 3) for x in xs], Bs, colTok=colTok)
    pair = capi.DeviceProfilePairs(dm, xs, Bs, colTok)
    try:
        postA, postB, ll = two.merged_row_posteriors()
        want, wl = pair.merged_row_posteriors()
        assert (wl > -math.inf).all() and logs_close(ll, wl, 1e-12) and np.abs(postB - want).max() <= 1e-12
        hot = np.exp(np.concatenate([th.one_hot(x, 3) for x in xs]))
        assert not postA[hot == 0.0].any() and np.abs(postA[hot == 1.0] - 1.0).max() <= ROW_TOL
        WORST["one-hot against the merged pair sweep"] = float(np.abs(postB - want).max())
    finally:
        two.close(); pair.close(); dm.close()


def test_no_input_rows_is_the_one_tape_sweep():
    """K = 0 against DeviceProfiles(dm, profiles, colTok).row_posteriors(): nothing reads the input tape."""
    em, colTok, _, Bs = tq.one_hot_case()
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [np.zeros((0, 4))] * len(Bs), Bs, colTok=colTok)
    prof = capi.DeviceProfiles(dm, Bs, colTok)
    try:
        postA, postB, ll = two.merged_row_posteriors()
        want, wl = prof.row_posteriors()
        assert postA.shape == (0, 4) and logs_close(ll, wl) and np.array_equal(ll > -math.inf, wl > -math.inf) and (wl > -math.inf).any()
        assert counts_close(postB, want), np.abs(postB - want).max()
    finally:
        two.close(); prof.close(); dm.close()


def test_finite_differences_of_the_device_forward():
    """Every entry of both tables of one (3, 3) pair at S = 8 moved up and down: the perturbed pairs as one batch, one launch of the
    rolling Forward."""
    em, colTok, A, B = tq.fd_case()
    many = tq.perturbed(A, B)
    dm, dev = open_pairs(em, colTok, many)
    _, one = open_pairs(em, colTok, [(A, B)])
    try:
        f = dev.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and len(f) == 2 * (A.size + B.size)
        postA, postB, ll = one.merged_row_posteriors()
        assert abs(ll[0]) < 100
        fd = (f[0::2] - f[1::2]) / (2 * FD_H)
        got = np.concatenate([postA.ravel(), postB.ravel()])
        WORST["finite differences"] = float(np.abs(fd - got).max())
        print("central differences of the device Forward off by at most %.3g" % WORST["finite differences"])
        assert np.abs(fd - got).max() <= FD_TOL, (fd, got)
    finally:
        dev.close(); one.close(); dm.close()


# ---- 5. the same bits, optional outputs, refusals ---------------------------------------------------------------------------------------
def _small_batch():
    """The small pairs of the ragged batch and two of its ring pairs, the dead pair among them."""
    em, colTok, pairs, refs = tq.ragged_refs()
    keep = [0, 1, 2, 3, 8, 11, 12, 13, 14]
    return em, colTok, [pairs[k] for k in keep], [refs[k] for k in keep]


def test_fixed_point_is_the_same_bits():
    """MB_DETERMINISTIC=1: under three table sizes against the default -- blocks of several lines, of one line, and a table no line
    fits -- and after set_profiles against a fresh object."""
    em, colTok, pairs, refs = _small_batch()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        first = dev.merged_row_posteriors()
        compare(em, colTok, *split(dev, first[0], first[1]), first[2], refs, "fixed point", fixed=True)
        for table in ("24", "3", "2"):
            capi.set_option("MB_ROWPOST_TABLE", table)
            got = dev.merged_row_posteriors()
            assert all(np.array_equal(x, y) for x, y in zip(got, first)), table
        capi.set_option("MB_ROWPOST_TABLE", None)
        new = [tm.merged_input(np.random.RandomState(7700 + k), em, len(colTok), len(A), len(B), pInf=0.0) for k, (A, B) in enumerate(pairs)]
        dev.set_profiles([A for A, _ in new], [B for _, B in new])
        _, fresh = open_pairs(em, colTok, new)
        try:
            got, want = dev.merged_row_posteriors(), fresh.merged_row_posteriors()
            assert all(np.array_equal(x, y) for x, y in zip(got, want)) and not np.array_equal(got[1], first[1])
        finally:
            fresh.close()
        dev.set_profiles([A for A, _ in pairs], [B for _, B in pairs])
        assert all(np.array_equal(x, y) for x, y in zip(dev.merged_row_posteriors(), first))
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_the_other_sweeps_keep_their_bits():
    """Forward, Viterbi with paths and counts of the object before and after a merged_row_posteriors() call."""
    em, colTok, pairs, _ = _small_batch()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, colTok, pairs)

    def sweeps():
        return (dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)) + tuple(dev.viterbi()) + tuple(np.asarray(x) for x in dev.counts())
    try:
        before = sweeps()
        dev.merged_row_posteriors()
        after = sweeps()
        assert len(before) == len(after) == 10 and all(np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_either_output_may_be_left_out():
    em, colTok, pairs, _ = _small_batch()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        postA, postB, ll = dev.merged_row_posteriors()
        a, none, la = dev.merged_row_posteriors(outputs=False)
        assert none is None and capi.last_launch_count() == 1 and capi.last_kernel_name() == KERNEL
        none, b, lb = dev.merged_row_posteriors(inputs=False)
        assert none is None and np.array_equal(a, postA) and np.array_equal(b, postB) and np.array_equal(la, ll) and np.array_equal(lb, ll)
        n0, n1, l2 = dev.merged_row_posteriors(inputs=False, outputs=False)
        assert n0 is None and n1 is None and np.array_equal(l2, ll) and capi.last_launch_count() == 1
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_refusals():
    """A plain object refuses the merged call, a merged object the plain one, each before anything is launched."""
    em, colTok, A, B = tq.fd_case()
    dm = capi.DeviceMachine(em)
    plain = capi.DeviceProfileTwos(dm, [A], [th.soft_profile(np.random.RandomState(1), 3, 3, 0.0)])
    merged = capi.DeviceProfileTwos(dm, [A], [B], colTok=colTok)
    try:
        plain.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="merged row posteriors take merged profiles"):
            plain.merged_row_posteriors()
        with pytest.raises(capi.MbError, match="row posteriors take plain profiles"):
            merged.row_posteriors()
        assert capi.last_launch_count() == n and capi.last_kernel_name() != KERNEL
    finally:
        plain.close(); merged.close(); dm.close()


# ---- 6. the layers above, on the device ---------------------------------------------------------------------------------------------------
def test_autograd_function_on_the_device():
    em, colTok, A0, B0 = tq.fd_case()
    A1, B1 = tm.merged_input(np.random.RandomState(4), em, 3, 2, 2, pInf=0.0)
    A, B, inOff, rowOff = np.concatenate([A0, A1]), np.concatenate([B0, B1]), [0, 3, 5], [0, 3, 5]
    weights = torch.tensor([1.0, -2.5], dtype=torch.float64)
    out = {}
    for backend in ("numpy", "device", "device-dm"):
        logA = torch.tensor(A, dtype=torch.float64, requires_grad=True)
        logB = torch.tensor(B, dtype=torch.float64, requires_grad=True)
        if backend == "device-dm":
            dm = capi.DeviceMachine(em)
            try:
                ll = merged_two_profile_loglike(dm, logA, inOff, logB, rowOff, colTok)
            finally:
                dm.close()
        else:
            ll = merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, backend=backend)
        (ll * weights).sum().backward()
        out[backend] = (ll.detach().numpy(), logA.grad.numpy(), logB.grad.numpy())
    for key in ("device", "device-dm"):
        assert logs_close(out[key][0], out["numpy"][0]) and np.isfinite(out["numpy"][0]).all()
        for g, w in zip(out[key][1:], out["numpy"][1:]):
            assert counts_close(np.abs(g), np.abs(w)) and np.array_equal(np.sign(g), np.sign(w))
    a = torch.tensor(A, dtype=torch.float64)
    b = torch.tensor(B, dtype=torch.float64, requires_grad=True)
    merged_two_profile_loglike(em, a, inOff, b, rowOff, colTok).sum().backward()
    assert capi.last_kernel_name() == KERNEL and a.grad is None and counts_close(b.grad.numpy(), out["numpy"][2] / np.repeat([1.0, -2.5], [3, 2])[:, None])


@pytest.mark.parametrize("T", tq.CTC_T)
def test_echo_transducer_is_the_ctc_loss_on_the_device(T):
    """x = 1 2 2 3 as a one-hot logA against log-softmax frames: -inf with zeros at T = 3 and 4, -ctc_loss and exp(lp) - d ctc_loss /
    d lp at 7 and 12."""
    lp = tq.ctc_frames(T, True)
    logA = torch.tensor(th.one_hot(tq.CTC_X, 3), dtype=torch.float64, requires_grad=True)
    logB = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
    ll = merged_two_profile_loglike(tq.echo_machine(), logA, [0, len(tq.CTC_X)], logB, [0, T], tq.CTC_COLTOK)
    ll.sum().backward()
    assert capi.last_kernel_name() == KERNEL
    loss, grad = tq.ctc_reference(lp)
    got, post, postA = float(ll.detach()[0]), logB.grad.numpy(), logA.grad.numpy()
    if T < 5:
        assert got == -math.inf and loss == math.inf and not post.any() and not postA.any()
        return
    assert abs(got + loss) <= 1e-9 * max(1.0, abs(loss)), (got, loss)
    assert counts_close(post, np.exp(lp) - grad), np.abs(post - (np.exp(lp) - grad)).max()
    assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL


def test_merged_two_posteriors_on_the_device(tmp_path):
    """boss.mergedTwoPosteriors on the device backend against the numpy backend: dnastore4, four input profiles of 3, 1, 2 and 3 rows
    against tiny_uc.csv read CTC-merged, the last of them dead (a row without a weight)."""
    from machineboss_amd.machine import Machine
    from machineboss_amd.profile import Profile
    m = Machine.fromFile("tests/golden/machine/dnastore4.json")
    par = m.getParamDefs(True)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    pa, pb = Profile.fromCsv(str(a)), Profile.fromCsv("tests/golden/csv/tiny_uc.csv")
    rows = [list(r) for r in pa.row]
    profs = [pa, Profile(pa.header, rows[:1]), Profile(pa.header, rows[1:]), Profile(pa.header, [[0.0] * len(pa.header)] + rows[1:])]
    want, wl = boss.mergedTwoPosteriors(m, profs, pb, backend="numpy", params=par)
    got, gl = boss.mergedTwoPosteriors(m, profs, pb, backend="device", params=par)
    assert capi.last_kernel_name() == KERNEL and len(got) == 4 and logs_close(gl, wl)
    assert [l > -math.inf for l in wl] == [True, True, True, False]
    for k, ((ga, gb), (wa, wb)) in enumerate(zip(got, want)):
        assert ga.shape == wa.shape == (len(profs[k]), 4) and gb.shape == wb.shape and len(gb) == len(pb)
        assert counts_close(ga, wa) and counts_close(gb, wb), k
        assert not ga[wa == 0.0].any() and not gb[wb == 0.0].any()
        if k < 3:
            assert np.abs(ga.sum(axis=1) - 1.0).max() <= ROW_TOL and np.abs(gb.sum(axis=1) - 1.0).max() <= ROW_TOL
        else:
            assert not ga.any() and not gb.any()
