"""GPU tests of the row posteriors of the two-profile sweeps (k_profile_two_rowpost in mb_profile_two.hip; docs/profile_tapes.md,
"Row posteriors of pairs of profiles"): capi.DeviceProfileTwos.row_posteriors() against profile.TwoProfileDP.rowPosteriors at the
places where the kernel changes form -- one wavefront of many cells (S = 1), one wavefront per cell and one lane more (S = 64, 65),
more columns than lanes on either tape, many blocks of lines and more blocks than a pair has workgroups, a table too small for a
line, chunks -- and against the device itself: grouped counts(), the pair sweep under a one-hot input, finite differences of
forward().  The inputs are those of twoposthelpers, held to their conditions without a GPU by test_profile_two_post_host.py.

Bounds (pairprofilehelpers): entries as counts, 1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; likelihoods 1e-9 relative
to max(1, |value|); row sums 1e-6; central differences at h = 1e-6 within 1e-7 absolute.  In fixed point a lane sum is rounded
once to the nearest 2^-36, so a bin fed by n items -- (K + 1) S for an output row, (L + 1) S for an input row -- may be off by
n 2^-37 more, and a row sum by that of its bins."""
import math

import numpy as np
import pytest
import torch

import twoposthelpers as tp
import twoprofilehelpers as th
from pairprofilehelpers import counts_close, logs_close, pair_machine
from twoposthelpers import FD_H, FD_TOL, ROW_TOL, WORST, check, compare, open_pairs, split, yardstick
from machineboss_amd import capi
from machineboss_amd.torchprofile import two_profile_loglike

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the two-profile row posteriors:", WORST)


# ---- 1. the suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,nIn,nOut", tp.SUITE_CASES)
def test_suite_against_the_yardstick(S, nIn, nOut):
    """The seven lattices on the machine with silent levels and without, each machine's pairs in one batch.  K = 0 and L = 0 give
    empty tables; S = 1 puts 64 cells in a wavefront, 64 and 65 lie on either side of one wavefront per cell."""
    case = tp.suite_case(S, nIn, nOut)
    live = []
    for em in {id(c[0]): c[0] for c in case}.values():
        pairs = [(A, B) for e, A, B in case if e is em]
        assert len(pairs) == len(th.SUITE_SHAPES)
        gotA, gotB, ll, _ = check(em, pairs, launches=1)
        assert [(len(a), len(b)) for a, b in zip(gotA, gotB)] == list(th.SUITE_SHAPES)
        live += list(ll > -math.inf)
    assert np.mean(live) >= 0.9, np.mean(live)


def test_many_blocks_of_lines():
    """S = 40, K = L = 40: five lines a block and eight blocks on either axis; under a table of 4 doubles one line a block."""
    em, A, B = tp.block_case()
    refs = yardstick(em, [(A, B)])
    gotA, gotB, ll, _ = check(em, [(A, B)], launches=1, refs=refs)
    assert ll[0] > -math.inf
    capi.set_option("MB_ROWPOST_TABLE", "4")
    try:
        a4, b4, _, _ = check(em, [(A, B)], launches=1, refs=refs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert counts_close(a4[0], gotA[0]) and counts_close(b4[0], gotB[0])


@pytest.mark.parametrize("table", (None, "16"))
@pytest.mark.parametrize("nIn,nOut", tp.COLUMN_ALPHABETS)
def test_more_columns_than_lanes(nIn, nOut, table):
    """71 columns on the input tape, then on the output tape, at S = 2.  With a table of 16 doubles the line does not fit it and is
    summed in its global bins, while the other axis takes four lines a block."""
    em, pairs = tp.column_case(nIn, nOut)
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        gotA, gotB, ll, _ = check(em, pairs, launches=1)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert (ll > -math.inf).all() and gotA[0].shape == (4, nIn + 1) and gotB[0].shape == (5, nOut + 1)


def test_ragged_batch_with_a_dead_pair():
    em, pairs = tp.ragged_case()
    gotA, gotB, ll, _ = check(em, pairs, launches=1)
    d = tp.RAGGED_DEAD
    assert ll[d] == -math.inf and not gotA[d].any() and not gotB[d].any() and gotB[d].shape == (6, em.nOutTok + 1)
    assert list(ll > -math.inf) == [k != d for k in range(len(pairs))]
    assert gotA[0].shape == (0, 4) and gotB[0].shape == (0, 6) and gotA[1].shape == (0, 4) and gotB[2].shape == (0, 6)


def test_sparse_profiles_give_exact_zeros():
    em, pairs = tp.sparse_case()
    gotA, gotB, ll, _ = check(em, pairs, launches=1)
    assert np.mean(ll > -math.inf) >= 0.9
    for ga, gb, (A, B) in zip(gotA, gotB, pairs):
        assert (A == -math.inf).any() and (B == -math.inf).any() and not ga[A == -math.inf].any() and not gb[B == -math.inf].any()


def test_lattice_far_below_zero():
    """Every entry of both profiles 700 lower: cells down to about -12 600, and the rows still sum to 1."""
    em, A, B, Afar, Bfar = th.far_case()
    gotA, gotB, ll, _ = check(em, [(A, B), (Afar, Bfar)], launches=1)
    assert ll[0] > -math.inf and ll[1] < -12000
    assert counts_close(gotA[1], gotA[0]) and counts_close(gotB[1], gotB[0])


# ---- 2. chunks, blocks past the groups ------------------------------------------------------------------------------------------------
def test_chunking():
    """Ten ragged pairs, the fifth dead, under a budget of about two pairs: floating point against the yardstick, the fixed point the
    bits of the unchunked call."""
    em, pairs = th.split_case()
    refs = yardstick(em, pairs)
    budget = tp.chunk_budget(em, pairs)
    dm, dev = open_pairs(em, pairs)
    try:
        a0, b0, l0 = dev.row_posteriors()
        assert capi.last_launch_count() == 1
        compare(em, *split(dev, a0, b0), l0, refs)
        capi.set_memory_budget(budget)
        a1, b1, l1 = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        compare(em, *split(dev, a1, b1), l1, refs)
        assert np.array_equal(l0, l1)
        capi.set_option("MB_DETERMINISTIC", "1")
        d0 = dev.row_posteriors()
        capi.set_memory_budget(budget)
        d1 = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert all(np.array_equal(x, y) for x, y in zip(d0, d1))
        compare(em, *split(dev, d0[0], d0[1]), d0[2], refs, "fixed point", fixed=True)
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


@pytest.mark.parametrize("K,L", tp.LONG_SHAPES)
def test_more_blocks_than_a_pair_has_workgroups(K, L):
    """S = 2 at (1, 1 100) and (1 100, 1) under a table of 4 doubles: 1 100 blocks of one line on the long axis for the 1 024
    workgroups a pair gets at the most, so 76 of them take a second block; a dead pair of the same shape beside it is all zeros."""
    em, pairs = tp.long_case(K, L)
    capi.set_option("MB_ROWPOST_TABLE", "4")
    try:
        gotA, gotB, ll, _ = check(em, pairs, launches=1)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert ll[0] > -math.inf and ll[1] == -math.inf and not gotA[1].any() and not gotB[1].any()
    long = gotA[0] if K > L else gotB[0]
    assert long.shape[0] == tp.LONG and (long[tp.ROWPOST_GROUPS_MAX:] > 0).any()


# ---- 3. the device against itself -------------------------------------------------------------------------------------------------------
def test_column_sums_are_the_grouped_counts():
    """The column sums of both tables over all pairs against counts() of the same object, added up by input and by output token."""
    em, pairs = tp.ragged_case()
    dm, dev = open_pairs(em, pairs)
    try:
        postA, postB, ll = dev.row_posteriors()
        c, _, ll2 = dev.counts()
        assert np.array_equal(ll, ll2)
        byIn, byOut = tp.grouped(em, c)
        assert counts_close(postA.sum(axis=0)[1:], byIn), (postA.sum(axis=0)[1:], byIn)
        assert counts_close(postB.sum(axis=0)[1:], byOut), (postB.sum(axis=0)[1:], byOut)
    finally:
        dev.close(); dm.close()


def test_one_hot_input_equals_the_pair_sweep():
    """A one-hot A against DeviceProfilePairs.row_posteriors() on the token strings, at 1e-12; postA comes back as the one-hot rows."""
    em = pair_machine(65, 165, True, 3, 2)
    rng = np.random.RandomState(165)
    xs = [rng.randint(1, 4, size=K).astype(np.int32) for K in (5, 0, 7, 1)]
    Bs = [th.soft_profile(rng, L, 2, pInf=0.0) for L in (9, 4, 2, 1)]
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [th.one_hot(x, 3) for x in xs], Bs)
    pair = capi.DeviceProfilePairs(dm, xs, Bs)
    try:
        postA, postB, ll = two.row_posteriors()
        want, wl = pair.row_posteriors()
        assert (wl > -math.inf).all() and logs_close(ll, wl, 1e-12) and np.abs(postB - want).max() <= 1e-12
        hot = np.exp(np.concatenate([th.one_hot(x, 3) for x in xs]))
        assert not postA[hot == 0.0].any() and np.abs(postA[hot == 1.0] - 1.0).max() <= ROW_TOL
        WORST["one-hot against the pair sweep"] = float(np.abs(postB - want).max())
    finally:
        two.close(); pair.close(); dm.close()


def test_finite_differences_of_the_device_forward():
    """Every entry of both tables of one (3, 3) pair at S = 8 moved up and down: the perturbed pairs as one batch, one launch of the
    rolling Forward."""
    em, A, B = tp.fd_case()
    many = tp.perturbed(A, B)
    dm, dev = open_pairs(em, many)
    _, one = open_pairs(em, [(A, B)])
    try:
        f = dev.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and len(f) == 2 * (A.size + B.size)
        postA, postB, ll = one.row_posteriors()
        assert abs(ll[0]) < 100
        fd = (f[0::2] - f[1::2]) / (2 * FD_H)
        got = np.concatenate([postA.ravel(), postB.ravel()])
        WORST["finite differences"] = float(np.abs(fd - got).max())
        print("central differences of the device Forward off by at most %.3g" % WORST["finite differences"])
        assert np.abs(fd - got).max() <= FD_TOL, (fd, got)
    finally:
        dev.close(); one.close(); dm.close()


# ---- 4. new rows, NULL outputs, fixed point, autograd -------------------------------------------------------------------------------------
def test_set_profiles():
    """Each table alone and both, against a fresh object; a refused table changes nothing and launches nothing."""
    em = pair_machine(65, 165, True, 3, 2)
    shapes = ((5, 9), (0, 4), (7, 2), (3, 0))
    old = [th.two_input(np.random.RandomState(90 + k), em, K, L, pInf=0.0) for k, (K, L) in enumerate(shapes)]
    new = [th.two_input(np.random.RandomState(190 + k), em, K, L, pInf=0.0) for k, (K, L) in enumerate(shapes)]
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, old)
    try:
        first = dev.row_posteriors()
        for inputs, outputs in ((True, False), (False, True), (True, True)):
            mixed = [(n[0] if inputs else o[0], n[1] if outputs else o[1]) for o, n in zip(old, new)]
            dev.set_profiles([A for A, _ in mixed] if inputs else None, [B for _, B in mixed] if outputs else None)
            _, fresh = open_pairs(em, mixed)
            try:
                got, want = dev.row_posteriors(), fresh.row_posteriors()
                assert all(np.array_equal(x, y) for x, y in zip(got, want)) and not np.array_equal(got[1], first[1])
                assert np.array_equal(dev.forward(), fresh.forward()) and np.array_equal(dev.counts()[0], fresh.counts()[0])
            finally:
                fresh.close()
            dev.set_profiles([A for A, _ in old], [B for _, B in old])
            assert all(np.array_equal(x, y) for x, y in zip(dev.row_posteriors(), first))
        compare(em, *split(dev, first[0], first[1]), first[2], yardstick(em, old), "fixed point", fixed=True)
        badB = [B.copy() for _, B in new]
        badB[2][1, 1] = np.nan
        badA = [A.copy() for A, _ in new]
        badA[0][2, 0] = np.inf
        dev.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="NaN"):
            dev.set_profiles([A for A, _ in new], badB)          # (the good input table is not taken either)
        with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
            dev.set_profiles(badA, None)
        assert capi.last_launch_count() == n
        with pytest.raises(ValueError):
            dev.set_profiles([A for A, _ in new][:2], None)
        with pytest.raises(ValueError):
            dev.set_profiles(None, [B for _, B in new][::-1])
        assert all(np.array_equal(x, y) for x, y in zip(dev.row_posteriors(), first))
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_either_output_may_be_left_out():
    em, pairs = tp.ragged_case()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, pairs)
    try:
        postA, postB, ll = dev.row_posteriors()
        a, none, la = dev.row_posteriors(outputs=False)
        assert none is None and capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_two_rowpost"
        none, b, lb = dev.row_posteriors(inputs=False)
        assert none is None and np.array_equal(a, postA) and np.array_equal(b, postB) and np.array_equal(la, ll) and np.array_equal(lb, ll)
        n0, n1, l2 = dev.row_posteriors(inputs=False, outputs=False)
        assert n0 is None and n1 is None and np.array_equal(l2, ll)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_fixed_point_is_the_same_bits():
    """MB_DETERMINISTIC=1: twice, every pair alone against the batch, and under every table size -- blocks of many lines, of one
    line, and a table no line fits."""
    em, pairs = tp.ragged_case()
    refs = yardstick(em, pairs)
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = open_pairs(em, pairs)
    try:
        postA, postB, ll = dev.row_posteriors()
        again = dev.row_posteriors()
        assert np.array_equal(postA, again[0]) and np.array_equal(postB, again[1]) and np.array_equal(ll, again[2])
        compare(em, *split(dev, postA, postB), ll, refs, "fixed point", fixed=True)
        for k, pair in enumerate(pairs):
            _, one = open_pairs(em, [pair])
            try:
                a, b, l1 = one.row_posteriors()
            finally:
                one.close()
            assert np.array_equal(a, postA[dev.inOff[k]:dev.inOff[k + 1]]) and np.array_equal(b, postB[dev.rowOff[k]:dev.rowOff[k + 1]]) and l1[0] == ll[k], k
        for table in ("24", "6", "2"):
            capi.set_option("MB_ROWPOST_TABLE", table)
            a, b, l1 = dev.row_posteriors()
            assert np.array_equal(a, postA) and np.array_equal(b, postB) and np.array_equal(l1, ll), table
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_autograd_function_on_the_device():
    em = pair_machine(8, 108, True, 2, 3)
    (A0, B0), (A1, B1) = th.two_input(np.random.RandomState(1), em, 2, 3, pInf=0.0), th.two_input(np.random.RandomState(2), em, 3, 2, pInf=0.0)
    A, B, inOff, rowOff = np.concatenate([A0, A1]), np.concatenate([B0, B1]), [0, 2, 5], [0, 3, 5]
    weights = torch.tensor([1.0, -2.5], dtype=torch.float64)
    out = {}
    for backend in ("numpy", "device", "device-dm"):
        logA = torch.tensor(A, dtype=torch.float64, requires_grad=True)
        logB = torch.tensor(B, dtype=torch.float64, requires_grad=True)
        if backend == "device-dm":
            dm = capi.DeviceMachine(em)
            try:
                ll = two_profile_loglike(dm, logA, inOff, logB, rowOff)
            finally:
                dm.close()
        else:
            ll = two_profile_loglike(em, logA, inOff, logB, rowOff, backend=backend)
        (ll * weights).sum().backward()
        out[backend] = (ll.detach().numpy(), logA.grad.numpy(), logB.grad.numpy())
    for key in ("device", "device-dm"):
        assert logs_close(out[key][0], out["numpy"][0]) and np.isfinite(out["numpy"][0]).all()
        for g, w in zip(out[key][1:], out["numpy"][1:]):
            assert counts_close(np.abs(g), np.abs(w)) and np.array_equal(np.sign(g), np.sign(w))
    a = torch.tensor(A, dtype=torch.float64)
    b = torch.tensor(B, dtype=torch.float64, requires_grad=True)
    two_profile_loglike(em, a, inOff, b, rowOff).sum().backward()
    assert capi.last_kernel_name() == "k_profile_two_rowpost" and a.grad is None and counts_close(b.grad.numpy(), out["numpy"][2] / np.repeat([1.0, -2.5], [3, 2])[:, None])


# ---- 5. the layers above, on the device ---------------------------------------------------------------------------------------------------
def test_score_two_profiles_and_the_command_line_on_the_device(tmp_path):
    """boss.scoreTwoProfiles(posteriors=True) on the device backend against the numpy backend: dnastore4, four input profiles of
    3, 1, 2 and 3 rows against tiny_uc.csv, the last of them dead (a row without a weight); then --profile-posteriors beside
    --generate-csv on the default backend."""
    import io
    import json
    from machineboss_amd import boss
    from machineboss_amd.machine import Machine
    from machineboss_amd.profile import Profile
    dnastore, csv = "tests/golden/machine/dnastore4.json", "tests/golden/csv/tiny_uc.csv"
    m = Machine.fromFile(dnastore)
    par = m.getParamDefs(True)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    pa, pb = Profile.fromCsv(str(a)), Profile.fromCsv(csv)
    rows = [list(r) for r in pa.row]
    profs = [pa, Profile(pa.header, rows[:1]), Profile(pa.header, rows[1:]), Profile(pa.header, [[0.0] * len(pa.header)] + rows[1:])]
    want, _ = boss.scoreTwoProfiles(m, profs, pb, backend="numpy", params=par, viterbi=True, posteriors=True)
    got, pc = boss.scoreTwoProfiles(m, profs, pb, backend="device", params=par, viterbi=True, posteriors=True)
    assert pc is None and [len(p) for p in profs] == [3, 1, 2, 3] and len(got["posteriors"]) == 4
    assert logs_close(got["loglike"], want["loglike"]) and logs_close(got["viterbi"], want["viterbi"], 1e-12)
    assert [l > -math.inf for l in want["loglike"]] == [True, True, True, False]
    for k, ((ga, gb), (wa, wb)) in enumerate(zip(got["posteriors"], want["posteriors"])):
        assert ga.shape == wa.shape == (len(profs[k]), 4) and gb.shape == wb.shape == (len(pb), wb.shape[1])
        assert counts_close(ga, wa) and counts_close(gb, wb), k
        assert not ga[wa == 0.0].any() and not gb[wb == 0.0].any()
        if k < 3:
            assert np.abs(ga.sum(axis=1) - 1.0).max() <= ROW_TOL and np.abs(gb.sum(axis=1) - 1.0).max() <= ROW_TOL
        else:
            assert not ga.any() and not gb.any()
    assert "posteriors" not in boss.scoreTwoProfiles(m, profs[:1], pb, backend="device", params=par)[0]
    out = io.StringIO()
    assert boss.run([dnastore, "--use-defaults", "--generate-csv", str(a), "--recognize-csv", csv, "-L", "--profile-posteriors"], out) == 0
    assert capi.last_kernel_name() == "k_profile_two_rowpost"
    lines = [json.loads(l) for l in out.getvalue().splitlines()]
    assert len(lines) == 2 and abs(lines[0][0][2] - want["loglike"][0]) <= 1e-4 and lines[1][0][:2] == [str(a), ""]
    wa, wb = want["posteriors"][0]
    assert np.abs(np.array(lines[1][0][2]["input"], float) - wa).max() <= 1e-5          # (%g: six significant digits)
    assert np.abs(np.array(lines[1][0][2]["output"], float) - wb).max() <= 1e-5
