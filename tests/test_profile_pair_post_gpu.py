"""GPU tests of the row posteriors of the two-tape profile sweeps (k_profile_pair_rowpost in mb_profile_pair.hip;
docs/profile_tapes.md, "Row posteriors"): capi.DeviceProfilePairs.row_posteriors() against profile.PairProfileDP.rowPosteriors over
the suites of pairprofilehelpers and pairenvhelpers, at the places where the kernel changes form -- one wavefront of many cells
(S = 1), one wavefront per cell and one lane more (S = 64, 65), more columns than lanes, many row blocks, a table too small for a
row, envelopes with rows of a single cell, chunks -- and against the device itself: grouped counts(), the one-tape sweeps at I = 0,
finite differences of forward().

Bounds (pairprofilehelpers): entries as counts, 1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; likelihoods 1e-9 relative
to max(1, |value|); row sums 1e-6 (non-negative entries, each within 1e-6 relative, that sum to 1); central differences at h = 1e-6
within 1e-7 absolute (truncation about h^2, rounding about 2 ulp(LL) / 2h < 1e-8)."""
import math

import numpy as np
import pytest
import torch

import pairenvhelpers as eh
import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close, pair_input, pair_machine
from profileprefixhelpers import random_profile
from randmachine import random_machine
from machineboss_amd import capi
from machineboss_amd.profile import PairProfileDP
from machineboss_amd.seqpair import Envelope
from machineboss_amd.torchprofile import pair_profile_loglike

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7
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
    print("worst deviations of the row posteriors:", WORST)


def _open(em, triples):
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    if any(t[2] is not None for t in triples):
        dev.set_envelopes([t[2] for t in triples])
    return dm, dev


def _split(dev, post):
    return [post[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)]


def _yardstick(em, triples):
    dp = PairProfileDP(em)
    return [dp.rowPosteriors(x, P, env=env) for x, P, env in triples]


def _compare(got, ll, refs, what="posteriors"):
    """The device's per-pair posteriors and likelihoods against the yardstick's: entries, exact zeros, row sums."""
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
            assert np.abs(g.sum(axis=1) - 1.0).max() <= ROW_TOL, (k, g.sum(axis=1))
        else:
            assert not g.any(), k


def _check(em, triples, launches=None):
    refs = _yardstick(em, triples)
    dm, dev = _open(em, triples)
    try:
        post, ll = dev.row_posteriors()
        if launches is not None:
            assert capi.last_launch_count() == launches
        assert post.shape == (dev.rowOff[-1], em.nOutTok + 1)
        got = _split(dev, post)
        _compare(got, ll, refs)
    finally:
        dev.close(); dm.close()
    return got, ll, refs


# ---- 1. the suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,nIn,nOut", [(S, a, b) for S in (1, 2, 8, 64, 65) for a, b in ph.SUITE_ALPHABETS])
def test_suite_against_the_yardstick(S, nIn, nOut):
    """The seven shapes on the machine with silent levels and without, each machine's pairs in one batch.  L = 0 gives an empty
    result; S = 1 puts 64 cells in a wavefront, 64 and 65 lie on either side of one wavefront per cell."""
    case = ph.suite_case(S, nIn, nOut)
    live = []
    for em in {id(c[0]): c[0] for c in case}.values():
        triples = [(x, P, None) for e, x, P in case if e is em]
        assert len(triples) == len(ph.SUITE_SHAPES)
        got, ll, refs = _check(em, triples, launches=1)
        assert capi.last_kernel_name() == "k_profile_pair_rowpost"
        assert [g.shape[0] for g in got] == [L for _, L in ph.SUITE_SHAPES]
        live += list(ll > -math.inf)
    assert np.mean(live) >= 0.85, np.mean(live)


def test_many_row_blocks():
    """S = 40, I = L = 40: 1 640 items a row, five rows a block, eight blocks; and a table of 4 doubles: one row a block."""
    em, x, P = ph.wide_case()
    got, ll, refs = _check(em, [(x, P, None)])
    assert ll[0] > -math.inf
    capi.set_option("MB_ROWPOST_TABLE", "4")
    try:
        got2, _, _ = _check(em, [(x, P, None)])
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
    assert counts_close(got2[0], got[0])


@pytest.mark.parametrize("table", (None, "16"))
def test_other_alphabets_and_more_columns_than_lanes(table):
    """(nIn, nOut) = (1, 4) and (5, 3) at S = 65; S = 2 with 70 output tokens at L = 5: 71 columns, more than a wavefront has lanes.
    With a table of 16 doubles the 71 columns of a row do not fit it and are summed in their global bins; the others take one to
    four rows a block."""
    capi.set_option("MB_ROWPOST_TABLE", table)
    try:
        for nIn, nOut in ((1, 4), (5, 3)):
            for em, pairs in ph.alphabet_case(nIn, nOut):
                got, ll, _ = _check(em, [(x, P, None) for x, P in pairs], launches=1)
                assert (ll > -math.inf).all()
        em = pair_machine(2, 270, False, 1, 70)
        pairs = [pair_input(np.random.RandomState(270 + I), em, I, 5) for I in (4, 0, 7)]
        got, ll, _ = _check(em, [(x, P, None) for x, P in pairs], launches=1)
        assert (ll > -math.inf).all() and got[0].shape == (5, 71)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)


def test_ragged_batch_with_a_dead_pair():
    em, pairs = ph.ragged_case()
    x, P = pair_input(np.random.RandomState(59), em, 5, 6)
    P = P.copy(); P[2] = -np.inf
    triples = [(a, b, None) for a, b in pairs[:5]] + [(x, P, None)] + [(a, b, None) for a, b in pairs[5:]]
    got, ll, _ = _check(em, triples, launches=1)
    assert ll[5] == -math.inf and not got[5].any() and got[5].shape == (6, em.nOutTok + 1)
    assert np.mean(ll > -math.inf) >= 0.85


def test_sparse_profiles_give_exact_zeros():
    em, pairs = ph.sparse_case()
    got, ll, _ = _check(em, [(x, P, None) for x, P in pairs], launches=1)
    assert (ll > -math.inf).any()
    for g, (_, P) in zip(got, pairs):
        assert (P == -math.inf).any() and not g[P == -math.inf].any()


def test_lattice_far_below_zero():
    """Every entry of the profile 700 lower: cells down to about -6 300, and the rows still sum to 1."""
    em, x, P, Pfar = ph.far_case()
    got, ll, refs = _check(em, [(x, P, None), (x, Pfar, None)], launches=1)
    assert ll[0] > -math.inf and ll[1] < -6000 and np.abs(got[1].sum(axis=1) - 1.0).max() <= ROW_TOL
    assert counts_close(got[1], got[0])


# ---- 2. envelopes -----------------------------------------------------------------------------------------------------------------------
def test_every_envelope_of_the_cell_suite():
    """cell_case(8): seven shapes under full, band(0), band(1), a path envelope and the staircase (rows of a single cell), with silent
    levels and without; the pairs of a machine in one launch."""
    case = eh.cell_case(8)
    live = []
    for em in {id(c[0]): c[0] for c in case}.values():
        triples = [(x, P, env) for e, x, P, kind, env in case if e is em]
        assert any(min(b - a for a, b in zip(env.inStart, env.inEnd)) == 1 for _, _, env in triples)
        got, ll, _ = _check(em, triples, launches=1)
        assert capi.last_kernel_name() == "k_profile_pair_env_rowpost"
        live += list(ll > -math.inf)
    assert np.mean(live) >= 0.85, np.mean(live)


@pytest.mark.parametrize("M", (34, 86))
def test_bands_at_the_ring_marks(M):
    x, P, env = eh.mark_case(M)
    got, ll, _ = _check(eh.mark_machine(), [(x, P, env)], launches=1)
    assert ll[0] > -math.inf


def test_enveloped_and_plain_pairs_in_one_call():
    """A pair without an envelope, a dead pair under a band and two live pairs under bands: two launches of each kernel (one per
    kind); and every pair alone has the bits of the batch under MB_DETERMINISTIC=1."""
    em = eh.mark_machine()
    (x0, P0, e0), (x1, P1, e1) = eh.mark_extras()
    x2, P2 = pair_input(np.random.RandomState(4492), em, 12, 9)
    x3, P3 = pair_input(np.random.RandomState(4493), em, 7, 7)
    triples = [(x2, P2, Envelope.band(12, 9, 4)), (x0, P0, e0), (x1, P1, e1), (x3, P3, Envelope.band(7, 7, 0))]
    got, ll, _ = _check(em, triples, launches=2)
    assert ll[2] == -math.inf and ll[1] > -math.inf and ll[0] > -math.inf
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = _open(em, triples)
    try:
        post, l0 = dev.row_posteriors()
        post2, _ = dev.row_posteriors()
        assert np.array_equal(post, post2)
        _compare(_split(dev, post), l0, _yardstick(em, triples), "fixed point")
        for k, t in enumerate(triples):
            _, one = _open(em, [t])
            try:
                p1, l1 = one.row_posteriors()
            finally:
                one.close()
            assert np.array_equal(p1, post[dev.rowOff[k]:dev.rowOff[k + 1]]) and l1[0] == l0[k], k
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 3. chunks --------------------------------------------------------------------------------------------------------------------------
def test_chunking():
    em, pairs = ph.chunk_case()
    S, n, I, L = ph.CHUNK_SHAPE
    triples = [(x, P, None) for x, P in pairs]
    refs = _yardstick(em, triples[:3])
    dm, dev = _open(em, triples)
    budget = (n // 3) * (I + 1) * (L + 1) * 2 * S * 8 * 2 + 4096      # a third of the pairs' two lattices: three chunks or more
    try:
        p0, l0 = dev.row_posteriors()
        assert capi.last_launch_count() == 1
        _compare(_split(dev, p0)[:3], l0[:3], refs)
        capi.set_memory_budget(budget)
        p1, l1 = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert np.array_equal(l0, l1) and counts_close(p1, p0) and np.abs(p1.sum(axis=1) - 1.0).max() <= ROW_TOL
        capi.set_option("MB_DETERMINISTIC", "1")
        d0, _ = dev.row_posteriors()
        d0b, _ = dev.row_posteriors()
        capi.set_memory_budget(budget)
        d1, _ = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        capi.set_memory_budget(0)
        assert np.array_equal(d0, d0b) and np.array_equal(d0, d1)
        assert counts_close(d0, p0) or np.allclose(d0, p0, rtol=1e-6, atol=1e-9)      # fixed point at 2^-36
        _, one = _open(em, triples[5:6])
        try:
            assert np.array_equal(one.row_posteriors()[0], d0[dev.rowOff[5]:dev.rowOff[6]])
        finally:
            one.close()
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 4. the device against itself ---------------------------------------------------------------------------------------------------------
def _grouped(em, counts):
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(em.outTok, np.int64), counts)
    return g[1:]


def test_column_sums_are_the_grouped_counts():
    """sum_r post[r][o] over all pairs against counts() of the same object, added up by output token; full and under bands."""
    em, pairs = ph.ragged_case()
    for envs in (None, [Envelope.band(len(x), len(P), 9) for x, P in pairs]):
        dm, dev = _open(em, [(x, P, None if envs is None else envs[k]) for k, (x, P) in enumerate(pairs)])
        try:
            post, ll = dev.row_posteriors()
            c, _, ll2 = dev.counts()
            assert np.array_equal(ll, ll2) and (ll > -math.inf).mean() >= 0.85
            assert counts_close(post.sum(axis=0)[1:], _grouped(em, c)), (post.sum(axis=0)[1:], _grouped(em, c))
        finally:
            dev.close(); dm.close()


def test_no_input_equals_device_profiles():
    em = random_machine(40, 0, 3, 31)
    profs = [random_profile(np.random.RandomState(31 + L), L, 3) for L in (0, 1, 9, 23)]
    dm = capi.DeviceMachine(em)
    try:
        for P in profs:
            a = capi.DeviceProfilePairs(dm, [[]], [P])
            b = capi.DeviceProfiles(dm, [P])
            try:
                post, ll = a.row_posteriors()
                c, _, lb = b.counts()
                assert logs_close(ll, lb, 1e-12)
                if ll[0] > -math.inf and len(P):
                    assert counts_close(post.sum(axis=0)[1:], _grouped(em, c)) and np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
            finally:
                a.close(); b.close()
    finally:
        dm.close()


def test_finite_differences_of_the_device_forward():
    """All 2 L C perturbed profiles of one (3, 3) pair at S = 8 as one batch, one launch of the rolling Forward."""
    em = pair_machine(8, 108, True, 2, 3)
    x, P = pair_input(np.random.RandomState(3), em, 3, 3, pZero=0.0)
    assert np.isfinite(P).all()
    L, C = P.shape
    profs = []
    for r in range(L):
        for o in range(C):
            for sgn in (1.0, -1.0):
                Q = P.copy(); Q[r, o] += sgn * FD_H
                profs.append(Q)
    dm = capi.DeviceMachine(em)
    many = capi.DeviceProfilePairs(dm, [x] * len(profs), profs)
    one = capi.DeviceProfilePairs(dm, [x], [P])
    try:
        f = many.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and len(f) == 2 * L * C
        post, ll = one.row_posteriors()
        assert abs(ll[0]) < 100
        fd = ((f[0::2] - f[1::2]) / (2 * FD_H)).reshape(L, C)
        WORST["finite differences"] = float(np.abs(fd - post).max())
        print("central differences of the device Forward off by at most %.3g" % WORST["finite differences"])
        assert np.abs(fd - post).max() <= FD_TOL, (fd, post)
    finally:
        many.close(); one.close(); dm.close()


# ---- 5. new rows, rejections, autograd ----------------------------------------------------------------------------------------------------
def test_set_profiles():
    em = pair_machine(65, 165, True, 3, 2)
    shapes = ((5, 9), (0, 4), (7, 2))
    old = [pair_input(np.random.RandomState(90 + k), em, I, L) for k, (I, L) in enumerate(shapes)]
    new = [(x, pair_input(np.random.RandomState(190 + k), em, len(x), len(P))[1]) for k, (x, P) in enumerate(old)]
    envs = [Envelope.band(5, 9, 5), None, None]
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = _open(em, [(x, P, e) for (x, P), e in zip(old, envs)])
    _, fresh = _open(em, [(x, P, e) for (x, P), e in zip(new, envs)])
    try:
        p_old, l_old = dev.row_posteriors()
        dev.set_profiles([P for _, P in new])
        p_new, l_new = dev.row_posteriors()
        want, wl = fresh.row_posteriors()
        assert np.array_equal(p_new, want) and np.array_equal(l_new, wl) and not np.array_equal(p_new, p_old)
        assert np.array_equal(dev.forward(), fresh.forward()) and np.array_equal(dev.counts()[0], fresh.counts()[0])
        _compare(_split(dev, p_new), l_new, _yardstick(em, [(x, P, e) for (x, P), e in zip(new, envs)]), "fixed point")
        bad = [P.copy() for _, P in old]
        bad[2][1, 1] = np.nan
        dev.forward()
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="NaN"):
            dev.set_profiles(bad)
        assert capi.last_launch_count() == n
        with pytest.raises(ValueError):
            dev.set_profiles([P for _, P in old][:2])
        assert np.array_equal(dev.row_posteriors()[0], want)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); fresh.close(); dm.close()


def test_merged_profiles_are_refused():
    em = pair_machine(8, 108, True, 2, 3)
    rng = np.random.RandomState(8)
    P = random_profile(rng, 4, 3)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [[1, 2]], [P], [1, 2, 3])
    try:
        assert dev.forward()[0] > -math.inf
        n = capi.last_launch_count()
        with pytest.raises(capi.MbError, match="row posteriors take plain profiles"):
            dev.row_posteriors()
        with pytest.raises(capi.MbError, match="row posteriors take plain profiles"):
            dev.set_profiles([P])
        assert capi.last_launch_count() == n
    finally:
        dev.close(); dm.close()


def test_autograd_function_on_the_device():
    em = pair_machine(8, 108, True, 2, 3)
    (x0, P0), (x1, P1) = pair_input(np.random.RandomState(1), em, 2, 3, pZero=0.0), pair_input(np.random.RandomState(2), em, 3, 2, pZero=0.0)
    xs, P, rowOff, envs = [x0, x1], np.concatenate([P0, P1]), [0, 3, 5], [None, Envelope.band(3, 2, 1)]
    weights = torch.tensor([1.0, -2.5], dtype=torch.float64)
    out = {}
    for backend, machine in (("numpy", em), ("device", em), ("device-dm", None)):
        logP = torch.tensor(P, dtype=torch.float64, requires_grad=True)
        if machine is None:
            dm = capi.DeviceMachine(em)
            try:
                ll = pair_profile_loglike(dm, xs, logP, rowOff, envs=envs)
            finally:
                dm.close()
        else:
            ll = pair_profile_loglike(machine, xs, logP, rowOff, envs=envs, backend=backend)
        (ll * weights).sum().backward()
        out[backend] = (ll.detach().numpy(), logP.grad.numpy())
    for key in ("device", "device-dm"):
        assert logs_close(out[key][0], out["numpy"][0]) and np.isfinite(out["numpy"][0]).all()
        g, w = out[key][1], out["numpy"][1]
        assert counts_close(np.abs(g), np.abs(w)) and np.array_equal(np.sign(g), np.sign(w))
