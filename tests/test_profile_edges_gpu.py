"""GPU tests of profile tapes at the edges of mb_profile.hip: lane counts and LDS sizes where the kernels change form, machines with an
input alphabet or no output alphabet, -inf weights and degenerate profiles, Viterbi ties, batch independence and bit-for-bit
self-consistency, chunking, long profiles checked without the restatement, and a cross-check through the composed machine."""

import numpy as np
import pytest

from profhelpers import _check_all, _close, _machine_of, _profiles, tie_census
from randmachine import quantised_machine, quantised_profile, random_machine
from machineboss_amd import algebra, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.profile import Profile, ProfileDP

pytestmark = pytest.mark.gpu

PF_LDS_MAX = 160 * 1024        # mb_profile.hip: three rolling state vectors of S doubles fit up to here, then global scratch


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


def _few_levels(S, nIn, nOut, seed):
    """A random machine with cycles and a few silent edges but no silent backbone: a handful of silent levels (a barrier each), and
    emitting edges into the end state from about 5% of the states."""
    em = random_machine(S, nIn, nOut, seed, density=1.5, silent_density=0.05, backbone=0.0, to_end=0.05)
    assert int(em.silentLevels().max(initial=0)) + 1 <= 16
    return em


def _path_weight(em, P, edges, rows):
    w = sum(float(em.logWeight[e]) for e in edges) + sum(float(P[r, em.outTok[e]]) for e, r in zip(edges, rows) if em.outTok[e])
    emitted = [int(r) for e, r in zip(edges, rows) if em.outTok[e]]
    return w + sum(float(P[r, 0]) for r in sorted(set(range(len(P))) - set(emitted))), emitted


def _check_path(em, P, v, edges, rows):
    """A Viterbi path chains from 0 to S-1, fires at ascending rows, emits at most once per row and weighs its score."""
    S = em.nStates
    if not len(edges):
        assert S == 1 or v == -np.inf
        return
    assert int(em.src[edges[0]]) == 0 and int(em.dst[edges[-1]]) == S - 1
    assert np.array_equal(em.dst[edges[:-1]], em.src[edges[1:]])
    assert np.all(np.diff(rows) >= 0) and rows[0] >= 0 and rows[-1] <= len(P)
    w, emitted = _path_weight(em, P, edges, rows)
    assert len(emitted) == len(set(emitted))
    assert abs(w - v) <= 1e-9 * max(1.0, abs(v)), (w, v)


# ---- A. the restatement at the shapes where the kernel changes form ------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, 1024, 1025])
def test_lane_count_edges(S):
    """pf_threads: 64 lanes up to S = 64, one lane per state up to 1 024, then lanes stride; S = 1: start = end."""
    em = _few_levels(S, 0, 3, 100 + S)
    dm, dev, _ = _check_all(em, _profiles(em, [0, 7, 23, 1, 40], S))
    assert dm.n_levels() <= 16 and np.isfinite(dev.forward()).sum() >= 2


@pytest.mark.parametrize("S", [2730, 2731, 6826, 6827])
def test_lds_boundary(S):
    """Both sides of 64 KiB of LDS (2 730 / 2 731 states) and of PF_LDS_MAX (6 826 in LDS, 6 827 in global scratch)."""
    assert 3 * 6826 * 8 <= PF_LDS_MAX < 3 * 6827 * 8
    em = _few_levels(S, 0, 4, 200 + S)
    dm, dev, _ = _check_all(em, _profiles(em, [12, 0, 30, 5], S))
    assert dm.n_levels() <= 16 and np.isfinite(dev.forward()).sum() >= 2


@pytest.mark.parametrize("nIn,nOut", [(0, 0), (1, 1), (1, 4), (3, 1), (3, 4)])
def test_alphabet_edges(nIn, nOut):
    """nOut = 0: an all-silent machine against blank-only rows.  nIn > 0: transitions that read input never fire (their counts are
    exactly 0, checked in _check_all), and one-hot profiles score as the token path with an empty input."""
    em = random_machine(60, nIn, nOut, 300 + 10 * nIn + nOut)
    dm, dev, _ = _check_all(em, _profiles(em, [0, 3, 17, 40, 9, 1], 300 + nIn, zeros=0.1))
    assert np.isfinite(dev.forward()).sum() >= 2
    if nOut:
        rng = np.random.RandomState(nIn)
        seqs = [rng.randint(1, nOut + 1, n) for n in (0, 1, 9, 23)]
        profs = []
        for y in seqs:
            P = np.full((len(y), nOut + 1), -np.inf)
            P[np.arange(len(y)), y] = 0.0
            profs.append(P)
        dev = capi.DeviceProfiles(dm, profs)
        b = capi.DeviceBatch.from_pairs(dm, [([], y) for y in seqs])
        assert _close(dev.forward(), b.forward(capi.MB_ROLLING), 1e-6)
        assert np.array_equal(dev.viterbi(paths=False)[0], b.viterbi(paths=False)[0])
        c = dev.counts()[0]
        assert np.allclose(c, b.counts()[0], rtol=1e-6, atol=1e-9)
        assert np.all(c[em.inTok != 0] == 0.0)


@pytest.mark.parametrize("seed", [1, 2])
def test_inf_weights_and_inf_rows(seed):
    em = random_machine(40, 0, 3, 400 + seed, allow_inf=True)
    lw = em.logWeight.copy()
    lw[np.random.RandomState(seed).choice(len(lw), len(lw) // 8, replace=False)] = -np.inf
    em = em.withLogWeights(lw)
    profs = _profiles(em, [10, 25, 0, 33, 18, 40], 400 + seed)
    profs[1][7] = -np.inf            # a whole row of -inf: the profile scores -inf
    profs[4][0] = -np.inf
    _, dev, _ = _check_all(em, profs)
    assert np.isfinite(dev.forward()).sum() >= 2


def test_all_blank_profile():
    """Every symbol column -inf, blank finite: the silent 0 -> S-1 score plus the blank column's sum; the path fires at row L."""
    em = random_machine(50, 0, 3, 502)
    dp = ProfileDP(em)
    rng = np.random.RandomState(501)
    P = np.full((30, 4), -np.inf)
    P[:, 0] = np.log(rng.uniform(0.1, 1.0, 30))
    silentF, silentV = dp.forward(np.zeros((0, 4)))[0], dp.forward(np.zeros((0, 4)), "max")[0]
    assert silentF > -np.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, [P])
    want = silentF + float(np.sum(P[:, 0]))
    assert _close(dev.forward(capi.MB_ROLLING), [want], 1e-12) and _close(dev.forward(capi.MB_MATERIALISE), [want], 1e-12)
    v, off, edges, rows = dev.viterbi()
    assert _close(v, [silentV + float(np.sum(P[:, 0]))], 1e-12)
    assert np.all(rows == 30) and np.all(em.outTok[edges] == 0)
    _check_path(em, P, v[0], edges, rows)
    c = dev.counts()[0]
    assert np.all(c[em.outTok != 0] == 0.0)
    _check_all(em, [P, P[:5]])


def test_all_inf_profile_and_empty_batch():
    em = random_machine(30, 0, 2, 502)
    dm = capi.DeviceMachine(em)
    P = np.full((12, 3), -np.inf)
    dev = capi.DeviceProfiles(dm, [P])
    assert dev.forward(capi.MB_ROLLING)[0] == -np.inf and dev.forward(capi.MB_MATERIALISE)[0] == -np.inf
    v, off, edges, rows = dev.viterbi()
    assert v[0] == -np.inf and off[0] == off[1] and len(edges) == 0
    c, s, ll = dev.counts()
    assert not c.any() and s == -np.inf and np.all(ll == -np.inf)
    empty = capi.DeviceProfiles(dm, [])
    assert empty.forward(capi.MB_ROLLING).shape == (0,) and empty.forward(capi.MB_MATERIALISE).shape == (0,)
    v, off, edges, rows = empty.viterbi()
    assert v.shape == (0,) and list(off) == [0] and len(edges) == 0
    assert empty.viterbi(paths=False)[0].shape == (0,)
    c, s, ll = empty.counts()
    assert not c.any() and s == 0.0 and ll.shape == (0,)


# ---- B. ties --------------------------------------------------------------------------------------------------------------------
def test_viterbi_ties_first_maximum():
    """Quantised weights ({0, log 1/2, log 1/4, -inf}): duplicate parallel edges, several emitting edges into one state, blank and
    symbol columns of equal weight.  The device traceback must take the documented first maximum (blank, then emitting edges in
    `incoming` order; no move, then silent edges) exactly as the restatement does; batches span several traceback blocks."""
    tot = {"blank": 0, "emit": 0, "stay": 0, "silent": 0}
    for S, nIn, nOut, seed in [(6, 0, 2, 1), (12, 0, 3, 2), (30, 0, 2, 3), (10, 2, 2, 4), (70, 0, 4, 5)]:
        em = quantised_machine(S, nIn, nOut, 600 + seed)
        rng = np.random.RandomState(seed)
        profs = [quantised_profile(rng, nOut, int(L)) for L in rng.randint(0, 41, 80)]
        dm, dev, _ = _check_all(em, profs, fill=(seed == 2))
        v, _, _, _ = dev.viterbi()
        assert np.array_equal(v, dev.viterbi(paths=False)[0])      # rolling and materialised max sweeps: the same bits
        dp = ProfileDP(em)
        for P in profs:
            for k, n in tie_census(dp, P).items():
                tot[k] += n
    assert sum(tot.values()) >= 300 and tot["blank"] >= 50 and tot["emit"] >= 100 and tot["stay"] >= 30, tot


# ---- C. batch independence, bit-for-bit self-consistency, chunking -----------------------------------------------------------------
def _mixed_batch(em, n, maxL, seed):
    rng = np.random.RandomState(seed)
    profs = _profiles(em, rng.randint(0, maxL + 1, n), seed)
    for k in range(3, n, 17):
        if len(profs[k]):
            profs[k][rng.randint(len(profs[k]))] = -np.inf     # some profiles score -inf
    return profs


@pytest.mark.parametrize("S,n,maxL", [(300, 300, 60), (6827, 12, 30)])
def test_batch_independence_and_self_consistency(S, n, maxL):
    em = _few_levels(S, 0, 4, 701 + S if S == 300 else 700 + S)
    dm = capi.DeviceMachine(em)
    assert dm.n_levels() <= 16
    profs = _mixed_batch(em, n, maxL, 700 + S)
    dev = capi.DeviceProfiles(dm, profs)
    fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
    v, off, edges, rows = dev.viterbi()
    vr = dev.viterbi(paths=False)[0]
    capi.set_option("MB_DETERMINISTIC", None)
    c, s, ll = dev.counts()
    assert np.array_equal(c, dev.counts()[0])          # reproducible without MB_DETERMINISTIC
    assert np.array_equal(fr, fm) and np.array_equal(v, vr) and np.array_equal(ll, fm)
    assert np.isfinite(fm).sum() >= n // 2 and (fm == -np.inf).any()
    acc = np.zeros(em.nTransitions)
    for k, P in enumerate(profs):
        one = capi.DeviceProfiles(dm, [P])
        assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.forward(capi.MB_MATERIALISE)[0] == fm[k], k
        v1, o1, e1, r1 = one.viterbi()
        assert v1[0] == v[k] and np.array_equal(e1, edges[off[k]:off[k + 1]]) and np.array_equal(r1, rows[off[k]:off[k + 1]]), k
        _, _, l1 = one.counts(acc)                       # accumulates in profile order, as k_profile_sum_counts does
        assert l1[0] == ll[k], k
        if k % 40 == 0 and len(P):
            assert capi.profile_fill(dm, capi.MB_FORWARD, P)[len(P), 1, S - 1] == fm[k]
    assert np.array_equal(acc, c)
    for k in range(n):
        if v[k] > -np.inf:
            _check_path(em, profs[k], v[k], edges[off[k]:off[k + 1]], rows[off[k]:off[k + 1]])

    # a budget that forces at least 3 chunks of unequal size (the profiles differ in length); outputs unchanged
    cells = [(len(P) + 1) * 2 * S * 8 + 8 * em.nTransitions for P in profs]
    budget = int(sum(cells) / 3.5)
    assert budget >= max(cells) * 1.2
    capi.set_memory_budget(budget)
    try:
        fm2 = dev.forward(capi.MB_MATERIALISE); fr2 = dev.forward(capi.MB_ROLLING)
        v2, off2, e2, r2 = dev.viterbi()
        c2, s2, ll2 = dev.counts()
        # below one profile's lattice: an error, then the normal budget works again
        capi.set_memory_budget(max(cells) // 2)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.counts()
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.viterbi()
    finally:
        capi.set_memory_budget(0)
    assert np.array_equal(fm2, fm) and np.array_equal(fr2, fr) and np.array_equal(ll2, ll)
    assert np.array_equal(v2, v) and np.array_equal(off2, off) and np.array_equal(e2, edges) and np.array_equal(r2, rows)
    assert np.allclose(c2, c, rtol=1e-12, atol=1e-15)
    assert np.array_equal(dev.counts()[0], c)


# ---- D. long profiles, checked without the restatement ------------------------------------------------------------------------
def _dna_generator(n, seed):
    rng = np.random.RandomState(seed)
    return EvaluatedMachine.fromMachine(algebra.generator(list(rng.choice(list("ACGT"), n)), "g"), {}, useDefaults=True)


def _dna_profiles(em, lengths, seed):
    """Basecaller-like rows over A, C, G, T + blank (one dominant column), as in scripts/bench_profile.py."""
    rng = np.random.RandomState(seed)
    return [Profile(["A", "C", "G", "T"], rng.dirichlet([0.3] * 5, L).astype(np.float32).astype(np.float64).tolist()).logRows(em) for L in lengths]


def _flow(em, c, nProf, Ltot):
    S = em.nStates
    fin = np.zeros(S); fout = np.zeros(S)
    np.add.at(fin, em.dst, c); np.add.at(fout, em.src, c)
    tol = 1e-8 * Ltot
    mid = np.arange(1, S - 1)
    assert np.abs(fin[mid] - fout[mid]).max(initial=0.0) <= tol
    assert abs(fout[0] - fin[0] - nProf) <= tol and abs(fin[S - 1] - fout[S - 1] - nProf) <= tol


@pytest.mark.parametrize("which", ["dna", "cycles", "cycles_input"])
def test_long_profiles_flow_and_paths(which):
    if which == "dna":
        em = _dna_generator(2000, 2)
        profs = _dna_profiles(em, [2000, 2600, 3100, 4000, 2300, 3500, 2000, 2900], 5)
    else:
        em = _few_levels(500, 2, 4, 804) if which == "cycles_input" else _few_levels(500, 0, 4, 801)
        profs = _profiles(em, [2000, 2600, 3100, 4000, 2300, 3500, 2000, 2900], 801, zeros=0.0)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs)
    Ltot = sum(len(P) for P in profs)
    c, s, ll = dev.counts()
    assert np.all(np.isfinite(ll)) and np.array_equal(ll, dev.forward(capi.MB_MATERIALISE))
    _flow(em, c, len(profs), Ltot)
    assert np.all(c >= 0.0) and np.all(c[em.inTok != 0] == 0.0)
    v, off, edges, rows = dev.viterbi()
    for k, P in enumerate(profs):
        assert v[k] <= ll[k]
        _check_path(em, P, v[k], edges[off[k]:off[k + 1]], rows[off[k]:off[k + 1]])
    if which == "cycles_input":
        return
    # without the blank every row is one emitting edge
    nb = [profs[0].copy(), profs[6].copy()] if which == "dna" else [P.copy() for P in profs[:3]]
    for P in nb:
        P[:, 0] = -np.inf
    cb, _, llb = capi.DeviceProfiles(dm, nb).counts()
    assert np.all(np.isfinite(llb))
    _flow(em, cb, len(nb), sum(len(P) for P in nb))
    assert abs(cb[(em.outTok != 0) & (em.inTok == 0)].sum() - sum(len(P) for P in nb)) <= 1e-8 * sum(len(P) for P in nb)


def test_long_counts_are_device_forward_derivatives():
    em = _few_levels(500, 0, 4, 801)
    profs = [P[:300] for P in _profiles(em, [2000, 2600, 3100, 4000], 801, zeros=0.0)]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs)
    c = dev.counts()[0]
    fin = np.nonzero(em.logWeight > -np.inf)[0]
    used = fin[c[fin] > 1e-3]
    pick = np.random.RandomState(1).choice(used, 6, replace=False)
    h = 1e-4
    try:
        for t in pick:
            lw = em.logWeight.copy(); lw[t] += h
            dm.set_weights(lw); up = dev.forward(capi.MB_ROLLING).sum()
            lw[t] -= 2 * h
            dm.set_weights(lw); dn = dev.forward(capi.MB_ROLLING).sum()
            d = (up - dn) / (2 * h)
            assert abs(d - c[t]) <= 1e-5 + 1e-4 * abs(c[t]), (t, d, c[t])
    finally:
        dm.set_weights(em.logWeight)
    assert np.array_equal(dev.counts()[0], c)


def test_long_profile_against_restatement():
    """One 2 100-row profile on the 2 000-symbol generator (which must emit 2 000 symbols) against the restatement."""
    em = _dna_generator(2000, 2)
    P = _dna_profiles(em, [2100], 9)[0]
    dm = capi.DeviceMachine(em)
    dp = ProfileDP(em)
    ll, _, _ = dp.forward(P)
    assert ll > -np.inf
    dev = capi.DeviceProfiles(dm, [P])
    assert _close(dev.forward(capi.MB_ROLLING), [ll], 1e-9) and _close(dev.forward(capi.MB_MATERIALISE), [ll], 1e-9)
    _, NB, WB = dp.backward(P)
    B = capi.profile_fill(dm, capi.MB_BACKWARD, P)
    assert _close(B[:, 0], NB, 1e-9) and _close(B[:, 1], WB, 1e-9)
    rc, _ = dp.counts(P)
    c = dev.counts()[0]
    assert np.allclose(c, rc, rtol=1e-6, atol=1e-9), np.abs(c - rc).max()
    rv, re_, rr = dp.viterbi(P)
    v, off, edges, rows = dev.viterbi()
    assert v[0] == rv and np.array_equal(edges, re_) and np.array_equal(rows, rr)


# ---- E. an independent cross-check through the composed machine ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["generator", "random"])
@pytest.mark.parametrize("zeros", [False, True])
def test_profile_sweep_equals_composed_machine(which, zeros):
    """compose(M, recogniser) with empty tapes on the token path (the route the profile kernels replace) against the profile sweep."""
    rng = np.random.RandomState(11 + zeros)
    if which == "generator":
        M = algebra.generator(list(rng.choice(list("ACGT"), 50)), "g")
        hdr = ["A", "C", "G", "T"]
    else:
        M = _machine_of(random_machine(6, 0, 3, 901 + 2 * zeros))
        hdr = ["a", "b", "c"]
    em = EvaluatedMachine.fromMachine(M, {}, useDefaults=True)
    rows = rng.dirichlet([0.5] * (len(hdr) + 1), 100).astype(np.float32).astype(np.float64)
    if zeros:
        rows[rng.rand(*rows.shape) < 0.1] = 0.0
    prof = Profile(hdr, rows.tolist())
    P = prof.logRows(em)
    assert (P == -np.inf).any() == zeros
    comp = algebra.compose(M, prof.recogniserMachine(), True, False)   # parallel transitions kept apart: Viterbi is per edge
    ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
    b = capi.DeviceBatch.from_pairs(capi.DeviceMachine(ec), [([], [])])
    dev = capi.DeviceProfiles(capi.DeviceMachine(em), [P])
    f, fc = dev.forward(capi.MB_ROLLING)[0], b.forward(capi.MB_ROLLING)[0]
    assert f > -np.inf and abs(f - fc) <= 1e-6 * abs(f), (f, fc)
    v, vc = dev.viterbi(paths=False)[0][0], b.viterbi(paths=False)[0][0]
    assert abs(v - vc) <= 1e-12 * abs(v), (v, vc)
