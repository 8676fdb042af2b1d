"""Posterior path samples of the two-profile sweeps on the device (mb_profile_twos_sample, k_profile_two_sample; docs/profile_tapes.md,
"Posterior path samples of pairs of profiles") against profile.TwoProfileDP.samplePaths, called per pair with the pair's own index:
sampled edges, output rows and input rows for equality, logq and the likelihoods to 1e-9 relative to max(1, |value|) with -inf exact,
and logq of every sampled path held to twoprofilehelpers.rescore minus the device's likelihood.  The cases, their seeds and the
margins that make equality a fair demand are twosamplehelpers'; test_profile_two_sample_host.py holds them to their conditions on the
CPU."""
import math

import numpy as np
import pytest

import twoenvhelpers as eh
import twoprofilehelpers as th
import twosamplehelpers as sh
from machineboss_amd import capi

pytestmark = pytest.mark.gpu

WORST = {}
PLAIN, ENV = "k_profile_two_sample", "k_profile_two_env_sample"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    print("worst deviations of the two-profile path samples:", WORST)


def _open(dm, triples):
    envs = [t[2] for t in triples]
    return capi.DeviceProfileTwos(dm, [t[0] for t in triples], [t[1] for t in triples], envs=envs if any(e is not None for e in envs) else None)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _worst(key, got, want):
    WORST[key] = max(WORST.get(key, 0.0), th.log_dev(got, want))


def _check(em, triples, refs, got, n, checked=None, what="samples"):
    """One sample_paths result of n samples per pair against the yardstick's first n (checked: only the first so many of each pair go
    against it); logq of every path held to its rescored weight minus the device's likelihood, its length to the bound."""
    ll, off, edges, rows, ins, logq = got
    want = np.array([r[0] for r in refs])
    _worst("loglike", ll, want)
    assert sh.log_close(ll, want), (what, ll, want)
    assert len(off) == len(triples) * n + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows) == len(ins) and len(logq) == len(triples) * n
    assert (np.diff(off) >= 0).all()
    nLev = sh.silent_levels(em)
    for k, ((A, B, _env), (wl, samples)) in enumerate(zip(triples, refs)):
        for j in range(n):
            sl = slice(off[k * n + j], off[k * n + j + 1])
            if wl == -math.inf:
                assert sl.start == sl.stop and logq[k * n + j] == -math.inf, (what, k, j)
                continue
            assert sl.stop - sl.start <= th.path_bound(nLev, len(A), len(B))
            w = th.rescore(em, A, B, edges[sl], rows[sl], ins[sl])
            assert sh.log_close([logq[k * n + j]], [w - ll[k]]), (what, k, j, logq[k * n + j], w - ll[k])
            _worst("logq against rescore - loglike", [logq[k * n + j]], [w - ll[k]])
            if checked is None or j < checked:
                we, wr, wi, wq = samples[j]
                assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr) and np.array_equal(ins[sl], wi), (what, k, j, edges[sl], we)
                assert sh.log_close([logq[k * n + j]], [wq]), (what, k, j, logq[k * n + j], wq)
                _worst("logq", [logq[k * n + j]], [wq])


def _run_case(name, counts, checked=None, name_of_kernel=None):
    """Every machine of a case: one object, sample_paths at each of `counts`, checked against the case's reference."""
    _, seed, groups = sh.case(name)
    refs = sh.reference(name)
    for (em, triples), ref in zip(groups, refs):
        dm = capi.DeviceMachine(em)
        dev = _open(dm, triples)
        try:
            for n in counts:
                got = dev.sample_paths(n, seed=seed)
                if name_of_kernel is not None:
                    assert capi.last_kernel_name() == name_of_kernel, capi.last_kernel_name()
                assert capi.last_launch_count() == 1
                _check(em, triples, ref, got, n, checked, "%s at %d samples" % (name, n))
        finally:
            dev.close(); dm.close()


# ---- 1. the basic suite, the seams of the blocks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sh.BASIC_STATES)
@pytest.mark.parametrize("nIn,nOut", sh.BASIC_ALPHABETS)
def test_basic_suite(S, nIn, nOut):
    """suite_case with and without silent levels at seven shapes; 1, 3, 64, 65 and 130 samples: one lane, a partial block, a block
    exactly, a pair's samples across two blocks, several blocks."""
    _run_case("basic%d_%d_%d" % (S, nIn, nOut), sh.BASIC_SAMPLES, name_of_kernel=PLAIN)


def test_dead_pairs_at_the_seams_of_the_blocks():
    """seam_case: 129 pairs with dead pairs at lanes 63, 64 and 128 of the 1-sample call; then 3 samples, where the seams fall inside
    pairs.  Dead pairs return empty paths and logq = -inf."""
    _run_case("seam", sh.SEAM_SAMPLES, name_of_kernel=PLAIN)


# ---- 2. envelopes ---------------------------------------------------------------------------------------------------------------------------
def test_every_envelope_kind():
    """cell_case(8): every shape under the full envelope, band(0), band(1), a path envelope and a staircase, 5 samples each -- Z cells
    whose input blank lies outside among them (test_profile_two_sample_host.py counts them)."""
    _run_case("envelopes", (sh.ENV_SAMPLES,), name_of_kernel=ENV)
    assert {k for ks in sh.env_kinds() for k in ks} == set(eh.ENV_KINDS)


def test_the_full_envelope_returns_the_bits_of_no_envelope():
    _, seed, groups = sh.case("envelopes")
    for (em, triples), kinds in zip(groups, sh.env_kinds()):
        sub = [t for t, kind in zip(triples, kinds) if kind == "full"]
        assert len(sub) >= 5
        dm = capi.DeviceMachine(em)
        a, b = _open(dm, sub), _open(dm, [(A, B, None) for A, B, _ in sub])
        try:
            ga = a.sample_paths(sh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == ENV
            gb = b.sample_paths(sh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == PLAIN
            assert _same(ga, gb) and len(ga[2]) > 0
        finally:
            a.close(); b.close(); dm.close()


def test_ragged_pairs_under_bands_with_a_dead_pair():
    """ragged_case under band(2) at 7 samples: 63 lanes of one wavefront on nine lattices, the sixth pair dead."""
    _run_case("ragged", (sh.RAGGED_SAMPLES,), name_of_kernel=ENV)
    assert sh.reference("ragged")[0][eh.RAGGED_DEAD][0] == -math.inf


# ---- 3. chunks, seeds, prefixes ---------------------------------------------------------------------------------------------------------------
def test_a_call_in_chunks_returns_the_bits_of_the_whole_call():
    """split_case under 1.8 times the bytes of the pair that costs this call most: at least three chunks, one Forward and one sample
    launch each, every pair's counter its index in the object.  Bit for bit the unsplit call, and the yardstick's paths."""
    _, seed, groups = sh.case("chunks")
    em, triples = groups[0]
    refs = sh.reference("chunks")[0]
    n = sh.CHUNK_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        whole = dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 1
        assert dm.n_levels() - 1 == sh.silent_levels(em)
        b = sh.sample_call_bytes(em, triples, n)
        budget = int(sh.CHUNK_BUDGET_FACTOR * max(b))
        chunks = th.lattice_chunks(b, budget)
        assert len(chunks) >= 3
        capi.set_memory_budget(budget)
        cut = dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == len(chunks) and capi.last_kernel_name() == PLAIN
        capi.set_memory_budget(0)
        _check(em, triples, refs, cut, n, what="in chunks")
        assert _same(whole, cut)
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


def test_seeds_and_prefixes():
    """The same seed twice gives the same bits, another seed another path, and the first 3 samples of a 130-sample call are the
    3-sample call's."""
    _, seed, groups = sh.case("chunks")
    em, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        a, b = dev.sample_paths(3, seed=seed), dev.sample_paths(3, seed=seed)
        assert _same(a, b)
        c = dev.sample_paths(3, seed=sh.SEED_B)
        assert np.array_equal(a[0], c[0]) and not (np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]))
        big = dev.sample_paths(130, seed=seed)
        assert np.array_equal(big[0], a[0])
        for k in range(len(triples)):
            for j in range(3):
                s, t = slice(a[1][k * 3 + j], a[1][k * 3 + j + 1]), slice(big[1][k * 130 + j], big[1][k * 130 + j + 1])
                assert all(np.array_equal(a[x][s], big[x][t]) for x in (2, 3, 4)) and a[5][k * 3 + j] == big[5][k * 130 + j], (k, j)
        # a 64-bit seed: both key words in use
        d = dev.sample_paths(3, seed=seed + (1 << 32))
        assert not (np.array_equal(a[1], d[1]) and np.array_equal(a[2], d[2]))
    finally:
        dev.close(); dm.close()


# ---- 4. one path per pair, long paths ---------------------------------------------------------------------------------------------------------
def test_one_path_per_pair_is_sampled_every_time():
    """Both profiles one-hot with -inf blanks on a machine with one path per pair, a K = 0, an L = 0 and a (0, 0) pair among them: every
    sample is the Viterbi path and logq = 0 within 1e-9."""
    _run_case("hot", (sh.HOT_SAMPLES,), name_of_kernel=PLAIN)
    _, seed, groups = sh.case("hot")
    em, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        v, voff, ve, vr, vi = dev.viterbi()
        ll, off, edges, rows, ins, logq = dev.sample_paths(sh.HOT_SAMPLES, seed=seed)
        n = sh.HOT_SAMPLES
        for k in range(len(triples)):
            for j in range(n):
                sl, vs = slice(off[k * n + j], off[k * n + j + 1]), slice(voff[k], voff[k + 1])
                assert np.array_equal(edges[sl], ve[vs]) and np.array_equal(rows[sl], vr[vs]) and np.array_equal(ins[sl], vi[vs]), (k, j)
        assert np.abs(logq).max() <= 1e-9 and sh.log_close(ll, v) and len(edges) > 0
    finally:
        dev.close(); dm.close()


def test_long_paths():
    """S = 40 at K = L = 120 under band(6), 256 samples of a few hundred edges: logq of every path held to its rescored weight minus
    the device's likelihood and its length to the bound; the first 8 against the yardstick."""
    _run_case("long", (sh.LONG_SAMPLES,), checked=sh.LONG_CHECKED, name_of_kernel=ENV)


# ---- 5. statistics without the yardstick ---------------------------------------------------------------------------------------------------------
def test_usage_of_4096_samples_meets_the_posterior_counts():
    """One pair at (3, 3), S = 3 with levels: the mean usage of every transition whose posterior count is at least 1e-3 lies within 5
    standard errors (from the sample variance) of DeviceProfileTwos.counts()."""
    em, A, B = sh.stat_case()
    dm = capi.DeviceMachine(em)
    dev = _open(dm, [(A, B, None)])
    try:
        counts, _, ll = dev.counts()
        got = dev.sample_paths(sh.STAT_SAMPLES, seed=sh.STAT_SEED)
        assert ll[0] > -math.inf and got[0][0] == ll[0]
        off, edges = got[1], got[2]
        u = sh.usage(em.nTransitions, [edges[off[j]:off[j + 1]] for j in range(sh.STAT_SAMPLES)])
        assert int((counts >= 1e-3).sum()) >= 8
        bad = sh.usage_within_bound(u, counts)
        assert not bad, bad
    finally:
        dev.close(); dm.close()


# ---- 6. errors, the layer above -------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_leave_the_object_usable():
    _, seed, groups = sh.case("chunks")
    em, triples = groups[0]
    refs = sh.reference("chunks")[0]
    n = sh.CHUNK_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    merged = capi.DeviceProfileTwos(dm, [triples[1][0]], [np.zeros((4, 3))], colTok=[1, 2])

    def usable():
        assert capi.last_launch_count() == 0
        _check(em, triples, refs, dev.sample_paths(n, seed=seed), n, what="after an error")
    try:
        with pytest.raises(capi.MbError, match="nSamples must be at least 1"):
            dev.sample_paths(0, seed=seed)
        usable()
        need = n * dev.path_cap()
        with pytest.raises(capi.MbError, match="pathCap too small.* %d entries.* %d" % (need - 1, need)):
            dev.sample_paths(n, seed=seed, cap=need - 1)
        usable()
        with pytest.raises(capi.MbError, match="sampling takes plain profiles"):
            merged.sample_paths(n, seed=seed)
        usable()
        L = capi.load()
        assert L.mb_profile_twos_sample(dev.h, n, seed, None, None, None, None, None, None, need) != 0 and "null argument" in L.mb_last_error().decode()
        usable()
        # three (0, 0) pairs on a machine without silent levels have path bound 0, so no pathCap is too small; under a budget that
        # keeps them in one chunk, 2^30 samples each are 3 * 2^30 lanes.  The call is refused before it writes to any array.
        flat = th.pair_machine(2, 32, False, 2, 3)
        fm = capi.DeviceMachine(flat)
        empty = capi.DeviceProfileTwos(fm, [np.zeros((0, flat.nInTok + 1))] * 3, [np.zeros((0, flat.nOutTok + 1))] * 3)
        try:
            assert empty.path_cap() == 0
            capi.set_memory_budget(1 << 50)
            off1, e1 = np.zeros(1, np.int64), np.zeros(1, np.uint32)
            rc = L.mb_profile_twos_sample(empty.h, 2 ** 30, seed, None, capi._p(off1, capi.C.c_int64), capi._p(e1, capi.C.c_uint32), None, None, None, 0)
            assert rc != 0 and "too many samples in one chunk: pairs times nSamples exceeds 2^31 - 1 lanes" in L.mb_last_error().decode()
            assert capi.last_launch_count() == 0
        finally:
            capi.set_memory_budget(0)
            empty.close(); fm.close()
        capi.set_memory_budget(max(sh.sample_call_bytes(em, triples, n)) - 1)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 0
        capi.set_memory_budget(0)
        usable()
    finally:
        capi.set_memory_budget(0)
        merged.close(); dev.close(); dm.close()


def test_sample_two_profiles_on_the_device_is_the_numpy_backend():
    """boss.sampleTwoProfiles: the device backend returns the numpy backend's paths, with logq and likelihoods to 1e-9."""
    from machineboss_amd import boss
    em = th.pair_machine(3, 31, True, 2, 3)
    m = th.machine_of(em)
    rng = np.random.RandomState(5)
    ins = [th.profile_of(em.inputTokenizer.tok2sym[1:], th.soft_profile(rng, K, em.nInTok, pInf=0.0)) for K in (2, 3, 0)]
    out = th.profile_of(em.outputTokenizer.tok2sym[1:], th.soft_profile(rng, 3, em.nOutTok, pInf=0.0))
    for band in (None, 2):
        pd, qd, ld = boss.sampleTwoProfiles(m, ins, out, 4, seed=9, band=band)
        pn, qn, ln = boss.sampleTwoProfiles(m, ins, out, 4, seed=9, backend="numpy", band=band)
        assert sh.log_close(ld, ln) and sh.log_close(np.ravel(qd), np.ravel(qn))
        assert [[p.steps for p in ps] for ps in pd] == [[p.steps for p in ps] for ps in pn]
