"""Posterior path samples of the pair profile sweeps on the device (mb_profile_pairs_sample, k_profile_pair_sample; docs/profile_tapes.md,
"Posterior path samples") against profile.PairProfileDP.samplePaths, called per pair with the pair's own index: sampled edges and
rows for equality, logq and the likelihoods to 1e-9 relative to max(1, |value|) with -inf exact, and every sampled path replayed
through dp.edgesToPath from the start state to the end state over exactly x and the L rows.  The cases, their seeds and the margins
that make equality a fair demand are pairsamplehelpers'; test_profile_pair_sample_host.py holds them to their conditions on the CPU."""
import math

import numpy as np
import pytest

import pairenvhelpers as eh
import pairprofilehelpers as ph
import pairsamplehelpers as sh
from machineboss_amd import capi

pytestmark = pytest.mark.gpu

WORST = {}
PLAIN, ENV = "k_profile_pair_sample", "k_profile_pair_env_sample"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    print("worst deviations of the path samples:", WORST)


def _open(dm, triples):
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    if any(t[2] is not None for t in triples):
        dev.set_envelopes([t[2] for t in triples])
    return dev


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _check(em, triples, refs, got, n, checked=None, what="samples"):
    """One sample_paths result of n samples per pair against the yardstick's first n (checked: only the first so many of each pair go
    against it); every path replayed and its logq held to its replayed weight minus the device's likelihood."""
    ll, off, edges, rows, logq = got
    want = np.array([r[0] for r in refs])
    WORST["loglike"] = max(WORST.get("loglike", 0.0), ph.log_dev(ll, want))
    assert sh.log_close(ll, want), (what, ll, want)
    assert len(off) == len(triples) * n + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows) and len(logq) == len(triples) * n
    assert (np.diff(off) >= 0).all()
    m = sh.machine_of(em)
    for k, ((x, P, _env), (wl, samples)) in enumerate(zip(triples, refs)):
        for j in range(n):
            sl = slice(off[k * n + j], off[k * n + j + 1])
            if wl == -math.inf:
                assert sl.start == sl.stop and logq[k * n + j] == -math.inf, (what, k, j)
                continue
            w = sh.replay(em, m, x, P, edges[sl], rows[sl])
            assert sh.log_close([logq[k * n + j]], [w - ll[k]]), (what, k, j, logq[k * n + j], w - ll[k])
            WORST["logq against the replay"] = max(WORST.get("logq against the replay", 0.0), ph.log_dev([logq[k * n + j]], [w - ll[k]]))
            if checked is None or j < checked:
                we, wr, wq = samples[j]
                assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr), (what, k, j, edges[sl], we)
                assert sh.log_close([logq[k * n + j]], [wq]), (what, k, j, logq[k * n + j], wq)
                WORST["logq"] = max(WORST.get("logq", 0.0), ph.log_dev([logq[k * n + j]], [wq]))


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
                _check(em, triples, ref, got, n, checked, "%s at %d samples" % (name, n))
        finally:
            dev.close(); dm.close()


# ---- 1. the basic suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sh.BASIC_STATES)
def test_basic_suite(S):
    """pair_machine with and without silent levels at six shapes; 1, 3, 64, 65 and 130 samples: one lane, a partial block, a block
    exactly, a pair's samples across two blocks, several blocks."""
    _run_case("basic%d" % S, sh.BASIC_SAMPLES, name_of_kernel=PLAIN)
    assert capi.last_launch_count() == 1


def test_block_boundaries_fall_inside_pairs():
    """Ten ragged pairs at 7 samples: 70 lanes, the block boundary inside pair 9's samples, lanes of one wavefront on ten lattices."""
    _run_case("ragged", (sh.RAGGED_SAMPLES,), name_of_kernel=PLAIN)


# ---- 2. envelopes ---------------------------------------------------------------------------------------------------------------------------
def test_every_envelope_kind():
    """cell_case(8): every shape under the full envelope, band(0), band(1), a path envelope and a staircase, 5 samples each."""
    _run_case("envelopes", (sh.ENV_SAMPLES,), name_of_kernel=ENV)
    kinds = {k for ks in sh.env_kinds() for k in ks}
    assert kinds == set(eh.ENV_KINDS)


def test_the_full_envelope_returns_the_bits_of_no_envelope():
    _, seed, groups = sh.case("envelopes")
    for (em, triples), kinds in zip(groups, sh.env_kinds()):
        sub = [t for t, kind in zip(triples, kinds) if kind == "full"]
        assert len(sub) >= 5
        dm = capi.DeviceMachine(em)
        a, b = _open(dm, sub), _open(dm, [(x, P, None) for x, P, _ in sub])
        try:
            ga = a.sample_paths(sh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == ENV
            gb = b.sample_paths(sh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == PLAIN
            assert _same(ga, gb) and len(ga[2]) > 0
        finally:
            a.close(); b.close(); dm.close()


# ---- 3. one call over both geometries, whole and in chunks ------------------------------------------------------------------------------------
def test_mixed_geometries():
    """mixed_case(8): twenty pairs, enveloped first and plain last, dead pairs of each kind.  Two launches, the envelope kernel's
    name, every pair's samples the yardstick's at its own index; dead pairs return empty paths and logq = -inf."""
    _, seed, groups = sh.case("mixed")
    em, triples = groups[0]
    refs = sh.reference("mixed")[0]
    n = sh.MIXED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        whole = dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 2 and capi.last_kernel_name() == ENV
        _check(em, triples, refs, whole, n, what="mixed")
        for k in eh.MIXED_DEAD:
            assert whole[0][k] == -math.inf and (whole[4][k * n:(k + 1) * n] == -math.inf).all() and whole[1][k * n] == whole[1][(k + 1) * n]
    finally:
        dev.close(); dm.close()


def test_mixed_geometries_in_chunks():
    """The mixed batch under 1.8 times the largest pair's bytes (for this call's cost per pair): several chunks, each with its own
    slots and its pairs' own indices in the counter.  The arrays are bit for bit those of the unchunked call, and the yardstick's."""
    _, seed, groups = sh.case("mixed")
    em, triples = groups[0]
    refs = sh.reference("mixed")[0]
    n = sh.MIXED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        whole = dev.sample_paths(n, seed=seed)
        assert dm.n_levels() - 1 == eh.silent_levels(em)
        b = sh.sample_call_bytes(em, triples, n)
        budget = int(eh.MIXED_BUDGET_FACTOR * max(b))
        chunks = eh.greedy_chunks(b, budget)
        assert len(chunks) >= 4
        capi.set_memory_budget(budget)
        cut = dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == eh.chunk_launches(chunks, [t[2] for t in triples]) and capi.last_kernel_name() == ENV
        capi.set_memory_budget(0)
        _check(em, triples, refs, cut, n, what="mixed in chunks")
        assert _same(whole, cut)
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


def test_seeds_and_prefixes():
    """The same seed twice gives the same bits, another seed another path, and the first 3 samples of a 130-sample call are the
    3-sample call's."""
    _, seed, groups = sh.case("mixed")
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
                assert np.array_equal(a[2][s], big[2][t]) and np.array_equal(a[3][s], big[3][t]) and a[4][k * 3 + j] == big[4][k * 130 + j], (k, j)
        # a 64-bit seed: both key words in use
        d = dev.sample_paths(3, seed=seed + (1 << 32))
        assert not (np.array_equal(a[1], d[1]) and np.array_equal(a[2], d[2]))
    finally:
        dev.close(); dm.close()


# ---- 4. slots, determinism, long paths ----------------------------------------------------------------------------------------------------------
def test_full_path_slots():
    """chain_case: every path has exactly the bound's length, so every slot is full end to end and none overflows."""
    _run_case("chain", (3,), name_of_kernel=PLAIN)
    _, seed, groups = sh.case("chain")
    em, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        ll, off, edges, rows, logq = dev.sample_paths(3, seed=seed)
        bounds = [eh.path_bound(dm.n_levels() - 1, len(x), len(P)) for x, P, _ in triples]
        assert list(np.diff(off)) == [b for b in bounds for _ in range(3)] and off[-1] == 3 * dev.path_cap()
    finally:
        dev.close(); dm.close()


def test_one_path_per_pair_is_sampled_every_time():
    """A one-hot profile on a machine with one path per pair: every sample is the Viterbi path and logq = 0 within 1e-9."""
    _run_case("hot", (sh.HOT_SAMPLES,))
    _, seed, groups = sh.case("hot")
    em, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        v, voff, ve, vr = dev.viterbi()
        ll, off, edges, rows, logq = dev.sample_paths(sh.HOT_SAMPLES, seed=seed)
        n = sh.HOT_SAMPLES
        for k in range(len(triples)):
            for j in range(n):
                sl = slice(off[k * n + j], off[k * n + j + 1])
                assert np.array_equal(edges[sl], ve[voff[k]:voff[k + 1]]) and np.array_equal(rows[sl], vr[voff[k]:voff[k + 1]]), (k, j)
        assert np.abs(logq).max() <= 1e-9 and sh.log_close(ll, v)
    finally:
        dev.close(); dm.close()


def test_long_paths():
    """S = 40 at I = L = 120 under band(6), 256 samples of a few hundred edges: every path replayed and its logq held to its
    replayed weight minus the device's likelihood; the first 8 against the yardstick."""
    _run_case("long", (sh.LONG_SAMPLES,), checked=sh.LONG_CHECKED, name_of_kernel=ENV)


# ---- 5. statistics without the yardstick ---------------------------------------------------------------------------------------------------------
def test_usage_of_4096_samples_meets_the_posterior_counts():
    """One pair at (3, 3), S = 3 with levels: the mean usage of every transition whose posterior count is at least 1e-3 lies within 5
    standard errors (from the sample variance) of DeviceProfilePairs.counts(), and the mean number of emitting edges plus the blank
    mass of the row posteriors is L to the same bound."""
    em, triples = sh._stat()[0]
    x, P, _ = triples[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        counts, _, ll = dev.counts()
        post, _ = dev.row_posteriors()
        got = dev.sample_paths(sh.STAT_SAMPLES, seed=sh.STAT_SEED)
        assert ll[0] > -math.inf and got[0][0] == ll[0]
        off, edges = got[1], got[2]
        u = sh.usage(em.nTransitions, [edges[off[j]:off[j + 1]] for j in range(sh.STAT_SAMPLES)])
        assert int((counts >= 1e-3).sum()) >= 8
        bad = sh.usage_within_bound(u, counts, np.nonzero(em.outTok > 0)[0], float(post[:, 0].sum()), len(P))
        assert not bad, bad
    finally:
        dev.close(); dm.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_leave_the_object_usable():
    _, seed, groups = sh.case("ragged")
    em, triples = groups[0]
    refs = sh.reference("ragged")[0]
    n = sh.RAGGED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    merged = capi.DeviceProfilePairs(dm, [triples[3][0]], [np.zeros((4, 3))], colTok=[1, 2])

    def usable():
        assert capi.last_launch_count() == 0
        _check(em, triples, refs, dev.sample_paths(n, seed=seed), n, what="after an error")
    try:
        with pytest.raises(capi.MbError, match="nSamples"):
            dev.sample_paths(0, seed=seed)
        usable()
        need = n * dev.path_cap()
        with pytest.raises(capi.MbError, match="pathCap too small.* %d entries.* %d" % (need - 1, need)):
            dev.sample_paths(n, seed=seed, cap=need - 1)
        usable()
        with pytest.raises(capi.MbError, match="sampling takes plain profiles"):
            merged.sample_paths(n, seed=seed)
        usable()
        capi.set_memory_budget(max(sh.sample_call_bytes(em, triples, n)) - 1)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 0
        capi.set_memory_budget(0)
        usable()
    finally:
        capi.set_memory_budget(0)
        merged.close(); dev.close(); dm.close()


def test_sample_profile_pairs_on_the_device_is_the_numpy_backend():
    """boss.sampleProfilePairs: the device backend returns the numpy backend's paths, with logq and likelihoods to 1e-9."""
    from machineboss_amd import boss
    m, prof, inputs = sh.boss_case()
    for band in sh.BOSS_BANDS:
        pd, qd, ld = boss.sampleProfilePairs(m, inputs, prof, sh.BOSS_SAMPLES, seed=sh.BOSS_SEED, band=band)
        pn, qn, ln = boss.sampleProfilePairs(m, inputs, prof, sh.BOSS_SAMPLES, seed=sh.BOSS_SEED, backend="numpy", band=band)
        assert sh.log_close(ld, ln) and sh.log_close(qd, qn)
        assert [[p.steps for p in ps] for ps in pd] == [[p.steps for p in ps] for ps in pn]
        assert ld[2] == -math.inf and all(not p.steps for p in pd[2])
