"""Posterior path samples of pairs against CTC-merged profiles on the device (mb_profile_pairs_sample_merged,
k_profile_pair_merge_sample; docs/profile_tapes.md, "Posterior path samples of pairs against a merged profile") against
profile.PairMergedProfileDP.samplePaths, called per pair with the pair's own index: sampled edges, rows and rowCol for equality, logq
and the likelihoods to 1e-9 relative to max(1, |value|) with -inf exact, and logq against pathWeight of the device's own lattice path
minus the device's likelihood under the same bound.  The cases, their seeds and the margins that make equality a fair demand are
pairmergesamplehelpers'; test_profile_pair_merge_sample_host.py holds them to their conditions on the CPU."""
import math

import numpy as np
import pytest

import pairenvhelpers as eh
import pairmergeenvhelpers as meh
import pairmergesamplehelpers as msh
import pairprofilehelpers as ph
import pairsamplehelpers as sh
from machineboss_amd import capi
from machineboss_amd.profile import PairMergedProfileDP

pytestmark = pytest.mark.gpu

WORST = {}
FULL, ENV = "k_profile_pair_merge_sample", "k_profile_pair_merge_env_sample"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    print("worst deviations of the merged path samples:", WORST)


def _open(dm, colTok, triples):
    return meh.open_pairs(dm, colTok, triples)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _worst(key, got, want):
    WORST[key] = max(WORST.get(key, 0.0), ph.log_dev(got, want))


def _labels(dev, rowCol, n, k, j):
    L = int(dev.rowOff[k + 1] - dev.rowOff[k])
    at = int(dev.rowOff[k]) * n + j * L
    return rowCol[at:at + L]


def _check(em, colTok, triples, refs, dev, got, n, checked=None, what="samples"):
    """One merged_sample_paths result of n samples per pair against the yardstick's first n (checked: only the first so many of each
    pair go against it); every lattice path replayed by pathWeight and its logq held to that weight minus the device's likelihood."""
    ll, off, edges, rows, rowCol, logq = got
    want = np.array([r[0] for r in refs])
    _worst("loglike", ll, want)
    assert msh.log_close(ll, want), (what, ll, want)
    assert len(off) == len(triples) * n + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows) and len(logq) == len(triples) * n
    assert (np.diff(off) >= 0).all() and len(rowCol) == int(dev.rowOff[-1]) * n
    dp = PairMergedProfileDP(em, colTok)
    for k, ((x, P, _env), (wl, samples)) in enumerate(zip(triples, refs)):
        for j in range(n):
            sl = slice(off[k * n + j], off[k * n + j + 1])
            rc = _labels(dev, rowCol, n, k, j)
            if wl == -math.inf:
                assert sl.start == sl.stop and logq[k * n + j] == -math.inf and (rc == -1).all(), (what, k, j)
                continue
            w = dp.pathWeight(x, P, edges[sl], rows[sl], rc)
            assert msh.log_close([logq[k * n + j]], [w - ll[k]]), (what, k, j, logq[k * n + j], w - ll[k])
            _worst("logq against the replay", [logq[k * n + j]], [w - ll[k]])
            if checked is None or j < checked:
                we, wr, wc, wq = samples[j]
                assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr), (what, k, j, edges[sl], we)
                assert np.array_equal(rc, wc), (what, k, j, rc, wc)
                assert msh.log_close([logq[k * n + j]], [wq]), (what, k, j, logq[k * n + j], wq)
                _worst("logq", [logq[k * n + j]], [wq])


def _run_case(name, counts, checked=None, name_of_kernel=None):
    """Every machine of a case: one object, merged_sample_paths at each of `counts`, checked against the case's reference."""
    _, seed, groups = msh.case(name)
    refs = msh.reference(name)
    for (em, colTok, triples), ref in zip(groups, refs):
        dm = capi.DeviceMachine(em)
        dev = _open(dm, colTok, triples)
        try:
            for n in counts:
                got = dev.merged_sample_paths(n, seed=seed)
                if name_of_kernel is not None:
                    assert capi.last_kernel_name() == name_of_kernel, capi.last_kernel_name()
                _check(em, colTok, triples, ref, dev, got, n, checked, "%s at %d samples" % (name, n))
        finally:
            dev.close(); dm.close()


# ---- 1. the basic suite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", msh.BASIC_STATES)
def test_basic_suite(S):
    """pair_machine with and without silent levels against 1, 2 and 4 columns at six shapes from (0, 0) to (5, 4); 1, 3, 64, 65 and
    130 samples: one lane, a partial block, a block exactly, a pair's samples across two blocks, several blocks."""
    _run_case("basic%d" % S, msh.BASIC_SAMPLES, name_of_kernel=FULL)
    assert capi.last_launch_count() == 1


def test_column_maps_and_a_generator():
    """Two columns on one token, every column on one token, a column whose token nothing emits, one column; I = 0 on a machine
    without an input alphabet."""
    _run_case("maps", (5,), name_of_kernel=FULL)


def test_block_boundaries_fall_inside_pairs():
    """Ten ragged pairs at 7 samples: 70 lanes, the block boundary inside pair 9's samples, lanes of one wavefront on ten lattices;
    the dead pair has empty paths, -inf and rowCol = -1 in every row (_check)."""
    _run_case("ragged", (msh.RAGGED_SAMPLES,), name_of_kernel=FULL)
    lls = [ll for ll, _ in msh.reference("ragged")[0]]
    assert sum(ll == -math.inf for ll in lls) == 1


# ---- 2. envelopes ---------------------------------------------------------------------------------------------------------------------------
def test_every_envelope_kind():
    """cell_case(2, 8): every shape under the full envelope, band(0), band(1), a path envelope and a staircase, 5 samples each."""
    _run_case("envelopes", (msh.ENV_SAMPLES,), name_of_kernel=ENV)
    assert {k for ks in msh.env_kinds() for k in ks} == set(eh.ENV_KINDS)


def test_the_full_envelope_returns_the_bits_of_no_envelope():
    _, seed, groups = msh.case("envelopes")
    for (em, colTok, triples), kinds in zip(groups, msh.env_kinds()):
        sub = [t for t, kind in zip(triples, kinds) if kind == "full"]
        assert len(sub) >= 5
        dm = capi.DeviceMachine(em)
        a, b = _open(dm, colTok, sub), _open(dm, colTok, [(x, P, None) for x, P, _ in sub])
        try:
            ga = a.merged_sample_paths(msh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == ENV
            gb = b.merged_sample_paths(msh.ENV_SAMPLES, seed=seed)
            assert capi.last_kernel_name() == FULL
            assert _same(ga, gb) and len(ga[2]) > 0
        finally:
            a.close(); b.close(); dm.close()


# ---- 3. one call over both kinds, whole and in chunks ---------------------------------------------------------------------------------------
def test_mixed_kinds():
    """mixed_case(8): twenty pairs, enveloped first and plain last, dead pairs of each kind.  Two launches, the envelope kernel's
    name, every pair's samples the yardstick's at its own index -- whatever slot the pair landed in."""
    _, seed, groups = msh.case("mixed")
    em, colTok, triples = groups[0]
    refs = msh.reference("mixed")[0]
    n = msh.MIXED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    try:
        whole = dev.merged_sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 2 and capi.last_kernel_name() == ENV
        _check(em, colTok, triples, refs, dev, whole, n, what="mixed")
        for k in eh.MIXED_DEAD:
            assert whole[0][k] == -math.inf and (whole[5][k * n:(k + 1) * n] == -math.inf).all() and whole[1][k * n] == whole[1][(k + 1) * n]
    finally:
        dev.close(); dm.close()


def test_mixed_kinds_in_chunks():
    """The mixed batch under 1.8 times the largest pair's bytes (for this call's cost per pair): several chunks, each with its own
    slots, its own block of rowCol and its pairs' own indices in the counter.  The arrays are bit for bit those of the unchunked
    call, and the yardstick's."""
    _, seed, groups = msh.case("mixed")
    em, colTok, triples = groups[0]
    refs = msh.reference("mixed")[0]
    n = msh.MIXED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    try:
        whole = dev.merged_sample_paths(n, seed=seed)
        assert dm.n_levels() - 1 == eh.silent_levels(em)
        b = msh.sample_call_bytes(em, len(colTok), triples, n)
        budget = int(eh.MIXED_BUDGET_FACTOR * max(b))
        chunks = eh.greedy_chunks(b, budget)
        assert len(chunks) >= 4
        capi.set_memory_budget(budget)
        cut = dev.merged_sample_paths(n, seed=seed)
        assert capi.last_launch_count() == eh.chunk_launches(chunks, [t[2] for t in triples]) and capi.last_kernel_name() == ENV
        capi.set_memory_budget(0)
        _check(em, colTok, triples, refs, dev, cut, n, what="mixed in chunks")
        assert _same(whole, cut)
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


def test_seeds_prefixes_and_batch_order():
    """The same seed twice gives the same bits, another seed another path, the first 3 samples of a 130-sample call are the 3-sample
    call's, and the batch reversed gives pair k the yardstick's samples under its new index k."""
    _, seed, groups = msh.case("mixed")
    em, colTok, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    try:
        a, b = dev.merged_sample_paths(3, seed=seed), dev.merged_sample_paths(3, seed=seed)
        assert _same(a, b)
        c = dev.merged_sample_paths(3, seed=msh.SEED_B)
        assert np.array_equal(a[0], c[0]) and not (np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]) and np.array_equal(a[4], c[4]))
        big = dev.merged_sample_paths(130, seed=seed)
        assert np.array_equal(big[0], a[0])
        for k in range(len(triples)):
            for j in range(3):
                s, t = slice(a[1][k * 3 + j], a[1][k * 3 + j + 1]), slice(big[1][k * 130 + j], big[1][k * 130 + j + 1])
                assert np.array_equal(a[2][s], big[2][t]) and np.array_equal(a[3][s], big[3][t]) and a[5][k * 3 + j] == big[5][k * 130 + j], (k, j)
                assert np.array_equal(_labels(dev, a[4], 3, k, j), _labels(dev, big[4], 130, k, j)), (k, j)
        # a 64-bit seed: both key words in use
        d = dev.merged_sample_paths(3, seed=seed + (1 << 32))
        assert not (np.array_equal(a[1], d[1]) and np.array_equal(a[2], d[2]) and np.array_equal(a[4], d[4]))
    finally:
        dev.close()
    back = triples[::-1][:6]
    dp = PairMergedProfileDP(em, colTok)
    margins = []
    refs = [dp.samplePaths(x, P, 3, seed=seed, pair=k, env=env, margins=margins) for k, (x, P, env) in enumerate(back)]
    assert min(margins) > msh.MARGIN
    dev = _open(dm, colTok, back)
    try:
        _check(em, colTok, back, refs, dev, dev.merged_sample_paths(3, seed=seed), 3, what="reversed")
    finally:
        dev.close(); dm.close()


# ---- 4. one lattice path, long paths -------------------------------------------------------------------------------------------------------
def test_one_hot_frames_are_sampled_as_their_argmax():
    """One-hot merged frames on a machine with one path per input: every sample is the Viterbi path with logq = 0 within 1e-9, and
    rowCol is the frames' argmax -- held symbols as repeats, the blanks between equal symbols as blanks."""
    _run_case("hot", (msh.HOT_SAMPLES,))
    _, seed, groups = msh.case("hot")
    em, colTok, triples = groups[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    try:
        v, voff, ve, vr = dev.viterbi()
        n = msh.HOT_SAMPLES
        ll, off, edges, rows, rowCol, logq = dev.merged_sample_paths(n, seed=seed)
        for k, labels in enumerate(msh.hot_labels()):
            for j in range(n):
                sl = slice(off[k * n + j], off[k * n + j + 1])
                assert np.array_equal(edges[sl], ve[voff[k]:voff[k + 1]]) and np.array_equal(rows[sl], vr[voff[k]:voff[k + 1]]), (k, j)
                assert np.array_equal(_labels(dev, rowCol, n, k, j), labels), (k, j)
        assert np.abs(logq).max() <= 1e-9 and msh.log_close(ll, v)
    finally:
        dev.close(); dm.close()


def test_long_paths():
    """S = 40, four columns, I = L = 60 under band(6), 256 samples: every lattice path replayed by pathWeight and its logq held to
    that weight minus the device's likelihood; the first 8 against the yardstick."""
    _run_case("long", (msh.LONG_SAMPLES,), checked=msh.LONG_CHECKED, name_of_kernel=ENV)


# ---- 5. statistics without the yardstick ---------------------------------------------------------------------------------------------------
def test_4096_samples_meet_the_posterior_counts_and_the_row_posteriors():
    """One pair at (3, 3), S = 3 with levels, two columns: the mean usage of every transition whose posterior count is at least 1e-3
    lies within 5 standard errors (from the sample variance) of DeviceProfilePairs.counts(), and the mean of rowCol == c per row
    within 5 standard errors of merged_row_posteriors()."""
    (em, colTok, triples), = msh._stat()
    x, P, _ = triples[0]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    try:
        counts, _, ll = dev.counts()
        post, _ = dev.merged_row_posteriors()
        n = msh.STAT_SAMPLES
        got = dev.merged_sample_paths(n, seed=msh.STAT_SEED)
        assert ll[0] > -math.inf and got[0][0] == ll[0]
        off, edges, rowCol = got[1], got[2], got[4]
        u = sh.usage(em.nTransitions, [edges[off[j]:off[j + 1]] for j in range(n)])
        assert int((counts >= 1e-3).sum()) >= 8
        rc = rowCol.reshape(n, len(P))
        t = np.nonzero(counts >= 1e-3)[0]
        mean, se = u.mean(axis=0), u.std(axis=0, ddof=1) / math.sqrt(n)
        bad = [(int(e), float(mean[e]), float(counts[e])) for e in t if not abs(mean[e] - counts[e]) <= 5.0 * se[e]]
        assert not bad, bad
        bad = msh.row_col_within_bound(rc, post)
        assert not bad, bad
    finally:
        dev.close(); dm.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_leave_the_object_usable():
    _, seed, groups = msh.case("ragged")
    em, colTok, triples = groups[0]
    refs = msh.reference("ragged")[0]
    n = msh.RAGGED_SAMPLES
    dm = capi.DeviceMachine(em)
    dev = _open(dm, colTok, triples)
    plain = capi.DeviceProfilePairs(dm, [triples[3][0]], [np.zeros((4, em.nOutTok + 1))])

    def usable():
        assert capi.last_launch_count() == 0
        _check(em, colTok, triples, refs, dev, dev.merged_sample_paths(n, seed=seed), n, what="after an error")
    try:
        with pytest.raises(capi.MbError, match="nSamples"):
            dev.merged_sample_paths(0, seed=seed)
        usable()
        need = n * dev.path_cap()
        with pytest.raises(capi.MbError, match="pathCap too small.* %d entries.* %d" % (need - 1, need)):
            dev.merged_sample_paths(n, seed=seed, cap=need - 1)
        usable()
        with pytest.raises(capi.MbError, match="merged sampling takes merged profiles"):
            plain.merged_sample_paths(n, seed=seed)
        usable()
        with pytest.raises(capi.MbError, match="sampling takes plain profiles"):
            dev.sample_paths(n, seed=seed)
        usable()
        capi.set_memory_budget(max(msh.sample_call_bytes(em, len(colTok), triples, n)) - 1)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.merged_sample_paths(n, seed=seed)
        assert capi.last_launch_count() == 0
        capi.set_memory_budget(0)
        usable()
    finally:
        capi.set_memory_budget(0)
        plain.close(); dev.close(); dm.close()


def test_sample_merged_pairs_on_the_device_is_the_numpy_backend():
    """boss.sampleMergedPairs: the device backend returns the numpy backend's paths and frame labels, with logq and likelihoods to 1e-9."""
    from machineboss_amd import boss
    m, prof, inputs = msh.boss_case()
    for band in msh.BOSS_BANDS:
        pd, cd, qd, ld = boss.sampleMergedPairs(m, inputs, prof, msh.BOSS_SAMPLES, seed=msh.BOSS_SEED, band=band)
        pn, cn, qn, ln = boss.sampleMergedPairs(m, inputs, prof, msh.BOSS_SAMPLES, seed=msh.BOSS_SEED, backend="numpy", band=band)
        assert msh.log_close(ld, ln) and msh.log_close(qd, qn)
        assert [[p.steps for p in ps] for ps in pd] == [[p.steps for p in ps] for ps in pn]
        assert all(np.array_equal(a, b) for ca, cb in zip(cd, cn) for a, b in zip(ca, cb))
        assert ld[2] == -math.inf and all(not p.steps for p in pd[2]) and all((c == -1).all() for c in cd[2])
