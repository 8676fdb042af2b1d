"""GPU tests of the two-tape profile sweeps where one call mixes plain and enveloped pairs (pair_profile_descs, PairWhere and fetch_loglike
in mb_profile_api.hip; docs/profile_tapes.md, "Where a call mixes geometries").  A chunk's plain pairs go through FullGeom in one launch and
its enveloped pairs through EnvGeom in a second; the per-pair outputs are written in slot order (plain first) and mapped back to pair
order, chunk by chunk, while lattices, path slots and scratch rings are packed in pair order.  The references are
profile.PairProfileDP(env=...) called per pair with that pair's envelope or None, PairProfileDP.rowPosteriors and
PairMergedProfileDP; the bounds are those of pairprofilehelpers: log values 1e-9 relative to max(1, |value|) with -inf exact; counts
and posteriors >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x value; row sums 1e-6; Viterbi scores at 1e-12; paths and rows
equal; fixed-point counts the floating-point bound plus 2^-36 per term.  The host's chunking is restated by mergehelpers.greedy_chunks
over pairenvhelpers.call_bytes; test_profile_pair_env_host.py, test_profile_pair_merge_host.py and test_profile_pair_post_host.py
hold the builders to their conditions on the CPU."""
import math

import numpy as np
import pytest

import pairenvhelpers as eh
import pairmergehelpers as pm
import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import capi
from machineboss_amd.profile import PairMergedProfileDP, PairProfileDP

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-6
WORST = {}
ENV_FWD = "k_profile_pair_env_fwd<%s>"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations where a call mixes geometries:", WORST)


def _open(dm, triples, envs=None):
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    envs = [t[2] for t in triples] if envs is None else envs
    if any(e is not None for e in envs):
        dev.set_envelopes(envs)
    return dev


def _split(dev, post):
    return [post[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)]


def _check_paths(v, off, edges, rows, refs, what="viterbi"):
    wv = np.array([r["v"] for r in refs])
    ph.note(what, v, wv, WORST)
    assert logs_close(v, wv, 1e-12), (v, wv)
    assert len(off) == len(refs) + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows)
    for k, r in enumerate(refs):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(edges[sl], r["path"][0]) and np.array_equal(rows[sl], r["path"][1]), (k, edges[sl], r["path"][0])


def _check_posteriors(got, ll, posts, what="posteriors"):
    """The device's per-pair posteriors and likelihoods against rowPosteriors: entries, exact zeros, row sums."""
    want = np.array([p[1] for p in posts])
    ph.note("loglike of " + what, ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    for k, (g, (w, wl)) in enumerate(zip(got, posts)):
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


def _fixed_counts_close(got, want, terms):
    """counts_close with the fixed point's quantum on top: a transition gets at most one term per cell, each rounded once to 2^-36
    (test_counts_past_the_lds_table_under_a_band)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.where(want >= 1e-3, 0.0, ph.COUNT_ABS) + ph.COUNT_REL * want + terms * 2.0 ** -36))


def _terms(triples):
    return sum(eh.n_cells(env) if env is not None else (len(x) + 1) * (len(P) + 1) for x, P, env in triples)


# ---- the mixed batch and its references, computed once per machine and never changed -----------------------------------------------------
_MIXED = {}


def _mixed(S):
    if S not in _MIXED:
        em, triples = eh.mixed_case(S)
        dp = PairProfileDP(em)
        refs = [eh.env_reference(dp, x, P, env, cells=False) for x, P, env in triples]
        posts = [dp.rowPosteriors(x, P, env=env) for x, P, env in triples]
        _MIXED[S] = (em, triples, refs, posts)
    return _MIXED[S]


# ---- 2. one call, everything -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_one_call_over_plain_and_enveloped_pairs(S):
    """The twenty pairs of mixed_case in one object: every call takes two launches and reports the envelope kernel; likelihoods,
    scores, paths, rows, counts, the counts call's per-pair likelihoods and the row posteriors against the per-pair reference; then
    every pair alone returns the bits it had in the batch, and the fixed-point counts of the batch are the exact sum of the pairs'."""
    em, triples, refs, posts = _mixed(S)
    want = np.array([r["ll"] for r in refs]); wv = np.array([r["v"] for r in refs])
    wc = np.sum([r["counts"] for r in refs], axis=0)
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)

    def ran(name):
        assert capi.last_launch_count() == 2 and capi.last_kernel_name() == name, (capi.last_launch_count(), capi.last_kernel_name())
    try:
        assert dev.cells() == sum(eh.lattice_doubles(S, *t) for t in triples)
        fr = dev.forward(capi.MB_ROLLING); ran(ENV_FWD % "sum,rolling")
        fm = dev.forward(capi.MB_MATERIALISE); ran(ENV_FWD % "sum,mat")
        ph.note("forward", fr, want, WORST)
        assert logs_close(fr, want), (fr, want)
        assert np.array_equal(fr, fm), (fr, fm)
        vs = dev.viterbi(paths=False)[0]; ran(ENV_FWD % "max,rolling")
        assert logs_close(vs, wv, 1e-12), (vs, wv)
        v, off, edges, rows = dev.viterbi(); ran(ENV_FWD % "max,mat")
        _check_paths(v, off, edges, rows, refs)
        assert all(off[k + 1] == off[k] and v[k] == -math.inf for k in eh.MIXED_DEAD)
        c, s, ll = dev.counts(); ran("k_profile_pair_env_counts")
        ph.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        ph.note("loglike of counts", ll, want, WORST)
        assert logs_close(ll, want), (ll, want)
        assert s == -math.inf
        post, pl = dev.row_posteriors(); ran("k_profile_pair_env_rowpost")
        assert post.shape == (dev.rowOff[-1], em.nOutTok + 1)
        _check_posteriors(_split(dev, post), pl, posts)
        capi.set_option("MB_DETERMINISTIC", "1")
        cd, sd, lld = dev.counts()
        pd, pld = dev.row_posteriors()
        ph.note_counts(cd, wc, WORST, "fixed-point counts")
        assert _fixed_counts_close(cd, wc, _terms(triples)), np.abs(cd - wc).max()
        assert np.array_equal(lld, ll) and np.array_equal(pld, pl)
        acc = np.zeros_like(cd)
        for k, t in enumerate(triples):
            one = _open(dm, [t])
            try:
                assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.forward(capi.MB_MATERIALISE)[0] == fm[k], k
                assert capi.last_launch_count() == 1 and capi.last_kernel_name() == ("k_profile_pair_fwd<sum,mat>" if t[2] is None else ENV_FWD % "sum,mat")
                assert one.viterbi(paths=False)[0][0] == vs[k], k
                v1, off1, e1, r1 = one.viterbi()
                sl = slice(off[k], off[k + 1])
                assert v1[0] == v[k] and np.array_equal(e1, edges[sl]) and np.array_equal(r1, rows[sl]), k
                c1, s1, l1 = one.counts()
                assert l1[0] == ll[k] and (s1 == ll[k] or (s1 == -math.inf and k in eh.MIXED_DEAD)), k
                acc += c1
                p1, pl1 = one.row_posteriors()
                assert np.array_equal(p1, pd[dev.rowOff[k]:dev.rowOff[k + 1]]) and pl1[0] == pl[k], k
            finally:
                one.close()
        assert np.array_equal(cd, acc) and cd.any(), np.abs(cd - acc).max()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 3. the same batch in chunks ---------------------------------------------------------------------------------------------------------------
def _restated_chunks(call, em, dm, triples):
    """(budget, chunks, launches) of a call over these pairs under mixed_budget, from the restated bytes and chunk rule."""
    assert dm.n_levels() - 1 == eh.silent_levels(em)
    budget = eh.mixed_budget(call, em, triples)
    chunks = eh.greedy_chunks(eh.call_bytes(call, em, triples), budget)
    return budget, chunks, eh.chunk_launches(chunks, [t[2] for t in triples])


@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_materialised_forward_and_paths_in_chunks(S):
    """Five chunks -- mixed with an enveloped pair first, plain, enveloped, mixed with a plain pair first, mixed -- and eight
    launches: every chunk has its own slot permutation, its lattices and path slots start at 0 again, and its likelihoods and path
    lengths land at d_ll + p0 and d_len + p0 in slot order.  The chunked calls return the bits of the unchunked ones."""
    em, triples, refs, _ = _mixed(S)
    want = np.array([r["ll"] for r in refs])
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        assert dev.path_cap() == sum(eh.path_bound(eh.silent_levels(em), len(x), len(P)) for x, P, _ in triples)
        f0 = dev.forward(capi.MB_MATERIALISE)
        p0 = dev.viterbi()
        assert capi.last_launch_count() == 2
        budget, chunks, launches = _restated_chunks("forward", em, dm, triples)
        assert chunks == eh.MIXED_CHUNKS and launches == 8
        capi.set_memory_budget(budget)
        f1 = dev.forward(capi.MB_MATERIALISE)
        assert capi.last_launch_count() == launches
        budget, chunks, launches = _restated_chunks("viterbi", em, dm, triples)
        assert chunks == eh.MIXED_CHUNKS and launches == 8
        capi.set_memory_budget(budget)
        p1 = dev.viterbi()
        assert capi.last_launch_count() == launches
        capi.set_memory_budget(0)
        assert np.array_equal(f0, f1) and logs_close(f1, want), (f0, f1, want)
        for a, b in zip(p0, p1):
            assert np.array_equal(a, b), (a, b)
        _check_paths(*p1, refs, what="viterbi in chunks")
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_counts_in_chunks(S):
    """The same five chunks for counts(): per-pair likelihoods with the unchunked bits, the sum -inf because of the dead pairs; in
    floating point the counts against the reference (the chunks' tables are added on the host, in another order than the atomics
    of one launch); in fixed point the unchunked bits; a preloaded array receives the total once.  Without the dead pairs the sum
    of the likelihoods is the reference's, chunked as well."""
    em, triples, refs, _ = _mixed(S)
    want = np.array([r["ll"] for r in refs]); wc = np.sum([r["counts"] for r in refs], axis=0)
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    live = [k for k in range(len(triples)) if k not in eh.MIXED_DEAD]
    sub = _open(dm, [triples[k] for k in live])
    try:
        c0, s0, l0 = dev.counts()
        assert capi.last_launch_count() == 2
        budget, chunks, launches = _restated_chunks("counts", em, dm, triples)
        assert chunks == eh.MIXED_CHUNKS and launches == 8
        capi.set_memory_budget(budget)
        c1, s1, l1 = dev.counts()
        assert capi.last_launch_count() == launches
        ph.note_counts(c1, wc, WORST, "counts in chunks")
        assert np.array_equal(l0, l1) and logs_close(l1, want) and s0 == s1 == -math.inf
        assert counts_close(c1, wc) and counts_close(c0, wc), (np.abs(c1 - wc).max(), np.abs(c0 - wc).max())
        capi.set_option("MB_DETERMINISTIC", "1")
        d1, _, ld1 = dev.counts()
        assert capi.last_launch_count() == launches
        pre = np.full(dm.nTrans, 2.5)
        got, _, _ = dev.counts(pre)
        assert got is pre and np.array_equal(pre, 2.5 + d1)
        capi.set_memory_budget(0)
        d0, _, ld0 = dev.counts()
        assert capi.last_launch_count() == 2
        assert np.array_equal(d0, d1) and np.array_equal(ld0, ld1) and np.array_equal(ld0, l0) and d0.any()
        assert _fixed_counts_close(d0, wc, _terms(triples))
        capi.set_option("MB_DETERMINISTIC", None)
        # the batch without its dead pairs: a finite sum
        ws = float(np.sum(want[live]))
        _, t0, m0 = sub.counts()
        budget, chunks, launches = _restated_chunks("counts", em, dm, [triples[k] for k in live])
        assert len(chunks) >= 4
        capi.set_memory_budget(budget)
        _, t1, m1 = sub.counts()
        assert capi.last_launch_count() == launches
        assert t0 == t1 and np.array_equal(m0, m1) and np.array_equal(m0, l0[live])
        assert abs(t1 - ws) <= 1e-9 * max(1.0, abs(ws)), (t1, ws)
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); sub.close(); dm.close()


@pytest.mark.parametrize("S", eh.MIXED_STATES)
def test_row_posteriors_in_chunks(S):
    """And for row_posteriors(): the rows go to rowBase in pair order whatever the chunk and the slot, the likelihoods come back
    through the permutation."""
    em, triples, _, posts = _mixed(S)
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        p0, l0 = dev.row_posteriors()
        assert capi.last_launch_count() == 2
        budget, chunks, launches = _restated_chunks("posteriors", em, dm, triples)
        assert chunks == eh.MIXED_CHUNKS and launches == 8
        capi.set_memory_budget(budget)
        p1, l1 = dev.row_posteriors()
        assert capi.last_launch_count() == launches
        assert np.array_equal(l0, l1)
        _check_posteriors(_split(dev, p1), l1, posts, "posteriors in chunks")
        capi.set_option("MB_DETERMINISTIC", "1")
        d1, ld1 = dev.row_posteriors()
        assert capi.last_launch_count() == launches
        capi.set_memory_budget(0)
        d0, ld0 = dev.row_posteriors()
        assert capi.last_launch_count() == 2
        assert np.array_equal(d0, d1) and np.array_equal(ld0, ld1) and np.array_equal(ld0, l0) and d0.any()
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_rolling_sweeps_in_chunks_of_scratch_rings():
    """S = 300: eight pairs at (12, 14) whose rings of 187 200 bytes lie in scratch, plain and under band(12), in the order
    E P P E E E P P, and four small pairs whose rings lie in LDS.  A budget of 2.5 rings: (E, P), (P, E), (E, E), (P, P) -- two mixed
    chunks of two launches, one of each kind alone -- with ringBase packed from 0 in pair order in each.  Rolling Forward and the
    rolling Viterbi scores have the bits of the unchunked call and of each pair alone."""
    em, triples = eh.roll_case()
    envs = [t[2] for t in triples]
    dp = PairProfileDP(em)
    want = np.array([dp.forward(x, P, env=env)[0] for x, P, env in triples])
    wv = np.array([dp.forward(x, P, "max", env=env)[0] for x, P, env in triples])
    chunks = eh.greedy_chunks(eh.call_bytes("rolling", em, triples), eh.ROLL_BUDGET)
    assert eh.chunk_kinds(chunks, envs) == ["EP", "PE", "E", "P"]
    dm = capi.DeviceMachine(em)
    dev = _open(dm, triples)
    try:
        f0, v0 = dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]
        assert capi.last_launch_count() == 2 and capi.last_kernel_name() == ENV_FWD % "max,rolling"
        capi.set_memory_budget(eh.ROLL_BUDGET)
        f1 = dev.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == eh.chunk_launches(chunks, envs) == 6
        v1 = dev.viterbi(paths=False)[0]
        assert capi.last_launch_count() == 6
        capi.set_memory_budget(0)
        ph.note("rolling forward in chunks", f1, want, WORST)
        assert np.array_equal(f0, f1) and logs_close(f1, want), (f0, f1, want)
        assert np.array_equal(v0, v1) and logs_close(v1, wv, 1e-12), (v0, v1, wv)
        for k, t in enumerate(triples):
            one = _open(dm, [t])
            try:
                assert one.forward(capi.MB_ROLLING)[0] == f1[k] and one.viterbi(paths=False)[0][0] == v1[k], k
            finally:
                one.close()
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


# ---- 4. envelopes set, changed and cleared on one object ---------------------------------------------------------------------------------
def _everything(dev):
    """cells() and, bit for bit comparable, materialised Forward, Viterbi with paths, fixed-point counts and posteriors."""
    out = [np.array([dev.cells()]), dev.forward(capi.MB_MATERIALISE)]
    out += list(dev.viterbi())
    c, s, ll = dev.counts()
    out += [c, np.array([s]), ll]
    out += list(dev.row_posteriors())
    return out


def test_envelopes_set_changed_and_cleared_on_one_object():
    """One object taken through: no envelopes, the mix, every pair enveloped, the mix with the kinds swapped, envelopes cleared.
    After each step it returns what a fresh object built in that state returns: nothing of the state before -- envelope tables,
    compact lattices in the workspace, the slot permutation -- is left behind."""
    em, triples, _, _ = _mixed(8)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    capi.set_option("MB_DETERMINISTIC", "1")
    seen = {}
    try:
        for name, envs in eh.mixed_states(triples):
            if name != "plain":
                dev.set_envelopes(envs)
            fresh = _open(dm, triples, envs if envs is not None else [None] * len(triples))
            try:
                want = _everything(fresh)
                launches = capi.last_launch_count()
            finally:
                fresh.close()
            got = _everything(dev)
            assert capi.last_launch_count() == launches == (2 if name in ("mixed", "swapped") else 1), name
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (name, a, b)
            seen[name] = got
        assert seen["plain"][0][0] == seen["cleared"][0][0] > seen["all"][0][0] == seen["mixed"][0][0]
        for a, b in zip(seen["plain"], seen["cleared"]):
            assert np.array_equal(a, b)
        for a, b in zip(seen["mixed"], seen["all"]):      # (the full envelope is no envelope, bit for bit: only the launches differ)
            assert np.array_equal(a, b)
        assert not np.array_equal(seen["mixed"][1], seen["swapped"][1]) and not np.array_equal(seen["mixed"][1], seen["plain"][1])
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 5. the traceback past one block of 64 lanes, per launch -----------------------------------------------------------------------------
def test_traceback_past_one_block_in_both_launches_of_a_call():
    """k_profile_pair_traceback<FullGeom> and <EnvGeom> run a lane per pair in blocks of 64.  129 plain pairs (three blocks, the last
    with one live lane) interleaved with 65 enveloped ones (two blocks) in one call; dead pairs in the last lane of block 0, the
    first of block 1 and the only one of block 2 of the plain launch, and at the first seam of the enveloped one.  The pairs of the
    first 64 slots of either launch, then of the first 65, as objects of their own return pair by pair what the whole batch does."""
    em, triples = eh.seam_case()
    dp = PairProfileDP(em)
    refs = [dict(v=v, path=(e, r)) for v, e, r in (dp.viterbi(x, P, env=env) for x, P, env in triples)]
    slots = eh.slots([t[2] for t in triples])
    dead = [k for k, s in enumerate(slots) if s in eh.SEAM_DEAD_PLAIN + tuple(eh.SEAM_PLAIN + e for e in eh.SEAM_DEAD_ENV)]
    assert len(dead) == 5 and all((refs[k]["v"] == -math.inf) == (k in dead) for k in range(len(refs)))
    dm = capi.DeviceMachine(em)
    got = {}
    try:
        for n in (64, 65, eh.SEAM_PLAIN):
            idx = eh.seam_prefix(triples, n)
            dev = _open(dm, [triples[k] for k in idx])
            try:
                got[n] = (idx,) + dev.viterbi()
                assert capi.last_launch_count() == 2 and capi.last_kernel_name() == ENV_FWD % "max,mat"
            finally:
                dev.close()
    finally:
        dm.close()
    assert got[eh.SEAM_PLAIN][0] == list(range(len(triples)))
    for n, (idx, v, off, edges, rows) in got.items():
        _check_paths(v, off, edges, rows, [refs[k] for k in idx], what="viterbi past one block")
        for j, k in enumerate(idx):
            assert k not in dead or (off[j + 1] == off[j] and v[j] == -math.inf), (n, k)
    _, w, offl, el, rl = got[eh.SEAM_PLAIN]
    for n in (64, 65):
        idx, v, off, edges, rows = got[n]
        for j, k in enumerate(idx):
            assert v[j] == w[k] and np.array_equal(edges[off[j]:off[j + 1]], el[offl[k]:offl[k + 1]]), (n, k)
            assert np.array_equal(rows[off[j]:off[j + 1]], rl[offl[k]:offl[k + 1]]), (n, k)


def test_merged_traceback_past_one_block():
    """k_profile_pair_merge_traceback: 129 pairs against merged profiles of two columns, dead pairs at 63, 64 and 128; batches of
    64 and 65 return for their pairs what the batch of 129 returns for its first."""
    em, colTok, pairs = pm.seam_case()
    dp = PairMergedProfileDP(em, colTok)
    refs = [dict(v=v, path=(e, r)) for v, e, r in (dp.viterbi(x, P) for x, P in pairs)]
    dm = capi.DeviceMachine(em)
    got = {}
    try:
        for n in (64, 65, pm.SEAM_PAIRS):
            dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs[:n]], [P for _, P in pairs[:n]], colTok)
            try:
                got[n] = dev.viterbi()
                assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_pair_merge_fwd<max,mat>"
            finally:
                dev.close()
    finally:
        dm.close()
    for n, (v, off, edges, rows) in got.items():
        assert len(v) == n
        _check_paths(v, off, edges, rows, refs[:n], what="merged viterbi past one block")
        for k in pm.SEAM_DEAD:
            assert k >= n or (off[k + 1] == off[k] and v[k] == -math.inf), (n, k)
    w, offl, el, rl = got[pm.SEAM_PAIRS]
    for n in (64, 65):
        v, off, edges, rows = got[n]
        end = off[-1]
        assert np.array_equal(w[:n], v) and np.array_equal(offl[:n + 1], off) and np.array_equal(el[:end], edges) and np.array_equal(rl[:end], rows), n


# ---- 6. row posteriors past 1 024 row blocks -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrap():
    em, x, P, Pdead = eh.wrap_case()
    dp = PairProfileDP(em)
    I, L = eh.WRAP_SHAPE
    dead = (np.zeros((L, em.nOutTok + 1)), -math.inf)
    return em, x, P, Pdead, {name: [dp.rowPosteriors(x, P, env=env), dead] for name, env in (("plain", None), ("full", eh.full(I, L)), ("stairs", eh.staircase(I, L)))}


@pytest.mark.parametrize("kind", ("plain", "full", "stairs"))
def test_row_posteriors_past_1024_row_blocks(wrap, kind):
    """(1, 1 100) at S = 2: with MB_ROWPOST_TABLE=4 a block is one row, 1 100 blocks for the 1 024 workgroups a pair gets at the
    most, so 76 workgroups take the second pass of the row-block loop (rb += groupsPerPair * R), which re-zeroes and re-stores the
    LDS table; with MB_ROWPOST_TABLE=2 a row does not fit the table and the bins are cleared and summed in global memory, behind a
    fence, with the same wrap.  Plain, under the full envelope and under a staircase (k_profile_pair_env_rowpost); a dead pair of
    the same shape rides along and must come back as exact zeros, rows 1 024 to 1 099 included.  In fixed point every table gives
    the same bits, twice."""
    em, x, P, Pdead, posts = wrap
    I, L = eh.WRAP_SHAPE
    env = {"plain": None, "full": eh.full(I, L), "stairs": eh.staircase(I, L)}[kind]
    name = "k_profile_pair_rowpost" if env is None else "k_profile_pair_env_rowpost"
    dm = capi.DeviceMachine(em)
    dev = _open(dm, [(x, P, env), (x, Pdead, env)])
    try:
        bits = {}
        for table in ("4", "2", None):
            capi.set_option("MB_ROWPOST_TABLE", table)
            capi.set_option("MB_DETERMINISTIC", None)
            post, ll = dev.row_posteriors()
            assert capi.last_launch_count() == 1 and capi.last_kernel_name() == name
            got = _split(dev, post)
            _check_posteriors(got, ll, posts[kind], "posteriors past 1 024 blocks")
            assert ll[1] == -math.inf and not got[1].any() and got[0][eh.WRAP_GROUPS:].any(axis=1).all()
            capi.set_option("MB_DETERMINISTIC", "1")
            d0, l0 = dev.row_posteriors()
            d1, _ = dev.row_posteriors()
            assert np.array_equal(d0, d1) and np.array_equal(l0, ll) and not d0[L:].any()
            bits[table] = d0
        assert np.array_equal(bits["4"], bits[None]) and np.array_equal(bits["2"], bits[None])
        # a bin gets one term per (cell, state) of its row, (I + 1) S = 4 at the most, each rounded once to 2^-36
        assert _fixed_counts_close(bits[None][:L], posts[kind][0][0], (I + 1) * em.nStates)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()
