"""GPU tests of pairs against CTC-merged profiles under an envelope (k_profile_pair_merge_env_* in mb_profile_pair_merge.hip;
docs/profile_tapes.md, "Pairs against a merged profile under an envelope").  The reference is profile.PairMergedProfileDP(env=...)
called per pair; the bounds are the family's (pairmergeenvhelpers): log values 1e-9 relative to max(1, |value|) with -inf exact;
counts and posteriors >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x value; row sums 1e-6; Viterbi scores at 1e-12 with
equal paths and rows; fixed-point quantities the same plus (cells of the call) x 2^-36; "the same bits" is ==.
test_profile_pair_merge_env_host.py holds the builders to their conditions on the CPU."""
import math

import numpy as np
import pytest

import pairmergeenvhelpers as me
import pairmergehelpers as mh
import pairprofilehelpers as ph
from pairenvhelpers import diag_max, full, n_cells, staircase
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import capi
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP
from machineboss_amd.seqpair import Envelope

pytestmark = pytest.mark.gpu

WORST = me.WORST


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the merged pairs under an envelope:", WORST)


def _kw(env):
    return {} if env is None else {"env": env}


def _everything(dev):
    """cells() and, bit for bit comparable (call under MB_DETERMINISTIC=1), rolling and materialised Forward, Viterbi scores, paths
    and rows, counts and merged row posteriors."""
    out = [np.array([dev.cells()]), dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]]
    out += list(dev.viterbi())
    c, s, ll = dev.counts()
    out += [c, np.array([s]), ll]
    out += list(dev.merged_row_posteriors())
    return out


def _same(a, b, what=None):
    for u, v in zip(a, b):
        assert np.array_equal(u, v), (what, u, v)


# ---- 1. every cell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", me.CELL_CASES)
def test_every_cell_under_every_envelope(nCols, S):
    """The machine with silent levels and without at seven lattices from (0, 0) to (9, 9) under the full envelope, band(0), band(1),
    a path envelope and a staircase, in one batch per machine: all three fills cell by cell with -inf outside in both layers and all
    planes, Forward rolling and materialised, Viterbi with paths, counts and merged row posteriors."""
    live = []
    for em, colTok, quads in me.cell_case(nCols, S):
        me.check_env_batch(em, colTok, [(x, P, env) for x, P, _, env in quads], fill=True, live=live)
        assert capi.last_kernel_name() == me.ENV_FWD % "max,mat"
    assert np.mean(live) >= (0.9 if nCols > 1 else 0.5), np.mean(live)      # (one column cannot take two rows in a row: band(0) on a square is dead)


# ---- 2. the ring marks ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def marks():
    em = me.mark_machine()
    dp = PairMergedProfileDP(em, me.MARK_COLTOK)
    triples = [me.mark_case(M) for M in me.MARK_M] + list(me.mark_extras())
    want = np.array([dp.forward(x, P, **_kw(env))[0] for x, P, env in triples])
    wv = np.array([dp.forward(x, P, "max", **_kw(env))[0] for x, P, env in triples])
    return em, triples, want, wv


def _scores(dev):
    return [dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0], dev.viterbi()[0], dev.counts()[2],
            dev.merged_row_posteriors()[1]]


def test_rings_either_side_of_the_marks(marks):
    """nCols = 4, S = 80, I = L = 40: the rolling ring of 336 M S bytes at M = 2 | 3 (64 KiB, where the dynamic-LDS attribute is
    raised) and 6 | 7 (160 KiB, where the ring moves to scratch); the X / T ring of the materialised sweeps, 96 M S bytes, at M = 8 | 9
    and 21 | 22.  Each pair alone, all of them in one ragged launch beside a pair without an envelope and a dead pair, and each alone
    again on the workspace the batch left behind: alone is the batch to the same bits, rolling is materialised to the same bits,
    the Backward's likelihood (through T in the same ring) is the Forward's within the bound."""
    em, triples, want, wv = marks
    S = em.nStates
    for M, lo in zip(me.MARK_ROLLING, (True, False, True, False)):
        assert (me.ring_bytes(S, 4, M) <= (me.LDS_DEFAULT if M < 5 else me.LDS_MAX)) == lo
    for M, lo in zip(me.MARK_MAT, (True, False, True, False)):
        assert (me.ring_bytes(S, 4, M, True) <= (me.LDS_DEFAULT if M < 15 else me.LDS_MAX)) == lo
    assert [diag_max(t[2]) for t in triples[:8]] == list(me.MARK_M)
    dm = capi.DeviceMachine(em)
    try:
        def alone(k):
            one = me.open_pairs(dm, me.MARK_COLTOK, [triples[k]])
            try:
                return [a[0] for a in _scores(one)]
            finally:
                one.close()
        first = [alone(k) for k in range(len(triples))]
        dev = me.open_pairs(dm, me.MARK_COLTOK, triples)
        try:
            batch = _scores(dev)
            assert capi.last_launch_count() == 2 and capi.last_kernel_name() == "k_profile_pair_merge_env_rowpost"
        finally:
            dev.close()
        again = [alone(k) for k in range(len(triples))]
    finally:
        dm.close()
    fr, fm, vr, vm, cl, pl = batch
    ph.note("forward at the marks", fr, want, WORST)
    assert logs_close(fr, want), (fr, want)
    assert logs_close(vr, wv, 1e-12), (vr, wv)
    assert np.array_equal(fr, fm) and np.array_equal(vr, vm) and np.array_equal(cl, fm) and np.array_equal(pl, fm)
    assert fr[-1] == -math.inf and np.all(fr[:-1] > -math.inf)
    for k in range(len(triples)):
        assert first[k] == again[k] == [a[k] for a in batch], (k, first[k], again[k])


def test_backward_through_the_t_ring_at_the_marks(marks):
    """The Backward lattices of the pairs whose T ring lies either side of 64 KiB and 160 KiB, against the yardstick's likelihood:
    NB[0][0][0][0] of the fill."""
    em, triples, want, _ = marks
    dm = capi.DeviceMachine(em)
    try:
        for k, M in enumerate(me.MARK_M):
            if M not in me.MARK_MAT:
                continue
            x, P, env = triples[k]
            got = capi.profile_pair_fill_merged(dm, capi.MB_BACKWARD, x, P, me.MARK_COLTOK, env)
            assert capi.last_kernel_name() == "k_profile_pair_merge_env_bwd"
            ph.note("backward at the marks", [got[0, 0, 0, 0, 0]], [want[k]], WORST)
            assert logs_close([got[0, 0, 0, 0, 0]], [want[k]]), (M, got[0, 0, 0, 0, 0], want[k])
    finally:
        dm.close()


# ---- 3. one call over both kinds ---------------------------------------------------------------------------------------------------------
_MIXED = {}


def _mixed(S):
    if S not in _MIXED:
        em, colTok, triples = me.mixed_case(S)
        dp = PairMergedProfileDP(em, colTok)
        _MIXED[S] = (em, colTok, triples, [me.env_reference(dp, x, P, env, cells=False) for x, P, env in triples])
    return _MIXED[S]


@pytest.mark.parametrize("S", me.MIXED_STATES)
def test_one_call_over_plain_and_enveloped_pairs(S):
    """Twenty pairs, enveloped and plain-merged interleaved, (0, 0), no rows, no input and a dead pair of each kind among them: every
    call takes two launches and reports the envelope kernel; everything against the per-pair reference; every pair alone returns its
    bits of the batch; the fixed-point counts of the batch are the exact sum of the pairs', its posteriors their stack."""
    em, colTok, triples, refs = _mixed(S)
    want = np.array([r["ll"] for r in refs]); wv = np.array([r["v"] for r in refs])
    wc = np.sum([r["counts"] for r in refs], axis=0)
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, triples)

    def ran(name):
        assert capi.last_launch_count() == 2 and capi.last_kernel_name() == name, (capi.last_launch_count(), capi.last_kernel_name())
    try:
        assert dev.cells() == sum(me.lattice_doubles(S, 4, *t) for t in triples)
        fr = dev.forward(capi.MB_ROLLING); ran(me.ENV_FWD % "sum,rolling")
        fm = dev.forward(capi.MB_MATERIALISE); ran(me.ENV_FWD % "sum,mat")
        ph.note("forward", fr, want, WORST)
        assert logs_close(fr, want), (fr, want)
        assert np.array_equal(fr, fm), (fr, fm)
        vs = dev.viterbi(paths=False)[0]; ran(me.ENV_FWD % "max,rolling")
        assert logs_close(vs, wv, 1e-12), (vs, wv)
        v, off, edges, rows = dev.viterbi(); ran(me.ENV_FWD % "max,mat")
        me.check_paths(v, off, edges, rows, refs)
        assert all(off[k + 1] == off[k] and v[k] == -math.inf for k in me.MIXED_DEAD)
        c, s, ll = dev.counts(); ran("k_profile_pair_merge_env_counts")
        ph.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and s == -math.inf
        post, pl = dev.merged_row_posteriors(); ran("k_profile_pair_merge_env_rowpost")
        me.check_posteriors(me.split(dev, post), pl, [r["post"] for r in refs])
        capi.set_option("MB_DETERMINISTIC", "1")
        cd, _, lld = dev.counts()
        pd, pld = dev.merged_row_posteriors()
        assert me.fixed_close(cd, wc, me.terms(4, triples)), np.abs(cd - wc).max()
        assert np.array_equal(lld, ll) and np.array_equal(pld, pl)
        acc = np.zeros_like(cd)
        for k, t in enumerate(triples):
            one = me.open_pairs(dm, colTok, [t])
            try:
                assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.forward(capi.MB_MATERIALISE)[0] == fm[k], k
                assert capi.last_launch_count() == 1 and capi.last_kernel_name() == (me.FULL_FWD if t[2] is None else me.ENV_FWD) % "sum,mat"
                assert one.viterbi(paths=False)[0][0] == vs[k], k
                v1, off1, e1, r1 = one.viterbi()
                sl = slice(off[k], off[k + 1])
                assert v1[0] == v[k] and np.array_equal(e1, edges[sl]) and np.array_equal(r1, rows[sl]), k
                c1, s1, l1 = one.counts()
                assert l1[0] == ll[k], k
                acc += c1
                p1, pl1 = one.merged_row_posteriors()
                assert np.array_equal(p1, pd[dev.rowOff[k]:dev.rowOff[k + 1]]) and pl1[0] == pl[k], k
            finally:
                one.close()
        assert np.array_equal(cd, acc) and cd.any(), np.abs(cd - acc).max()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


@pytest.mark.parametrize("S", me.MIXED_STATES)
def test_the_mixed_batch_in_chunks(S):
    """The same batch under a budget of 1.8 times the largest pair of each call: chunks of every kind -- mixed with an enveloped pair
    first, plain only, enveloped only, mixed with a plain pair first -- whose lattices, path slots and rings start at 0 again and
    whose per-pair outputs land in slot order.  The chunked results are the unchunked bits (fixed point for the sums)."""
    em, colTok, triples, refs = _mixed(S)
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, triples)
    assert dm.n_levels() - 1 == me.eh.silent_levels(em)
    calls = {"forward": lambda: [dev.forward(capi.MB_MATERIALISE)], "viterbi": lambda: list(dev.viterbi()),
             "counts": lambda: [a if i != 1 else np.array([a]) for i, a in enumerate(dev.counts())], "posteriors": lambda: list(dev.merged_row_posteriors())}
    try:
        capi.set_option("MB_DETERMINISTIC", "1")
        for call, run in calls.items():
            capi.set_memory_budget(0)
            whole = run()
            assert capi.last_launch_count() == 2
            budget, chunks, kinds, launches = me.mixed_chunks(call, em, triples)
            assert set(kinds) == me.CHUNK_KINDS and launches == len(chunks) + sum(len(k) == 2 for k in kinds)
            capi.set_memory_budget(budget)
            parts = run()
            assert capi.last_launch_count() == launches, (call, capi.last_launch_count(), launches)
            _same(whole, parts, call)
        capi.set_memory_budget(0)
        me.check_paths(*dev.viterbi(), refs, what="viterbi in chunks")
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 4. the full envelope is no envelope ---------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope_on_the_device():
    """Rolling and materialised Forward, Viterbi scores, paths and rows, fixed-point counts and posteriors of the mixed batch's pairs
    under the full envelope are the bits they have without one; only the kernels differ."""
    em, colTok, triples, _ = _mixed(8)
    dm = capi.DeviceMachine(em)
    capi.set_option("MB_DETERMINISTIC", "1")
    plain = me.open_pairs(dm, colTok, triples, [None] * len(triples))
    env = me.open_pairs(dm, colTok, triples, [full(len(x), len(P)) for x, P, _ in triples])
    try:
        a = _everything(plain)
        assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_pair_merge_rowpost"
        b = _everything(env)
        assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_pair_merge_env_rowpost"
        _same(a, b)
        assert np.isfinite(a[1]).sum() >= 17
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        plain.close(); env.close(); dm.close()


# ---- 5. envelopes set, changed, cleared --------------------------------------------------------------------------------------------------
def test_envelopes_set_changed_and_cleared_on_one_object():
    """One object taken through: no envelopes, the mix, every pair enveloped, the mix with the kinds swapped, envelopes cleared.
    After each step it returns what a fresh object built in that state returns.  set_merged_profiles leaves the envelopes in place."""
    em, colTok, triples, _ = _mixed(8)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples], colTok)
    capi.set_option("MB_DETERMINISTIC", "1")
    seen = {}
    try:
        for name, envs in me.mixed_states(triples):
            if name != "plain":
                dev.set_merged_envelopes(envs)
            fresh = me.open_pairs(dm, colTok, triples, envs if envs is not None else [None] * len(triples))
            try:
                want = _everything(fresh)
                launches = capi.last_launch_count()
            finally:
                fresh.close()
            got = _everything(dev)
            assert capi.last_launch_count() == launches == (2 if name in ("mixed", "swapped") else 1), name
            _same(got, want, name)
            seen[name] = got
        assert seen["plain"][0][0] == seen["cleared"][0][0] > seen["all"][0][0] == seen["mixed"][0][0]
        _same(seen["plain"], seen["cleared"])
        assert not np.array_equal(seen["mixed"][2], seen["swapped"][2]) and not np.array_equal(seen["mixed"][2], seen["plain"][2])
        # new rows under the envelopes that are there
        envs = [t[2] for t in triples]
        dev.set_merged_envelopes(envs)
        moved = [(x, P + 0.125 * np.arange(P.shape[1]), env) for x, P, env in triples]
        dev.set_merged_profiles([t[1] for t in moved])
        fresh = me.open_pairs(dm, colTok, moved)
        try:
            want = _everything(fresh)
        finally:
            fresh.close()
        got = _everything(dev)
        assert capi.last_launch_count() == 2
        _same(got, want, "new rows")
        assert not np.array_equal(got[2], seen["mixed"][2])
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 6. counts past 8 192 transitions under a band ---------------------------------------------------------------------------------------
def test_counts_past_the_lds_table_under_a_band():
    """11 204 transitions: CountsAcc adds into global memory.  Three pairs and a dead one under band(2), in floating and in fixed
    point (every term rounded once to 2^-36, at most one term per (cell, plane) of the call for a transition)."""
    em, colTok, triples = me.big_counts_env_case()
    dp = PairMergedProfileDP(em, colTok)
    res = [dp.counts(x, P, env=env) for x, P, env in triples]
    wc = np.sum([r[0] for r in res], axis=0); want = np.array([r[1] for r in res])
    assert want[-1] == -math.inf and np.all(want[:-1] > -math.inf) and em.nTransitions > 8192
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, triples)
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_pair_merge_env_counts" and capi.last_launch_count() == 1
        ph.note_counts(c, wc, WORST, "counts past the table")
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and s == -math.inf
        capi.set_option("MB_DETERMINISTIC", "1")
        d0, _, l0 = dev.counts()
        d1, _, _ = dev.counts()
        assert np.array_equal(d0, d1) and np.array_equal(l0, ll) and d0.any()
        assert me.fixed_close(d0, wc, me.terms(len(colTok), triples)), np.abs(d0 - wc).max()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 7. ties -------------------------------------------------------------------------------------------------------------------------------
def test_ties_under_a_band():
    """merged_tie_machine on tie_pairs under band(1): weights that are multiples of log 0.5, so candidates tie exactly, and the band
    cuts off the source cell of a repeat, an output-only or an input-only candidate.  Scores, paths and rows are the yardstick's."""
    em = mh.merged_tie_machine()
    triples = me.tie_env_pairs()
    dp = PairMergedProfileDP(em, mh.TIE_COLTOK)
    census = {}
    refs = [dict(v=v, path=(e, r)) for v, e, r in (dp.viterbi(x, P, census=census, env=env) for x, P, env in triples)]
    assert all(census.get(k, 0) >= 1 for k in mh.TIE_KINDS), census
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, mh.TIE_COLTOK, triples)
    try:
        v, off, edges, rows = dev.viterbi()
        assert np.array_equal(v, np.array([r["v"] for r in refs]))      # (sums of multiples of log 0.5 in one order: no rounding to differ by)
        me.check_paths(v, off, edges, rows, refs, what="ties")
        assert np.array_equal(dev.viterbi(paths=False)[0], v)
    finally:
        dev.close(); dm.close()


# ---- 8. the traceback past one block -------------------------------------------------------------------------------------------------------
def test_traceback_past_one_block_in_both_launches_of_a_call():
    """129 enveloped pairs (three blocks of 64 lanes, the last with one live lane) interleaved with 65 plain-merged ones (two
    blocks); dead pairs in the last lane of block 0, the first of block 1 and the only one of block 2 of the enveloped launch, and at
    the first seam of the plain one.  The pairs of the first 64 slots of either launch, then of the first 65, as objects of their
    own return pair by pair what the whole batch does."""
    em, colTok, triples = me.seam_case()
    dp = PairMergedProfileDP(em, colTok)
    refs = [dict(v=v, path=(e, r)) for v, e, r in (dp.viterbi(x, P, **_kw(env)) for x, P, env in triples)]
    slots = me.eh.slots([t[2] for t in triples])
    dead = [k for k, s in enumerate(slots) if s in me.SEAM_DEAD_PLAIN + tuple(me.SEAM_PLAIN + e for e in me.SEAM_DEAD_ENV)]
    assert len(dead) == 5 and all(refs[k]["v"] == -math.inf for k in dead)
    assert sum(r["v"] > -math.inf for r in refs) >= 0.9 * len(refs)      # (a narrow envelope against two columns may admit no path: a few more)
    dm = capi.DeviceMachine(em)
    got = {}
    try:
        for n in (64, 65, me.SEAM_ENV):
            idx = me.seam_prefix(triples, n)
            dev = me.open_pairs(dm, colTok, [triples[k] for k in idx])
            try:
                got[n] = (idx,) + dev.viterbi()
                assert capi.last_launch_count() == 2 and capi.last_kernel_name() == me.ENV_FWD % "max,mat"
            finally:
                dev.close()
    finally:
        dm.close()
    assert got[me.SEAM_ENV][0] == list(range(len(triples)))
    for n, (idx, v, off, edges, rows) in got.items():
        me.check_paths(v, off, edges, rows, [refs[k] for k in idx], what="viterbi past one block")
        for j, k in enumerate(idx):
            assert k not in dead or (off[j + 1] == off[j] and v[j] == -math.inf), (n, k)
    _, w, offl, el, rl = got[me.SEAM_ENV]
    for n in (64, 65):
        idx, v, off, edges, rows = got[n]
        for j, k in enumerate(idx):
            assert v[j] == w[k] and np.array_equal(edges[off[j]:off[j + 1]], el[offl[k]:offl[k + 1]]), (n, k)
            assert np.array_equal(rows[off[j]:off[j + 1]], rl[offl[k]:offl[k + 1]]), (n, k)


# ---- 9. row posteriors past the table and past 1 024 row blocks ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrap():
    em, colTok, x, P, Pdead = me.wrap_case()
    dp = PairMergedProfileDP(em, colTok)
    I, L = me.WRAP_SHAPE
    dead = (np.zeros((L, len(colTok) + 1)), -math.inf)
    return em, colTok, x, P, Pdead, {name: [dp.rowPosteriors(x, P, env=env), dead] for name, env in (("full", full(I, L)), ("stairs", staircase(I, L)))}


@pytest.mark.parametrize("kind", ("full", "stairs"))
def test_row_posteriors_past_the_table_and_past_1024_row_blocks(wrap, kind):
    """(1, 1 100) at S = 2, nCols = 4: with MB_ROWPOST_TABLE at 4 and at 2 a row of five bins does not fit the table, its bins are
    cleared and summed in global memory behind a fence, one row a block: 1 100 blocks for the 1 024 workgroups a pair gets, so 76
    workgroups take a second pass of the row-block loop.  The default keeps blocks of rows in LDS.  Under the full envelope and
    under a staircase, whose rows have one or two cells; a dead pair rides along and comes back as exact zeros.  In fixed point the
    bits are the same twice and under every table."""
    em, colTok, x, P, Pdead, posts = wrap
    I, L = me.WRAP_SHAPE
    env = {"full": full(I, L), "stairs": staircase(I, L)}[kind]
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, [(x, P, env), (x, Pdead, env)])
    try:
        bits = {}
        for table in ("4", "2", None):
            capi.set_option("MB_ROWPOST_TABLE", table)
            capi.set_option("MB_DETERMINISTIC", None)
            post, ll = dev.merged_row_posteriors()
            assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_pair_merge_env_rowpost"
            got = me.split(dev, post)
            me.check_posteriors(got, ll, posts[kind], "posteriors past 1 024 blocks")
            assert ll[1] == -math.inf and not got[1].any() and got[0][me.WRAP_GROUPS:].any(axis=1).all()
            capi.set_option("MB_DETERMINISTIC", "1")
            d0, l0 = dev.merged_row_posteriors()
            d1, _ = dev.merged_row_posteriors()
            assert np.array_equal(d0, d1) and np.array_equal(l0, ll) and not d0[L:].any()
            bits[table] = d0
        assert np.array_equal(bits["4"], bits[None]) and np.array_equal(bits["2"], bits[None])
        # a bin gets one term per (cell, plane, state) of its row, (I + 1) (nCols + 1) S = 20 at the most, each rounded once to 2^-36
        assert me.fixed_close(bits[None][:L], posts[kind][0][0], (I + 1) * (len(colTok) + 1) * em.nStates)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 10. compactness -----------------------------------------------------------------------------------------------------------------------
def test_compact_lattices_under_a_budget_below_one_rectangle():
    """S = 65, nCols = 4 at I = L = 300 under band(4): a rectangle is 301 x 301 x 2 x 5 x 65 doubles, 471 MB; the compact lattice
    2 S (nCols + 1) sum(inEnd - inStart) doubles, 14 MB.  With the memory budget at a tenth of one rectangle counts() and the row
    posteriors run, chunk by chunk; the likelihood against the yardstick's Forward, the sums by their identities."""
    em, colTok, pairs, env = me.pool_case()
    S, I, w = me.POOL
    dp = PairMergedProfileDP(em, colTok)
    want = np.array([dp.forward(pairs[0][0], pairs[0][1], env=env)[0]])
    rect = 8 * (I + 1) * (I + 1) * 2 * 5 * S
    reads = np.nonzero(em.inTok > 0)[0]
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, [(x, P, env) for x, P in pairs])
    try:
        assert dev.cells() == len(pairs) * 2 * S * 5 * n_cells(env) and 8 * dev.cells() // len(pairs) < rect // 30
        capi.set_memory_budget(rect // 10)
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        ph.note("forward at I = L = 300", fr[:1], want, WORST)
        assert logs_close(fr[:1], want) and np.array_equal(fr, fm) and np.all(fr > -math.inf)
        c, s, ll = dev.counts()
        assert np.array_equal(ll, fm) and abs(c[reads].sum() - len(pairs) * I) <= 1e-6 * len(pairs) * I
        post, pl = dev.merged_row_posteriors()
        assert np.array_equal(pl, fm) and np.abs(post.sum(axis=1) - 1.0).max() <= me.ROW_TOL
        capi.set_memory_budget(8 * dev.cells() // len(pairs) + 8 * dev.cells() // (4 * len(pairs)))      # one pair's two lattices do not fit
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.counts()
    finally:
        capi.set_memory_budget(0)
        dev.close(); dm.close()


# ---- 11. at scale, without the yardstick ---------------------------------------------------------------------------------------------------
def test_identities_at_scale():
    """I = L = 1 500, S = 8, nCols = 4, band(3), four pairs: rolling and materialised to the same bits, the counts call's per-pair
    likelihoods those of the Forward, row sums 1 within 1e-6, the counts of the input-reading edges I per pair within 1e-6 relative."""
    em, colTok, pairs, env = me.scale_case()
    S, I, w, n = me.SCALE
    reads = np.nonzero(em.inTok > 0)[0]
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, [(x, P, env) for x, P in pairs])
    try:
        assert dev.cells() == n * 2 * S * 5 * n_cells(env)
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        assert np.array_equal(fr, fm) and np.all(fr > -math.inf), (fr, fm)
        c, s, ll = dev.counts()
        assert np.array_equal(ll, fm) and abs(s - fm.sum()) <= 1e-9 * abs(fm.sum())
        assert abs(c[reads].sum() - n * I) <= 1e-6 * n * I, c[reads].sum()
        post, pl = dev.merged_row_posteriors()
        assert np.array_equal(pl, fm)
        WORST["row sums at scale"] = float(np.abs(post.sum(axis=1) - 1.0).max())
        assert WORST["row sums at scale"] <= me.ROW_TOL
        v, off, edges, rows = dev.viterbi()
        assert np.array_equal(v, dev.viterbi(paths=False)[0]) and np.all(v <= fm) and np.all(np.diff(off) >= I)
    finally:
        dev.close(); dm.close()


# ---- 12. no input ------------------------------------------------------------------------------------------------------------------------------
def test_no_input_under_its_only_envelope_is_the_one_tape_sweep():
    """I = 0: the only envelope is the column i = 0, and what is left of the pair sweep is the one-tape merged sweep over the
    machine's output-only and silent edges, DeviceProfiles (merged)."""
    em, colTok, pairs = mh.lane_case(4, 13)[0]
    rng = np.random.RandomState(13)
    profiles = [mh.merged_input(rng, em, 4, 0, L, zeros=0.05)[1] for L in (0, 1, 7, 40)]
    dm = capi.DeviceMachine(em)
    dev = me.open_pairs(dm, colTok, [(np.zeros(0, np.int32), P, full(0, len(P))) for P in profiles])
    one = capi.DeviceProfiles(dm, profiles, colTok)
    try:
        got, want = dev.forward(capi.MB_ROLLING), one.forward()
        assert capi.last_kernel_name() != me.ENV_FWD % "sum,rolling"
        ph.note("no input", got, want, WORST)
        assert logs_close(got, want) and np.all(want > -math.inf), (got, want)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), got)
        dp = MergedProfileDP(em, colTok)
        assert logs_close(got, [dp.forward(P)[0] for P in profiles])
    finally:
        dev.close(); one.close(); dm.close()


# ---- 13. errors ------------------------------------------------------------------------------------------------------------------------------
BAD_ENVELOPES = (([0, 0], [4, 4], "Envelope/sequence mismatch"), ([0, 0, 0], [4, 4, 5], "Envelope/sequence mismatch"),
                 ([0, 2, 3], [1, 3, 4], "Envelope is not connected"), ([0, 1, 0], [4, 4, 4], "Envelope is not monotone"))


def test_errors_leave_the_object_usable_and_launch_nothing():
    em, colTok, pairs = mh.lane_case(2, 1)[0]
    x, P = np.ones(3, np.int32), pairs[4][1][:2]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x], [P], colTok)
    plain = capi.DeviceProfilePairs(dm, [x], [np.zeros((2, em.nOutTok + 1))])
    try:
        want = dev.forward(capi.MB_MATERIALISE)
        band = dev.cells()
        for st, en, msg in BAD_ENVELOPES:
            dev.set_merged_envelopes([Envelope.band(3, 2, 1)])
            assert dev.cells() < band
            with pytest.raises(capi.MbError, match=msg):
                dev.set_merged_envelopes([(st, en)])
            assert dev.cells() == band and np.array_equal(dev.forward(capi.MB_MATERIALISE), want)      # (a rejected call leaves no envelopes)
            assert capi.last_kernel_name() == me.FULL_FWD % "sum,mat"
            with pytest.raises(capi.MbError, match=msg):
                capi.profile_pair_fill_merged(dm, capi.MB_FORWARD, x, P, colTok, (st, en))
        with pytest.raises(capi.MbError, match="merged envelopes take merged profiles"):
            plain.set_merged_envelopes([Envelope.band(3, 2, 1)])
        with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
            dev.set_envelopes([Envelope.band(3, 2, 1)])
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), want)
        assert plain.forward(capi.MB_ROLLING)[0] > -math.inf
    finally:
        dev.close(); plain.close(); dm.close()


# ---- 14. the layers above --------------------------------------------------------------------------------------------------------------------
def _layer_case():
    import os
    from machineboss_amd.machine import Machine
    from machineboss_amd.profile import Profile
    here = os.path.dirname(os.path.abspath(__file__))
    machine = Machine.fromFile(os.path.join(here, "golden", "machine", "dnastore4.json"))
    profile = Profile.fromCsv(os.path.join(here, "golden", "csv", "tiny_uc.csv"))
    return machine, machine.getParamDefs(True), profile


LAYER_INPUTS = [["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"], ["1_3"], ["0_3", "2_3", "1_3", "2_3", "0_3"]]


def test_score_merged_pairs_on_the_device():
    from machineboss_amd import boss
    machine, par, profile = _layer_case()
    inputs = LAYER_INPUTS
    kw = dict(params=par, loglike=True, viterbi=True, counts=True, posteriors=True, band=2)
    sd, cd = boss.scoreMergedPairs(machine, inputs, profile, "device", **kw)
    sn, cn = boss.scoreMergedPairs(machine, inputs, profile, "numpy", **kw)
    assert logs_close(sd["loglike"], sn["loglike"]) and logs_close(sd["viterbi"], sn["viterbi"], 1e-12)
    assert sd["loglike"][1] == -math.inf and np.isfinite(sd["loglike"]).sum() >= 3
    for a, b in zip(sd["posteriors"], sn["posteriors"]):
        assert counts_close(a, b), np.abs(a - b).max()
    assert sorted(cd) == sorted(cn)
    for k in cd:
        assert counts_close(np.array([cd[k]]), np.array([cn[k]])), (k, cd[k], cn[k])
    pd, ld = boss.mergedPairPosteriors(machine, inputs, profile, "device", params=par, band=2)
    pn, ln = boss.mergedPairPosteriors(machine, inputs, profile, "numpy", params=par, band=2)
    assert logs_close(ld, ln) and logs_close(ld, sn["loglike"])
    for a, b in zip(pd, pn):
        assert counts_close(a, b), np.abs(a - b).max()


def test_merged_pair_profile_loglike_on_the_device():
    import torch

    import pairmergeposthelpers as mp
    from machineboss_amd.torchprofile import merged_pair_profile_loglike
    em, colTok, triples = me.mixed_case(8)
    keep = [t for t in triples if len(t[1])][:8]
    rowOff = np.concatenate([[0], np.cumsum([len(t[1]) for t in keep])])
    res = {}
    for backend in ("device", "numpy"):
        logP = torch.tensor(np.concatenate([t[1] for t in keep]), dtype=torch.float64, requires_grad=True)
        ll = merged_pair_profile_loglike(em, [t[0] for t in keep], logP, rowOff, colTok, envs=[t[2] for t in keep], backend=backend)
        w = torch.arange(1, len(keep) + 1, dtype=torch.float64)
        torch.where(torch.isfinite(ll), ll, torch.zeros_like(ll)).mul(w).sum().backward()
        res[backend] = (ll.detach().numpy(), logP.grad.numpy())
    assert logs_close(res["device"][0], res["numpy"][0]) and counts_close(res["device"][1], res["numpy"][1])
    assert np.isfinite(res["numpy"][0]).sum() >= 6 and res["numpy"][1].any()
    # the echo transducer: CTC under the full envelope, never above it under a band
    echo = capi.DeviceMachine(mp.echo_machine())
    try:
        for T in mp.CTC_T:
            lp = mp.ctc_frames(T, True)
            loss, grad = mp.ctc_reference(lp)
            I = len(mp.CTC_X)
            t = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
            ll = merged_pair_profile_loglike(echo, [mp.CTC_X], t, [0, T], mp.CTC_COLTOK, envs=[full(I, T)])
            if not math.isfinite(loss):
                assert ll.item() == -math.inf
                continue
            ll.sum().backward()
            assert logs_close([-ll.item()], [loss]), (T, ll.item(), loss)
            # (torch hands back the gradient in the logits behind the log-softmax frames: exp(lp) less the posteriors)
            assert counts_close(t.grad.numpy(), np.exp(lp) - grad), np.abs(t.grad.numpy() - (np.exp(lp) - grad)).max()
            for w in range(0, 4):
                try:
                    env = Envelope.band(I, T, w)
                except Exception:
                    continue
                b = merged_pair_profile_loglike(echo, [mp.CTC_X], torch.tensor(lp), [0, T], mp.CTC_COLTOK, envs=[env]).item()
                assert b <= ll.item() + 1e-9 * max(1.0, abs(ll.item())), (T, w, b, ll.item())
    finally:
        echo.close()
