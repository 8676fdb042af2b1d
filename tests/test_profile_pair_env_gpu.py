"""GPU tests of the two-tape profile sweeps under an envelope (mb_profile_pair.hip, EnvGeom; docs/profile_tapes.md, "Pairs under an
envelope").  The reference is profile.PairProfileDP(env=...) and the bounds are those of pairprofilehelpers: log values 1e-9 relative
to max(1, |value|) with -inf exact; counts >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x count; Viterbi scores and cells
at 1e-12; paths and rows equal.  test_profile_pair_env_host.py holds the same builders to their liveness conditions on the CPU."""
import math
import os

import numpy as np
import pytest

import pairenvhelpers as eh
import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import boss, capi
from machineboss_amd.machine import Machine
from machineboss_amd.profile import PairProfileDP, Profile
from machineboss_amd.seqpair import Envelope

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    print("worst deviations under envelopes:", eh.WORST)


def _pairs(dm, triples, env=True):
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    if env:
        dev.set_envelopes([t[2] for t in triples])
    return dev


# ---- 1. every cell ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", eh.CELL_STATES)
def test_every_cell_under_every_envelope(S):
    """Forward, Viterbi and Backward lattices of profile_pair_fill(..., env) against the masked restatement, with silent levels and
    without, at seven shapes under the full envelope, two bands, a path envelope and a staircase; cells outside are -inf in both
    layers; and the batch calls (likelihoods both ways, paths, counts) on the same pairs in one launch."""
    case = eh.cell_case(S)
    live = []
    for em in dict.fromkeys(id(c[0]) for c in case):
        sub = [c for c in case if id(c[0]) == em]
        eh.check_env_batch(sub[0][0], [(x, P, env) for _, x, P, _, env in sub], fill=True, live=live)
    assert np.mean(live) >= 0.9


# ---- 2. the full envelope is no envelope ------------------------------------------------------------------------------------------------
def test_full_envelope_has_the_bits_of_no_envelope():
    em, pairs = ph.ragged_case()
    dm = capi.DeviceMachine(em)
    plain = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    enved = _pairs(dm, [(x, P, eh.full(len(x), len(P))) for x, P in pairs])
    try:
        assert enved.cells() == plain.cells() == sum(2 * em.nStates * (len(x) + 1) * (len(P) + 1) for x, P in pairs)
        for flags in (capi.MB_ROLLING, capi.MB_MATERIALISE):
            a, b = plain.forward(flags), enved.forward(flags)
            assert np.array_equal(a, b), (flags, a, b)
        assert capi.last_kernel_name().startswith("k_profile_pair_env_fwd")
        assert np.array_equal(plain.viterbi(paths=False)[0], enved.viterbi(paths=False)[0])
        for a, b in zip(plain.viterbi(), enved.viterbi()):
            assert np.array_equal(a, b)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            (ca, sa, la), (cb, sb, lb) = plain.counts(), enved.counts()
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        assert np.array_equal(ca, cb) and sa == sb and np.array_equal(la, lb) and ca.any()
        enved.set_envelopes(None)
        assert np.array_equal(plain.forward(), enved.forward()) and capi.last_kernel_name().startswith("k_profile_pair_fwd")
        for x, P in pairs[3:6]:
            for mode in (capi.MB_FORWARD, capi.MB_VITERBI, capi.MB_BACKWARD):
                want = capi.profile_pair_fill(dm, mode, x, P)
                assert np.array_equal(want, capi.profile_pair_fill(dm, mode, x, P, eh.full(len(x), len(P))))
                got = np.empty_like(want)
                xs = np.ascontiguousarray(x, np.int32); Pc = np.ascontiguousarray(P, np.float64)
                rc = capi.load().mb_profile_pair_fill_env(dm.h, mode, capi._p(xs, capi.C.c_int32), len(xs), capi._p(Pc, capi.C.c_double), len(Pc),
                                                          None, None, capi._p(got, capi.C.c_double))
                assert rc == 0 and np.array_equal(want, got)
    finally:
        plain.close(); enved.close(); dm.close()


# ---- 3. the ring marks ----------------------------------------------------------------------------------------------------------------------
_MARK = {}


def _mark_ref(key, x, P, env):
    if key not in _MARK:      # computed once, shared, never changed
        dp = PairProfileDP(eh.mark_machine())
        _MARK[key] = (dp.forward(x, P, env=env)[0], dp.forward(x, P, "max", env=env)[0])
    return _MARK[key]


def _ring_bytes(S, M):
    return 48 * M * S


@pytest.mark.parametrize("M", eh.MARK_M)
def test_ring_marks_alone(M):
    """S = 40, I = L = 120 under a band with at most M cells on a diagonal: a ring of 48 M S bytes, 65 280 (the last below the
    64 KiB from which the kernel must be told), 67 200, 163 200 (the last in LDS) and 165 120 (global scratch).  Rolling Forward has
    the bits of materialised Forward; both and the Viterbi score against the restatement."""
    x, P, env = eh.mark_case(M)
    assert eh.diag_max(env) == M
    assert (_ring_bytes(eh.MARK_S, M) <= 64 * 1024) == (M == 34) and (_ring_bytes(eh.MARK_S, M) <= 160 * 1024) == (M != 86)
    want, wv = _mark_ref(M, x, P, env)
    assert want > -math.inf
    dm = capi.DeviceMachine(eh.mark_machine())
    dev = _pairs(dm, [(x, P, env)])
    try:
        got = dev.forward(capi.MB_ROLLING)
        ph.note("forward", got, [want], eh.WORST)
        assert capi.last_kernel_name() == "k_profile_pair_env_fwd<sum,rolling>" and capi.last_launch_count() == 1
        mat = dev.forward(capi.MB_MATERIALISE)
        assert logs_close(got, [want]) and np.array_equal(got, mat), (got, mat, want)
        assert logs_close(dev.viterbi(paths=False)[0], [wv], 1e-12)
        assert dev.cells() == 2 * eh.MARK_S * eh.n_cells(env)
    finally:
        dev.close(); dm.close()


def test_ring_marks_in_one_ragged_launch():
    """The four beside a pair without an envelope and a dead pair: LDS rings below and above 64 KiB, a scratch ring, the full
    sweep's kernel in a launch of its own.  Same bits as each alone, and rolling = materialised."""
    triples = [eh.mark_case(M) for M in eh.MARK_M]
    plain, dead = eh.mark_extras()
    refs = [_mark_ref(M, *t) for M, t in zip(eh.MARK_M, triples)]
    dp = PairProfileDP(eh.mark_machine())
    refs += [(dp.forward(*plain[:2])[0], dp.forward(plain[0], plain[1], "max")[0]), (-math.inf, -math.inf)]
    assert dp.forward(dead[0], dead[1], env=dead[2])[0] == -math.inf
    batch = triples[:2] + [plain] + triples[2:] + [dead]
    want = np.array([refs[k][0] for k in (0, 1, 4, 2, 3, 5)]); wv = np.array([refs[k][1] for k in (0, 1, 4, 2, 3, 5)])
    dm = capi.DeviceMachine(eh.mark_machine())
    dev = _pairs(dm, batch)
    try:
        got = dev.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 2
        ph.note("forward", got, want, eh.WORST)
        assert logs_close(got, want), (got, want)
        assert np.array_equal(got, dev.forward(capi.MB_MATERIALISE))
        v = dev.viterbi(paths=False)[0]
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, t in enumerate(batch):
            one = _pairs(dm, [t], env=t[2] is not None)
            try:
                assert one.forward(capi.MB_ROLLING)[0] == got[k] and one.viterbi(paths=False)[0][0] == v[k], k
            finally:
                one.close()
    finally:
        dev.close(); dm.close()


# ---- 4. i mod M -----------------------------------------------------------------------------------------------------------------------------
def test_cells_found_by_i_mod_m_on_slopes_and_areas():
    """(I, L, w) = (200, 40, 6): i advances five positions per row; (40, 200, 2): none on most rows; and the path-area envelope of a
    random alignment, whose diagonals change length as they go.  Everything the batch computes, against the restatement."""
    triples = [eh.slope_case(*c) for c in eh.SLOPE_CASES] + [eh.area_case()]
    for (x, P, env), c in zip(triples, eh.SLOPE_CASES):
        assert eh.diag_max(env) < min(c[0], c[1]) + 1
    live = []
    eh.check_env_batch(eh.slope_machine(), triples, live=live)
    assert all(live)


# ---- 5. many workgroups sharing the scratch buffer -----------------------------------------------------------------------------------------
def test_many_scratch_rings_under_envelopes():
    """Twenty-four pairs at S = 300, I = L = 60 under band(w = 20): rings of 302 400 bytes, all in the scratch buffer, three
    workgroups to a die.  Every pair alone returns the bits it had in the batch."""
    em, pairs, env = eh.pack_case()
    assert _ring_bytes(em.nStates, eh.diag_max(env)) > 160 * 1024
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, [(x, P, env) for x, P in pairs])
    try:
        f, v = dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]
        assert capi.last_launch_count() == 1 and np.mean(f > -math.inf) >= 0.9
        assert np.array_equal(f, dev.forward(capi.MB_MATERIALISE))
        for k, (x, P) in enumerate(pairs):
            one = _pairs(dm, [(x, P, env)])
            try:
                assert one.forward(capi.MB_ROLLING)[0] == f[k] and one.viterbi(paths=False)[0][0] == v[k], k
            finally:
                one.close()
    finally:
        dev.close(); dm.close()


# ---- 6. the compact pool --------------------------------------------------------------------------------------------------------------------
def test_compact_pool_under_a_budget_below_the_rectangle():
    """S = 65, I = L = 300 under band(w = 4): about 2 700 cells of 90 601.  The budget holds the compact lattices (two per pair for
    the counts) and not one rectangle; then a budget of one pair at a time: the chunked calls give the unchunked bits."""
    em, pairs, env = eh.pool_case()
    S, I, _ = eh.POOL
    compact, rect = 16 * S * eh.n_cells(env), 16 * S * (I + 1) * (I + 1)
    dp = PairProfileDP(em)
    refs = [eh.env_reference(dp, x, P, env, cells=False) for x, P in pairs]
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, [(x, P, env) for x, P in pairs])
    try:
        assert dev.cells() == len(pairs) * 2 * S * eh.n_cells(env)
        budget = 8 * len(pairs) * compact
        assert budget < rect
        capi.set_option("MB_DETERMINISTIC", "1")
        capi.set_memory_budget(budget)
        try:
            c, s, ll = dev.counts()
            assert capi.last_launch_count() == 1
            v, off, edges, rows = dev.viterbi()
            capi.set_memory_budget(3 * compact)
            c2, s2, ll2 = dev.counts()
            assert capi.last_launch_count() == len(pairs)
            v2, off2, edges2, rows2 = dev.viterbi()
        finally:
            capi.set_memory_budget(0)
            capi.set_option("MB_DETERMINISTIC", None)
        want = np.array([r["ll"] for r in refs]); wc = np.sum([r["counts"] for r in refs], axis=0)
        assert np.all(want > -math.inf)
        ph.note("forward", ll, want, eh.WORST); ph.note_counts(c, wc, eh.WORST)
        assert logs_close(ll, want) and counts_close(c, wc)
        assert logs_close(v, [r["v"] for r in refs], 1e-12)
        for k, r in enumerate(refs):
            assert np.array_equal(edges[off[k]:off[k + 1]], r["path"][0]) and np.array_equal(rows[off[k]:off[k + 1]], r["path"][1]), k
        assert np.array_equal(c, c2) and np.array_equal(ll, ll2) and np.array_equal(v, v2)
        assert np.array_equal(off, off2) and np.array_equal(edges, edges2) and np.array_equal(rows, rows2)
        capi.set_memory_budget(compact // 2)
        try:
            with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
                dev.forward(capi.MB_MATERIALISE)
        finally:
            capi.set_memory_budget(0)
    finally:
        dev.close(); dm.close()


# ---- 7. counts ------------------------------------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table_under_a_band():
    """11 204 transitions (global atomics) under band(w = 2), a dead pair among them: against the restatement, and in fixed point the
    same bits from call to call."""
    em, triples = eh.big_counts_env_case()
    assert em.nTransitions > 8192
    dp = PairProfileDP(em)
    refs = [dp.counts(x, P, env=env) for x, P, env in triples]
    wc = np.sum([r[0] for r in refs], axis=0); want = np.array([r[1] for r in refs])
    assert np.sum(want > -math.inf) == len(triples) - 1
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, triples)
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_pair_env_counts"
        ph.note_counts(c, wc, eh.WORST)
        assert counts_close(c, wc) and logs_close(ll, want)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            d0, d1 = dev.counts()[0], dev.counts()[0]
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        assert np.array_equal(d0, d1)
        big = wc >= 1e-3      # the fixed point's quantum, 2^-36 per term, on top of the floating-point bound
        terms = sum(eh.n_cells(env) for _, _, env in triples)      # a transition gets at most one term per cell, each rounded once
        assert np.all(np.abs(d0[big] - wc[big]) <= ph.COUNT_REL * wc[big] + terms * 2.0 ** -36)
    finally:
        dev.close(); dm.close()


# ---- 8. ties ----------------------------------------------------------------------------------------------------------------------------------
def test_ties_under_a_band_follow_candidate_order():
    em = ph.tie_machine()
    triples = eh.tie_env_pairs()
    dp = PairProfileDP(em)
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, triples)
    try:
        v, off, edges, rows = dev.viterbi()
        for k, (x, P, env) in enumerate(triples):
            wv, we, wr = dp.viterbi(x, P, env=env)
            assert v[k] == wv and np.array_equal(edges[off[k]:off[k + 1]], we) and np.array_equal(rows[off[k]:off[k + 1]], wr), k
    finally:
        dev.close(); dm.close()


# ---- 9. against the token sweeps under the same envelope ---------------------------------------------------------------------------------
def test_onehot_profile_is_the_token_pair_under_the_same_envelope():
    """A one-hot profile with a -inf blank is a token string: the banded Forward likelihood of (x, P) is DeviceBatch.forward of (x, y)
    under the same envelope through mb_batch_set_envelopes -- no numpy between the two.  The token side runs its generic family
    (set_kernel(1)), whose sums are the exact fp64 log-sum-exp of the pair sweeps; the default families add the correction term of
    the log-sum-exp in fp32 (mb_device_math.h) and sit 1.2e-7 away on this pair, as test_profile_gpu.py notes for the one-tape case."""
    em, x, y, P, env = eh.onehot_case()
    capi.set_kernel(1)
    try:
        dm = capi.DeviceMachine(em)
        tok = capi.DeviceBatch.from_pairs(dm, [(x, y)])
        try:
            tok.set_envelopes([(env.inStart, env.inEnd)])
            want = tok.forward()[0]
        finally:
            tok.close(); dm.close()
    finally:
        capi.set_kernel(0)
    dm = capi.DeviceMachine(em)
    dev = _pairs(dm, [(x, P, env)])
    try:
        got = dev.forward(capi.MB_ROLLING)[0]
        ph.note("token cross-check", [got], [want], eh.WORST)
        assert want > -math.inf and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
        assert dev.forward(capi.MB_MATERIALISE)[0] == got
    finally:
        dev.close(); dm.close()


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------------------
def test_rejected_envelopes_launch_nothing_and_leave_the_pairs_usable():
    em = ph.pair_machine(8, 5, True, 2, 3)
    x, P = ph.pair_input(np.random.RandomState(5), em, 3, 2)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x, x], [P, P])
    merged = capi.DeviceProfilePairs(dm, [x], [np.zeros((2, 3))], colTok=[1, 2])
    try:
        base = dev.forward()
        ok = ([0, 0, 0], [4, 4, 4])
        for env, msg in ((([0, 0], [4, 4]), "Envelope/sequence mismatch"), (([0, 0, 0], [4, 4, 5]), "Envelope/sequence mismatch"),
                         (([-1, 0, 0], [4, 4, 4]), "Envelope/sequence mismatch"), (([0, 2, 3], [1, 3, 4]), "Envelope is not connected"),
                         (([1, 1, 1], [4, 4, 4]), "Envelope is not connected"), (([0, 0, 0], [4, 4, 3]), "Envelope is not connected"),
                         (([0, 1, 0], [4, 4, 4]), "Envelope is not monotone"), (([0, 0, 0], [4, 3, 4]), "Envelope is not monotone")):
            launches = capi.last_launch_count()
            with pytest.raises(capi.MbError, match=msg):
                dev.set_envelopes([ok, env])
            assert capi.last_launch_count() == launches      # (the count of the call before: set_envelopes launches nothing itself)
            assert np.array_equal(dev.forward(), base) and capi.last_launch_count() == 1
            with pytest.raises(capi.MbError, match=msg):
                capi.profile_pair_fill(dm, capi.MB_FORWARD, x, P, env)
            # a fill call starts its count at 0 (a row count rejected in Python never gets that far)
            assert capi.last_launch_count() == (1 if len(env[0]) != len(P) + 1 else 0)
        with pytest.raises(capi.MbError, match="envelopes take plain profiles"):
            merged.set_envelopes([ok])
        merged.forward()
        dev.set_envelopes([None, ([0, 0, 1], [2, 3, 4])])
        got = dev.forward()
        assert got[0] == base[0] and got[1] < base[1]
    finally:
        dev.close(); merged.close(); dm.close()


# ---- 11. the command line's function ------------------------------------------------------------------------------------------------------
def test_score_profile_pairs_band_device_against_numpy():
    m = Machine.fromFile(os.path.join(HERE, "golden", "machine", "dnastore4.json"))
    par = m.getParamDefs(True)
    prof = Profile.fromCsv(os.path.join(HERE, "golden", "csv", "tiny_uc.csv"))
    seqs = [[], ["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"]]
    kw = dict(params=par, loglike=True, viterbi=True, counts=True, band=3)
    (sd, cd), (sn, cn) = boss.scoreProfilePairs(m, seqs, prof, backend="device", **kw), boss.scoreProfilePairs(m, seqs, prof, backend="numpy", **kw)
    assert logs_close(sd["loglike"], sn["loglike"]) and logs_close(sd["viterbi"], sn["viterbi"], 1e-12)
    keys = sorted(cn)
    assert sorted(cd) == keys and counts_close(np.array([cd[k] for k in keys]), np.array([cn[k] for k in keys]))
