"""The merged two-profile recurrence under an envelope, held without a GPU (docs/profile_tapes.md, "Pairs of profiles against a
merged profile under an envelope"): profile.TwoMergedProfileDP(env=...) is the yardstick of the envelope kernels of
mb_profile_two_merge.hip, so it is first held to things it does not compute -- every path enumerated one by one, the sibling
families it reduces to, its own identities (Forward meets Backward, the conservation of rows, row sums, central differences) -- then
the inputs of test_profile_two_merge_env_gpu.py are held to the conditions that module assumes (finite likelihoods, ring bytes,
tie kinds, chunk counts), and the wrappers to the yardstick.

Bounds: enumerations 1e-9; reductions 1e-12; row sums 1e-6; central differences at h = 1e-6 within 1e-7 (truncation about h^2,
rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100)."""
import math
import os

import numpy as np
import pytest

import twomergeenvhelpers as tv
import twomergehelpers as tm
import twomergeposthelpers as tq
import twoprofilehelpers as th
from pairenvhelpers import diag_max, envelopes, full, mask, n_cells, staircase
from twoprofilehelpers import logs_close, pair_machine
from machineboss_amd import boss
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile, TwoMergedProfileDP, TwoProfileDP
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(HERE, "golden", "csv", "tiny_uc.csv")
DNASTORE = os.path.join(HERE, "golden", "machine", "dnastore4.json")


def _same(a, b):
    return a == b or (a != a and b != b)


# ---- 1. every path ----------------------------------------------------------------------------------------------------------------------
def test_forward_is_the_sum_over_the_paths_inside():
    """Forward and the Viterbi score under an envelope against the paths enumerated one by one over (i, r, plane, state, stage), at
    1e-9, and every plane of every layer of a cell outside exactly -inf.  The cap (twomergeenvhelpers.ENUM_CAP) leaves out the
    envelopes of more than nine cells on the machines with silent levels and of more than ten on those without: the full envelope
    past (2, 2) (section 2 holds it to env=None bit for bit), band(1) at (3, 2) and (3, 3) with levels and at (3, 3) beyond ten
    cells.  At least half the enumerated cases under each envelope kind have a finite likelihood."""
    n, live, tot, cut = 0, {}, {}, 0
    for key, em, colTok, A, B, kind, env in tv.enum_cases():
        if n_cells(env) > tv.ENUM_CAP[key[1]]:
            continue
        ll, best, count = tv.enumerate_paths(em, colTok, A, B, env)
        dp = TwoMergedProfileDP(em, colTok)
        got, N, W, Z = dp.forward(A, B, env=env)
        assert logs_close([got], [ll], 1e-9), (key, got, ll)
        assert logs_close([dp.forward(A, B, "max", env=env)[0]], [best], 1e-9), key
        out = ~mask(env, len(A))
        assert np.all(N[out] == -math.inf) and np.all(W[out] == -math.inf) and np.all(Z[out] == -math.inf)
        n += 1
        tot[kind] = tot.get(kind, 0) + 1
        live[kind] = live.get(kind, 0) + (count > 0)
        cut += count > 0 and kind != "full" and got < dp.forward(A, B)[0] - 1e-9      # the envelope took paths away
    assert n >= 150 and cut >= 20, (n, cut)
    assert set(tot) == {"full", "band0", "band1", "stairs"} and all(2 * live[k] >= tot[k] for k in tot), (live, tot)


# ---- 2. the full envelope ------------------------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope_bit_for_bit():
    n = 0
    for key, em, colTok, A, B in tm.host_cases():
        if key[2] or key[3] != "plain":
            continue
        dp = TwoMergedProfileDP(em, colTok)
        env = full(len(A), len(B))
        for mode in ("exact", "max"):
            a, b = dp._sweep(A, B, mode), dp._sweep(A, B, mode, env)
            assert _same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), key
        a, b = dp.backward(A, B), dp.backward(A, B, env=env)
        assert _same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), key
        ba, bb = [], []
        a, b = dp.counts(A, B, ba), dp.counts(A, B, bb, env=env)
        assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and ba == bb, key
        ra, rb = [], []
        a, b = dp.mergedRowPosteriors(A, B, ra), dp.mergedRowPosteriors(A, B, rb, env=(env.inStart, env.inEnd))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same(a[2], b[2]) and np.array_equal(ra[0], rb[0]), key
        ca, cb = {}, {}
        a, b = dp.viterbi(A, B, ca), dp.viterbi(A, B, cb, env=env)
        assert _same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and ca == cb, key
        n += 1
    assert n == 84


def test_restatement_rejects_what_the_device_rejects():
    dp = TwoMergedProfileDP(pair_machine(3, 0, True, 2, 3), (1, 2))
    A, B = tm.merged_input(np.random.RandomState(0), dp.em, 2, 3, 2, pInf=0.0)
    for st, en, msg in (([0, 0], [4, 4], "Envelope/sequence mismatch"), ([0, 0, 0], [4, 4, 5], "Envelope/sequence mismatch"),
                        ([0, 2, 3], [1, 3, 4], "Envelope is not connected"), ([1, 0, 0], [4, 4, 4], "Envelope is not connected"),
                        ([0, 0, 0], [4, 3, 4], "Envelope is not monotone")):
        for call in (dp.forward, dp.backward, dp.counts, dp.mergedRowPosteriors, dp.viterbi):
            with pytest.raises(MachineError, match=msg):
                call(A, B, env=(st, en))
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        dp.rowPosteriors(A, B, env=full(3, 2))


# ---- 3. the sibling families ----------------------------------------------------------------------------------------------------------------
def test_reductions_to_the_sibling_families():
    """K = 0 (one envelope only: the one row of cells) is MergedProfileDP; a one-hot A (its blank -inf) is
    PairMergedProfileDP(env=...) on its tokens at 1e-12 in likelihood, layers, counts and output-row posteriors; one column per token
    with every B row one-hot on a run-free, blank-free string is TwoProfileDP(env=...) on that string's plain rows."""
    n = 0
    for S, levels in ((5, True), (8, False), (3, True)):
        em = pair_machine(S, 3, levels, 2, 3)
        rng = np.random.RandomState(S)
        colTok = (3, 1, 3, 2)
        two, pair = TwoMergedProfileDP(em, colTok), PairMergedProfileDP(em, colTok)
        B = tm.merged_rows(rng, 4, 4, zeros=0.1)
        ll, N, W, Z = two.forward(np.zeros((0, 3)), B, env=full(0, 4))
        pl, PN, PW = MergedProfileDP(em, colTok).forward(B)
        assert logs_close([ll], [pl], 1e-12) and logs_close(N[0], PN, 1e-12) and logs_close(W[0], PW, 1e-12) and logs_close(Z[0], PW, 1e-12)
        for K, L in ((3, 3), (4, 6), (6, 4), (5, 5)):
            x = rng.randint(1, 3, size=K)
            B = tm.merged_rows(rng, 4, L, zeros=0.05)
            hot = th.one_hot(x, 2)
            for kind, env in envelopes(rng, K, L):
                ll, N, W, Z = two.forward(hot, B, env=env)
                ql, QN, QW = pair.forward(x, B, env=env)
                assert logs_close([ll], [ql], 1e-12) and logs_close(N, QN, 1e-12) and logs_close(W, QW, 1e-12) and logs_close(Z, QW, 1e-12)
                assert logs_close([two.forward(hot, B, "max", env=env)[0]], [pair.forward(x, B, "max", env=env)[0]], 1e-12)
                c, _ = two.counts(hot, B, env=env)
                qc, _ = pair.counts(x, B, env=env)
                assert np.allclose(c, qc, rtol=1e-12, atol=1e-12), (S, K, L, kind)
                pa, pb, _ = two.mergedRowPosteriors(hot, B, env=env)
                qb, _ = pair.rowPosteriors(x, B, env=env)
                assert np.allclose(pb, qb, rtol=1e-12, atol=1e-12), (S, K, L, kind)
                if ll > -math.inf:      # every input row was read as its token
                    assert np.allclose(pa[np.arange(K), x], 1.0, rtol=0, atol=1e-9) and np.allclose(pa.sum(), K, rtol=0, atol=1e-9)
                n += ll > -math.inf
        y = np.array([1, 3, 1, 2, 3])
        hotB = th.one_hot(y, 3)
        A = th.soft_profile(rng, 4, 2, 0.1)
        one, plain = TwoMergedProfileDP(em, (1, 2, 3)), TwoProfileDP(em)
        for kind, env in envelopes(rng, 4, 5):
            tl, tvit = plain.forward(A, hotB, env=env)[0], plain.forward(A, hotB, "max", env=env)[0]
            assert logs_close([one.forward(A, hotB, env=env)[0]], [tl]) and logs_close([one.forward(A, hotB, "max", env=env)[0]], [tvit], 1e-12)
            assert th.counts_close(one.counts(A, hotB, env=env)[0], plain.counts(A, hotB, env=env)[0])
    assert n >= 30, n


# ---- 4. conservation ------------------------------------------------------------------------------------------------------------------------
def test_forward_meets_backward_and_the_rows_are_conserved():
    """Under every envelope kind: the Backward's likelihood is the Forward's; emitting counts + output-blank mass + repeat mass = L;
    input-reading counts + input-blank mass = K; the rows of both posterior tables sum to 1 within 1e-6; postB less its repeats,
    grouped by token, and postA by column are the counts grouped by token; a dead pair has zeros."""
    seen, finite = set(), 0
    for key, em, colTok, A, B in tm.host_cases():
        S, levels, seed, variant, nCols, K, L = key
        if seed or variant != "plain":
            continue
        dp = TwoMergedProfileDP(em, colTok)
        for kind, env in envelopes(np.random.RandomState(10 * K + L), K, L):
            ll = dp.forward(A, B, env=env)[0]
            assert logs_close([dp.backward(A, B, env=env)[0]], [ll]), (key, kind)
            blanks, reps = [], []
            c, cl = dp.counts(A, B, blanks, env=env)
            pa, pb, pl = dp.mergedRowPosteriors(A, B, reps, env=env)
            assert _same(cl, ll) and _same(pl, ll)
            if not ll > -math.inf:
                assert not c.any() and not pa.any() and not pb.any()
                continue
            seen.add(kind); finite += 1
            outBlank, repeat, inBlank = blanks[0]
            assert abs(c[em.outTok > 0].sum() + outBlank + repeat - L) <= 1e-9 * max(1, L), (key, kind)
            assert abs(c[em.inTok > 0].sum() + inBlank - K) <= 1e-9 * max(1, K), (key, kind)
            assert (K == 0 or np.abs(pa.sum(axis=1) - 1.0).max() <= 1e-6) and (L == 0 or np.abs(pb.sum(axis=1) - 1.0).max() <= 1e-6), (key, kind)
            ga, gb = tq.grouped(em, colTok, c)
            assert th.counts_close(pa[:, 1:].sum(axis=0), ga), (key, kind)
            assert th.counts_close(tq.by_token(em, colTok, (pb - reps[0])[:, 1:].sum(axis=0)), gb), (key, kind)
            assert abs(pb[:, 0].sum() - outBlank) <= 1e-9 * max(1, L) and abs(reps[0].sum() - repeat) <= 1e-9 * max(1, L)
            assert abs(pa[:, 0].sum() - inBlank) <= 1e-9 * max(1, K)
    assert seen == set(tv.ENV_KINDS) and finite >= 150, (seen, finite)


# ---- 5. gradients ---------------------------------------------------------------------------------------------------------------------------
def test_posteriors_are_the_gradient_of_the_banded_likelihood():
    """Central differences of the banded likelihood in every entry of A and of B at h = 1e-6 are the entries of
    mergedRowPosteriors(env=...), within 1e-7, at (3, 3) under band(1) and the staircase and at (2, 3) under band(1)."""
    em, colTok, A, B = tq.fd_case()
    dp = TwoMergedProfileDP(em, colTok)
    n = 0
    for A_, B_, env in ((A, B, Envelope.band(3, 3, 1)), (A, B, staircase(3, 3)), (A[:2], B, Envelope.band(2, 3, 1))):
        pa, pb, ll = dp.mergedRowPosteriors(A_, B_, env=env)
        assert ll > -math.inf and ll < dp.forward(A_, B_)[0] and abs(ll) < 100
        for t, (T, post) in enumerate(((A_, pa), (B_, pb))):
            for r in range(T.shape[0]):
                for c in range(T.shape[1]):
                    hi, lo = T.copy(), T.copy()
                    hi[r, c] += tq.FD_H; lo[r, c] -= tq.FD_H
                    args = ((hi, B_), (lo, B_)) if t == 0 else ((A_, hi), (A_, lo))
                    fd = (dp.forward(*args[0], env=env)[0] - dp.forward(*args[1], env=env)[0]) / (2 * tq.FD_H)
                    assert abs(fd - post[r, c]) <= tq.FD_TOL, (t, r, c, fd, post[r, c])
                    n += 1
    assert n >= 60


def test_torch_gradcheck_under_a_band():
    import torch
    from machineboss_amd.torchprofile import merged_two_profile_loglike
    em, colTok, A, B = tq.fd_case()
    A1, B1 = tm.merged_input(np.random.RandomState(4), em, 3, 2, 2, pInf=0.0)
    inOff, rowOff = np.array([0, 3, 5]), np.array([0, 3, 5])
    envs = [Envelope.band(3, 3, 1), None]
    logA = torch.tensor(np.concatenate([A, A1]), dtype=torch.float64, requires_grad=True)
    logB = torch.tensor(np.concatenate([B, B1]), dtype=torch.float64, requires_grad=True)
    fn = lambda a, b: merged_two_profile_loglike(em, a, inOff, b, rowOff, colTok, envs=envs, backend="numpy")
    ll = fn(logA, logB)
    dp = TwoMergedProfileDP(em, colTok)
    assert ll.tolist() == [dp.forward(A, B, env=envs[0])[0], dp.forward(A1, B1)[0]]
    assert torch.autograd.gradcheck(fn, (logA, logB), eps=1e-6, atol=1e-6, rtol=1e-5)
    plain = merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, backend="numpy")
    assert plain[0] > ll[0] and plain[1] == ll[1]
    assert torch.equal(plain, merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, None, "numpy"))      # (envs sits before backend)
    with pytest.raises(ValueError, match="one envelope"):
        merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, envs=envs[:1], backend="numpy")
    with pytest.raises(MachineError, match="not monotone"):
        merged_two_profile_loglike(em, logA[:3], [0, 3], logB[:3], [0, 3], colTok, envs=[([0, 1, 0, 0], [4, 4, 4, 4])], backend="numpy")


# ---- 6. the Python layers on the numpy backend ------------------------------------------------------------------------------------------
def _dnastore_inputs(tmp_path):
    from machineboss_amd.evalmachine import EvaluatedMachine
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    return m, par, em, Profile.fromCsv(str(a)), Profile.fromCsv(CSV)


def test_score_merged_twos_numpy_band(tmp_path):
    """scoreMergedTwos and mergedTwoPosteriors(band=) through the numpy backend are the yardstick called directly under
    Envelope.band of each pair; a band does not raise a likelihood; the pinned refusals are still raised."""
    m, par, em, pa, pb = _dnastore_inputs(tmp_path)
    short = Profile(pa.header, pa.row[:1])
    B, colTok = pb.mergeRows(em)
    dp = TwoMergedProfileDP(em, colTok)
    sc, pc = boss.scoreMergedTwos(m, [pa, short], pb, backend="numpy", params=par, viterbi=True, counts=True, posteriors=True, band=1)
    posts, lls = boss.mergedTwoPosteriors(m, [pa, short], pb, backend="numpy", params=par, band=1)
    narrowed = 0
    for k, p in enumerate((pa, short)):
        A = p.logRowsIn(em)
        env = Envelope.band(len(A), len(B), 1)
        narrowed += not env.isFull()
        assert sc["loglike"][k] == lls[k] == dp.forward(A, B, env=env)[0] and sc["viterbi"][k] == dp.forward(A, B, "max", env=env)[0]
        wa, wb, _ = dp.mergedRowPosteriors(A, B, env=env)
        for got in (sc["posteriors"][k], posts[k]):
            assert np.array_equal(got[0], wa) and np.array_equal(got[1], wb)
    assert narrowed >= 1 and sc["loglike"][0] > -math.inf and pc == {}      # (dnastore4 has no parameters)
    whole = boss.scoreMergedTwos(m, [pa, short], pb, backend="numpy", params=par)[0]
    assert "posteriors" not in whole and whole["viterbi"] is None
    assert all(b <= f + 1e-9 * max(1.0, abs(f)) for b, f in zip(sc["loglike"], whole["loglike"]) if f > -math.inf)
    assert whole["loglike"] == boss.scoreTwoProfiles(m, [pa, short], pb, backend="numpy", params=par, merge=True)[0]["loglike"]
    assert boss.mergedTwoPosteriors(m, [pa], pb, backend="numpy", params=par)[1] == [whole["loglike"][0]]
    with pytest.raises(MachineError, match="envelopes take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par, merge=True, band=2)
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par, merge=True, posteriors=True)
    with pytest.raises(MachineError, match='backend is "device" or "numpy"'):
        boss.scoreMergedTwos(m, [pa], pb, backend="cuda", params=par)


def test_the_c_abi_declares_the_new_entries():
    from machineboss_amd import capi
    text = open(os.path.join(os.path.dirname(HERE), "include", "mbhip.h")).read()
    for name in ("mb_profile_twos_set_envelopes_merged", "mb_profile_two_fill_merged_env"):
        assert name in capi.EXPORTS and ("int %s(" % name) in text


# ---- 7. the builders of the GPU suite -----------------------------------------------------------------------------------------------------
def _live(lls):
    return float(np.mean(np.asarray(lls) > -math.inf))


def test_gpu_inputs_are_live():
    """Every condition test_profile_two_merge_env_gpu.py assumes of its inputs, on the yardstick alone."""
    # the lane cases: three in four of all likelihoods finite, half under every envelope kind, every kind met by every case
    by_kind, every = {}, []
    for nCols, S in tv.LANE_CASES:
        kinds = set()
        for em, colTok, quads in tv.lane_case(nCols, S):
            assert len(colTok) == nCols and em.nStates == S
            dp = TwoMergedProfileDP(em, colTok)
            for A, B, kind, env in quads:
                ll = dp.forward(A, B, env=env)[0]
                by_kind.setdefault(kind, []).append(ll); every.append(ll); kinds.add(kind)
            assert {(len(A), len(B)) for A, B, _, _ in quads} == set(tv.LANE_SHAPES)
        assert kinds == set(tv.ENV_KINDS)
    assert _live(every) >= 0.75 and all(_live(v) >= 0.5 for v in by_kind.values()), (_live(every), {k: _live(v) for k, v in by_kind.items()})
    # the ring marks: bytes either side of 64 KiB and of 160 KiB, M as named, every pair finite
    S, lo, hi = tv.MARK_S, tv.LDS_DEFAULT, tv.LDS_MAX
    assert (lo, hi) == (65536, 163840) and tv.ring_bytes(S, 4, 1) == 44160 and tv.ring_bytes(S, 4, 1, True) == 15360
    a, b, c, d = (tv.ring_bytes(S, 4, M) for M in tv.MARK_ROLLING)
    assert a <= lo < b <= hi and b <= c <= hi < d
    a, b, c, d = (tv.ring_bytes(S, 4, M, True) for M in tv.MARK_MAT)
    assert a <= lo < b <= hi and b <= c <= hi < d
    assert set(tv.MARK_M) == set(tv.MARK_ROLLING) | set(tv.MARK_MAT)
    dp = TwoMergedProfileDP(tv.mark_machine(), tv.MARK_COLTOK)
    for M in tv.MARK_M:
        A, B, env = tv.mark_case(M)
        assert diag_max(env) == M and len(A) == len(B) == tv.MARK_LEN
        assert dp.forward(A, B, env=env)[0] > -math.inf and dp.forward(A, B, "max", env=env)[0] > -math.inf
    (A0, B0, e0), (Az, Bz, ez), (A1, B1, e1) = tv.mark_extras()
    assert e0 is None and ez is None and len(Az) == len(Bz) == 0
    assert dp.forward(A0, B0)[0] > -math.inf and dp.forward(Az, Bz)[0] > -math.inf and dp.forward(A1, B1, env=e1)[0] == -math.inf
    # scratch rings: at least eighteen pairs whose rolling ring is past 160 KiB, a None beside an envelope
    em, triples = tv.packed_case()
    big = [tv.ring_bytes(em.nStates, 2, min(len(A), len(B)) + 1) > hi for A, B, _ in triples]
    assert len(triples) == 24 and sum(big) == 18 and {t[2] is None for t in triples} == {True, False}
    # the ragged batch: (0, 0), an empty tape of either kind, a dead pair
    em, colTok, pairs = tv.ragged_case()
    dp = TwoMergedProfileDP(em, colTok)
    lls = [dp.forward(A, B)[0] for A, B in pairs]
    shapes = {(len(A), len(B)) for A, B in pairs}
    assert (0, 0) in shapes and (0, 5) in shapes and (5, 0) in shapes and lls[-1] == -math.inf and all(v > -math.inf for v in lls[:-1])
    # counts past the LDS table
    em, colTok, triples = tv.big_counts_env_case()
    dp = TwoMergedProfileDP(em, colTok)
    lls = [dp.forward(A, B, env=env)[0] for A, B, env in triples]
    assert em.nTransitions == 11204 and lls[-1] == -math.inf and all(v > -math.inf for v in lls[:-1])
    assert any(not env.isFull() for _, _, env in triples)
    # the axis-1 traversal: columns of many, two and one cell; the long shapes past 1 024 lines
    em, colTok, A, B, env = tv.post_stairs_case()
    runs = mask(env, len(A)).sum(axis=1)
    assert runs[0] >= 10 and 2 in runs and 1 in runs and TwoMergedProfileDP(em, colTok).forward(A, B, env=env)[0] > -math.inf
    for K, L in tv.LONG_SHAPES:
        em, colTok, triples = tv.long_case(K, L)
        dp = TwoMergedProfileDP(em, colTok)
        assert em.nStates == 2 and max(K, L) > 1024 and not triples[0][2].isFull()
        assert dp.forward(*triples[0][:2], env=triples[0][2])[0] > -math.inf and dp.forward(*triples[1][:2], env=triples[1][2])[0] == -math.inf
    # chunking: one pair's two compact lattices fit the budget, a second pair's do not, and one lattice alone exceeds a tenth of it
    budget = tv.chunk_budget()
    for call in ("counts", "posteriors"):
        assert tv.chunk_pair_bytes(call) <= budget < 2 * tv.chunk_pair_bytes(call)
    assert tv.chunk_pair_bytes("forward") > budget // 10
    # ties under band(1): every tie kind, and a loser outside of each of the four kinds
    dp = TwoMergedProfileDP(tm.tie_machine(), tm.TIE_COLTOK)
    census = {}
    pairs = tv.tie_env_pairs()
    assert len(pairs) >= 10
    for A, B, env in pairs:
        assert dp.viterbi(A, B, census, env=env)[0] > -math.inf
    for kinds in tm.TIE_KINDS:
        first, second = kinds[0], kinds[-1]
        assert any(first in k and second in k for k in census if k[0] != "outside"), (kinds, census)
    for kind in tv.TIE_OUTSIDE:
        assert census.get(("outside", kind), 0) >= 1, census
    # the traceback's blocks
    em, triples = tv.seam_case()
    dp = TwoMergedProfileDP(em, tv.SEAM_COLTOK)
    v = [dp.forward(A, B, "max", env=env)[0] for A, B, env in triples]
    assert len(triples) == 129 and all(v[k] == -math.inf for k in tv.SEAM_DEAD) and _live(v) >= 0.75
    # the reductions
    em, colTok, x, A, B, env = tv.onehot_case()
    assert TwoMergedProfileDP(em, colTok).forward(A, B, env=env)[0] > -math.inf and not env.isFull()
