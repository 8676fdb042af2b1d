"""CPU tests of pairs against CTC-merged profiles under an envelope (docs/profile_tapes.md, "Pairs against a merged profile under an
envelope"): the masked restatement profile.PairMergedProfileDP(env=...) against a brute-force sum over paths, its identities, the
conditions the builders of test_profile_pair_merge_env_gpu.py are held to, and the Python layers on the numpy backend."""
import math
import os

import numpy as np
import pytest

import pairenvhelpers as eh
import pairmergeenvhelpers as me
import pairmergehelpers as mh
import pairmergeposthelpers as mp
import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import boss
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the masked restatement against brute force ------------------------------------------------------------------------------------------
class _TooMany(Exception):
    pass


def _brute_forward(dp, x, P, inside, budget=300000):
    """The sum over all paths from N(0, 0, plane 0, state 0) to W(I, L, any plane, S-1) of the UNMASKED recurrence that stay inside
    the envelope, enumerated one by one: a walk over (i, r, plane, state, stage) by the terms of the recurrence, with nothing shared
    between paths -- no exclusion vector, an emitting edge simply may not enter the plane it leaves.  Raises _TooMany past `budget`
    nodes."""
    I, L, S, PL = len(x), len(P), dp.S, dp.PL
    P = [[float(v) for v in row] for row in P]
    cols = [[c for c in range(1, PL) if dp.colTok[c - 1] == o] for o in range(dp.em.nOutTok + 1)]

    def by_source(tab):
        out = [[] for _ in range(S)]
        _, s, d, w, o = tab
        for k in range(len(s)):
            out[int(s[k])].append((int(d[k]), float(w[k]), int(o[k])))
        return out
    ins = [by_source(t) for t in dp.ins]; match = [by_source(t) for t in dp.match]
    emit = by_source((None, dp.eS, dp.eD, dp.eW, dp.eO)); sil = by_source((None, dp.sS, dp.sD, dp.sW, np.zeros(len(dp.sS), np.int64)))
    inside = inside.tolist()
    total = []
    seen = [0]

    def at_n(i, r, p, q, w):
        if not inside[i][r] or w == -math.inf:
            return
        at_w(i, r, p, q, w)                                    # no move
        if r < L:
            at_n(i, r + 1, 0, q, w + P[r][0])                  # the blank reads N, out of any plane
            if p:
                at_n(i, r + 1, p, q, w + P[r][p])              # the repeat reads N, and stays

    def at_w(i, r, p, q, w):
        if not inside[i][r] or w == -math.inf:
            return
        seen[0] += 1
        if seen[0] > budget:
            raise _TooMany()
        if i == I and r == L and q == S - 1:
            total.append(w)
        if i < I:
            for d, ww, _o in ins[x[i]][q]:
                at_w(i + 1, r, p, d, w + ww)
        for d, ww, _o in sil[q]:
            at_w(i, r, p, d, w + ww)
        if r < L:
            if i < I:
                for d, ww, o in match[x[i]][q]:
                    for c in cols[o]:
                        if c != p:
                            at_n(i + 1, r + 1, c, d, (w + ww) + P[r][c])
            for d, ww, o in emit[q]:
                for c in cols[o]:
                    if c != p:
                        at_n(i, r + 1, c, d, (w + ww) + P[r][c])

    at_n(0, 0, 0, 0, 0.0)
    return float(np.logaddexp.reduce(total)) if total else -math.inf


BRUTE_SHAPES = ((2, 2), (3, 3), (4, 3), (5, 4))


BRUTE_COLTOK = ((1,), (2, 1), (1, 1))


@pytest.mark.parametrize("levels", (True, False))
@pytest.mark.parametrize("S", (4, 5))
def test_masked_forward_is_the_sum_over_paths_inside(S, levels):
    """Lattices up to (5, 4), three seeds, every envelope kind, one and two columns (two of them on one token).  An envelope with
    more paths than the enumeration's budget is left out; the narrow ones reach (5, 4).  (One column cannot take two rows in a row,
    so band(0) and the staircase, whose rows are joined by matches alone, are finite with two columns only.)"""
    worst, kinds, largest, finite = 0.0, set(), 0, {}
    for colTok in BRUTE_COLTOK:
        for seed in range(3):
            em = ph.pair_machine(S, 10 * S + seed, levels, 2, 2)
            dp = PairMergedProfileDP(em, colTok)
            for I, L in BRUTE_SHAPES:
                rng = np.random.RandomState(100 * seed + 10 * I + L)
                x, P = mh.merged_input(rng, em, len(colTok), I, L, zeros=0.1)
                for kind, env in eh.envelopes(rng, I, L):
                    if kind == "full" and I + L > 4:
                        continue
                    try:
                        want = _brute_forward(dp, x, P, eh.mask(env, I))
                    except _TooMany:
                        continue
                    got = dp.forward(x, P, env=env)[0]
                    assert logs_close([got], [want]), (S, colTok, levels, seed, I, L, kind, got, want)
                    if want > -math.inf:
                        finite[(seed, I, L)] = finite.get((seed, I, L), 0) + 1
                        kinds.add(kind); largest = max(largest, I + L)
                    worst = max(worst, ph.log_dev([got], [want]))
    assert len(finite) == 3 * len(BRUTE_SHAPES), sorted(finite)          # at least one finite case per seed and shape
    assert kinds == set(eh.ENV_KINDS) and largest == 9, (kinds, largest)
    print("masked merged Forward against the path sum, worst deviation: %.3g over %d finite cases" % (worst, sum(finite.values())))


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope_bit_for_bit():
    for em, colTok, pairs in mh.lane_case(2, 13) + mh.lane_case(4, 2):
        dp = PairMergedProfileDP(em, colTok)
        for x, P in pairs:
            e = eh.full(len(x), len(P))
            for a, b in ((dp.forward(x, P), dp.forward(x, P, env=e)), (dp.forward(x, P, "max"), dp.forward(x, P, "max", env=e)),
                         (dp.backward(x, P), dp.backward(x, P, env=(e.inStart, e.inEnd)))):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert np.array_equal(dp.counts(x, P)[0], dp.counts(x, P, env=e)[0])
            assert np.array_equal(dp.rowPosteriors(x, P)[0], dp.rowPosteriors(x, P, env=e)[0])
            va, vb = dp.viterbi(x, P), dp.viterbi(x, P, env=e)
            assert va[0] == vb[0] and np.array_equal(va[1], vb[1]) and np.array_equal(va[2], vb[2])


def test_no_input_is_the_one_tape_merged_sweep():
    """I = 0: the only envelope is the column i = 0, and the masked pair sweep is MergedProfileDP."""
    em, colTok, _ = mh.lane_case(4, 13)[0]
    rng = np.random.RandomState(13)
    for L in (0, 1, 7):
        P = mh.merged_input(rng, em, 4, 0, L)[1]
        ll, N, W = PairMergedProfileDP(em, colTok).forward(np.zeros(0, np.int32), P, env=eh.full(0, L))
        ref = MergedProfileDP(em, colTok).forward(P)
        assert logs_close([ll], [ref[0]]) and ll > -math.inf
        assert N.shape == (1, L + 1, 5, em.nStates)


def test_restatement_rejects_what_the_device_rejects():
    em = ph.pair_machine(2, 1, False, 1, 1)
    dp = PairMergedProfileDP(em, (1,))
    x, P = np.ones(3, np.int32), np.zeros((2, 2))
    for st, en, msg in (([0, 0], [4, 4], "mismatch"), ([0, 0, 0], [4, 4, 5], "mismatch"), ([0, 2, 3], [1, 3, 4], "not connected"),
                        ([0, 1, 0], [4, 4, 4], "not monotone")):
        for call in (dp.forward, dp.backward, dp.counts, dp.rowPosteriors, dp.viterbi):
            with pytest.raises(MachineError, match=msg):
                call(x, P, env=(st, en))


def test_forward_meets_backward_and_the_sums_hold():
    """Under every envelope kind: one likelihood from both ends, -inf outside in every plane, the counts of the input-reading edges
    sum to I, the emitting counts plus the blank and repeat mass to L, every row of the posteriors to 1."""
    finite = 0
    for nCols, S, levels in ((2, 5, True), (4, 8, False), (3, 8, True)):
        em = ph.pair_machine(S, 30 + S, levels, 2, 3)
        colTok = np.random.RandomState(S).randint(1, 4, nCols)
        dp = PairMergedProfileDP(em, colTok)
        reads, writes = np.nonzero(em.inTok > 0)[0], np.nonzero(em.outTok > 0)[0]
        for I, L in ((3, 3), (9, 4), (4, 9), (12, 12)):
            rng = np.random.RandomState(10 * I + L)
            x, P = mh.merged_input(rng, em, nCols, I, L, zeros=0.05)
            for kind, env in eh.envelopes(rng, I, L):
                ll, N, W = dp.forward(x, P, env=env)
                bl, NB, WB = dp.backward(x, P, env=env)
                assert logs_close([bl], [ll]), (kind, bl, ll)
                out = ~eh.mask(env, I)
                assert all(np.all(A[out] == -math.inf) for A in (N, W, NB, WB))
                blanks = []
                c = dp.counts(x, P, blanks=blanks, env=env)[0]
                post = dp.rowPosteriors(x, P, env=env)[0]
                if ll > -math.inf:
                    finite += 1
                    assert abs(c[reads].sum() - I) <= 1e-9 * max(1, I), (kind, c[reads].sum(), I)
                    assert abs(c[writes].sum() + blanks[0] - L) <= 1e-9 * max(1, L), (kind, c[writes].sum(), blanks[0], L)
                    assert np.abs(post.sum(axis=1) - 1.0).max() <= 1e-9, (kind, post.sum(axis=1))
                else:
                    assert not c.any() and not post.any()
    assert finite >= 30, finite


def test_posteriors_are_the_gradient_of_the_banded_likelihood():
    """A central finite difference of the banded likelihood in every entry of P, at the step and the bound of fd_case."""
    em, colTok, x, P = mp.fd_case()
    dp = PairMergedProfileDP(em, colTok)
    for env in (Envelope.band(3, 3, 1), eh.staircase(3, 3)):
        post, ll = dp.rowPosteriors(x, P, env=env)
        assert ll > -math.inf and ll < dp.forward(x, P)[0]
        for r in range(P.shape[0]):
            for c in range(P.shape[1]):
                hi, lo = P.copy(), P.copy()
                hi[r, c] += mp.FD_H; lo[r, c] -= mp.FD_H
                fd = (dp.forward(x, hi, env=env)[0] - dp.forward(x, lo, env=env)[0]) / (2 * mp.FD_H)
                assert abs(fd - post[r, c]) <= mp.FD_TOL, (r, c, fd, post[r, c])


# ---- the builders of the GPU suite -----------------------------------------------------------------------------------------------------
def _live(lls):
    return float(np.mean(np.asarray(lls) > -math.inf))


def test_cell_cases_are_live_under_every_envelope_kind():
    """Nine in ten likelihoods of every case with two columns or more are finite and every envelope kind is met; with one column a
    band of width 0 on a square admits no path at all (one column cannot take two rows in a row), which is half the case."""
    every = []
    for nCols, S in me.CELL_CASES:
        lls, kinds = [], set()
        for em, colTok, quads in me.cell_case(nCols, S):
            dp = PairMergedProfileDP(em, colTok)
            lls += [dp.forward(x, P, env=env)[0] for x, P, _, env in quads]
            kinds |= {kind for _, _, kind, _ in quads}
        assert kinds == set(eh.ENV_KINDS)
        assert _live(lls) >= (0.9 if nCols > 1 else 0.5), (nCols, S, _live(lls))
        every += lls
    assert _live(every) >= 0.9, _live(every)


def test_ring_bytes_straddle_the_marks():
    S = me.MARK_S
    lo, hi = me.LDS_DEFAULT, me.LDS_MAX
    a, b, c, d = (me.ring_bytes(S, 4, M) for M in me.MARK_ROLLING)
    assert a <= lo < b <= hi and b <= c <= hi < d
    a, b, c, d = (me.ring_bytes(S, 4, M, True) for M in me.MARK_MAT)
    assert a <= lo < b <= hi and b <= c <= hi < d
    dp = PairMergedProfileDP(me.mark_machine(), me.MARK_COLTOK)
    for M in me.MARK_M:
        x, P, env = me.mark_case(M)
        assert eh.diag_max(env) == M and len(x) == len(P) == me.MARK_LEN
    for M in (me.MARK_M[0], me.MARK_M[-1]):
        x, P, env = me.mark_case(M)
        assert dp.forward(x, P, env=env)[0] > -math.inf
    (x0, P0, e0), (x1, P1, e1) = me.mark_extras()
    assert e0 is None and dp.forward(x0, P0)[0] > -math.inf and dp.forward(x1, P1, env=e1)[0] == -math.inf


def test_tie_batch_shows_every_tie_with_a_loser_outside():
    """merged_tie_machine on tie_pairs under band(1): every kind of tie shows at least once, and at least once each a repeat, an
    output-only and an input-only candidate loses because its source cell lies outside the envelope."""
    dp = PairMergedProfileDP(mh.merged_tie_machine(), mh.TIE_COLTOK)
    census = {}
    pairs = me.tie_env_pairs()
    assert len(pairs) >= 10
    for x, P, env in pairs:
        assert dp.viterbi(x, P, census=census, env=env)[0] > -math.inf
    for kind in mh.TIE_KINDS:
        assert census.get(kind, 0) >= 1, (kind, census)
    for kind in ("repeat", "emit", "input"):
        assert census.get(("outside", kind), 0) >= 1, census


@pytest.mark.parametrize("S", me.MIXED_STATES)
def test_mixed_batch_composition_liveness_and_chunks(S):
    em, colTok, triples = me.mixed_case(S)
    dp = PairMergedProfileDP(em, colTok)
    lls = [dp.forward(x, P, **({} if env is None else {"env": env}))[0] for x, P, env in triples]
    assert [k for k, v in enumerate(lls) if v == -math.inf] == list(me.MIXED_DEAD)
    envs = [t[2] for t in triples]
    assert {envs[k] is None for k in me.MIXED_DEAD} == {True, False}
    shapes = {(len(x), len(P)) for x, P, _ in triples}
    assert (0, 0) in shapes and any(i and not l for i, l in shapes) and any(l and not i for i, l in shapes)
    assert 8 <= sum(e is None for e in envs) <= 12 and len(triples) == 20
    for call in ("forward", "viterbi", "counts", "posteriors"):
        budget, chunks, kinds, launches = me.mixed_chunks(call, em, triples)
        assert set(kinds) == me.CHUNK_KINDS, (call, kinds)
        assert budget >= max(me.call_bytes(call, em, 4, triples)) and launches == len(chunks) + sum(len(k) == 2 for k in kinds)


def test_seam_batch_puts_dead_pairs_at_the_block_seams_of_both_launches():
    em, colTok, triples = me.seam_case()
    envs = [t[2] for t in triples]
    assert sum(e is not None for e in envs) == me.SEAM_ENV == 129 and sum(e is None for e in envs) == me.SEAM_PLAIN == 65
    dp = PairMergedProfileDP(em, colTok)
    v = [dp.forward(x, P, "max", **({} if env is None else {"env": env}))[0] for x, P, env in triples]
    slots = eh.slots(envs)
    dead = [k for k, s in enumerate(slots) if s in me.SEAM_DEAD_PLAIN + tuple(me.SEAM_PLAIN + e for e in me.SEAM_DEAD_ENV)]
    assert len(dead) == 5 and all(v[k] == -math.inf for k in dead) and _live(v) >= 0.9
    assert max(len(x) for x, _, _ in triples) <= 3 and max(len(P) for _, P, _ in triples) <= 3
    assert len(me.seam_prefix(triples, 64)) == 128 and len(me.seam_prefix(triples, 65)) == 130


def test_the_other_builders_hold_their_conditions():
    em, colTok, triples = me.big_counts_env_case()
    dp = PairMergedProfileDP(em, colTok)
    lls = [dp.forward(x, P, env=env)[0] for x, P, env in triples]
    assert em.nTransitions > 8192 and lls[-1] == -math.inf and all(v > -math.inf for v in lls[:-1])
    em, colTok, x, P, Pd = me.wrap_case()
    I, L = me.WRAP_SHAPE
    assert (len(x), len(P), em.nStates, len(colTok)) == (I, L, 2, 4) and L > me.WRAP_GROUPS
    dp = PairMergedProfileDP(em, colTok)
    for env in (eh.full(I, L), eh.staircase(I, L)):
        assert dp.forward(x, P, env=env)[0] > -math.inf and dp.forward(x, Pd, env=env)[0] == -math.inf
    S, I, w = me.POOL
    env = me.pool_case()[3]
    assert 30 * 2 * S * 5 * eh.n_cells(env) < (I + 1) * (I + 1) * 2 * 5 * S


# ---- the Python layers on the numpy backend ------------------------------------------------------------------------------------------
CSV = os.path.join(HERE, "golden", "csv", "tiny_uc.csv")
DNASTORE = os.path.join(HERE, "golden", "machine", "dnastore4.json")
SEQS = [["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"], ["1_3"]]


def test_score_merged_pairs_numpy_band():
    """scoreMergedPairs and mergedPairPosteriors(band=) through the numpy backend are the yardstick under Envelope.band of each
    input; an input that cannot be tokenised scores -inf and gets zeros; a band does not raise a likelihood."""
    from machineboss_amd.evalmachine import EvaluatedMachine
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(CSV)
    P, colTok = prof.mergeRows(em)
    dp = PairMergedProfileDP(em, colTok)
    sc, pc = boss.scoreMergedPairs(m, SEQS, prof, backend="numpy", params=par, viterbi=True, counts=True, posteriors=True, band=1)
    posts, lls = boss.mergedPairPosteriors(m, SEQS, prof, backend="numpy", params=par, band=1)
    total = np.zeros(em.nTransitions)
    for k, seq in enumerate(SEQS):
        if k == 1:
            assert sc["loglike"][k] == sc["viterbi"][k] == lls[k] == -math.inf and not sc["posteriors"][k].any() and not posts[k].any()
            continue
        x = em.inputTokenizer.tokenize(seq)
        env = Envelope.band(len(x), len(P), 1)
        assert k != 2 or not env.isFull()
        assert sc["loglike"][k] == lls[k] == dp.forward(x, P, env=env)[0] and sc["viterbi"][k] == dp.forward(x, P, "max", env=env)[0]
        want = dp.rowPosteriors(x, P, env=env)[0]
        assert np.array_equal(sc["posteriors"][k], want) and np.array_equal(posts[k], want)
        total += dp.counts(x, P, env=env)[0]
    assert isinstance(pc, dict) and total.any()
    full = boss.scoreMergedPairs(m, SEQS, prof, backend="numpy", params=par)[0]
    assert "posteriors" not in full and full["viterbi"] is None
    assert all(b <= f + 1e-9 * max(1.0, abs(f)) for b, f in zip(sc["loglike"], full["loglike"]) if f > -math.inf)
    assert full["loglike"] == boss.scoreProfilePairs(m, SEQS, prof, backend="numpy", params=par, merge=True)[0]["loglike"]
    # the pinned refusals stay
    with pytest.raises(MachineError, match="envelopes take plain profiles"):
        boss.scoreProfilePairs(m, SEQS, prof, backend="numpy", params=par, merge=True, band=2)
    with pytest.raises(MachineError, match='backend is "device" or "numpy"'):
        boss.scoreMergedPairs(m, SEQS, prof, backend="cuda", params=par)


def test_merged_pair_profile_loglike_numpy():
    import torch
    from machineboss_amd.torchprofile import merged_pair_profile_loglike, pair_profile_loglike
    em, colTok, x, P = mp.fd_case()
    x1, P1 = mh.merged_input(np.random.RandomState(4), em, 3, 2, 2, zeros=0.0)
    rowOff = np.array([0, 3, 5])
    envs = [Envelope.band(3, 3, 1), None]
    logP = torch.tensor(np.concatenate([P, P1]), dtype=torch.float64, requires_grad=True)
    fn = lambda t: merged_pair_profile_loglike(em, [x, x1], t, rowOff, colTok, envs=envs, backend="numpy")
    ll = fn(logP)
    dp = PairMergedProfileDP(em, colTok)
    assert ll.tolist() == [dp.forward(x, P, env=envs[0])[0], dp.forward(x1, P1)[0]]
    assert torch.autograd.gradcheck(fn, (logP,), eps=1e-6, atol=1e-6, rtol=1e-5)
    plain = merged_pair_profile_loglike(em, [x, x1], logP, rowOff, colTok, backend="numpy")
    assert plain[0] > ll[0] and plain[1] == ll[1]
    assert torch.equal(plain, pair_profile_loglike(em, [x, x1], logP, rowOff, backend="numpy", colTok=colTok))
    with pytest.raises(ValueError, match="envelopes take plain profiles"):
        pair_profile_loglike(em, [x, x1], logP, rowOff, envs=envs, backend="numpy", colTok=colTok)
    with pytest.raises(ValueError, match="one envelope"):
        merged_pair_profile_loglike(em, [x, x1], logP, rowOff, colTok, envs=envs[:1], backend="numpy")
    with pytest.raises(MachineError, match="not monotone"):
        merged_pair_profile_loglike(em, [x], logP[:3], [0, 3], colTok, envs=[([0, 1, 0, 0], [4, 4, 4, 4])], backend="numpy")


def test_the_c_abi_declares_the_new_entries():
    from machineboss_amd import capi
    text = open(os.path.join(os.path.dirname(HERE), "include", "mbhip.h")).read()
    for name in ("mb_profile_pairs_set_envelopes_merged", "mb_profile_pair_fill_merged_env"):
        assert name in capi.EXPORTS and ("int %s(" % name) in text
    assert "merged envelopes take merged profiles" in text
