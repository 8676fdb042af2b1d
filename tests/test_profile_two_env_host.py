"""The two-profile recurrence under an envelope, held without a GPU (docs/profile_tapes.md, "Pairs of profiles under an envelope"):
profile.TwoProfileDP(env=...) is the yardstick of the envelope kernels of mb_profile_two.hip, so it is first held to things it does
not compute -- every path enumerated one by one, the pair sweep under a one-hot input, its own identities (row sums, grouped counts,
central differences), the transposed problem -- then the inputs of test_profile_two_env_gpu.py are held to the conditions that
module names (finite likelihoods, ring sizes, chunk and block counts), and the wrappers to the yardstick."""
import math

import numpy as np
import pytest
import torch

import twoenvhelpers as te
import twoposthelpers as tp
import twoprofilehelpers as th
from pairenvhelpers import full, mask, n_cells, staircase
from twoprofilehelpers import logs_close, pair_machine
from machineboss_amd import boss
from machineboss_amd.machine import MachineError
from machineboss_amd.profile import PairProfileDP, TwoProfileDP
from machineboss_amd.seqpair import Envelope
from machineboss_amd.torchprofile import two_profile_loglike


# ---- 1. every path ----------------------------------------------------------------------------------------------------------------------
def test_forward_is_the_sum_over_the_paths_inside():
    """Forward and the Viterbi score under an envelope against the paths enumerated one by one (input blanks included), at 1e-9.
    Envelopes of more than nine cells are left to the machines without silent levels, and there to ten (band(1) at (3, 3)): with
    levels ten cells have up to 14.5 million paths and the full (3, 3) lattice tens of millions, half a minute and more each.  So the
    full envelope is enumerated up to (2, 2) -- section 2 holds it to env=None bit for bit -- and the bands and the staircase up to
    (3, 3)."""
    n = live = cut = 0
    for key, em, A, B, kind, env in te.enum_cases():
        K, L = len(A), len(B)
        if n_cells(env) > (9 if key[1] else 10):
            continue
        ll, best, count = te.enumerate_paths(em, A, B, env)
        dp = TwoProfileDP(em)
        got, N, W, Z = dp.forward(A, B, env=env)
        assert logs_close([got], [ll], 1e-9), (key, got, ll)
        assert logs_close([dp.forward(A, B, "max", env=env)[0]], [best], 1e-9), key
        out = ~mask(env, K)
        assert np.all(N[out] == -math.inf) and np.all(W[out] == -math.inf) and np.all(Z[out] == -math.inf)
        n += 1; live += count > 0
        cut += count > 0 and kind != "full" and got < dp.forward(A, B)[0] - 1e-9      # the envelope took paths away
    assert n >= 60 and live >= 0.75 * n and cut >= 10, (n, live, cut)


# ---- 2. the full envelope ------------------------------------------------------------------------------------------------------------------
def test_full_envelope_is_no_envelope():
    n = 0
    for key, em, (A, B) in th.host_cases():
        if key[2]:
            continue
        dp = TwoProfileDP(em)
        env = full(len(A), len(B))
        for mode in ("exact", "max"):
            a, b = dp.forward(A, B, mode), dp.forward(A, B, mode, env=env)
            assert a[0] == b[0] or (a[0] != a[0]) == (b[0] != b[0]), key
            assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), key
        a, b = dp.backward(A, B), dp.backward(A, B, env=env)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), key
        ba, bb = [], []
        a, b = dp.counts(A, B, ba), dp.counts(A, B, bb, env=env)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and ba == bb, key
        a, b = dp.rowPosteriors(A, B), dp.rowPosteriors(A, B, env=env)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], key
        a, b = dp.viterbi(A, B), dp.viterbi(A, B, env=(env.inStart, env.inEnd))
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), key
        n += 1
    assert n == 42


def test_rejected_envelopes():
    dp = TwoProfileDP(pair_machine(3, 0, True, 2, 3))
    A, B = th.two_input(np.random.RandomState(0), dp.em, 3, 2, pInf=0.0)
    for st, en, msg in (([0, 0], [4, 4], "Envelope/sequence mismatch"), ([0, 0, 0], [4, 4, 5], "Envelope/sequence mismatch"),
                        ([0, 2, 3], [1, 3, 4], "Envelope is not connected"), ([1, 0, 0], [4, 4, 4], "Envelope is not connected"),
                        ([0, 0, 0], [4, 3, 4], "Envelope is not monotone")):
        for call in (dp.forward, dp.backward, dp.counts, dp.rowPosteriors, dp.viterbi):
            with pytest.raises(MachineError, match=msg):
                call(A, B, env=(st, en))


# ---- 3. a one-hot input is the pair sweep ---------------------------------------------------------------------------------------------------
def test_one_hot_input_reduces_to_the_pair_sweep():
    """With a one-hot A (its blank -inf) the banded likelihood, counts and output-row posteriors are those of PairProfileDP under
    the same envelope on the token string, at 1e-12."""
    n = 0
    for S, levels in ((5, True), (8, False), (3, True)):
        em = pair_machine(S, 3, levels, 2, 3)
        rng = np.random.RandomState(S)
        for K, L in ((3, 3), (4, 6), (6, 4), (5, 5)):
            x = rng.randint(1, 3, size=K)
            B = th.soft_profile(rng, L, 3, pInf=0.05)
            for kind, env in te.envelopes(rng, K, L):
                two, one = TwoProfileDP(em), PairProfileDP(em)
                ll, N, W, Z = two.forward(th.one_hot(x, 2), B, env=env)
                ql, QN, QW = one.forward(x, B, env=env)
                assert logs_close([ll], [ql], 1e-12) and logs_close(N, QN, 1e-12) and logs_close(W, QW, 1e-12) and logs_close(Z, QW, 1e-12)
                c, _ = two.counts(th.one_hot(x, 2), B, env=env)
                qc, _ = one.counts(x, B, env=env)
                assert np.allclose(c, qc, rtol=1e-12, atol=1e-12), (S, K, L, kind)
                pa, pb, _ = two.rowPosteriors(th.one_hot(x, 2), B, env=env)
                qb, _ = one.rowPosteriors(x, B, env=env)
                assert np.allclose(pb, qb, rtol=1e-12, atol=1e-12), (S, K, L, kind)
                if ll > -math.inf:      # every input row was read as its token
                    assert np.allclose(pa[np.arange(K), x], 1.0, rtol=0, atol=1e-9) and np.allclose(pa.sum(), K, rtol=0, atol=1e-9)
                n += ll > -math.inf
    assert n >= 30, n


# ---- 4. identities under bands ----------------------------------------------------------------------------------------------------------------
def test_identities_under_bands():
    """band(0 / 1 / 3) over the seven lattices of the host suite: both posterior tables have row sums 1 (1e-6), their column sums
    are the counts grouped by token, and for K, L <= 3 and |LL| < 100 the central differences of forward() at h = 1e-6 are the
    entries, within 1e-7 (error about h^2 plus 1e-16 / h: 1e-9)."""
    n = fd = 0
    for key, em, (A, B) in th.host_cases():
        S, levels, seed, K, L = key
        if seed:
            continue
        dp = TwoProfileDP(em)
        for w in (0, 1, 3):
            try:
                env = Envelope.band(K, L, w)
            except MachineError:
                continue
            pa, pb, ll = dp.rowPosteriors(A, B, env=env)
            c, cl = dp.counts(A, B, env=env)
            assert ll == cl == dp.forward(A, B, env=env)[0]
            if not ll > -math.inf:
                assert not pa.any() and not pb.any() and not c.any()
                continue
            n += 1
            assert (K == 0 or np.abs(pa.sum(axis=1) - 1.0).max() <= 1e-6) and (L == 0 or np.abs(pb.sum(axis=1) - 1.0).max() <= 1e-6), (key, w)
            ga, gb = tp.grouped(em, c)
            assert np.allclose(pa[:, 1:].sum(axis=0), ga, rtol=1e-9, atol=1e-12) and np.allclose(pb[:, 1:].sum(axis=0), gb, rtol=1e-9, atol=1e-12), (key, w)
            assert not pa[A == -math.inf].any() and not pb[B == -math.inf].any()
            if K <= 3 and L <= 3 and abs(ll) < 100:
                h = 1e-6
                for t, (T, post) in enumerate(((A, pa), (B, pb))):
                    for idx in np.ndindex(*T.shape):
                        if T[idx] == -math.inf:
                            continue
                        up, dn = T.copy(), T.copy()
                        up[idx] += h; dn[idx] -= h
                        d = (dp.forward(*((up, B) if t == 0 else (A, up)), env=env)[0] - dp.forward(*((dn, B) if t == 0 else (A, dn)), env=env)[0]) / (2 * h)
                        assert abs(d - post[idx]) <= 1e-7, (key, w, t, idx, d, post[idx])
                        fd += 1
    assert n >= 60 and fd >= 300, (n, fd)


# ---- 5. transposition ------------------------------------------------------------------------------------------------------------------------
def test_transposition_under_an_envelope():
    """The transposed envelope -- the columns of the envelope are its rows seen from the other tape, which is the colStart / colEnd
    construction of mb_profile_twos_set_envelopes -- has the same cells, and the likelihood of (M, A, B, env) is that of
    (transpose M, B, A, env transposed) WHERE THE ENVELOPE TREATS THE TWO CORNERS OF A DIAGONAL STEP ALIKE.  The two blanks are not
    treated alike: a path that takes the blank of A[i] and the blank (or an output-only edge) of B[r] goes through (i, r + 1),
    because the output blank fires on arrival and the input blank after the commit, and its image in the transposed problem goes
    through (i + 1, r).  Over the rectangle both corners exist and the sums agree (test_profile_two_host.py::test_transposition);
    an envelope that holds (i, r) and (i + 1, r + 1) but only one of the corners keeps one of the two paths.  So the identity is
    asserted for the corner-symmetric envelopes, and the others are seen to differ."""
    def symmetric(env, K):
        m = mask(env, K)
        return all(m[i + 1, r] == m[i, r + 1] for i in range(m.shape[0] - 1) for r in range(m.shape[1] - 1) if m[i, r] and m[i + 1, r + 1])
    n = differ = 0
    for key, em, (A, B) in th.host_cases():
        S, levels, seed, K, L = key
        if seed > 1 or (K, L) == (0, 0):
            continue
        rng = np.random.RandomState(n)
        A, B = th.two_input(rng, em, K, L, pInf=0.0)
        for kind, env in te.envelopes(rng, K, L) + [("band2", te.band_or_full(K, L, 2))]:
            t = te.transposed_env(env, K)
            assert t.connected() and t.monotone() and n_cells(t) == n_cells(env) and np.array_equal(mask(t, L), mask(env, K).T)
            back = te.transposed_env(t, L)
            assert back.inStart == env.inStart and back.inEnd == env.inEnd
            a, b = TwoProfileDP(em).forward(A, B, env=env)[0], TwoProfileDP(th.transposed(em)).forward(B, A, env=t)[0]
            if symmetric(env, K):
                assert logs_close([a], [b]), (key, kind, a, b)
                n += a > -math.inf
            else:
                differ += not logs_close([a], [b])
    assert n >= 100 and differ >= 10, (n, differ)


# ---- 6. the inputs of the GPU module -------------------------------------------------------------------------------------------------------------
def test_gpu_suite_inputs_are_live():
    """At least three in four of all likelihoods test_profile_two_env_gpu.py compares are finite, and at least half under every
    kind of envelope; the rings, chunks and blocks it names are what the host's rules give."""
    lls, byKind = [], {}
    dps = {}
    for name, cases in te.builders().items():
        for em, A, B, env in cases:
            ll = dps.setdefault(id(em), TwoProfileDP(em)).forward(A, B, env=env)[0]
            lls.append(ll > -math.inf)
    for S in te.CELL_STATES:
        for em, A, B, kind, env in te.cell_case(S):
            byKind.setdefault(kind, []).append(dps.setdefault(id(em), TwoProfileDP(em)).forward(A, B, env=env)[0] > -math.inf)
    assert np.mean(lls) >= 0.75, np.mean(lls)
    assert set(byKind) == set(te.ENV_KINDS) and all(np.mean(v) >= 0.5 for v in byKind.values()), {k: np.mean(v) for k, v in byKind.items()}
    # the ring marks
    Ms = [te.diag_max(te.mark_case(M)[2]) for M in te.MARK_M]
    assert tuple(Ms) == te.MARK_M and [te.ring_bytes(te.MARK_S, M) for M in Ms] == [63360, 66240, 161280, 164160]
    assert 63360 <= 65536 < 66240 and 161280 <= te.LDS_MAX < 164160
    em = te.mark_machine()
    extras = te.mark_extras()
    dp = TwoProfileDP(em)
    assert [dp.forward(A, B, env=env)[0] > -math.inf for A, B, env in extras] == [True, True, False] and extras[1][0].shape[0] == 0
    # i mod M with K far past M
    for K, L, w in te.SLOPE_CASES:
        M = te.diag_max(te.slope_case(K, L, w)[2])
        assert max(K, L) >= 8 * M and te.ring_bytes(8, M) <= 65536, (K, L, M)
    # scratch rings
    S, n, K, w = te.PACK
    assert te.diag_max(te.pack_case()[2]) == 9 and te.ring_bytes(S, 9) == 194400 > te.LDS_MAX and n == 24
    # counts past the LDS table
    em, triples = te.big_counts_env_case()
    assert em.nTransitions > 8192 and TwoProfileDP(em).forward(*triples[-1][:2], env=triples[-1][2])[0] == -math.inf
    # the column staircase: runs of many, two and one cell
    em, A, B, env = te.post_stairs_case()
    cols = mask(env, len(A)).sum(axis=1)
    assert cols[0] >= 8 and 2 in cols and (cols[4:] == 1).all() and TwoProfileDP(em).forward(A, B, env=env)[0] > -math.inf
    # more than 1 024 line blocks on either axis under a table of 4
    for K, L in te.LONG_SHAPES:
        em, triples = te.long_case(K, L)
        axis = 1 if K > L else 0
        assert te.env_rowpost_blocks(2, triples[0][2], K, axis, 2, 3, 4) == te.LONG > tp.ROWPOST_GROUPS_MAX
        lls = [TwoProfileDP(em).forward(A, B, env=env)[0] > -math.inf for A, B, env in triples]
        assert lls == [True, False]
    # chunks: the budget is below one rectangle and holds one pair's two compact lattices, not two pairs'
    S, K, w, n = te.CHUNK
    em, pairs, env = te.chunk_case()
    one = 2 * te.lattice_bytes(S, env)
    assert te.chunk_budget() < 8 * 3 * S * (K + 1) ** 2 and one <= te.chunk_budget() < 2 * one
    assert len(th.lattice_chunks([one] * n, te.chunk_budget())) == 3
    # ties
    census = {}
    em = th.tie_machine()
    for A, B, env in te.tie_env_pairs():
        v, e, r, i = TwoProfileDP(em).viterbi(A, B, census, env=env)
        assert v > -math.inf and th.rescore(em, A, B, e, r, i) == v
        assert all(env.inStart[rr] <= ii < env.inEnd[rr] for rr, ii in zip(r, i))
    assert len(te.tie_env_pairs()) >= 8
    for first, second in th.TIE_KINDS:
        assert any(first in k and second in k and k.index(first) < k.index(second) for k in census), (first, second, census)


# ---- 7. the wrappers ---------------------------------------------------------------------------------------------------------------------------
def test_torch_gradcheck_under_a_band():
    em = pair_machine(5, 1, True, 2, 3)
    rng = np.random.RandomState(7)
    shapes = ((3, 3), (2, 4))
    pairs = [th.two_input(rng, em, K, L, pInf=0.0) for K, L in shapes]
    envs = [Envelope.band(K, L, 1) for K, L in shapes]
    inOff, rowOff = np.cumsum([0] + [K for K, _ in shapes]), np.cumsum([0] + [L for _, L in shapes])
    logA = torch.tensor(np.concatenate([A for A, _ in pairs]), dtype=torch.float64, requires_grad=True)
    logB = torch.tensor(np.concatenate([B for _, B in pairs]), dtype=torch.float64, requires_grad=True)
    ll = two_profile_loglike(em, logA, inOff, logB, rowOff, envs=envs, backend="numpy")
    want = [TwoProfileDP(em).forward(A, B, env=e)[0] for (A, B), e in zip(pairs, envs)]
    assert np.array_equal(ll.detach().numpy(), want) and ll[0] < TwoProfileDP(em).forward(*pairs[0])[0]
    assert torch.autograd.gradcheck(lambda a, b: two_profile_loglike(em, a, inOff, b, rowOff, envs=envs, backend="numpy"), (logA, logB),
                                    eps=1e-6, atol=1e-6, rtol=1e-5)
    with pytest.raises(ValueError, match="one envelope"):
        two_profile_loglike(em, logA, inOff, logB, rowOff, envs=envs[:1], backend="numpy")


def test_score_two_profiles_band_numpy():
    em = pair_machine(5, 2, True, 2, 3)
    rng = np.random.RandomState(2)
    pairs = [th.two_input(rng, em, K, 5, pInf=0.0) for K in (4, 6)]
    B = pairs[0][1]
    m = th.machine_of(em)
    pb = th.profile_of(em.outputTokenizer.tok2sym[1:], B)
    pas = [th.profile_of(em.inputTokenizer.tok2sym[1:], A) for A, _ in pairs]
    sc, pc = boss.scoreTwoProfiles(m, pas, pb, backend="numpy", viterbi=True, posteriors=True, band=1)
    ev = boss.EvaluatedMachine.fromMachine(m, None)
    dp = TwoProfileDP(ev)
    Bl = pb.logRows(ev)
    for k, p in enumerate(pas):
        Al = p.logRowsIn(ev)
        env = Envelope.band(len(Al), len(Bl), 1)
        assert sc["loglike"][k] == dp.forward(Al, Bl, env=env)[0] < dp.forward(Al, Bl)[0]
        assert sc["viterbi"][k] == dp.forward(Al, Bl, "max", env=env)[0]
        wa, wb, _ = dp.rowPosteriors(Al, Bl, env=env)
        assert np.array_equal(sc["posteriors"][k][0], wa) and np.array_equal(sc["posteriors"][k][1], wb)
    plain, _ = boss.scoreTwoProfiles(m, pas, pb, backend="numpy")
    assert plain["loglike"] == [dp.forward(p.logRowsIn(ev), Bl)[0] for p in pas]
    long = th.profile_of(em.inputTokenizer.tok2sym[1:], th.soft_profile(rng, 12, 2, pInf=0.0))
    with pytest.raises(MachineError, match="Envelope is not connected"):
        boss.scoreTwoProfiles(m, [long], pb, backend="numpy", band=0)
