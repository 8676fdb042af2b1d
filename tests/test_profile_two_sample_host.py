"""Posterior path samples of the two-profile sweeps, without a GPU (docs/profile_tapes.md, "Posterior path samples of pairs of
profiles"): the yardstick profile.TwoProfileDP.samplePaths / pathProbability against an enumeration of every path, the frequencies of
its draws, the rule of its decision counter, and the conditions the GPU module (test_profile_two_sample_gpu.py) relies on for its
inputs -- every uniform clear of every partial sum, live and dead pairs where the cases say so.  The generator's known answers are
test_profile_pair_sample_host.py's: the two-profile sampler draws through the same profile.sample_uniform."""
import ctypes
import math
import os

import numpy as np
import pytest

import twoenvhelpers as eh
import twoprofilehelpers as th
import twosamplehelpers as sh
from machineboss_amd import profile
from machineboss_amd.machine import MachineError
from machineboss_amd.profile import TwoMergedProfileDP, TwoProfileDP
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))


def _close(a, b):
    return (a == b) if (a == -math.inf or b == -math.inf) else abs(a - b) <= sh.LOG_TOL * max(1.0, abs(b))


# ---- 1. the yardstick against every path, one by one --------------------------------------------------------------------------------------
ENUM_BUDGET = 40000


@pytest.mark.parametrize("S", eh.ENUM_STATES)
@pytest.mark.parametrize("levels", (True, False))
def test_path_probabilities_are_the_posterior_of_every_path(S, levels):
    """ENUM_STATES x ENUM_SHAPES of twoenvhelpers, plain and under the envelopes of enum_envelopes: for every path, enumerated one by
    one with its edges and both coordinate arrays, pathProbability is weight - loglike; the probabilities sum to 1; and there are as
    many paths as twoenvhelpers.enumerate_paths counts.  A lattice whose walk takes more than ENUM_BUDGET steps is left out, as in
    test_profile_pair_sample_host.py: the paths of a plain (2, 3) lattice number 10^7, those of (3, 3) 10^10."""
    em = th.pair_machine(S, 30 + S, levels, 2, 3)
    dp = TwoProfileDP(em)
    finite, kinds, worst, most, skipped = 0, set(), 0.0, 0, 0
    for K, L in eh.ENUM_SHAPES:
        A, B = th.two_input(np.random.RandomState(100 * S + 10 * K + L), em, K, L, pInf=0.1)
        for kind, env in [("plain", None)] + eh.enum_envelopes(K, L):
            try:
                paths = sh.enumerate_paths(em, A, B, env, budget=ENUM_BUDGET)
            except sh.TooMany:
                skipped += 1
                continue
            wantLL, _best, count = eh.enumerate_paths(em, A, B, env)
            assert len(paths) == count, (S, levels, K, L, kind)
            ll = dp.forward(A, B, env=env)[0] if env is not None else dp.forward(A, B)[0]
            assert _close(ll, wantLL), (S, levels, K, L, kind, ll, wantLL)
            if not paths:
                assert ll == -math.inf and dp.pathProbability(A, B, [], [], [], env=env) == -math.inf
                continue
            assert len({p[:3] for p in paths}) == len(paths)      # (edges with both coordinates tell the paths apart)
            finite += 1; kinds.add(kind); most = max(most, len(paths))
            total = 0.0
            for edges, rows, ins, weight in paths:
                got = dp.pathProbability(A, B, edges, rows, ins, env=env)
                assert _close(got, weight - ll), (S, levels, K, L, kind, edges, got, weight - ll)
                worst = max(worst, abs(got - (weight - ll)))
                total += math.exp(got)
            assert abs(total - 1.0) <= sh.LOG_TOL, (S, levels, K, L, kind, total)
    assert finite >= 10 and {"plain", "full", "band0", "band1", "stairs"} <= kinds and most >= 100, (finite, kinds, most)
    print("path probabilities against path weights: worst %.3g over %d lattices, up to %d paths, %d lattices past the budget" % (worst, finite, most, skipped))


def test_path_probability_refuses_what_is_no_path():
    em = th.pair_machine(3, 33, True, 2, 3)
    dp = TwoProfileDP(em)
    A, B = th.two_input(np.random.RandomState(322), em, 2, 2, pInf=0.0)
    paths = sh.enumerate_paths(em, A, B)
    edges, rows, ins, _w = max(paths, key=lambda p: len(p[0]))
    assert len(edges) >= 2
    with pytest.raises(MachineError):
        dp.pathProbability(A, B, edges[1:], rows[1:], ins[1:])
    with pytest.raises(MachineError):
        dp.pathProbability(A, B, edges, rows, ins[:-1])
    # a path of the rectangle that leaves band(0)
    outside = [p for p in paths if any(i != r for e, r, i in zip(*p[:3]) if em.inTok[e] and em.outTok[e])]
    assert outside
    with pytest.raises(MachineError):
        dp.pathProbability(A, B, *outside[0][:3], env=Envelope.band(2, 2, 0))


# ---- 2. frequencies -----------------------------------------------------------------------------------------------------------------------
FREQ_SEED = 1


def test_frequencies_of_4096_draws_follow_the_enumerated_posterior():
    """One pair at (2, 2), S = 3 with levels, one symbol on either tape (7 649 paths; with two and three symbols there are 88 098, so
    many of them rare that a few are drawn twice under any seed): the count of every enumerated path lies within
    5 sqrt(n q (1 - q)) + 1 of n q.  The seed is fixed so that this holds; a seed is a property checked here."""
    em = th.pair_machine(3, 103, True, 1, 1)
    dp = TwoProfileDP(em)
    A, B = th.two_input(np.random.RandomState(2203), em, 2, 2, pInf=0.0)
    paths = sh.enumerate_paths(em, A, B)
    assert len(paths) >= 10
    n = 4096
    ll, samples = dp.samplePaths(A, B, n, seed=FREQ_SEED)
    seen = {}
    for edges, rows, ins, logq in samples:
        key = sh.path_key(edges, rows, ins)
        seen[key] = seen.get(key, 0) + 1
    assert set(seen) <= {p[:3] for p in paths}
    for edges, rows, ins, weight in paths:
        q = math.exp(weight - ll)
        got = seen.get((edges, rows, ins), 0)
        assert abs(got - n * q) <= 5.0 * math.sqrt(n * q * (1.0 - q)) + 1.0, (edges, got, n * q)
    assert len(seen) >= 10


# ---- 3. replay, prefixes, dead pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sh.CASES))
def test_logq_of_every_yardstick_sample_is_its_rescored_weight_minus_the_likelihood(name):
    """The edges with both coordinates determine the lattice path -- output blanks happen only in N, directly after an emitting edge
    arrives, input blanks only in Z, directly before an input-reading edge -- so logq = rescore(path) - loglike."""
    _, _, groups = sh.case(name)
    worst, live = 0.0, 0
    for (em, triples), refs in zip(groups, sh.reference(name)):
        for (A, B, _env), (ll, samples) in zip(triples, refs):
            for edges, rows, ins, logq in samples:
                if ll == -math.inf:
                    assert logq == -math.inf and len(edges) == 0
                    continue
                w = th.rescore(em, A, B, edges, rows, ins)
                assert _close(logq, w - ll), (name, logq, w - ll)
                worst = max(worst, abs(logq - (w - ll))); live += 1
    assert live > 0
    print("%s: logq against rescore - loglike, worst %.3g over %d samples" % (name, worst, live))


def test_samples_are_prefixes_and_depend_on_their_own_index():
    em = th.pair_machine(3, 31, True, 2, 3)
    dp = TwoProfileDP(em)
    A, B = th.two_input(np.random.RandomState(32), em, 2, 3, pInf=0.0)

    def same(p, q):
        return all(np.array_equal(u, v) for u, v in zip(p[:3], q[:3])) and p[3] == q[3]
    a = dp.samplePaths(A, B, 3, seed=3, pair=2)[1]
    b = dp.samplePaths(A, B, 9, seed=3, pair=2)[1]
    assert all(same(p, q) for p, q in zip(a, b))
    c = dp.samplePaths(A, B, 9, seed=3, pair=3)[1]
    assert any(not same(p, q) for p, q in zip(b, c))
    for edges, rows, ins, logq in b:
        assert _close(dp.pathProbability(A, B, edges, rows, ins), logq)
    Bd = B.copy(); Bd[1] = -np.inf
    ll, samples = dp.samplePaths(A, Bd, 4)
    assert ll == -math.inf and len(samples) == 4
    assert all(len(e) == 0 and len(r) == 0 and len(i) == 0 and q == -math.inf for e, r, i, q in samples)


# ---- 4. the decision counter ----------------------------------------------------------------------------------------------------------------
def test_a_z_visit_with_one_candidate_still_takes_a_counter_value(monkeypatch):
    """(2, 2) under band(0): the cells are the diagonal, so at Z[2][2] and Z[1][1] the input blank lies outside and "wait" is the only
    candidate.  Every decision -- those included -- takes the next counter value, Z[0][0] takes none, and the path is the one a draw
    with u = sample_uniform(seed, pair, j, t) over the logged candidates of decision t gives."""
    em = th.pair_machine(2, 32, True, 2, 3)
    A, B = th.two_input(np.random.RandomState(232), em, 2, 2, pInf=0.0)
    env = Envelope.band(2, 2, 0)
    assert list(zip(env.inStart, env.inEnd)) == [(0, 1), (1, 2), (2, 3)]
    dp = sh.LoggedTwoProfileDP(em)
    cells = dp.forward(A, B, env=env)[1:]
    asked = []
    real = profile.sample_uniform

    def noted(seed, k, j, t):
        asked.append((seed, k, j, t))
        return real(seed, k, j, t)
    monkeypatch.setattr(profile, "sample_uniform", noted)
    nS, seed, pair = 6, 17, 5
    ll, samples = dp.samplePaths(A, B, nS, seed=seed, pair=pair, env=env)
    assert ll > -math.inf and len(asked) == len(dp.log)
    starts = [k for k, a in enumerate(asked) if a[3] == 0] + [len(asked)]
    assert len(starts) == nS + 1
    lone = 0
    for j, (edges, rows, ins, logq) in enumerate(samples):
        got = []
        for t, at in enumerate(range(starts[j], starts[j + 1])):
            layer, i, r, q, cand = dp.log[at]
            assert not (layer == 2 and i == 0)                       # (Z[0][r] is no decision)
            assert asked[at] == (seed, pair, j, t)                   # every decision the next counter value
            if layer == 2 and len(cand) == 1:
                assert cand[0][0] == "wait" and i > 0
                lone += 1
                assert dp.log[at + 1][:4] == (1, i, r, q) and asked[at + 1] == (seed, pair, j, t + 1)
            u, acc, pick, last = real(seed, pair, j, t), 0.0, None, None
            for c in cand:
                p = math.exp(c[3] - float(cells[layer][i, r, q])) if c[3] > -math.inf else 0.0
                acc += p
                last = c if p > 0.0 else last
                if pick is None and u < acc:
                    pick = c
            pick = pick or last
            if pick[1] >= 0:
                got.append(pick[1])
        assert got[::-1] == [int(e) for e in edges], (j, got, edges)
    assert lone >= 2 * nS


# ---- 5. the inputs of the GPU module --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sh.CASES))
def test_gpu_suite_inputs_are_live(name):
    """For every case the GPU module compares with the yardstick: the least distance of a uniform from a partial sum of its decision,
    over all decisions of all samples, is above 1e-9 -- the device's Forward cells sit within a few 1e-15 relative of the yardstick's
    (docs/profile_tapes.md), so its partial sums differ by about 1e-12 at most, and a margin of 1e-9 leaves three orders of magnitude.
    Every case has a finite pair; the cases that say so have a dead pair (None: the suite's own share, some dead and nine in ten
    live over the basic cases together is test_basic_cases_have_dead_pairs')."""
    n, seed, dead, _ = sh.CASES[name]
    margins = []
    refs = sh.reference(name, margins)
    lls = np.array([ll for group in refs for ll, _ in group])
    assert len(margins) > 0 and min(margins) > sh.MARGIN, (name, min(margins))
    assert (lls > -math.inf).any()
    if dead is not None:
        assert ((lls == -math.inf).any()) == dead, (name, lls)
    for group in refs:
        for ll, samples in group:
            assert len(samples) == n and all((s[3] == -math.inf) == (ll == -math.inf) for s in samples)
    print("%s: %d decisions, least margin %.3g, %d pairs, %d dead" % (name, len(margins), min(margins), len(lls), int((lls == -math.inf).sum())))


def test_basic_cases_have_dead_pairs():
    lls = np.array([ll for name in sh.CASES if name.startswith("basic") for group in sh.reference(name) for ll, _ in group])
    assert (lls == -math.inf).any() and np.mean(lls > -math.inf) >= 0.8, np.mean(lls > -math.inf)


def test_gpu_suite_shapes_are_what_the_cases_need():
    """The seam's dead pairs sit at lanes 63, 64 and 128; the envelope case visits Z cells whose input blank lies outside, with
    decisions behind them, under every kind of envelope; the one-hot pairs have one path each, a K = 0 and an L = 0 pair among them;
    the long case has paths of a few hundred edges; the budget of the chunked call cuts its batch at least three times, and a
    second seed changes it."""
    refs = sh.reference("seam")[0]
    assert len(refs) == th.SEAM_PAIRS and all(refs[k][0] == -math.inf for k in th.SEAM_DEAD)
    logs = []
    sh.reference("envelopes", logs=logs)
    lone = sum(1 for lg in logs for k, (layer, i, r, q, cand) in enumerate(lg) if layer == 2 and len(cand) == 1 and k + 1 < len(lg) and lg[k + 1][0] == 1)
    two = sum(1 for lg in logs for layer, i, r, q, cand in lg if layer == 2 and len(cand) == 2)
    assert lone >= 100 and two >= 100, (lone, two)
    assert {k for ks in sh.env_kinds() for k in ks} == set(eh.ENV_KINDS)
    _, _, groups = sh.case("hot")
    em, triples = groups[0]
    dp = TwoProfileDP(em)
    shapes = [(len(A), len(B)) for A, B, _ in triples]
    assert any(K == 0 and L > 0 for K, L in shapes) and any(L == 0 and K > 0 for K, L in shapes) and (0, 0) in shapes
    for (A, B, _), (ll, samples) in zip(triples, sh.reference("hot")[0]):
        assert len(sh.enumerate_paths(em, A, B)) == 1
        v, edges, rows, ins = dp.viterbi(A, B)
        assert all(np.array_equal(s[0], edges) and np.array_equal(s[1], rows) and np.array_equal(s[2], ins) and abs(s[3]) <= 1e-9 for s in samples)
    lens = [len(s[0]) for s in sh.reference("long")[0][0][1]]
    assert min(lens) >= 200, lens
    _, seed, groups = sh.case("chunks")
    em, triples = groups[0]
    b = sh.sample_call_bytes(em, triples, sh.CHUNK_SAMPLES)
    assert len(th.lattice_chunks(b, int(sh.CHUNK_BUDGET_FACTOR * max(b)))) >= 3
    refs = sh.reference("chunks")[0]
    other = [TwoProfileDP(em).samplePaths(A, B, sh.CHUNK_SAMPLES, seed=sh.SEED_B, pair=k)[1] for k, (A, B, _) in enumerate(triples[:4])]
    assert any(not np.array_equal(a[0], b_[0]) for k in range(4) for a, b_ in zip(refs[k][1], other[k]))


def test_statistics_case_is_met_by_the_yardsticks_own_samples():
    """The bound the GPU test applies to the device's 4 096 samples against the device's counts, applied to the yardstick's samples
    against the yardstick's counts, under the same seed."""
    em, A, B = sh.stat_case()
    dp = TwoProfileDP(em)
    counts, ll = dp.counts(A, B)
    assert ll > -math.inf and int((counts >= 1e-3).sum()) >= 8
    margins = []
    _, samples = dp.samplePaths(A, B, sh.STAT_SAMPLES, seed=sh.STAT_SEED, margins=margins)
    assert min(margins) > sh.MARGIN
    bad = sh.usage_within_bound(sh.usage(em.nTransitions, [s[0] for s in samples]), counts)
    assert not bad, bad


# ---- 6. refusal, the interface ----------------------------------------------------------------------------------------------------------------
def test_merged_two_profile_objects_are_not_sampled():
    em = th.pair_machine(3, 31, True, 2, 3)
    dp = TwoMergedProfileDP(em, [1, 2])
    A = th.soft_profile(np.random.RandomState(1), 2, 2, pInf=0.0)
    B = th.soft_profile(np.random.RandomState(2), 2, 2, pInf=0.0)
    assert dp.forward(A, B)[0] > -math.inf
    with pytest.raises(MachineError, match="sampling takes plain profiles"):
        dp.samplePaths(A, B, 2)
    with pytest.raises(MachineError, match="sampling takes plain profiles"):
        dp.pathProbability(A, B, [], [], [])


def test_the_c_abi_declares_the_entry():
    from machineboss_amd import capi
    text = open(os.path.join(os.path.dirname(HERE), "include", "mbhip.h")).read()
    assert "mb_profile_twos_sample" in capi.EXPORTS and "int mb_profile_twos_sample(" in text
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mb_profile_twos_sample")
    assert hasattr(capi.DeviceProfileTwos, "sample_paths")


def test_sample_two_profiles_numpy_backend():
    """boss.sampleTwoProfiles with the numpy backend: MachinePaths from the start to the end state, logq, likelihoods; a band can
    only lower a likelihood."""
    from machineboss_amd import boss
    em = th.pair_machine(3, 31, True, 2, 3)
    m = th.machine_of(em)
    rng = np.random.RandomState(5)
    ins = [th.profile_of(em.inputTokenizer.tok2sym[1:], th.soft_profile(rng, K, em.nInTok, pInf=0.0)) for K in (2, 3, 0)]
    out = th.profile_of(em.outputTokenizer.tok2sym[1:], th.soft_profile(rng, 3, em.nOutTok, pInf=0.0))
    full = None
    for band in (None, 2):
        paths, logq, ll = boss.sampleTwoProfiles(m, ins, out, 4, seed=9, backend="numpy", band=band)
        assert len(paths) == 3 and all(len(p) == 4 for p in paths) and min(ll) > -math.inf
        assert all(-80.0 < q <= 0.0 for qs in logq for q in qs)
        full = ll if band is None else full
        assert all(a <= b + 1e-12 for a, b in zip(ll, full))
    with pytest.raises(Exception):
        boss.sampleTwoProfiles(m, ins, out, 0, backend="numpy")
