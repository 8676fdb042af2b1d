"""Posterior path samples of the pair profile sweeps, without a GPU (docs/profile_tapes.md, "Posterior path samples"): the generator's
known answers, the yardstick profile.PairProfileDP.samplePaths against an enumeration of every path, the frequencies of its draws,
and the conditions the GPU module (test_profile_pair_sample_gpu.py) relies on for its inputs -- every uniform clear of every partial
sum, the share of live pairs, the statistics bound met by the yardstick's own samples."""
import ctypes
import math
import os

import numpy as np
import pytest

import pairenvhelpers as eh
import pairprofilehelpers as ph
import pairsamplehelpers as sh
from machineboss_amd.profile import PairProfileDP, philox4x32, sample_uniform
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. the generator -------------------------------------------------------------------------------------------------------------------
PHILOX_VECTORS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,want", PHILOX_VECTORS)
def test_philox_known_answers(counter, key, want):
    assert tuple(philox4x32(counter, key)) == want


def test_sample_uniform_is_a_53_bit_fraction_of_the_first_two_words():
    for seed, k, j, t in ((0, 0, 0, 0), (1, 2, 3, 4), (2 ** 64 - 1, 2 ** 40 + 5, 129, 700), (0x9e3779b97f4a7c15, 7, 0, 1)):
        u = sample_uniform(seed, k, j, t)
        assert 0.0 <= u < 1.0 and (u * 2.0 ** 53) == int(u * 2.0 ** 53)
        x0, x1, _, _ = philox4x32((t, j, k & 0xffffffff, k >> 32), (seed & 0xffffffff, seed >> 32))
        assert u == ((x0 >> 5) * 67108864 + (x1 >> 6)) / 9007199254740992.0
    us = [sample_uniform(5, 0, j, t) for j in range(40) for t in range(40)]
    assert len(set(us)) == len(us) and 0.4 < np.mean(us) < 0.6
    assert sample_uniform(5, 1, 0, 0) != sample_uniform(5, 0, 1, 0) != sample_uniform(5, 0, 0, 1)


# ---- 2. the yardstick against every path, one by one --------------------------------------------------------------------------------------
def _enum_envelopes(I, L):
    out = [("plain", None), ("stairs", eh.staircase(I, L))]
    try:
        out.append(("band1", Envelope.band(I, L, 1)))
    except Exception:
        pass
    return out


@pytest.mark.parametrize("S,levels", [(2, True), (2, False), (3, True), (5, True), (5, False)])
def test_choice_probabilities_multiply_to_the_posterior_of_every_path(S, levels):
    """Lattices up to (3, 3), S up to 5, plain, under band(1) and under a staircase: for every path, enumerated one by one, the
    product of the probabilities of its choices is exp(weight - loglike), the weight summed from the path's own edges, profile
    entries and blanks; and the products of all paths sum to 1."""
    finite, kinds, worst, most = 0, set(), 0.0, 0
    for seed in range(2):
        em = ph.pair_machine(S, 10 * S + seed, levels, 2, 2)
        dp = PairProfileDP(em)
        for I, L in ((0, 0), (0, 2), (2, 0), (1, 1), (2, 2), (3, 2), (3, 3)):
            x, P = ph.pair_input(np.random.RandomState(100 * seed + 10 * I + L), em, I, L, pZero=0.3)
            for kind, env in _enum_envelopes(I, L):
                try:
                    ll, paths = sh.enumerate_paths(dp, x, P, env, budget=30000)
                except sh.TooMany:
                    continue
                if not ll > -math.inf:
                    assert not paths
                    continue
                finite += 1; kinds.add(kind); most = max(most, len(paths))
                total = 0.0
                for (edges, rows), (prob, weight) in paths.items():
                    want = math.exp(weight - ll)
                    assert abs(prob - want) <= 1e-9 * max(1.0, abs(want)), (S, levels, I, L, kind, prob, want)
                    worst = max(worst, abs(prob - want))
                    total += prob
                assert abs(total - 1.0) <= 1e-9, (S, levels, I, L, kind, total)
    assert finite >= 12 and kinds == {"plain", "band1", "stairs"} and most >= 100, (finite, kinds, most)
    print("choice products against path weights: worst %.3g over %d lattices, up to %d paths" % (worst, finite, most))


def test_logq_of_a_sample_is_its_path_weight_minus_the_likelihood():
    """samplePaths' own logq, its paths replayed through dp.edgesToPath, and the enumeration agree."""
    em = ph.pair_machine(3, 31, True, 2, 2)
    dp = PairProfileDP(em)
    m = sh.machine_of(em)
    x, P = ph.pair_input(np.random.RandomState(32), em, 2, 2, pZero=0.3)
    for env in (None, Envelope.band(2, 2, 1)):
        ll, paths = sh.enumerate_paths(dp, x, P, env)
        got, samples = dp.samplePaths(x, P, 50, seed=3, pair=2, env=env)
        assert got == ll and ll > -math.inf
        for edges, rows, logq in samples:
            prob, weight = paths[(tuple(int(e) for e in edges), tuple(int(r) for r in rows))]
            assert abs(logq - math.log(prob)) <= 1e-9 * max(1.0, abs(logq))
            w = sh.replay(em, m, x, P, edges, rows)
            assert abs(w - weight) <= 1e-12 * max(1.0, abs(w)) and abs(logq - (w - ll)) <= 1e-9 * max(1.0, abs(logq))
    # samples are prefixes of longer calls and depend on their own (seed, pair, j) alone
    a = dp.samplePaths(x, P, 3, seed=3, pair=2)[1]
    b = dp.samplePaths(x, P, 9, seed=3, pair=2)[1]
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2] for p, q in zip(a, b))
    c = dp.samplePaths(x, P, 9, seed=3, pair=3)[1]
    assert any(not np.array_equal(p[0], q[0]) for p, q in zip(b, c))


def test_a_dead_pair_gives_empty_paths():
    em = ph.pair_machine(3, 31, True, 2, 2)
    x, P = ph.pair_input(np.random.RandomState(32), em, 2, 3)
    P = P.copy(); P[1] = -np.inf
    ll, samples = PairProfileDP(em).samplePaths(x, P, 4)
    assert ll == -math.inf and len(samples) == 4
    assert all(len(e) == 0 and len(r) == 0 and q == -math.inf for e, r, q in samples)


# ---- 3. frequencies -----------------------------------------------------------------------------------------------------------------------
FREQ_SEED = 2          # (seed 1 draws one path of posterior 6e-6 twice: the next seed)


def test_frequencies_of_4096_draws_follow_the_enumerated_posterior():
    """One pair at (2, 2), S = 3 with levels: the count of every distinct path lies within 5 sqrt(n q (1 - q)) + 1 of n q.  The seed
    is fixed so that this holds; a seed is a property checked here."""
    em = ph.pair_machine(3, 103, True, 2, 3)
    dp = PairProfileDP(em)
    x, P = ph.pair_input(np.random.RandomState(2203), em, 2, 2)
    ll, paths = sh.enumerate_paths(dp, x, P)
    assert ll > -math.inf and len(paths) >= 10
    n = 4096
    _, samples = dp.samplePaths(x, P, n, seed=FREQ_SEED)
    seen = {}
    for edges, rows, _ in samples:
        key = (tuple(int(e) for e in edges), tuple(int(r) for r in rows))
        seen[key] = seen.get(key, 0) + 1
    assert set(seen) <= set(paths)
    for key, (q, _w) in paths.items():
        assert abs(seen.get(key, 0) - n * q) <= 5.0 * math.sqrt(n * q * (1.0 - q)) + 1.0, (key, seen.get(key, 0), n * q)
    assert len(seen) >= 10


# ---- 4. the inputs of the GPU module --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sh.CASES))
def test_gpu_suite_inputs_are_live(name):
    """For every case the GPU module compares with the yardstick: the least distance of a uniform from a partial sum of its decision,
    over all decisions of all samples, is above 1e-9 -- the device's Forward cells sit within a few 1e-15 relative of the yardstick's
    (docs/profile_tapes.md), so its partial sums differ by about 1e-12 at most, and a margin of 1e-9 leaves three orders of magnitude.
    And the share of finite likelihoods the GPU test relies on: a dead pair where the case says so, nine in ten live."""
    n, seed, dead, _ = sh.CASES[name]
    margins = []
    refs = sh.reference(name, margins)
    lls = np.array([ll for group in refs for ll, _ in group])
    assert len(margins) > 0 and min(margins) > sh.MARGIN, (name, min(margins))
    assert ((lls == -math.inf).any()) == dead, (name, lls)
    assert np.mean(lls > -math.inf) >= 0.9, (name, np.mean(lls > -math.inf))
    for group in refs:
        for ll, samples in group:
            assert len(samples) == n and all((q == -math.inf) == (ll == -math.inf) for _e, _r, q in samples)
    print("%s: %d decisions, least margin %.3g, %d pairs, %d dead" % (name, len(margins), min(margins), len(lls), int((lls == -math.inf).sum())))


def test_gpu_suite_shapes_are_what_the_cases_need():
    """The mixed batch has dead pairs of each kind and differs under a second seed; the chain's paths fill their slots; the one-hot
    pairs have one path each; the long case has paths of a few hundred edges; the chunked call cuts the mixed batch several times."""
    _, seed, groups = sh.case("mixed")
    em, triples = groups[0]
    refs = sh.reference("mixed")[0]
    assert {triples[k][2] is None for k in eh.MIXED_DEAD} == {True, False}
    other = [PairProfileDP(em).samplePaths(x, P, sh.MIXED_SAMPLES, seed=sh.SEED_B, pair=k, env=env)[1] for k, (x, P, env) in enumerate(triples[:4])]
    assert any(not np.array_equal(a[0], b[0]) for k in range(4) for a, b in zip(refs[k][1], other[k]))
    b = sh.sample_call_bytes(em, triples, sh.MIXED_SAMPLES)
    chunks = eh.greedy_chunks(b, int(eh.MIXED_BUDGET_FACTOR * max(b)))
    assert len(chunks) >= 4 and {"P", "E"} <= set("".join(eh.chunk_kinds(chunks, [t[2] for t in triples]))), chunks
    _, _, groups = sh.case("chain")
    em, triples = groups[0]
    nLev = eh.silent_levels(em)
    for (x, P, _), (ll, samples) in zip(triples, sh.reference("chain")[0]):
        assert ll > -math.inf and all(len(e) == eh.path_bound(nLev, len(x), len(P)) for e, _r, _q in samples)
    _, _, groups = sh.case("hot")
    em, triples = groups[0]
    dp = PairProfileDP(em)
    for (x, P, _), (ll, samples) in zip(triples, sh.reference("hot")[0]):
        assert len(sh.enumerate_paths(dp, x, P)[1]) == 1
        v, edges, rows = dp.viterbi(x, P)
        assert all(np.array_equal(e, edges) and np.array_equal(r, rows) and abs(q) <= 1e-9 for e, r, q in samples)
    lens = [len(e) for e, _r, _q in sh.reference("long")[0][0][1]]
    assert min(lens) >= 200, lens


def test_statistics_case_is_met_by_the_yardsticks_own_samples():
    """The bound the GPU test applies to the device's 4 096 samples against the device's counts, applied to the yardstick's samples
    against the yardstick's counts, under the same seed."""
    em, triples = sh._stat()[0]
    x, P, _ = triples[0]
    dp = PairProfileDP(em)
    blanks = []
    counts, ll = dp.counts(x, P, blanks=blanks)
    assert ll > -math.inf and int((counts >= 1e-3).sum()) >= 8
    margins = []
    _, samples = dp.samplePaths(x, P, sh.STAT_SAMPLES, seed=sh.STAT_SEED, margins=margins)
    assert min(margins) > sh.MARGIN
    u = sh.usage(em.nTransitions, [e for e, _r, _q in samples])
    bad = sh.usage_within_bound(u, counts, np.nonzero(em.outTok > 0)[0], blanks[0], len(P))
    assert not bad, bad


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_declares_the_entry():
    from machineboss_amd import capi
    text = open(os.path.join(os.path.dirname(HERE), "include", "mbhip.h")).read()
    assert "mb_profile_pairs_sample" in capi.EXPORTS and "int mb_profile_pairs_sample(" in text
    assert "sampling takes plain profiles" in text
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mb_profile_pairs_sample")
    assert hasattr(capi.DeviceProfilePairs, "sample_paths")


def test_sample_profile_pairs_numpy_backend():
    """boss.sampleProfilePairs with the numpy backend: MachinePaths whose transitions spell the input, logq, likelihoods; an input that
    cannot be tokenised gets empty paths and -inf."""
    from machineboss_amd import boss
    from machineboss_amd.evalmachine import EvaluatedMachine
    m, prof, inputs = sh.boss_case()
    n = sh.BOSS_SAMPLES
    full = None
    for band in sh.BOSS_BANDS:
        paths, logq, ll = boss.sampleProfilePairs(m, inputs, prof, n, seed=sh.BOSS_SEED, backend="numpy", band=band)
        assert len(paths) == 4 and all(len(p) == n for p in paths) and ll[2] == -math.inf and min(ll[0], ll[1], ll[3]) > -math.inf
        assert all(q == -math.inf and not p.trans for p, q in zip(paths[2], logq[2]))
        for k in (0, 1, 3):
            for p, q in zip(paths[k], logq[k]):
                assert [t.inp for t in p.trans if t.inp] == inputs[k] and -50.0 < q <= 0.0
        full = ll if band is None else full
        assert all(a <= b for a, b in zip(ll, full))
        # the device test compares these paths for equality: the margins of its inputs (the tokenisable inputs, numbered in order)
        ev = EvaluatedMachine.fromMachine(m, None)
        P, margins = prof.logRows(ev), []
        for k, seq in enumerate(s for s in inputs if s != ["z"]):
            x = ev.inputTokenizer.tokenize(seq)
            PairProfileDP(ev).samplePaths(x, P, n, seed=sh.BOSS_SEED, pair=k, margins=margins,
                                          env=None if band is None else Envelope.band(len(x), len(P), band))
        assert margins and min(margins) > sh.MARGIN
    with pytest.raises(Exception):
        boss.sampleProfilePairs(m, [["a"]], prof, 0, backend="numpy")
