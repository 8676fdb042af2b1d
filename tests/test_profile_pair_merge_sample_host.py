"""Posterior path samples of pairs against CTC-merged profiles, without a GPU (docs/profile_tapes.md, "Posterior path samples of pairs
against a merged profile"): the yardstick profile.PairMergedProfileDP.samplePaths against an enumeration of every lattice path written
from the recurrence, pathWeight against the labelling rules, the frequencies of the draws, and the conditions the GPU module
(test_profile_pair_merge_sample_gpu.py) relies on for its inputs -- every uniform clear of every partial sum, the share of live
pairs, the statistics bounds met by the yardstick's own samples."""
import ctypes
import math
import os

import numpy as np
import pytest

import pairenvhelpers as eh
import pairmergehelpers as mh
import pairmergesamplehelpers as msh
import pairsamplehelpers as sh
from pairprofilehelpers import pair_machine
from machineboss_amd.profile import PairMergedProfileDP
from machineboss_amd.seqpair import Envelope

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _inside(dp, x, P, env):
    rows = dp.envelopeRows(env, len(x), len(P))
    return None if rows is None else [set(rs) for rs in rows]


def _forward(dp, x, P, env):
    return dp.forward(x, P, env=env) if env is not None else dp.forward(x, P)


# ---- 1. the yardstick against every lattice path, one by one --------------------------------------------------------------------------------
ENUM_SHAPES = ((0, 0), (0, 2), (2, 0), (1, 1), (2, 2), (3, 2), (3, 3))
# (S, silent levels, colTok, machine seed): nCols in {1, 2}, and two columns on one token; the seeds are those under which at least nine
# in ten of the machine's lattices score above -inf, asserted below; (0, 0) goes to the machines with levels alone -- without a silent edge
# nothing can move there and the pair is dead whatever the seed
ENUM_MACHINES = ((2, True, (1,), 20), (2, False, (2, 1), 21), (3, True, (1, 2), 36), (4, True, (2, 2), 40), (4, False, (1, 2), 42), (3, False, (2,), 31))


def _enum_envelopes(I, L):
    out = [("plain", None), ("stairs", eh.staircase(I, L))]
    try:
        out.append(("band1", Envelope.band(I, L, 1)))
    except Exception:
        pass
    return out


def _check_enumeration(dp, x, P, env):
    """(loglike, paths, worst): the three assertions of one lattice; paths is None where the enumeration outgrew its budget."""
    ll, N, W = _forward(dp, x, P, env)
    try:
        paths = msh.enumerate_lattice_paths(dp, x, P, env)
    except msh.TooMany:
        return ll, None, 0.0
    weights = [dp.pathWeight(x, P, e, r, c) for e, r, c, _steps in paths]
    assert all(w > -math.inf for w in weights) or not ll > -math.inf
    assert len({p[:3] for p in paths}) == len(paths)          # (edges, rows, rowCol) names the lattice path
    live = [(p, w) for p, w in zip(paths, weights) if w > -math.inf]
    if not ll > -math.inf:
        assert not live
        return ll, paths, 0.0
    total = sum(math.exp(w - ll) for _p, w in live)
    assert abs(total - 1.0) <= 1e-9, (total, len(live))         # sum exp(weight) = exp(loglike)
    inside = _inside(dp, x, P, env)
    worst, psum = 0.0, 0.0
    for (_e, _r, _c, steps), w in live:
        prob, want = msh.choice_product(dp, x, P, ll, N, W, inside, steps), math.exp(w - ll)
        assert abs(prob - want) <= 1e-9 * max(1.0, abs(want)), (prob, want)
        worst = max(worst, abs(prob - want))
        psum += prob
    assert abs(psum - 1.0) <= 1e-9, psum
    return ll, paths, worst


@pytest.mark.parametrize("S,levels,colTok,seed", ENUM_MACHINES)
def test_choice_probabilities_multiply_to_the_posterior_of_every_lattice_path(S, levels, colTok, seed):
    """Lattices up to (3, 3), plain, under band(1) and under a staircase.  Every lattice path comes from a forward recursion over
    (i, r, plane, state, layer) written from the recurrence; its weight from pathWeight.  The weights sum to the likelihood; for every
    path the product of the yardstick's choice probabilities is exp(weight - loglike) at 1e-9; the products sum to 1 at 1e-9.  A
    staircase with one column is left out of the count of live lattices (see test_a_staircase_with_one_column_is_dead)."""
    em = pair_machine(S, seed, levels, 2, 2)
    dp = PairMergedProfileDP(em, colTok)
    finite, tried, kinds, worst, most = 0, 0, set(), 0.0, 0
    for I, L in ENUM_SHAPES:
        if (I, L) == (0, 0) and not levels:
            continue
        x, P = mh.merged_input(np.random.RandomState(100 * seed + 10 * I + L), em, len(colTok), I, L, zeros=0.05)
        for kind, env in _enum_envelopes(I, L):
            if kind == "stairs" and len(colTok) == 1:
                continue
            ll, paths, w = _check_enumeration(dp, x, P, env)
            if paths is None:
                continue
            tried += 1
            if ll > -math.inf:
                finite += 1; kinds.add(kind); most = max(most, len(paths)); worst = max(worst, w)
    assert tried >= 10 and finite >= 0.9 * tried and kinds >= {"plain", "band1"}, (finite, tried, kinds)
    print("choice products against path weights: worst %.3g over %d of %d lattices, up to %d lattice paths" % (worst, finite, tried, most))


def test_a_staircase_with_one_column_is_dead():
    """At I = L = 2 every row of the staircase is one cell, so each row is a match; two matches in a row need two columns."""
    em = pair_machine(3, 30, True, 2, 2)
    dp = PairMergedProfileDP(em, (1,))
    x, P = mh.merged_input(np.random.RandomState(5), em, 1, 2, 2, zeros=0.0)
    env = eh.staircase(2, 2)
    ll, paths, _ = _check_enumeration(dp, x, P, env)
    assert ll == -math.inf and paths == []
    got, samples = dp.samplePaths(x, P, 3, env=env)
    assert got == -math.inf and all(len(e) == 0 and q == -math.inf and (c == -1).all() and len(c) == 2 for e, _r, c, q in samples)
    assert dp.forward(x, P)[0] > -math.inf


# ---- 2. draw counts, 3. replay --------------------------------------------------------------------------------------------------------------
FREQ_SEED = 1


def _freq_case():
    em = pair_machine(3, 103, True, 2, 3)
    x, P = mh.merged_input(np.random.RandomState(2203), em, 2, 2, 2, zeros=0.0)
    return em, (1, 2), x, P


def test_frequencies_of_4096_draws_follow_the_enumerated_posterior():
    """One pair at (2, 2), S = 3 with levels, two columns: the count of every lattice path lies within 5 sqrt(n q (1 - q)) + 1 of
    n q.  The seed is fixed so that this holds; a seed is a property checked here."""
    em, colTok, x, P = _freq_case()
    dp = PairMergedProfileDP(em, colTok)
    paths = msh.enumerate_lattice_paths(dp, x, P)
    n = 4096
    ll, samples = dp.samplePaths(x, P, n, seed=FREQ_SEED)
    assert ll > -math.inf and len(paths) >= 10
    q = {p[:3]: math.exp(dp.pathWeight(x, P, *p[:3]) - ll) for p in paths}
    seen = {}
    for e, r, c, _lq in samples:
        k = msh.key_of(e, r, c)
        seen[k] = seen.get(k, 0) + 1
    assert set(seen) <= set(q)
    for k, qk in q.items():
        assert abs(seen.get(k, 0) - n * qk) <= 5.0 * math.sqrt(n * qk * (1.0 - qk)) + 1.0, (k, seen.get(k, 0), n * qk)
    assert len(seen) >= 10


def test_logq_of_a_sample_is_its_path_weight_minus_the_likelihood():
    """pathWeight of every sampled (edges, rows, rowCol) minus loglike is logq at 1e-9, plain and under a band; rowCol is 0 on exactly
    the rows the lattice path took as blanks; samples are prefixes of longer calls and depend on (seed, pair, j) alone."""
    em, colTok, x, P = _freq_case()
    dp = PairMergedProfileDP(em, colTok)
    for env in (None, Envelope.band(2, 2, 1)):
        steps = {p[:3]: p[3] for p in msh.enumerate_lattice_paths(dp, x, P, env)}
        ll, samples = dp.samplePaths(x, P, 60, seed=3, pair=2, env=env)
        assert ll > -math.inf
        blanks = 0
        for e, r, c, lq in samples:
            w = dp.pathWeight(x, P, e, r, c)
            assert abs(lq - (w - ll)) <= 1e-9 * max(1.0, abs(lq)), (lq, w - ll)
            took = msh.blank_rows(steps[msh.key_of(e, r, c)])
            assert [int(v) for v in np.nonzero(c == 0)[0]] == took
            blanks += len(took)
        assert blanks > 0
    a = dp.samplePaths(x, P, 3, seed=3, pair=2)[1]
    b = dp.samplePaths(x, P, 9, seed=3, pair=2)[1]
    assert all(msh.key_of(*p[:3]) == msh.key_of(*q[:3]) and p[3] == q[3] for p, q in zip(a, b))
    c = dp.samplePaths(x, P, 9, seed=3, pair=3)[1]
    assert any(msh.key_of(*p[:3]) != msh.key_of(*q[:3]) for p, q in zip(b, c))


def test_path_weight_refuses_what_is_no_lattice_path():
    """The labelling rules of pathWeight on one sampled path with a blank, a repeat and an emission in it: each broken on its own."""
    em, colTok, x, P = _freq_case()
    dp = PairMergedProfileDP(em, colTok)
    ll, samples = dp.samplePaths(x, P, 400, seed=5)
    with_repeat = with_blank = None
    for e, r, c, _q in samples:
        free = [k for k in range(len(c)) if k not in set(int(v) for v in r[em.outTok[e] > 0])]
        if with_repeat is None and any(c[k] > 0 for k in free):
            with_repeat = (e, r, c, [k for k in free if c[k] > 0][0])
        if with_blank is None and any(c[k] == 0 for k in free):
            with_blank = (e, r, c, [k for k in free if c[k] == 0][0])
    assert with_repeat is not None and with_blank is not None
    e, r, c, k = with_repeat
    assert k > 0 and c[k - 1] == c[k] and dp.pathWeight(x, P, e, r, c) > -math.inf
    bad = c.copy(); bad[k] = 3 - c[k]                      # a row no edge consumed under another column than the row before
    assert dp.pathWeight(x, P, e, r, bad) == -math.inf
    e, r, c, k = with_blank
    bad = c.copy(); bad[k] = 1 if (k == 0 or c[k - 1] != 1) else 2      # label c >= 1 with no edge and no such row before it
    assert dp.pathWeight(x, P, e, r, bad) == -math.inf
    emitted = [int(v) for v in r[em.outTok[e] > 0]]
    if emitted:
        bad = c.copy(); bad[emitted[0]] = 0                # the blank on a row an edge consumed
        assert dp.pathWeight(x, P, e, r, bad) == -math.inf
        bad = c.copy(); bad[emitted[0]] = 3 - c[emitted[0]]      # the other column: the edge does not write its token
        assert dp.pathWeight(x, P, e, r, bad) == -math.inf
    assert dp.pathWeight(x, P, e[:-1], r[:-1], c) == -math.inf if len(e) else True
    assert dp.pathWeight(x, P, e, r, c[:-1]) == -math.inf
    # two columns on one token: a fresh emission into the column the row before took is no lattice path, the other column is
    dp2 = PairMergedProfileDP(em, (1, 1))
    _, s2 = dp2.samplePaths(x, P, 200, seed=6)
    hit = 0
    for e, r, c, _q in s2:
        for row in (int(v) for v in r[em.outTok[e] > 0]):
            if row > 0 and c[row - 1] > 0 and c[row - 1] != c[row]:
                bad = c.copy(); bad[row] = c[row - 1]
                assert dp2.pathWeight(x, P, e, r, bad) == -math.inf
                hit += 1
    assert hit > 0


# ---- 4. the inputs of the GPU module --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(msh.CASES))
def test_gpu_suite_inputs_are_live(name):
    """For every case the GPU module compares with the yardstick: the least distance of a uniform from a partial sum of its decision,
    over all decisions of all samples, is above 1e-9 -- the device's Forward cells sit within a few 1e-15 relative of the yardstick's
    (docs/profile_tapes.md), so its partial sums differ by about 1e-12 at most.  And the share of finite likelihoods the case claims:
    a dead pair where it says so, nine in ten live (LIVE_SHARE where a case claims another share)."""
    n, seed, dead, _ = msh.CASES[name]
    margins = []
    refs = msh.reference(name, margins)
    lls = np.array([ll for group in refs for ll, _ in group])
    assert len(margins) > 0 and min(margins) > msh.MARGIN, (name, min(margins))
    assert ((lls == -math.inf).any()) == dead, (name, lls)
    assert np.mean(lls > -math.inf) >= msh.LIVE_SHARE.get(name, 0.9), (name, np.mean(lls > -math.inf))
    for (em, colTok, triples), group in zip(msh.case(name)[2], refs):
        for (x, P, _env), (ll, samples) in zip(triples, group):
            assert len(samples) == n
            for _e, _r, c, q in samples:
                assert (q == -math.inf) == (ll == -math.inf) and len(c) == len(P) and ((c == -1).all() if ll == -math.inf else (c >= 0).all())
    print("%s: %d decisions, least margin %.3g, %d pairs, %d dead" % (name, len(margins), min(margins), len(lls), int((lls == -math.inf).sum())))


def test_gpu_suite_shapes_are_what_the_cases_need():
    """The mixed batch has dead pairs of each kind, differs under a second seed and is cut several times by the chunked call; the
    ragged batch has ten pairs, one dead; the column maps hold two columns on one token, a column nothing emits and a generator; the
    one-hot pairs have one lattice path each, whose labels are the frames' argmax; the long case has paths of a hundred edges."""
    _, seed, groups = msh.case("mixed")
    em, colTok, triples = groups[0]
    refs = msh.reference("mixed")[0]
    assert {triples[k][2] is None for k in eh.MIXED_DEAD} == {True, False}
    dp = PairMergedProfileDP(em, colTok)
    other = [dp.samplePaths(x, P, msh.MIXED_SAMPLES, seed=msh.SEED_B, pair=k, env=env)[1] for k, (x, P, env) in enumerate(triples[:4])]
    assert any(msh.key_of(*a[:3]) != msh.key_of(*b[:3]) for k in range(4) for a, b in zip(refs[k][1], other[k]))
    back = triples[::-1][:6]          # the batch order test: the last six pairs reversed, each under its new index
    margins = []
    for k, (x, P, env) in enumerate(back):
        dp.samplePaths(x, P, 3, seed=seed, pair=k, env=env, margins=margins)
    assert min(margins) > msh.MARGIN and {t[2] is None for t in back} == {True, False}
    b = msh.sample_call_bytes(em, len(colTok), triples, msh.MIXED_SAMPLES)
    chunks = eh.greedy_chunks(b, int(eh.MIXED_BUDGET_FACTOR * max(b)))
    assert len(chunks) >= 4 and {"P", "E"} <= set("".join(eh.chunk_kinds(chunks, [t[2] for t in triples]))), chunks
    (_, _, ragged), = msh.case("ragged")[2]
    lls = [ll for ll, _ in msh.reference("ragged")[0]]
    assert len(ragged) == 10 and sum(ll == -math.inf for ll in lls) == 1
    maps = msh.case("maps")[2]
    assert any(len(set(int(t) for t in ct)) < len(ct) for _e, ct, _t in maps) and any(e.nInTok == 0 for e, _c, _t in maps)
    assert any(not np.any(np.isin(e.outTok, [int(t)])) for e, ct, _t in maps for t in ct)
    (em, colTok, triples), = msh.case("hot")[2]
    dp = PairMergedProfileDP(em, colTok)
    for (x, P, _), (ll, samples), labels in zip(triples, msh.reference("hot")[0], msh.hot_labels()):
        assert len(msh.enumerate_lattice_paths(dp, x, P)) == 1
        v, edges, rows = dp.viterbi(x, P)
        assert all(np.array_equal(e, edges) and np.array_equal(r, rows) and np.array_equal(c, labels) and abs(q) <= 1e-9 for e, r, c, q in samples)
    assert any((labels[1:] == labels[:-1]).any() and (labels == 0).any() for labels in msh.hot_labels() if len(labels) > 1)
    lens = [len(e) for e, _r, _c, _q in msh.reference("long")[0][0][1]]
    assert min(lens) >= 100, lens


def test_statistics_case_is_met_by_the_yardsticks_own_samples():
    """The bounds the GPU test applies to the device's 4 096 samples against the device's counts and merged row posteriors, applied to
    the yardstick's samples against the yardstick's, under the same seed."""
    (em, colTok, triples), = msh._stat()
    x, P, _ = triples[0]
    dp = PairMergedProfileDP(em, colTok)
    blanks = []
    counts, ll = dp.counts(x, P, blanks=blanks)
    post, _ = dp.rowPosteriors(x, P)
    assert ll > -math.inf and int((counts >= 1e-3).sum()) >= 8 and int((post >= 1e-3).sum()) >= 6
    margins = []
    _, samples = dp.samplePaths(x, P, msh.STAT_SAMPLES, seed=msh.STAT_SEED, margins=margins)
    assert min(margins) > msh.MARGIN
    u = sh.usage(em.nTransitions, [e for e, _r, _c, _q in samples])
    bad = sh.usage_within_bound(u, counts, np.nonzero(em.outTok > 0)[0], blanks[0], len(P))
    assert not bad, bad
    bad = msh.row_col_within_bound([c for _e, _r, c, _q in samples], post)
    assert not bad, bad


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_declares_the_entry():
    from machineboss_amd import capi
    text = open(os.path.join(ROOT, "include", "mbhip.h")).read()
    assert "mb_profile_pairs_sample_merged" in capi.EXPORTS and "int mb_profile_pairs_sample_merged(" in text
    assert "merged sampling takes merged profiles" in text
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mb_profile_pairs_sample_merged")
    assert hasattr(capi.DeviceProfilePairs, "merged_sample_paths") and hasattr(capi.DeviceProfilePairs, "sample_paths")
    api = open(os.path.join(ROOT, "machineboss_amd", "csrc", "mb_profile_api.hip")).read()
    assert '"sampling takes plain profiles"' in api and '"merged sampling takes merged profiles"' in api


def test_sample_merged_pairs_numpy_backend():
    """boss.sampleMergedPairs with the numpy backend: MachinePaths whose transitions spell the input, a label for every frame, logq,
    likelihoods; an input that cannot be tokenised gets empty paths, labels of -1 and -inf."""
    from machineboss_amd import boss
    from machineboss_amd.evalmachine import EvaluatedMachine
    m, prof, inputs = msh.boss_case()
    n = msh.BOSS_SAMPLES
    full = None
    for band in msh.BOSS_BANDS:
        paths, rowCols, logq, ll = boss.sampleMergedPairs(m, inputs, prof, n, seed=msh.BOSS_SEED, backend="numpy", band=band)
        assert len(paths) == 4 and all(len(p) == n for p in paths) and ll[2] == -math.inf and min(ll[0], ll[1], ll[3]) > -math.inf
        assert all(q == -math.inf and not p.trans and (c == -1).all() for p, c, q in zip(paths[2], rowCols[2], logq[2]))
        for k in (0, 1, 3):
            for p, c, q in zip(paths[k], rowCols[k], logq[k]):
                assert [t.inp for t in p.trans if t.inp] == inputs[k] and -50.0 < q <= 0.0
                assert len(c) == len(prof) and (c >= 0).all() and (c <= 2).all()
                emitted = [t.out for t in p.trans if t.out]
                fresh = [int(v) for r, v in enumerate(c) if v and (r == 0 or c[r - 1] != v)]
                assert emitted == [("x", "y")[v - 1] for v in fresh]      # a fresh column is an emission, a held one a repeat
        full = ll if band is None else full
        assert all(a <= b for a, b in zip(ll, full))
        # the device test compares these paths for equality: the margins of its inputs (the tokenisable inputs, numbered in order)
        ev = EvaluatedMachine.fromMachine(m, None)
        P, colTok = boss._mergedRows(prof, ev)
        margins = []
        for k, seq in enumerate(s for s in inputs if s != ["z"]):
            x = ev.inputTokenizer.tokenize(seq)
            PairMergedProfileDP(ev, colTok).samplePaths(x, P, n, seed=msh.BOSS_SEED, pair=k, margins=margins,
                                                        env=None if band is None else Envelope.band(len(x), len(P), band))
        assert margins and min(margins) > msh.MARGIN
    with pytest.raises(Exception):
        boss.sampleMergedPairs(m, [["a"]], prof, 0, backend="numpy")
