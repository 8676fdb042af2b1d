"""CPU tests of the two-tape merged (CTC) profile sweeps (machineboss_amd/profile.py: PairMergedProfileDP): the numpy restatement
against the oracle's exact Forward on algebra.compose(M, merging recogniser) run on input x with an empty output, its reductions
(I = 0 is MergedProfileDP, Backward = Forward, input-reading counts sum to I, counts against finite differences), the tie census,
boss.scoreProfilePairs, and the liveness of the GPU suite's inputs (docs/profile_tapes.md, "Pairs against a merged profile")."""
import math

import numpy as np
import pytest

import pairmergehelpers as pm
from mergehelpers import merged_rows
from pairprofilehelpers import counts_close, logs_close, pair_machine
from profhelpers import _machine_of
from machineboss_amd import algebra, boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile

SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (5, 2))
MACHINES = [(S, lv) for S in (5, 8) for lv in (True, False)]
COLS = (1, 2, 4)
SEEDS = range(3)
CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"
DNA_SEQS = ([], ["0_3"], ["0_3", "2_3"], ["0_3", "2_3", "1_3"], ["1_3", "1_3", "0_3", "2_3"])


def _profile_of(em, P, colTok):
    """The Profile whose mergeRows(em) is (P, colTok): one header column per entry of colTok, the blank last."""
    return Profile([em.outputTokenizer.tok2sym[t] for t in colTok], [list(np.exp(row[1:])) + [float(np.exp(row[0]))] for row in P])


def _composite_loglike(oracle_mod, M, em, x, profile):
    comp = algebra.compose(M, profile.mergingRecogniserMachine(), True, False)
    ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
    syms = [em.inputTokenizer.tok2sym[t] for t in x]
    if not ec.inputTokenizer.canTokenize(syms):
        return -math.inf
    return oracle_mod.OracleMachine(ec).loglike(ec.inputTokenizer.tokenize(syms), [], oracle_mod.SUM_EXACT)


def _cases():
    for S, lv in MACHINES:
        for nCols in COLS:
            for seed in SEEDS:
                em = pair_machine(S, seed, lv, 2, 3)
                rng = np.random.RandomState(7 * seed + nCols)
                colTok = rng.randint(1, 4, nCols)
                for I, L in SHAPES:
                    x = rng.randint(1, 3, size=I).astype(np.int32)
                    yield (S, lv, nCols, seed, I, L), em, colTok, x, merged_rows(rng, nCols, L, zeros=0.1)


@pytest.fixture(scope="module")
def swept():
    out, dps = {}, {}
    for key, em, colTok, x, P in _cases():
        dp = dps.setdefault(key[:4], PairMergedProfileDP(em, colTok))
        out[key] = dict(em=em, colTok=colTok, x=x, P=P, dp=dp, ll=dp.forward(x, P)[0])
    return out


def test_forward_equals_composition(oracle_mod, swept):
    """The proposed recurrence is the composite's: 1e-9 relative, -inf exact, at least nine in ten likelihoods finite."""
    fin = []
    for key, c in swept.items():
        em = c["em"]
        want = _composite_loglike(oracle_mod, _machine_of(em), em, c["x"], _profile_of(em, c["P"], c["colTok"]))
        assert logs_close([c["ll"]], [want]), (key, c["ll"], want)
        fin.append(want > -math.inf)
    assert len(fin) == len(MACHINES) * len(COLS) * len(SEEDS) * len(SHAPES) and np.mean(fin) >= 0.9, np.mean(fin)


def test_dnastore_against_tiny_csv(oracle_mod):
    m = Machine.fromFile(DNASTORE)
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    prof = Profile.fromCsv(CSV)
    P, colTok = prof.mergeRows(em)
    assert len(colTok) >= 1
    dp = PairMergedProfileDP(em, colTok)
    fin = 0
    for seq in DNA_SEQS:
        x = em.inputTokenizer.tokenize(seq)
        got, want = dp.forward(x, P)[0], _composite_loglike(oracle_mod, m, em, x, prof)
        assert logs_close([got], [want]), (seq, got, want)
        fin += want > -math.inf
    assert fin >= 1


def test_reductions(swept):
    for key, c in swept.items():
        em, x, P, dp = c["em"], c["x"], c["P"], c["dp"]
        bl = dp.backward(x, P)[0]
        assert logs_close([bl], [c["ll"]]), (key, bl, c["ll"])
        counts, ll = dp.counts(x, P)
        if not ll > -math.inf:
            assert not counts.any()
            continue
        assert abs(counts[em.inTok > 0].sum() - len(x)) <= 1e-9 * max(1, len(x)), key
        net = np.zeros(em.nStates)
        np.add.at(net, em.dst.astype(np.int64), counts); np.subtract.at(net, em.src.astype(np.int64), counts)
        want = np.zeros(em.nStates); want[-1] += 1.0; want[0] -= 1.0
        assert np.allclose(net, want, rtol=0, atol=1e-9), (key, net)
        if len(x) == 0:
            one = MergedProfileDP(em, c["colTok"])
            l1, N1, W1 = one.forward(P)
            l2, N2, W2 = dp.forward(x, P)
            assert logs_close([l2], [l1], 1e-12) and logs_close(N2[0], N1, 1e-12) and logs_close(W2[0], W1, 1e-12), key
            assert np.allclose(counts, one.counts(P)[0], rtol=1e-12, atol=1e-15), key
            v1, e1, r1 = one.viterbi(P); v2, e2, r2 = dp.viterbi(x, P)
            assert logs_close([v2], [v1], 1e-12) and np.array_equal(e1, e2) and np.array_equal(r1, r2), key


def test_counts_equal_finite_differences():
    """d loglike / d w_t = the count of t: central differences at 1e-6 on a lattice of six cells, every transition."""
    em = pair_machine(5, 1, True, 2, 3)
    colTok = [1, 2, 1]
    rng = np.random.RandomState(3)
    x, P = np.array([1, 2], np.int32), merged_rows(rng, 3, 1, zeros=0.0)
    counts, ll = PairMergedProfileDP(em, colTok).counts(x, P)
    assert ll > -math.inf and counts.sum() > 1.0
    h = 1e-6
    for t in range(em.nTransitions):
        d = np.zeros(em.nTransitions); d[t] = h
        up = PairMergedProfileDP(em.withLogWeights(em.logWeight + d), colTok).forward(x, P)[0]
        dn = PairMergedProfileDP(em.withLogWeights(em.logWeight - d), colTok).forward(x, P)[0]
        assert abs((up - dn) / (2 * h) - counts[t]) <= 1e-6 * max(1.0, counts[t]), (t, (up - dn) / (2 * h), counts[t])


def _path_weight(em, colTok, x, P, edges, rows):
    """The weight of a Viterbi path with the best reading of its rows (mergehelpers.merged_path_weight) -- and its edges read x."""
    from mergehelpers import merged_path_weight
    assert [int(em.inTok[e]) for e in edges if em.inTok[e]] == list(x)
    return merged_path_weight(em, P, colTok, edges, rows)


def test_tie_census_and_replay(swept):
    """On the doubled tie machine (weights multiples of log 0.5) against quantised rows every kind of tie is met at least once and
    every sum is exact: the path replays to the score exactly.  On the random cases the path replays to 1e-9."""
    em = pm.merged_tie_machine()
    dp = PairMergedProfileDP(em, pm.TIE_COLTOK)
    census = {}
    pairs = pm.tie_pairs()
    for x, P in pairs:
        v, edges, rows = dp.viterbi(x, P, census)
        assert v > -math.inf and _path_weight(em, pm.TIE_COLTOK, x, P, edges, rows) == v
    assert len(pairs) == 16 and all(census.get(k, 0) >= 1 for k in pm.TIE_KINDS), census
    for key, c in swept.items():
        v, edges, rows = c["dp"].viterbi(c["x"], c["P"])
        if v > -math.inf:
            w = _path_weight(c["em"], c["colTok"], c["x"], c["P"], edges, rows)
            assert abs(w - v) <= 1e-9 * max(1.0, abs(v)) and list(rows) == sorted(rows), (key, w, v)
        else:
            assert len(edges) == 0


def test_checks():
    em = pair_machine(5, 0, True, 2, 3)
    with pytest.raises(MachineError):
        PairMergedProfileDP(em, [])
    with pytest.raises(MachineError):
        PairMergedProfileDP(em, [1, 4])
    dp = PairMergedProfileDP(em, [1, 2])
    P = np.zeros((2, 3))
    for bad in ([0], [3]):
        with pytest.raises(MachineError):
            dp.forward(bad, P)
    for v in (np.nan, np.inf):
        Q = P.copy(); Q[1, 2] = v
        with pytest.raises(MachineError):
            dp.forward([1], Q)


def test_score_profile_pairs_numpy():
    """boss.scoreProfilePairs(merge=True) through the numpy backend is PairMergedProfileDP on Profile.mergeRows; an input that cannot
    be tokenised scores -inf."""
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(CSV)
    P, colTok = prof.mergeRows(em)
    dp = PairMergedProfileDP(em, colTok)
    seqs = [["0_3", "2_3"], ["0_3", "zz"], ["0_3", "2_3", "1_3"]]
    sc, pc = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par, merge=True, loglike=True, viterbi=True, counts=True)
    for k, seq in enumerate(seqs):
        if k == 1:
            assert sc["loglike"][k] == -math.inf and sc["viterbi"][k] == -math.inf
            continue
        x = em.inputTokenizer.tokenize(seq)
        assert sc["loglike"][k] == dp.forward(x, P)[0] and sc["viterbi"][k] == dp.forward(x, P, "max")[0]
    assert isinstance(pc, dict)
    plain, none = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par)
    assert none is None and plain["viterbi"] is None and len(plain["loglike"]) == 3


def test_edge_suite_inputs_are_live():
    """The inputs of test_profile_pair_merge_gpu.py under the restatement: finite shares, the tie census, the rings on the intended
    side of 64 KiB and 160 KiB, the chunk count under the lowered budget, the counts case past the LDS table and under the
    fixed point's error budget."""
    for nCols, S in pm.LANE_CASES:
        fin = []
        for em, colTok, pairs in pm.lane_case(nCols, S):
            dp = PairMergedProfileDP(em, colTok)
            fin += [dp.forward(x, P)[0] > -math.inf for x, P in pairs]
        assert np.mean(fin) >= 0.9, (nCols, S, np.mean(fin))
    rb = [pm.ring_bytes(pm.RING_S, 4, I, L) for I, L in pm.RING_SHAPES]
    assert rb[0] == 336 * 4 * 40 <= 64 * 1024 < rb[1] <= pm.LDS_MAX and rb[2] <= pm.LDS_MAX < rb[3] and rb[4] == rb[3]
    em, colTok, pairs = pm.ragged_case()
    dp = PairMergedProfileDP(em, colTok)
    lls = [dp.forward(x, P)[0] for x, P in pairs]
    assert all(v > -math.inf for v in lls[:-1]) and lls[-1] == -math.inf
    scratch = [0 if pm.ring_bytes(pm.RING_S, 4, len(x), len(P)) <= pm.LDS_MAX else pm.ring_bytes(pm.RING_S, 4, len(x), len(P)) for x, P in pairs]
    assert sum(b > 0 for b in scratch) == 2
    assert len(pm.greedy_chunks(scratch, pm.RAGGED_BUDGET)) >= 2
    em, colTok, pairs = pm.packed_case()
    assert len(pairs) == 24 and all(pm.ring_bytes(pm.PACKED_S, 4, len(x), len(P)) > pm.LDS_MAX for x, P in pairs)
    dp = PairMergedProfileDP(em, colTok)
    assert np.mean([dp.forward(x, P)[0] > -math.inf for x, P in pairs]) >= 0.9
    em, colTok, pairs, dead = pm.big_counts_case()
    dp = PairMergedProfileDP(em, colTok)
    assert em.nTransitions > 8192 and all(dp.forward(x, P)[0] > -math.inf for x, P in pairs) and dp.forward(*dead)[0] == -math.inf
    # adds per transition: at most nCols + 1 = 3 per cell (an emitting edge once per plane other than its column's, an output-less
    # edge once per plane), each rounded to the nearest 2^-36
    assert sum((I + 1) * (L + 1) for I, L in pm.COUNT_SHAPES) * 3 * 2.0 ** -37 < 1e-9
    em, colTok, pairs = pm.chain_case()
    dp = PairMergedProfileDP(em, colTok)
    for x, P in pairs:
        v, edges, _ = dp.viterbi(x, P)
        assert v > -math.inf and len(edges) == len(x) + len(P) + (len(x) + len(P) + 1) * (pm.CHAIN_S - 1)
    for name, (em, colTok, pairs) in list(pm.column_map_cases().items()) + list(pm.row_cases().items()):
        dp = PairMergedProfileDP(em, colTok)
        fin = [dp.forward(x, P)[0] > -math.inf for x, P in pairs]
        assert sum(fin) >= len(fin) - 1, name


def test_merged_seam_batch_is_live_but_at_the_seams():
    """seam_case of test_profile_pair_mixed_gpu.py: 129 pairs at shapes up to (3, 3) against two columns; the pairs at 63, 64 and
    128 -- the seams of the traceback's blocks of 64 lanes -- are dead and every other pair has a Viterbi path."""
    em, colTok, pairs = pm.seam_case()
    assert len(pairs) == pm.SEAM_PAIRS == 129 and pm.SEAM_DEAD == (63, 64, 128) and len(colTok) == 2 and em.nStates == 8
    assert max(max(len(x), len(P)) for x, P in pairs) <= 3
    dp = PairMergedProfileDP(em, colTok)
    for k, (x, P) in enumerate(pairs):
        v, edges, rows = dp.viterbi(x, P)
        assert (v == -math.inf) == (k in pm.SEAM_DEAD) and (len(edges) == 0) == (k in pm.SEAM_DEAD), k
