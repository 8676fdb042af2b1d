"""Two-profile sweeps against CTC-merged output profiles ("Pairs of profiles against a merged profile", docs/profile_tapes.md) without
a GPU: the numpy restatement (profile.TwoMergedProfileDP) against the oracle's exact Forward on
compose(A.machine(), compose(M, mergingRecogniserMachine())) with empty tapes, its Backward, the identities of its counts, its
reductions to MergedProfileDP, PairMergedProfileDP and TwoProfileDP, its tie order, boss.scoreTwoProfiles(merge=True) on the numpy
path, and the liveness of the GPU suite's inputs.

Bounds (twomergehelpers): log values 1e-9 relative to max(1, |value|), -inf exact; counts >= 1e-3 at 1e-6 relative, below
1e-9 + 1e-6 x count absolute; Viterbi scores 1e-12; paths equal."""
import math

import numpy as np
import pytest

import twomergehelpers as tm
import twoprofilehelpers as th
from prefixhelpers import machine_edges, machine_from_edges
from twoprofilehelpers import logs_close, pair_machine
from machineboss_amd import algebra, boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile, TwoMergedProfileDP, TwoProfileDP

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"


def composite_loglike(oracle_mod, em, colTok, A, B):
    """The oracle's exact Forward, with empty tapes, on compose(A.machine(), compose(M, mergingRecogniserMachine())), built as
    test_profile_two_host._composite_ll builds its own."""
    gen = th.profile_of(em.inputTokenizer.tok2sym[1:], A).machine()
    rec = tm.merged_profile_of(em, B, colTok).mergingRecogniserMachine()
    comp = algebra.compose(gen, algebra.compose(th.machine_of(em), rec, True, False), True, False)
    ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
    return oracle_mod.OracleMachine(ec).loglike([], [], oracle_mod.SUM_EXACT)


@pytest.fixture(scope="module")
def swept(oracle_mod):
    """Per case of the grid: the restatement's results and the oracle's likelihood of the composite, computed once."""
    out = {}
    for key, em, colTok, A, B in tm.host_cases():
        dp = TwoMergedProfileDP(em, colTok)
        ll, N, W, Z = dp.forward(A, B)
        blanks = []
        c, _ = dp.counts(A, B, blanks)
        out[key] = dict(em=em, A=A, B=B, dp=dp, ll=ll, Z=Z, counts=c, blanks=blanks[0] if blanks else (0.0, 0.0, 0.0),
                        exact=composite_loglike(oracle_mod, em, colTok, A, B))
    return out


def test_forward_equals_composition(swept):
    """The recurrence as written, over the 504 cases: plain machines and the end-loop variant, one, two and four columns (the random
    maps repeat tokens), with and without silent levels.  At least nine in ten likelihoods are finite."""
    assert len(swept) == 504
    worst = 0.0
    for key, c in swept.items():
        assert logs_close([c["ll"]], [c["exact"]]), (key, c["ll"], c["exact"])
        worst = max(worst, th.log_dev([c["ll"]], [c["exact"]]))
    fin = [c["exact"] > -math.inf for c in swept.values()]
    print("worst relative gap to the composite: %.3g over %d cases, %d finite" % (worst, len(swept), sum(fin)))
    assert np.mean(fin) >= 0.9, np.mean(fin)


def test_backward_equals_forward(swept):
    for key, c in swept.items():
        bl, NB, WB, ZB = c["dp"].backward(c["A"], c["B"])
        assert logs_close([bl], [c["ll"]]), (key, bl, c["ll"])
        if c["ll"] > -math.inf:      # the end cell splits the likelihood over its planes
            with np.errstate(invalid="ignore"):
                assert logs_close([float(np.logaddexp.reduce((c["Z"][-1, -1] + ZB[-1, -1]).ravel()))], [c["ll"]]), key


def test_counts_identities(swept):
    """Every output row is an emission, a blank or a repeat; every input row a read or a blank; the flow is conserved."""
    for key, c in swept.items():
        em, A, B = c["em"], c["A"], c["B"]
        if not c["ll"] > -math.inf:
            assert not c["counts"].any()
            continue
        net = np.zeros(em.nStates)
        np.add.at(net, em.dst.astype(np.int64), c["counts"]); np.subtract.at(net, em.src.astype(np.int64), c["counts"])
        want = np.zeros(em.nStates); want[-1] += 1.0; want[0] -= 1.0
        assert np.allclose(net, want, rtol=0, atol=1e-9), (key, net)
        outBlank, repeat, inBlank = c["blanks"]
        assert abs(c["counts"][em.outTok > 0].sum() + outBlank + repeat - len(B)) <= 1e-9 * max(1, len(B)), key
        assert abs(c["counts"][em.inTok > 0].sum() + inBlank - len(A)) <= 1e-9 * max(1, len(A)), key


def test_counts_equal_finite_differences():
    """d loglike / d log w_t is the count of t: central differences at h = 1e-6 (error about h^2 plus 1e-16 / h: 1e-9)."""
    em = pair_machine(5, 1, True, 2, 3)
    colTok = (2, 1, 2, 3)
    A, B = tm.merged_input(np.random.RandomState(5), em, 4, 3, 3, pInf=0.0)
    c, ll = TwoMergedProfileDP(em, colTok).counts(A, B)
    assert ll > -math.inf
    edges = machine_edges(em)
    h = 1e-6
    for t in range(em.nTransitions):
        up, dn = list(edges), list(edges)
        up[t] = edges[t][:4] + (edges[t][4] + h,); dn[t] = edges[t][:4] + (edges[t][4] - h,)
        d = (TwoMergedProfileDP(machine_from_edges(em.nStates, 2, 3, up), colTok).forward(A, B)[0] -
             TwoMergedProfileDP(machine_from_edges(em.nStates, 2, 3, dn), colTok).forward(A, B)[0]) / (2 * h)
        silentLoop = em.src[t] >= em.dst[t] and not em.inTok[t] and not em.outTok[t]
        assert abs(d - c[t]) <= 1e-7 * max(1.0, c[t]) and (c[t] == 0.0 or not silentLoop), (t, d, c[t])


def test_reductions():
    """K = 0 is MergedProfileDP; a one-hot A is PairMergedProfileDP on its tokens; one column per token with every B row one-hot on a
    run-free, blank-free string is TwoProfileDP on that string's plain rows."""
    for S, levels in ((5, True), (8, False)):
        em = pair_machine(S, 3, levels, 2, 3)
        rng = np.random.RandomState(S)
        colTok = (3, 1, 3, 2)
        B = tm.merged_rows(rng, 4, 4, zeros=0.1)
        two = TwoMergedProfileDP(em, colTok)
        ll, N, W, Z = two.forward(np.zeros((0, 3)), B)
        pl, PN, PW = MergedProfileDP(em, colTok).forward(B)
        assert pl > -math.inf and logs_close([ll], [pl]) and logs_close(N[0], PN) and logs_close(W[0], PW) and logs_close(Z[0], PW)
        assert two.forward(np.zeros((0, 3)), B, "max")[0] == MergedProfileDP(em, colTok).forward(B, "max")[0]
        x = rng.randint(1, 3, size=3)
        pair = PairMergedProfileDP(em, colTok)
        ll, N, W, Z = two.forward(th.one_hot(x, 2), B)
        ql, QN, QW = pair.forward(x, B)
        assert ql > -math.inf and logs_close([ll], [ql]) and logs_close(N, QN) and logs_close(W, QW) and logs_close(Z, QW)
        assert two.forward(th.one_hot(x, 2), B, "max")[0] == pair.forward(x, B, "max")[0]
        v, e, r, i = two.viterbi(th.one_hot(x, 2), B)
        pv, pe, pr = pair.viterbi(x, B)
        assert v == pv and np.array_equal(e, pe) and np.array_equal(r, pr)
        c, _ = two.counts(th.one_hot(x, 2), B)
        assert th.counts_close(c, pair.counts(x, B)[0])
        # distinct tokens, one-hot rows on a string without runs: no blank, no repeat, so the planes say nothing new
        y = np.array([1, 3, 1, 2, 3])
        hot = th.one_hot(y, 3)
        A = th.soft_profile(rng, 4, 2, 0.1)
        one = TwoMergedProfileDP(em, (1, 2, 3))
        ll, v = one.forward(A, hot)[0], one.forward(A, hot, "max")[0]
        tl, tv = TwoProfileDP(em).forward(A, hot)[0], TwoProfileDP(em).forward(A, hot, "max")[0]
        assert tl > -math.inf and logs_close([ll], [tl]) and logs_close([v], [tv], 1e-12)
        assert th.counts_close(one.counts(A, hot)[0], TwoProfileDP(em).counts(A, hot)[0])


def _walk_ok(em, edges, rows, ins):
    return (list(rows) == sorted(rows) and list(ins) == sorted(ins) and int(em.src[edges[0]]) == 0 and int(em.dst[edges[-1]]) == em.nStates - 1 and
            all(int(em.dst[a]) == int(em.src[b]) for a, b in zip(edges[:-1], edges[1:])))


def test_tie_census():
    """Every tie kind is met on the quantised machine, the first candidate wins, and every path rescored edge by edge (its blanks and
    repeats filled in) is the Viterbi score."""
    em = tm.tie_machine()
    dp = TwoMergedProfileDP(em, tm.TIE_COLTOK)
    census = {}
    for A, B in tm.tie_pairs():
        v, edges, rows, ins = dp.viterbi(A, B, census)
        # (the rescoring adds the same twenty-odd multiples of log 1/2 in another order: the Viterbi bound, 1e-12)
        assert v > -math.inf and abs(tm.rescore(em, A, B, tm.TIE_COLTOK, edges, rows, ins) - v) <= 1e-12 * max(1.0, abs(v))
        assert _walk_ok(em, edges, rows, ins)
    for kinds in tm.TIE_KINDS:
        first, second = kinds[0], kinds[-1]
        assert any(first in k and second in k and k.index(first) <= k.index(second) for k in census), (kinds, census)
    for em, colTok, A, B, edges, rows, ins in tm.hand_tie_cases():
        v, e, r, i = TwoMergedProfileDP(em, colTok).viterbi(A, B)
        assert v == 0.0 and list(e) == edges and list(r) == rows and list(i) == ins
    # random machines: paths rescore to the score and keep the bound
    n = 0
    for key, em, colTok, A, B in tm.host_cases():
        if key[2] == 0:
            dp = TwoMergedProfileDP(em, colTok)
            v, e, r, i = dp.viterbi(A, B)
            if v > -math.inf:
                assert abs(tm.rescore(em, A, B, colTok, e, r, i) - v) <= 1e-9 * max(1.0, abs(v)), key
                assert len(e) <= len(A) + len(B) + (len(A) + len(B) + 1) * len(dp.fLevels)
                n += 1
            else:
                assert len(e) == 0
    assert n >= 100
    em, colTok, pairs = tm.chain_case()
    for A, B in pairs:
        dp = TwoMergedProfileDP(em, colTok)
        v, e, r, i = dp.viterbi(A, B)
        assert v > -math.inf and len(e) == th.path_bound(len(dp.fLevels), len(A), len(B))


def _dnastore_inputs(tmp_path):
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    return m, par, em, Profile.fromCsv(str(a)), Profile.fromCsv(CSV)


def test_score_two_profiles_merge_numpy(tmp_path):
    m, par, em, pa, pb = _dnastore_inputs(tmp_path)
    short = Profile(pa.header, pa.row[:1])
    sc, pc = boss.scoreTwoProfiles(m, [pa, short], pb, backend="numpy", params=par, loglike=True, viterbi=True, counts=True, merge=True)
    B, colTok = pb.mergeRows(em)
    assert len(colTok) >= 1
    dp = TwoMergedProfileDP(em, colTok)
    for k, p in enumerate((pa, short)):
        assert sc["loglike"][k] == dp.forward(p.logRowsIn(em), B)[0] and sc["viterbi"][k] == dp.forward(p.logRowsIn(em), B, "max")[0]
    assert sc["loglike"][0] > -math.inf
    plain, _ = boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par)
    assert plain["loglike"][0] != sc["loglike"][0]            # (merge=False keeps the plain reading)
    assert pc == {}                                           # (dnastore4 has no parameters)
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par, merge=True, posteriors=True)
    with pytest.raises(MachineError, match="envelopes take plain profiles"):
        boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par, merge=True, band=2)


def test_gpu_inputs_are_live():
    """What test_profile_two_merge_gpu.py asserts of its inputs, held here without a GPU: finite shares, tie kinds, chunk counts and
    ring bytes."""
    # lanes: nine in ten likelihoods finite and more than half of the Forward cells alive, case by case
    for nCols, S in tm.LANE_CASES:
        colTok, cases = tm.lane_case(nCols, S)
        fwd = [TwoMergedProfileDP(em, colTok).forward(A, B) for em, A, B in cases]
        assert np.mean([f[0] > -math.inf for f in fwd]) >= 0.9, (nCols, S)
        assert sum(int(np.isfinite(f[3]).sum()) for f in fwd) > 0.5 * sum(f[3].size for f in fwd), (nCols, S)
    # ring marks: on both sides of 64 KiB and of 160 KiB, by i and by r
    by = [tm.ring_bytes(tm.RING_S, tm.RING_COLS, K, L) for K, L in tm.RING_SHAPES]
    assert by[:4] == [62400, 68640, 162240, 168480] and by[4:] == by[:4]
    assert by[0] <= 64 * 1024 < by[1] and by[2] <= tm.RING_LDS_MAX < by[3]
    assert all(tm.ring_bytes(tm.RING_S, tm.RING_COLS, K, L) <= 64 * 1024 for K, L in tm.MIXED_EXTRA)
    # packed: eighteen rings in scratch, six in LDS
    n = [tm.ring_bytes(tm.PACKED_S, 2, K, L) > tm.RING_LDS_MAX for K, L in tm.PACKED_SHAPES]
    assert sum(n) == 18 and len(n) == 24
    # counts past the LDS table
    em, _, _ = tm.big_counts_case()
    assert em.nTransitions > 8192
    # the tie batch meets every kind
    em = tm.tie_machine()
    census = {}
    for A, B in tm.tie_pairs():
        TwoMergedProfileDP(em, tm.TIE_COLTOK).viterbi(A, B, census)
    assert all(any(k[0] in c and k[-1] in c for c in census) for k in tm.TIE_KINDS), census
    # the budget of the chunked test: two of the largest count footprints; every ring of the materialised sweeps is in LDS
    sizes = [2 * tm.cell_bytes(tm.BUDGET_S, 3, K, L) for K, L in tm.BUDGET_SHAPES]
    assert len(th.lattice_chunks(sizes, 2 * max(sizes) + 4096)) >= 3
    assert all(tm.ring_bytes(tm.BUDGET_S, 3, K, L, mat=True) <= tm.RING_LDS_MAX for K, L in tm.BUDGET_SHAPES)
