"""CPU tests of CTC-merged profile tapes (machineboss_amd/profile.py: Profile.mergingMachine / mergeRows, MergedProfileDP): the numpy
restatement of the merged recurrence against compose(M, transpose(CSVProfile::mergingMachine())) scored by the oracle with empty
tapes, small cases by hand, counts against finite differences, the boundaries, and `boss --recognize-merge-csv` on the numpy path."""
import io
import json
import math

import numpy as np
import pytest

from conftest import golden_path, load_json
import mergehelpers as mh
from mergehelpers import merged_path_weight, random_merge_profile
from profhelpers import _machine_of
from randmachine import quantised_machine, random_machine
from machineboss_amd import algebra, boss, dp
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, Profile, ProfileDP

SEEDS = range(50)


def _case(seed):
    """The machines of test_restatement_equals_composition (seeds 0-29 random, 30-39 quantised weights, 40-49 with an input
    alphabet) against profiles whose header holds every output symbol, one of them twice, and a foreign symbol."""
    rng = np.random.RandomState(1000 + seed)
    S = int(rng.randint(1, 9))
    if seed < 30:
        em0 = random_machine(S, 0, int(rng.randint(1, 4)), 500 + seed)
    elif seed < 40:
        em0 = quantised_machine(S, 0, int(rng.randint(1, 4)), 500 + seed)
    else:
        em0 = random_machine(S, int(rng.randint(1, 4)), int(rng.randint(1, 4)), 500 + seed)
    M = _machine_of(em0)
    em = EvaluatedMachine.fromMachine(M, {}, useDefaults=True)
    prof = random_merge_profile(rng, em, int(rng.randint(0, 41)), quantised=30 <= seed < 40)
    return M, em, prof


@pytest.fixture(scope="module")
def composition(oracle_mod):
    """Per seed: (restatement Forward, Backward, Viterbi score, oracle exact, oracle Viterbi, plain ProfileDP Forward)."""
    out = {}
    for seed in SEEDS:
        M, em, prof = _case(seed)
        P, colTok = prof.mergeRows(em)
        mdp = MergedProfileDP(em, colTok)
        comp = algebra.compose(M, prof.mergingRecogniserMachine(), True, False)
        om = oracle_mod.OracleMachine(EvaluatedMachine.fromMachine(comp, {}, useDefaults=True))
        v, edges, rows = mdp.viterbi(P)
        out[seed] = dict(em=em, P=P, colTok=colTok, fwd=mdp.forward(P)[0], bwd=mdp.backward(P)[0], vit=v, edges=edges, rows=rows,
                         exact=om.loglike([], [], oracle_mod.SUM_EXACT), ovit=float(om.viterbi([], [])[-1, -1, -1]),
                         plain=ProfileDP(em).forward(prof.logRows(em))[0])
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_composition(composition, seed):
    c = composition[seed]
    exact, vit = c["exact"], c["ovit"]
    if exact == -math.inf:
        assert c["fwd"] == -math.inf and c["bwd"] == -math.inf
    else:
        assert abs(c["fwd"] - exact) <= 1e-9 * max(1.0, abs(exact)), (c["fwd"], exact)
        assert abs(c["bwd"] - exact) <= 1e-9 * max(1.0, abs(exact)), (c["bwd"], exact)
    v = c["vit"]
    assert (v == -math.inf and vit == -math.inf) or abs(v - vit) <= 1e-12 * max(1.0, abs(vit)), (v, vit)
    if v > -math.inf:     # the path's weight, with its blank and repeat rows filled in the best way, is the score
        em, edges, rows = c["em"], c["edges"], c["rows"]
        w = merged_path_weight(em, c["P"], c["colTok"], edges, rows)
        assert abs(w - v) <= 1e-9 * max(1.0, abs(v)), (w, v)
        emitted = [r for e, r in zip(edges, rows) if em.outTok[e]]
        assert list(rows) == sorted(rows) and len(emitted) == len(set(emitted))
        assert all(em.inTok[e] == 0 for e in edges)
        assert int(em.src[edges[0]]) == 0 if len(edges) else True
    else:
        assert len(c["edges"]) == 0


def test_finite_cases(composition):
    """The cases are no row of -inf = -inf: at least half are finite, and at least a quarter of those differ from the plain sweep."""
    fin = [c for c in composition.values() if c["exact"] > -math.inf]
    differ = [c for c in fin if not abs(c["fwd"] - c["plain"]) <= 1e-9 * max(1.0, abs(c["fwd"]))]
    print("finite %d/%d, differ from the plain sweep %d/%d" % (len(fin), len(composition), len(differ), len(fin)))
    assert 2 * len(fin) >= len(composition), (len(fin), len(composition))
    assert 4 * len(differ) >= len(fin), (len(differ), len(fin))


# ---- by hand -----------------------------------------------------------------------------------------------------------------------
def _by_hand(seq, rows):
    em = EvaluatedMachine.fromMachine(algebra.generator(list(seq), "g"), {}, useDefaults=True)
    prof = Profile(["A"], rows)
    P, colTok = prof.mergeRows(em)
    return math.exp(MergedProfileDP(em, colTok).forward(P)[0]), math.exp(ProfileDP(em).forward(prof.logRows(em))[0])


def test_by_hand():
    a1, b1, a2, b2, a3, b3 = .3, .7, .6, .4, .2, .8
    merged, plain = _by_hand("A", [[a1, b1], [a2, b2]])
    assert merged == pytest.approx(a1 * a2 + a1 * b2 + b1 * a2, rel=1e-12) and plain == pytest.approx(a1 * b2 + b1 * a2, rel=1e-12)
    merged, plain = _by_hand("AA", [[a1, b1], [a2, b2]])
    assert merged == 0.0 and plain == pytest.approx(a1 * a2, rel=1e-12)
    merged, _ = _by_hand("AA", [[a1, b1], [a2, b2], [a3, b3]])
    assert merged == pytest.approx(a1 * b2 * a3, rel=1e-12)


# ---- counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_counts_are_forward_derivatives(seed):
    rng = np.random.RandomState(77 + seed)
    em = random_machine(int(rng.randint(2, 7)), 0, 2, 900 + seed)
    P, colTok = random_merge_profile(rng, em, int(rng.randint(1, 12))).mergeRows(em)
    c, ll = MergedProfileDP(em, colTok).counts(P)
    if ll == -math.inf:
        assert not c.any()
        return
    h = 1e-5
    for t in range(em.nTransitions):
        if em.inTok[t] or em.logWeight[t] == -math.inf:
            continue
        lw = em.logWeight.copy(); lw[t] += h
        up = MergedProfileDP(em.withLogWeights(lw), colTok).forward(P)[0]
        lw[t] -= 2 * h
        dn = MergedProfileDP(em.withLogWeights(lw), colTok).forward(P)[0]
        assert abs((up - dn) / (2 * h) - c[t]) <= 1e-6 + 1e-5 * abs(c[t]), (t, (up - dn) / (2 * h), c[t])


def test_counts_with_input_alphabet_are_zero_on_input_edges():
    em = random_machine(6, 2, 2, 45)
    rng = np.random.RandomState(3)
    P, colTok = random_merge_profile(rng, em, 6).mergeRows(em)
    c, _ = MergedProfileDP(em, colTok).counts(P)
    assert np.all(c[np.asarray(em.inTok) != 0] == 0.0)


# ---- boundaries --------------------------------------------------------------------------------------------------------------------
def test_no_rows_and_one_row():
    em = EvaluatedMachine.fromMachine(algebra.generator(["A"], "g"), {}, useDefaults=True)
    P, colTok = Profile(["A"], []).mergeRows(em)
    assert P.shape == (0, 2) and list(colTok) == [1]
    mdp = MergedProfileDP(em, colTok)
    assert mdp.forward(P)[0] == -math.inf and mdp.backward(P)[0] == -math.inf      # "A" cannot be emitted against no rows
    em0 = EvaluatedMachine.fromMachine(algebra.generator([], "g"), {}, useDefaults=True)
    assert MergedProfileDP(em0, []).forward(np.zeros((0, 1)))[0] == 0.0
    P, colTok = Profile(["A"], [[.25, .5]]).mergeRows(em)
    assert MergedProfileDP(em, colTok).forward(P)[0] == pytest.approx(math.log(.25), rel=1e-12)
    v, edges, rows = MergedProfileDP(em, colTok).viterbi(P)
    assert v == pytest.approx(math.log(.25), rel=1e-12) and len(edges) == 1 and list(rows) == [0]


def test_merge_rows_short_rows_duplicates_and_foreign():
    em = EvaluatedMachine.fromMachine(algebra.generator(["a", "c"], "g"), {}, useDefaults=True)      # tokens: 1 = a, 2 = c
    P, colTok = Profile(["x", "a", "c", "a"], [[.5, .25, .125, .0625, .03125, 9], [.5, .25], [.5, .25, .125, .0625]]).mergeRows(em)
    assert list(colTok) == [1, 2, 1]                        # header order; "x" dropped; "a" twice is two columns
    assert P.shape == (3, 4)
    assert list(P[0]) == [math.log(.03125), math.log(.25), math.log(.125), math.log(.0625)]      # column 4 = the blank, 5 ignored
    assert list(P[1]) == [-math.inf, math.log(.25), -math.inf, -math.inf]                          # short row, no blank
    assert list(P[2]) == [-math.inf, math.log(.25), math.log(.125), math.log(.0625)]               # all symbols, no blank
    with pytest.raises(MachineError):
        Profile(["a"], [[-1.0]]).mergeRows(em)


def test_empty_header_is_an_error():
    em = EvaluatedMachine.fromMachine(algebra.generator(["a"], "g"), {}, useDefaults=True)
    p = Profile([], [[1.0]])
    for f in (p.mergingMachine, p.mergingRecogniserMachine, lambda: p.mergeRows(em)):
        with pytest.raises(MachineError, match="Need header"):
            f()
    with pytest.raises(MachineError, match="outside"):
        MergedProfileDP(em, [2])


@pytest.mark.parametrize("L", [1, 2, 5])
def test_recogniser_state_count_and_shape(L):
    hdr = ["A", "C", "A"]
    p = Profile(hdr, [[.1, .2, .3, .4]] * L)
    r = p.mergingRecogniserMachine()
    assert len(r.state) == (L - 1) * (len(hdr) + 1) + 2
    assert r.inputAlphabet() == ["A", "C"] and not r.outputAlphabet()
    assert [t.inp for t in r.state[0].trans] == ["A", "C", "A", ""]
    if L > 1:          # from "row 0 took column 0": the repeat is silent, the second A column is not
        assert [t.inp for t in r.state[1].trans] == ["", "C", "A", ""]
    assert len(Profile(hdr, []).mergingMachine().state) == 1


# ---- command line (numpy path) -----------------------------------------------------------------------------------------------------
CSV = "tests/golden/csv/tiny_uc.csv"
LOOP = {"state": [{"id": "S", "trans": [{"out": s, "to": "S", "weight": "p" + s} for s in "ACGT"] + [{"to": "E", "weight": "pE"}]},
                  {"id": "E", "trans": []}]}
LOOP_PARAMS = {"pA": .4, "pC": .1, "pG": .2, "pT": .1, "pE": .2}


def _run(*args):
    out = io.StringIO()
    assert boss.run(list(args) + ["--decode-backend", "numpy"], out) == 0
    return out.getvalue()


def test_cli_scores_equal_composed_route(oracle_mod, tmp_path):
    (tmp_path / "loop.json").write_text(json.dumps(LOOP))
    (tmp_path / "par.json").write_text(json.dumps(LOOP_PARAMS))
    base = [str(tmp_path / "loop.json"), "-P", str(tmp_path / "par.json"), "--recognize-merge-csv", CSV]
    M = Machine.fromFile(str(tmp_path / "loop.json"))
    prof = Profile.fromCsv(golden_path("csv", "tiny_uc.csv"))
    comp = algebra.compose(M, prof.mergingRecogniserMachine(), True, False)
    ec = EvaluatedMachine.fromMachine(comp, LOOP_PARAMS)
    om = oracle_mod.OracleMachine(ec)
    ll = om.loglike([], [], oracle_mod.SUM_EXACT)
    assert ll > -math.inf
    got = json.loads(_run(*base, "-L"))
    assert got[0][:2] == ["", ""] and abs(got[0][2] - ll) <= 1e-5 * abs(ll)
    got = json.loads(_run(*base, "-V"))
    vit = float(om.viterbi([], [])[-1, -1, -1])
    assert abs(got[0][2] - vit) <= 1e-5 * abs(vit)
    counts = dp.MachineCounts(ec)
    om.counts_add([], [], counts._flat, oracle_mod.SUM_EXACT)
    want = counts.paramCounts(comp, LOOP_PARAMS)
    got = json.loads(_run(*base, "-C"))
    assert got.keys() == want.keys() and all(abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])) for k in want), (got, want)
    # -L and -V in one run print both lines
    assert len(_run(*base, "-L", "-V").splitlines()) == 2


def test_cli_viterbi_decode(oracle_mod):
    """--viterbi-decode: the printed input is decodePath of the restatement's merged Viterbi path of the input-silenced machine,
    whose score is the Viterbi score of the composed route."""
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    par = m.getParamDefs(True)
    prof = Profile.fromCsv(golden_path("csv", "tiny_uc.csv"))
    got = json.loads(_run(golden_path("machine", "dnastore4.json"), "--use-defaults", "--recognize-merge-csv", CSV, "--viterbi-decode"))
    silent = algebra.silenceInput(m)
    ev = EvaluatedMachine.fromMachine(silent, par)
    P, colTok = prof.mergeRows(ev)
    v, edges, _ = MergedProfileDP(ev, colTok).viterbi(P)
    comp = algebra.compose(silent, prof.mergingRecogniserMachine(), True, False)
    vit = float(oracle_mod.OracleMachine(EvaluatedMachine.fromMachine(comp, par)).viterbi([], [])[-1, -1, -1])
    assert v > -math.inf and abs(v - vit) <= 1e-12 * max(1.0, abs(vit))
    assert got == [{"input": {"name": "input", "sequence": algebra.decodePath(dp.edgesToPath(ev, silent, edges), m, par)},
                    "output": {"name": "", "sequence": []}}]
    assert boss.viterbiDecodeProfile(m, prof, "numpy", par, merge=True) == got[0]["input"]["sequence"]


def test_cli_rejections():
    base = ["--generate-json", "tests/golden/io/tiny_uc.json", "--decode-backend", "numpy"]
    with pytest.raises(MachineError, match="cannot be combined"):
        boss.run(base + ["--recognize-merge-csv", CSV, "--recognize-csv", CSV, "-L"], io.StringIO())
    with pytest.raises(MachineError, match="cannot be prefix-decoded"):
        boss.run(["tests/golden/machine/dnastore4.json", "--use-defaults", "--recognize-merge-csv", CSV, "--prefix-decode"], io.StringIO())
    with pytest.raises(MachineError, match="empty input alphabet"):
        boss.run(["tests/golden/machine/dnastore4.json", "--use-defaults", "--recognize-merge-csv", CSV, "-L", "--decode-backend", "numpy"], io.StringIO())
    with pytest.raises(MachineError, match="needs -L, -V or -C"):
        boss.run(base + ["--recognize-merge-csv", CSV], io.StringIO())
    with pytest.raises(MachineError, match="no other sequence data"):
        boss.run(base + ["--recognize-merge-csv", CSV, "-L", "--output-chars", "A"], io.StringIO())


# ---- the inputs of the GPU edge suite ------------------------------------------------------------------------------------------------
def _finite(em, colTok, profs):
    mdp = MergedProfileDP(em, colTok)
    return np.array([mdp.forward(P)[0] > -math.inf for P in profs])


def test_edge_suite_inputs_are_live():
    """test_profile_merge_edges_gpu.py asserts, from the restatement, that its inputs score finite, tie and split into chunks as its
    cases need; the same builders of mergehelpers.py are held to the same conditions here, so the seeds are verified without a GPU.
    (Backward and counts from 1 024 planes on are computed by the restatement nowhere.)"""
    for nCols, S in mh.LANE_CASES:
        em, colTok, profs = mh.lane_case(nCols, S)
        assert len(colTok) == nCols and em.nStates == S and 1 <= min(colTok) and max(colTok) <= 3
        assert max(len(P) for P in profs) <= (23 if nCols + 1 <= 66 else 3)
        assert int(em.silentLevels().max(initial=0)) + 1 <= 16
        assert _finite(em, colTok, profs).sum() >= 3, (nCols, S)
    assert max(nc + 1 for nc, _ in mh.LANE_CASES) > mh.PM_THREADS
    for S in mh.LDS_CASES:
        em, colTok, profs = mh.lds_case(S)
        assert 1 < int(em.silentLevels().max(initial=0)) + 1 <= 16
        assert _finite(em, colTok, profs).sum() >= 2, S
    for nIn, nOut in mh.ALPHABET_CASES:
        em, colTok, profs = mh.alphabet_case(nIn, nOut)
        assert np.sum(em.inTok != 0) >= 10 and np.sum((em.inTok != 0) & (em.outTok != 0)) >= 1
        assert _finite(em, colTok, profs).sum() >= 3, (nIn, nOut)
        em, colTok, hot, seqs = mh.alphabet_one_hot_case(nIn, nOut)
        f = _finite(em, colTok, hot)
        assert f[:6].sum() >= 4 and f[6:].all(), (nIn, nOut, f)
        mdp = MergedProfileDP(em, colTok)
        assert mdp.forward(hot[-3])[0] == pytest.approx(mdp.forward(hot[-2])[0], rel=1e-12) != pytest.approx(mdp.forward(hot[-1])[0], rel=1e-6)
    for name, (em, colTok, profs) in mh.column_map_cases().items():
        assert _finite(em, colTok, profs).sum() >= 3, name
    for name, (em, colTok, profs) in mh.degenerate_cases().items():
        f = _finite(em, colTok, profs)
        assert f.sum() >= (2 if name == "noblank" else 3), (name, f)
        assert name != "infrow" or (not f[1] and not f[4])
    em, colTok, P = mh.all_blank_case()
    assert MergedProfileDP(em, colTok).forward(np.zeros((0, len(colTok) + 1)))[0] > -math.inf
    # ties: every kind at least 5 times (the counts in the GPU test's docstring)
    tot = {}
    for em, colTok, profs in mh.tie_cases():
        assert len(profs) > 64
        mdp = MergedProfileDP(em, colTok)
        for P in profs:
            mdp.viterbi(P, tot)
    assert all(tot.get(kind, 0) >= 5 for kind in mh.TIE_KINDS), tot
    print("tie census", tot)
    # batches: at least half finite and some -inf (Viterbi is finite where Forward is), and a budget that cuts >= 3 unequal chunks
    for S, n, maxL in mh.BATCH_CASES:
        em, colTok, profs = mh.batch_case(S, n, maxL)
        levels = int(em.silentLevels().max(initial=0)) + 1
        assert levels <= 16
        mdp = MergedProfileDP(em, colTok)
        fin = np.array([mdp.forward(P, "max")[0] > -math.inf for P in profs])
        assert fin.sum() >= n // 2 and not fin.all()
        cb, vb = mh.batch_bytes(em, 4, profs, levels)
        budget = int(sum(cb) / 3.5)
        assert budget >= max(cb) * 1.2 and budget >= max(vb) * 1.2
        for b in (cb, vb):
            chunks = mh.greedy_chunks(b, budget)
            assert len(chunks) >= 3 and len({p1 - p0 for p0, p1 in chunks}) >= 2, chunks
    # long profiles: the 300-row cuts of the derivative check and the shortest whole profile score finite
    for with_input in (False, True):
        em, colTok, profs = mh.long_case(with_input)
        assert (np.sum(em.inTok != 0) > 0) == with_input and int(em.silentLevels().max(initial=0)) + 1 <= 16
        assert _finite(em, colTok, [P[:300] for P in profs] + profs[:1]).all()
    em, colTok, P = mh.long_restatement_case()
    assert _finite(em, colTok, [P]).all()
    for which in ("generator", "random"):
        for zeros in (False, True):
            M, em, prof = mh.composed_case(which, zeros)
            P, colTok = prof.mergeRows(em)
            assert len(set(colTok)) < len(colTok) and (P == -math.inf).any() == zeros
            assert _finite(em, colTok, [P]).all(), (which, zeros)
