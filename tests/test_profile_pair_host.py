"""CPU tests of the two-tape profile sweeps (machineboss_amd/profile.py: PairProfileDP): the numpy restatement against the oracle's
two-tape DP on compose(M, profile recogniser) with (x, empty output), against ProfilePrefixDP chained along x, its identities,
its tie order, `boss --recognize-csv` beside input data on the numpy path, and the liveness of the GPU suite's inputs.

The machines are pairprofilehelpers.pair_machine: populated_machine plus edges between the start and the end state (see there --
without them the small shapes cannot reach the end state of a machine without levels, and nine in ten likelihoods could not be finite)."""
import io
import json
import math

import numpy as np
import pytest

import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close, pair_input, pair_machine
from profileprefixhelpers import composite_machine, random_profile
from randmachine import random_machine
from machineboss_amd import algebra, boss, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError, MachineState, MachineTransition
from machineboss_amd.profile import PairProfileDP, Profile, ProfileDP

SEEDS = range(8)
SHAPES = [(I, L) for I in (0, 1, 2, 4) for L in (0, 1, 2, 6)]
MACHINES = [(S, lv) for S in (5, 8) for lv in (True, False)]
CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"


def _machine_of(em):
    m = Machine()
    for _ in range(em.nStates):
        m.state.append(MachineState())
    isym, osym = em.inputTokenizer.tok2sym, em.outputTokenizer.tok2sym
    for e in range(em.nTransitions):
        m.state[int(em.src[e])].trans.append(MachineTransition(dest=int(em.dst[e]), inp=isym[em.inTok[e]] if em.inTok[e] else "",
                                                                out=osym[em.outTok[e]] if em.outTok[e] else "",
                                                                weight=float(np.exp(em.logWeight[e]))))
    return m


def _profile_of(em, P):
    """The Profile whose logRows(em) is P: header = the output symbols, the blank last."""
    return Profile(list(em.outputTokenizer.tok2sym[1:]), [list(np.exp(row[1:])) + [float(np.exp(row[0]))] for row in P])


def _cases():
    for S, lv in MACHINES:
        for seed in SEEDS:
            em = pair_machine(S, seed, lv, 2, 3)
            for I, L in SHAPES:
                yield (S, lv, seed, I, L), em, pair_input(np.random.RandomState(97 * seed + 10 * I + L), em, I, L)


@pytest.fixture(scope="module")
def swept(oracle_mod):
    """Per case: the restatement's results and the oracle's on the composite, computed once."""
    out = {}
    dps = {}
    for key, em, (x, P) in _cases():
        dp = dps.setdefault(key[:3], PairProfileDP(em))
        ll, N, W = dp.forward(x, P)
        blanks = []
        c, _ = dp.counts(x, P, blanks)
        C, origin = composite_machine(em, P, origins=True)
        om = oracle_mod.OracleMachine(C)
        oc = np.zeros(C.nTransitions)
        if ll > -math.inf:
            om.counts_add(x, [], oc, oracle_mod.SUM_EXACT)
        want = np.zeros(em.nTransitions)
        np.add.at(want, origin[origin >= 0], oc[origin >= 0])
        out[key] = dict(em=em, x=x, P=P, dp=dp, ll=ll, N=N, W=W, counts=c, blank=blanks[0] if blanks else 0.0,
                        exact=om.loglike(x, [], oracle_mod.SUM_EXACT), ovit=float(om.viterbi(x, [])[-1, -1, -1]), ocounts=want)
    return out


def test_nine_in_ten_likelihoods_are_finite(swept):
    fin = [c["exact"] > -math.inf for c in swept.values()]
    assert len(fin) == len(MACHINES) * len(SEEDS) * len(SHAPES) and np.mean(fin) >= 0.9, np.mean(fin)


def test_forward_equals_composition(oracle_mod, swept):
    """Forward against the oracle's two-tape Forward on algebra.compose(M, recogniser) with (x, empty output); the same number from
    the composite built directly (profileprefixhelpers.composite_machine), which the counts and Viterbi cases use."""
    for key, c in swept.items():
        assert logs_close([c["ll"]], [c["exact"]]), (key, c["ll"], c["exact"])
    for key in [k for k in swept if k[2] < 2]:          # the algebra route, which builds a Machine per case: two seeds of each
        c = swept[key]
        em, x, P = c["em"], c["x"], c["P"]
        comp = algebra.compose(_machine_of(em), _profile_of(em, P).recogniserMachine(), True, False)
        ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
        syms = [em.inputTokenizer.tok2sym[t] for t in x]
        got = -math.inf
        if ec.inputTokenizer.canTokenize(syms):
            got = oracle_mod.OracleMachine(ec).loglike(ec.inputTokenizer.tokenize(syms), [], oracle_mod.SUM_EXACT)
        assert logs_close([c["ll"]], [got]), (key, c["ll"], got)


def test_w_layer_equals_chained_prefix_fills(swept):
    for key, c in swept.items():
        em, x, P = c["em"], c["x"], c["P"]
        pdp = prefixtree.ProfilePrefixDP(em, np.full((em.nStates, em.nStates), -np.inf))
        cells, sp, _ = pdp.fill(P)
        assert logs_close(c["W"][0], cells[:, 0]), key
        for i, a in enumerate(x):
            cells, sp, _ = pdp.fill(P, cells, int(a))
            assert logs_close(c["W"][i + 1], cells[:, 0]), (key, i)
        assert logs_close([c["ll"]], [sp]), key


def test_viterbi_equals_composition(swept):
    for key, c in swept.items():
        v, edges, rows = c["dp"].viterbi(c["x"], c["P"])
        vit = c["ovit"]
        assert (v == -math.inf and vit == -math.inf) or abs(v - vit) <= 1e-12 * max(1.0, abs(vit)), (key, v, vit)
        if v > -math.inf:
            em, x = c["em"], c["x"]
            assert [int(em.inTok[e]) for e in edges if em.inTok[e]] == list(x), key
            assert len(edges) == 0 or (int(em.src[edges[0]]) == 0 and int(em.dst[edges[-1]]) == em.nStates - 1)
            assert all(int(em.dst[a]) == int(em.src[b]) for a, b in zip(edges[:-1], edges[1:]))
            assert list(rows) == sorted(rows)
            # the path's weight, its blank rows filled in, is the score
            used = {int(r) for e, r in zip(edges, rows) if em.outTok[e]}
            w = sum(em.logWeight[e] for e in edges) + sum(c["P"][r][em.outTok[e]] for e, r in zip(edges, rows) if em.outTok[e]) + \
                sum(c["P"][r][0] for r in range(len(c["P"])) if r not in used)
            assert abs(w - v) <= 1e-9 * max(1.0, abs(v)), (key, w, v)
        else:
            assert len(edges) == 0


def test_counts_equal_composition(swept):
    for key, c in swept.items():
        assert counts_close(c["counts"], c["ocounts"]), (key, np.abs(c["counts"] - c["ocounts"]).max())


def test_identities(swept):
    for key, c in swept.items():
        em, x, P, dp = c["em"], c["x"], c["P"], c["dp"]
        bl, NB, WB = dp.backward(x, P)
        assert logs_close([bl], [c["ll"]]), (key, bl, c["ll"])
        if not c["ll"] > -math.inf:
            assert not c["counts"].any()
            continue
        # flow: a path enters and leaves every inner state equally often, leaves the start once more and enters the end once more
        net = np.zeros(em.nStates)
        np.add.at(net, em.dst.astype(np.int64), c["counts"]); np.subtract.at(net, em.src.astype(np.int64), c["counts"])
        want = np.zeros(em.nStates); want[-1] += 1.0; want[0] -= 1.0
        assert np.allclose(net, want, rtol=0, atol=1e-9), (key, net)
        # every row is consumed once: by an emitting edge or by a blank
        assert abs(c["counts"][em.outTok > 0].sum() + c["blank"] - len(P)) <= 1e-9 * max(1, len(P)), key
        # and every input symbol once
        assert abs(c["counts"][em.inTok > 0].sum() - len(x)) <= 1e-9 * max(1, len(x)), key


@pytest.mark.parametrize("seed", range(8))
def test_no_input_equals_profile_dp(seed):
    em = random_machine(6, 0, 3, 300 + seed)
    P = random_profile(np.random.RandomState(seed), 7, 3)
    a, b = PairProfileDP(em), ProfileDP(em)
    la, Na, Wa = a.forward([], P); lb, Nb, Wb = b.forward(P)
    assert logs_close([la], [lb], 1e-12) and logs_close(Na[0], Nb, 1e-12) and logs_close(Wa[0], Wb, 1e-12)
    ca, cb = a.counts([], P)[0], b.counts(P)[0]
    assert np.allclose(ca, cb, rtol=1e-12, atol=1e-15)
    va, ea, ra = a.viterbi([], P); vb, eb, rb = b.viterbi(P)
    assert logs_close([va], [vb], 1e-12) and np.array_equal(ea, eb) and np.array_equal(ra, rb)


HALF = ph.HALF
_tie_machine = ph.tie_machine          # (the GPU edge suite runs the same machine on the device)


def test_tie_census():
    """On a machine whose weights are multiples of log 0.5, against a one-hot profile (one symbol; its blank of weight 1 too, or no
    blank could tie), every kind of tie fires, and at each the candidate taken is the first in the documented order -- N: blank,
    match, output-only; W: no move, input-only, silent."""
    em = _tie_machine()
    dp = PairProfileDP(em)
    census = {}
    order = {"blank": 0, "match": 1, "emit": 2, "stay": 0, "ins": 1, "silent": 2}
    for I in range(1, 5):
        for L in range(1, 5):
            x, P = np.ones(I, np.int32), np.zeros((L, 2))
            v, edges, rows = dp.viterbi(x, P, census)
            assert v > -math.inf and v == 2 * HALF, (I, L, v)
            assert sum(em.logWeight[e] for e in edges) == v          # every profile weight is 1
    pairs = {(a, b) for kinds in census for a in kinds for b in kinds if a != b}
    for a, b in (("blank", "match"), ("match", "emit"), ("stay", "ins"), ("ins", "silent")):
        assert (a, b) in pairs, (a, b, census)
    for kinds in census:
        assert list(kinds) == sorted(kinds, key=order.get), kinds       # the taken candidate, kinds[0], is the first in the order
    # by hand: 0 -> 0 and 0 -> 1 reading a, 0 -> 1 silent, all of weight 1, on x = a without rows.  W[1][0][1] is attained by the
    # input-only edge from W[0][0][0] and by the silent edge from W[1][0][0]: input-only is listed first, so the path is that one
    # edge, not the loop and then the silent edge.  With a row of blank 1 and symbol 1 and 0 -> 1 also as a match and as an
    # output-only edge: N[1][1][1] is attained by the match from W[0][0][0] and by the output-only edge from W[1][0][0]: the match.
    from prefixhelpers import machine_from_edges
    em2 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 0, 0.0), (0, 1, 0, 0, 0.0)])
    v, edges, rows = PairProfileDP(em2).viterbi([1], np.zeros((0, 2)))
    assert v == 0.0 and [(int(em2.src[e]), int(em2.dst[e]), int(em2.inTok[e])) for e in edges] == [(0, 1, 1)] and list(rows) == [0]
    em3 = machine_from_edges(2, 1, 1, [(0, 0, 1, 0, 0.0), (0, 1, 1, 1, 0.0), (0, 1, 0, 1, 0.0)])
    v, edges, rows = PairProfileDP(em3).viterbi([1], np.zeros((1, 2)))
    assert v == 0.0 and [(int(em3.inTok[e]), int(em3.outTok[e])) for e in edges] == [(1, 1)] and list(rows) == [0]


def _run(*args):
    out = io.StringIO()
    assert boss.run(list(args) + ["--decode-backend", "numpy"], out) == 0
    return out.getvalue()


def test_cli_equals_restatement(tmp_path):
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(CSV)
    P = prof.logRows(em)
    dp = PairProfileDP(em)
    (tmp_path / "x.json").write_text(json.dumps({"name": "x1", "sequence": ["0_3", "2_3", "1_3"]}))
    (tmp_path / "x.fa").write_text(">f1\n\n")
    x1 = em.inputTokenizer.tokenize(["0_3", "2_3", "1_3"])
    base = [DNASTORE, "--use-defaults", "--recognize-csv", CSV]
    # --input-chars on dnastore4, whose input symbols have three characters each: the empty string is the one sequence it can
    # spell (I = 0), anything else cannot be tokenised and scores -inf like a pair of the --loglike loop
    for flag, mode in (("-L", "exact"), ("-V", "max")):
        got = json.loads(_run(*base, "--input-chars", "", flag))
        want = dp.forward([], P, mode)[0]
        assert got[0][:2] == ["", ""] and want > -math.inf and abs(got[0][2] - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
        assert json.loads(_run(*base, "--input-chars", "012", flag)) == [["012", "", "-Infinity"]]
        got = json.loads(_run(*base, "--input-json", str(tmp_path / "x.json"), "--input-chars", "", flag))
        w1 = dp.forward(x1, P, mode)[0]
        assert [g[:2] for g in got] == [["", ""], ["x1", ""]] and w1 > -math.inf
        assert abs(got[1][2] - w1) <= 1e-5 * max(1.0, abs(w1)) and abs(got[0][2] - want) <= 1e-5 * max(1.0, abs(want))
    assert json.loads(_run(*base, "--input-chars", "", "-C")) == {}          # (dnastore4 has no parameters)
    # a machine with parameters and one-character input symbols: bitnoise
    bit = ["tests/golden/machine/bitnoise.json", "-P", "tests/golden/io/params.json", "--recognize-csv", "tests/golden/csv/prof001.csv"]
    mb = Machine.fromFile(bit[0])
    pb = json.load(open(bit[2]))
    eb = EvaluatedMachine.fromMachine(mb, pb)
    Pb = Profile.fromCsv(bit[4]).logRows(eb)
    db = PairProfileDP(eb)
    from machineboss_amd import dp as dpmod
    for x in ("101", "0"):
        xt = eb.inputTokenizer.tokenize(list(x))
        for flag, mode in (("-L", "exact"), ("-V", "max")):
            got = json.loads(_run(*bit, "--input-chars", x, flag))
            want = db.forward(xt, Pb, mode)[0]
            assert got[0][:2] == [x, ""] and (got[0][2] == "-Infinity" if want == -math.inf else abs(got[0][2] - want) <= 1e-5 * max(1.0, abs(want)))
    counts = dpmod.MachineCounts(eb)
    for x in ("101", "001"):
        counts._flat += db.counts(eb.inputTokenizer.tokenize(list(x)), Pb)[0]
    want = counts.paramCounts(mb, pb)
    (tmp_path / "two.fa").write_text(">a\n101\n>b\n001\n")
    got = json.loads(_run(*bit, "--input-fasta", str(tmp_path / "two.fa"), "-C"))
    assert got.keys() == want.keys() and all(abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])) for k in want), (got, want)
    assert len(_run(*bit, "--input-chars", "101", "-L", "-V").splitlines()) == 2


def test_cli_rejections():
    base = [DNASTORE, "--use-defaults", "--recognize-csv", CSV, "--decode-backend", "numpy"]

    def fails(args, msg):
        with pytest.raises(MachineError, match=msg):
            boss.run(args, io.StringIO())
    for flag in ("-L", "-V", "-C"):
        fails(base + [flag], "needs a machine with an empty input alphabet")
    for extra in (["--output-chars", "A"], ["-D", "tests/golden/io/seqpairlist.json"], ["--recognize-chars", "A"]):
        fails(base + ["-L", "--input-chars", ""] + extra, "takes no other sequence data")
        fails(base + ["-L"] + extra, "takes no other sequence data")
    for flag in ("--prefix-decode", "--viterbi-decode"):
        fails(base + [flag, "--input-chars", ""], "takes no other sequence data")
    fails([DNASTORE, "--use-defaults", "--recognize-merge-csv", CSV, "-L", "--input-chars", "", "--decode-backend", "numpy"],
          "two-tape sweeps take plain profiles")
    for flag in ("-A", "-T"):
        fails(base + [flag, "--input-chars", ""], "supports -L, -V and -C")
    fails(base + ["--input-chars", ""], "needs -L, -V or -C")
    # input data for a machine without an input alphabet is still "other sequence data"
    fails(["--generate-json", "tests/golden/io/tiny_uc.json", "--recognize-csv", CSV, "-L", "--input-chars", "A", "--decode-backend", "numpy"],
          "takes no other sequence data")
    dp = PairProfileDP(pair_machine(5, 0, True, 2, 3))
    with pytest.raises(MachineError, match="outside 1..nInTok"):
        dp.forward([3], np.zeros((1, 4)))
    with pytest.raises(MachineError, match="outside 1..nInTok"):
        dp.forward([0], np.zeros((1, 4)))
    with pytest.raises(MachineError, match="NaN"):
        dp.forward([1], np.full((1, 4), np.nan))


# ---- the inputs of the GPU suite ------------------------------------------------------------------------------------------------
def _live(cases):
    """(fraction of finite likelihoods, fraction of finite cells) of [(em, x, P)] under the restatement."""
    lls, fin, tot = [], 0, 0
    dps = {}
    for em, x, P in cases:
        ll, N, W = dps.setdefault(id(em), PairProfileDP(em)).forward(x, P)
        lls.append(ll > -math.inf)
        fin += int(np.isfinite(N).sum() + np.isfinite(W).sum()); tot += N.size + W.size
    return float(np.mean(lls)), fin / tot


def test_pair_suite_inputs_are_live():
    """test_profile_pair_gpu.py asserts, from the restatement, that nine in ten of the likelihoods and half of the cells it compares
    in a case are finite; the same builders are held to that here, so the seeds are verified without a GPU."""
    for S, nIn, nOut in ph.SUITE_CASES:
        ll, cells = _live(ph.suite_case(S, nIn, nOut))
        assert ll >= 0.9 and cells >= 0.5, (S, nIn, nOut, ll, cells)
    for cases in ([ph.wide_case()], [(ph.ragged_case()[0],) + p for p in ph.ragged_case()[1]],
                  [(ph.chained_case()[0],) + p for p in ph.chained_case()[1]]):
        ll, cells = _live(cases)
        assert ll >= 0.9 and cells >= 0.5, (ll, cells)
    for S in ph.LDS_STATES:                            # (scores only are compared there: every one finite)
        em, x, P = ph.lds_case(S)
        assert PairProfileDP(em).forward(x, P)[0] > -math.inf, S
    em, pairs = ph.chunk_case()
    ll, cells = _live([(em,) + p for p in pairs[:4]])
    assert ll >= 0.9 and cells >= 0.5, (ll, cells)
    em, pairs = ph.sparse_case()                       # a dead-input case: held only to being neither all dead nor all live
    lls = [PairProfileDP(em).forward(x, P)[0] > -math.inf for x, P in pairs]
    assert any(lls), lls


def test_pair_edge_suite_inputs_are_live():
    """test_profile_pair_edges_gpu.py asserts the same two conditions per case; its builders are held to them here.  Cases that
    compare scores, paths or counts but no cells are held to the likelihoods alone."""
    def both(cases):
        ll, cells = _live(cases)
        assert ll >= 0.9 and cells >= 0.5, (ll, cells)

    def scores(cases):
        assert _live(cases)[0] >= 0.9
    for levels in (True, False):
        for I, L in ph.RING_SHAPES:
            scores([ph.ring_case(I, L, levels)])
    em, pairs = ph.mixed_case()
    scores([(em,) + p for p in pairs])
    em, pairs = ph.packed_case()
    scores([(em,) + p for p in pairs])
    em, pairs, dead = ph.big_counts_case()
    assert em.nTransitions > 8192 and PairProfileDP(em).forward(*dead)[0] == -math.inf
    scores([(em,) + p for p in pairs])
    em, pairs = ph.flat_counts_case()
    assert em.nTransitions > 8192
    scores([(em,) + p for p in pairs])
    em = ph.tie_machine()
    both([(em,) + p for p in ph.tie_pairs()])
    both(ph.hand_tie_cases())
    em, pairs = ph.twin_case()
    both([(em,) + p for p in pairs])
    em, pairs = ph.chain_case()
    scores([(em,) + p for p in pairs])
    for I, L in ph.FLAT_SHAPES:
        em, pairs = ph.flat_diagonals_case(I, L)
        both([(em,) + p for p in pairs])
    for nIn, nOut in ph.SMALL_ALPHABETS:
        both([(em,) + p for em, pairs in ph.alphabet_case(nIn, nOut) for p in pairs])
    em, pairs = ph.pair_self_loop_case()
    both([(em,) + p for p in pairs])
    em, x, P, Pfar = ph.far_case()
    both([(em, x, Pfar)])
