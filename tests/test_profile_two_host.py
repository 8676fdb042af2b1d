"""CPU tests of the two-profile sweeps (machineboss_amd/profile.py: TwoProfileDP; docs/profile_tapes.md, "Pairs of profiles"): the
numpy restatement against the oracle's exact Forward on compose(A.machine(), compose(M, B.recogniserMachine())) with empty tapes,
its Backward, the identities of its counts, its reductions to ProfileDP and PairProfileDP, the transposition identity, its tie
order, boss.scoreTwoProfiles and `boss --generate-csv` on the numpy path, and the liveness of the GPU suite's inputs.

Bounds (twoprofilehelpers): log values 1e-9 relative to max(1, |value|), -inf exact; counts >= 1e-3 at 1e-6 relative, below
1e-9 + 1e-6 x count absolute; Viterbi scores 1e-12; paths equal."""
import io
import json
import math

import numpy as np
import pytest

import twoprofilehelpers as th
from prefixhelpers import machine_edges, machine_from_edges
from twoprofilehelpers import logs_close, pair_machine
from machineboss_amd import algebra, boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import PairProfileDP, Profile, ProfileDP, TwoProfileDP

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"


def _composite_ll(oracle_mod, M, gen, rec):
    comp = algebra.compose(gen, algebra.compose(M, rec, True, False), True, False)
    ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
    return oracle_mod.OracleMachine(ec).loglike([], [], oracle_mod.SUM_EXACT)


def composite_loglike(oracle_mod, em, A, B):
    """The oracle's exact Forward, with empty tapes, on compose(A.machine(), compose(M, B.recogniserMachine()))."""
    return _composite_ll(oracle_mod, th.machine_of(em), th.profile_of(em.inputTokenizer.tok2sym[1:], A).machine(),
                         th.profile_of(em.outputTokenizer.tok2sym[1:], B).recogniserMachine())


@pytest.fixture(scope="module")
def swept(oracle_mod):
    """Per case of the grid: the restatement's results and the oracle's likelihood of the composite, computed once; the same for the
    variant whose end state has only an output-only self-loop."""
    out = {}
    for key, em, (A, B) in th.host_cases():
        for variant, m in (("plain", em), ("endloop", th.end_loop_variant(em))):
            dp = TwoProfileDP(m)
            ll, N, W, Z = dp.forward(A, B)
            blanks = []
            c, _ = dp.counts(A, B, blanks)
            out[key + (variant,)] = dict(em=m, A=A, B=B, dp=dp, ll=ll, N=N, W=W, Z=Z, counts=c, blanks=blanks[0] if blanks else (0.0, 0.0),
                                         exact=composite_loglike(oracle_mod, m, A, B))
    return out


def test_nine_in_ten_likelihoods_are_finite(swept):
    fin = [c["exact"] > -math.inf for k, c in swept.items() if k[-1] == "plain"]
    assert len(fin) == 126 and np.mean(fin) >= 0.9, np.mean(fin)


def test_forward_equals_composition(swept):
    """The recurrence as written, on the plain machines and on the variant whose end state has only an output-only self-loop (a mask
    that forbids the input blank at states without input-reading edges fails there)."""
    worst = 0.0
    for key, c in swept.items():
        assert logs_close([c["ll"]], [c["exact"]]), (key, c["ll"], c["exact"])
        worst = max(worst, th.log_dev([c["ll"]], [c["exact"]]))
    print("worst relative gap to the composite: %.3g over %d cases" % (worst, len(swept)))


def test_backward_equals_forward(swept):
    for key, c in swept.items():
        bl, NB, WB, ZB = c["dp"].backward(c["A"], c["B"])
        assert logs_close([bl], [c["ll"]]), (key, bl, c["ll"])
        # every cell splits the likelihood: the paths through the Z stage of (i, r) for i = K, and of r = L through N
        if c["ll"] > -math.inf:
            K = len(c["A"])
            with np.errstate(invalid="ignore"):
                assert logs_close([float(np.logaddexp.reduce((c["Z"][K, -1] + ZB[K, -1])))], [c["ll"]]), key


def test_counts_identities(swept):
    for key, c in swept.items():
        em, A, B = c["em"], c["A"], c["B"]
        if not c["ll"] > -math.inf:
            assert not c["counts"].any()
            continue
        net = np.zeros(em.nStates)
        np.add.at(net, em.dst.astype(np.int64), c["counts"]); np.subtract.at(net, em.src.astype(np.int64), c["counts"])
        want = np.zeros(em.nStates); want[-1] += 1.0; want[0] -= 1.0
        if em.nStates == 1:
            want[:] = 0.0
        assert np.allclose(net, want, rtol=0, atol=1e-9), (key, net)
        outBlank, inBlank = c["blanks"]
        assert abs(c["counts"][em.outTok > 0].sum() + outBlank - len(B)) <= 1e-9 * max(1, len(B)), key
        assert abs(c["counts"][em.inTok > 0].sum() + inBlank - len(A)) <= 1e-9 * max(1, len(A)), key


def test_counts_equal_finite_differences():
    """d loglike / d log w_t is the count of t: central differences at h = 1e-6 (error about h^2 plus 1e-16 / h: 1e-9)."""
    em = pair_machine(5, 1, True, 2, 3)
    A, B = th.two_input(np.random.RandomState(5), em, 3, 3, pInf=0.0)
    c, ll = TwoProfileDP(em).counts(A, B)
    assert ll > -math.inf
    edges = machine_edges(em)
    h = 1e-6
    for t in range(em.nTransitions):
        up, dn = list(edges), list(edges)
        up[t] = edges[t][:4] + (edges[t][4] + h,); dn[t] = edges[t][:4] + (edges[t][4] - h,)
        d = (TwoProfileDP(machine_from_edges(em.nStates, 2, 3, up)).forward(A, B)[0] -
             TwoProfileDP(machine_from_edges(em.nStates, 2, 3, dn)).forward(A, B)[0]) / (2 * h)
        silentLoop = em.src[t] >= em.dst[t] and not em.inTok[t] and not em.outTok[t]
        assert abs(d - c[t]) <= 1e-7 * max(1.0, c[t]) and (c[t] == 0.0 or not silentLoop), (t, d, c[t])


def test_reductions():
    """K = 0 is ProfileDP; a one-hot A is PairProfileDP on its tokens: likelihood, the N and W layers, Viterbi score."""
    for S, levels in ((5, True), (8, False)):
        em = pair_machine(S, 3, levels, 2, 3)
        rng = np.random.RandomState(S)
        B = th.soft_profile(rng, 4, 3)
        two = TwoProfileDP(em)
        ll, N, W, Z = two.forward(np.zeros((0, 3)), B)
        pl, PN, PW = ProfileDP(em).forward(B)
        assert logs_close([ll], [pl]) and logs_close(N[0], PN) and logs_close(W[0], PW) and logs_close(Z[0], PW)
        assert two.forward(np.zeros((0, 3)), B, "max")[0] == ProfileDP(em).forward(B, "max")[0]
        x = rng.randint(1, 3, size=3)
        ll, N, W, Z = two.forward(th.one_hot(x, 2), B)
        ql, QN, QW = PairProfileDP(em).forward(x, B)
        assert logs_close([ll], [ql]) and logs_close(N, QN) and logs_close(W, QW) and logs_close(Z, QW)
        assert two.forward(th.one_hot(x, 2), B, "max")[0] == PairProfileDP(em).forward(x, B, "max")[0]
        v, e, r, i = two.viterbi(th.one_hot(x, 2), B)
        pv, pe, pr = PairProfileDP(em).viterbi(x, B)
        assert v == pv and np.array_equal(e, pe) and np.array_equal(r, pr)


def test_transposition():
    """The likelihood of (M, A, B) is that of (transpose M, B, A), although the two blanks are treated differently."""
    n = 0
    for key, em, (A, B) in th.host_cases():
        if key[2] > 1 or key[3:] == (0, 0):
            continue
        A, B = th.two_input(np.random.RandomState(n), em, key[3], key[4], pInf=0.0)
        a, b = TwoProfileDP(em).forward(A, B)[0], TwoProfileDP(th.transposed(em)).forward(B, A)[0]
        assert a > -math.inf and logs_close([a], [b]), (key, a, b)
        n += 1
    assert n >= 60


def test_tie_census():
    """Every tie kind is met on the quantised machine, the first candidate wins, and every path rescored edge by edge (its blanks
    filled in) is the Viterbi score."""
    em = th.tie_machine()
    dp = TwoProfileDP(em)
    census = {}
    for A, B in th.tie_pairs():
        v, edges, rows, ins = dp.viterbi(A, B, census)
        assert v > -math.inf and th.rescore(em, A, B, edges, rows, ins) == v
        assert list(rows) == sorted(rows) and list(ins) == sorted(ins)
        assert int(em.src[edges[0]]) == 0 and int(em.dst[edges[-1]]) == em.nStates - 1
        assert all(int(em.dst[a]) == int(em.src[b]) for a, b in zip(edges[:-1], edges[1:]))
    for first, second in th.TIE_KINDS:
        assert any(first in k and second in k and k.index(first) < k.index(second) for k in census), (first, second, census)
    for em, A, B, edges, rows, ins in th.hand_tie_cases():
        v, e, r, i = TwoProfileDP(em).viterbi(A, B)
        assert v == 0.0 and list(e) == edges and list(r) == rows and list(i) == ins
    # random machines: paths rescore to the score
    for key, em, (A, B) in th.host_cases():
        if key[2] == 0:
            v, e, r, i = TwoProfileDP(em).viterbi(A, B)
            if v > -math.inf:
                assert abs(th.rescore(em, A, B, e, r, i) - v) <= 1e-9 * max(1.0, abs(v)), key
                assert len(e) <= len(A) + len(B) + (len(A) + len(B) + 1) * len(TwoProfileDP(em).fLevels)
            else:
                assert len(e) == 0


def _dnastore_inputs(tmp_path):
    """dnastore4 with its defaults, tiny_uc.csv as the output profile and a small input profile over its three input symbols."""
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    return m, par, em, str(a), Profile.fromCsv(str(a)), Profile.fromCsv(CSV)


def test_dnastore_equals_composition(oracle_mod, tmp_path):
    m, par, em, _, pa, pb = _dnastore_inputs(tmp_path)
    A, B = pa.logRowsIn(em), pb.logRows(em)
    assert A.shape == (3, 4) and np.allclose(np.exp(A[0]), [.125, .5, .25, .125])
    ll = TwoProfileDP(em).forward(A, B)[0]
    want = _composite_ll(oracle_mod, th.machine_of(em), pa.machine(), pb.recogniserMachine())
    assert ll > -math.inf and logs_close([ll], [want]), (ll, want)


def test_score_two_profiles_numpy(tmp_path):
    m, par, em, _, pa, pb = _dnastore_inputs(tmp_path)
    short = Profile(pa.header, pa.row[:1])
    sc, pc = boss.scoreTwoProfiles(m, [pa, short], pb, backend="numpy", params=par, loglike=True, viterbi=True, counts=True)
    dp = TwoProfileDP(em)
    B = pb.logRows(em)
    for k, p in enumerate((pa, short)):
        assert sc["loglike"][k] == dp.forward(p.logRowsIn(em), B)[0] and sc["viterbi"][k] == dp.forward(p.logRowsIn(em), B, "max")[0]
    assert pc == {}                                       # (dnastore4 has no parameters)
    sc, pc = boss.scoreTwoProfiles(m, [pa], pb, backend="numpy", params=par, loglike=False)
    assert sc == {"loglike": None, "viterbi": None} and pc is None
    noIn = Machine.fromFile("tests/golden/machine/bitnoise.json")
    gen = algebra.compose(algebra.generator(["0"], "g"), noIn)
    with pytest.raises(MachineError, match="two-profile sweeps need a machine with an input alphabet"):
        boss.scoreTwoProfiles(gen, [pa], pb, backend="numpy", params=json.load(open("tests/golden/io/params.json")))


def _run(*args):
    out = io.StringIO()
    assert boss.run(list(args) + ["--decode-backend", "numpy"], out) == 0
    return out.getvalue()


def test_cli_equals_restatement(tmp_path):
    m, par, em, a, pa, pb = _dnastore_inputs(tmp_path)
    dp = TwoProfileDP(em)
    A, B = pa.logRowsIn(em), pb.logRows(em)
    base = [DNASTORE, "--use-defaults", "--generate-csv", a, "--recognize-csv", CSV]
    for flag, mode in (("-L", "exact"), ("-V", "max")):
        got = json.loads(_run(*base, flag))
        want = dp.forward(A, B, mode)[0]
        assert got[0][:2] == [a, ""] and want > -math.inf and abs(got[0][2] - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    assert json.loads(_run(*base, "-C")) == {}
    assert len(_run(*base, "-L", "-V").splitlines()) == 2


def test_cli_rejections(tmp_path):
    _, _, _, a, _, _ = _dnastore_inputs(tmp_path)
    only = "--generate-csv goes with --recognize-csv and -L, -V or -C"

    def fails(args, msg):
        with pytest.raises(MachineError, match=msg):
            boss.run(args + ["--decode-backend", "numpy"], io.StringIO())
    gen = [DNASTORE, "--use-defaults", "--generate-csv", a]
    fails(gen + ["-L"], only)                                                           # without --recognize-csv
    fails(gen + ["-L", "--input-chars", ""], only)
    fails(gen + ["--recognize-merge-csv", CSV, "-L"], only)
    fails(gen + ["--recognize-csv", CSV, "--recognize-merge-csv", CSV, "-L"], only)
    for extra in (["--input-chars", ""], ["--input-json", "tests/golden/io/tiny_uc.json"], ["--input-fasta", "tests/golden/io/tiny_uc.json"]):
        fails(gen + ["--recognize-csv", CSV, "-L"] + extra, only)                        # beside an input sequence
    for flag in ("--prefix-decode", "--viterbi-decode", "--prefix-encode", "--viterbi-encode", "--random-encode"):
        fails(gen + ["--recognize-csv", CSV, flag], only)
    fails(gen + ["--recognize-csv", CSV, "-L", "--profile-band", "2"], only)
    # the rejections of --recognize-csv keep their words beside --generate-csv
    for flag in ("-A", "-T"):
        fails(gen + ["--recognize-csv", CSV, flag], "supports -L, -V and -C")
    fails(gen + ["--recognize-csv", CSV], "needs -L, -V or -C")
    fails(gen + ["--recognize-csv", CSV, "-L", "--output-chars", "A"], "takes no other sequence data")
    fails(gen + ["--recognize-csv", str(tmp_path / "none.csv"), "-L"], "CSV file not found")
    fails(["--generate-json", "tests/golden/io/tiny_uc.json", "--generate-csv", a, "--recognize-csv", CSV, "-L"],
          "two-profile sweeps need a machine with an input alphabet")
    # and without --generate-csv nothing changed
    fails([DNASTORE, "--use-defaults", "--recognize-csv", CSV, "-L"], "needs a machine with an empty input alphabet")
    dp = TwoProfileDP(pair_machine(5, 0, True, 2, 3))
    with pytest.raises(MachineError, match="NaN"):
        dp.forward(np.full((1, 3), np.nan), np.zeros((1, 4)))
    with pytest.raises(MachineError, match="NaN or \\+infinity"):
        dp.forward(np.zeros((1, 3)), np.full((1, 4), np.inf))


# ---- the inputs of the GPU suite ------------------------------------------------------------------------------------------------
def _live(cases):
    """(fraction of finite likelihoods, fraction of finite cells) of [(em, A, B)] under the restatement."""
    lls, fin, tot = [], 0, 0
    dps = {}
    for em, A, B in cases:
        ll, N, W, Z = dps.setdefault(id(em), TwoProfileDP(em)).forward(A, B)
        lls.append(ll > -math.inf)
        fin += int(np.isfinite(N).sum() + np.isfinite(W).sum() + np.isfinite(Z).sum()); tot += 3 * N.size
    return float(np.mean(lls)), fin / tot


def test_two_suite_inputs_are_live():
    """test_profile_two_gpu.py asserts, from the restatement, that nine in ten of the likelihoods and half of the cells it compares
    in a suite case are finite; the same builders are held to that here, so the seeds are verified without a GPU.  Cases that
    compare scores, paths or counts but no cells are held to the likelihoods alone."""
    for S, nIn, nOut in th.SUITE_CASES:
        ll, cells = _live(th.suite_case(S, nIn, nOut))
        assert ll >= 0.9 and cells >= 0.5, (S, nIn, nOut, ll, cells)
    em, pairs = th.ring_pairs()
    sizes = [th.ring_bytes(th.RING_S, len(A), len(B)) for A, B in pairs[:8]]
    assert sizes == [63360, 66240, 161280, 164160] * 2 and 63360 <= 65536 < 66240 and 161280 <= th.RING_LDS_MAX < 164160
    lls = [TwoProfileDP(em).forward(A, B)[0] > -math.inf for A, B in pairs[:2] + pairs[8:]]       # (the pairs the GPU test scores here)
    assert lls == [True] * 5 + [False], lls
    em, pairs = th.packed_case()
    assert th.ring_bytes(th.PACKED_S, 3, 3) > th.RING_LDS_MAX >= th.ring_bytes(th.PACKED_S, 2, 3)
    assert _live([(em,) + p for p in pairs[:4]])[0] == 1.0
    em, pairs, dead = th.big_counts_case()
    assert em.nTransitions > 8192 and TwoProfileDP(em).forward(*dead)[0] == -math.inf
    assert _live([(em,) + p for p in pairs])[0] == 1.0
    em, pairs = th.special_profiles()
    lls = [TwoProfileDP(em).forward(A, B)[0] > -math.inf for A, B in pairs]
    assert lls[:3] == [True] * 3 and lls[3:5] == [False] * 2 and any(lls[5:]), lls
    em, pairs = th.chain_case()
    dp = TwoProfileDP(em)
    for A, B in pairs:
        v, e, r, i = dp.viterbi(A, B)
        assert v > -math.inf and len(e) == len(A) + len(B) + (len(A) + len(B) + 1) * (th.CHAIN_S - 1)
    em, A, B, Afar, Bfar = th.far_case()
    ll, far = TwoProfileDP(em).forward(A, B)[0], TwoProfileDP(em).forward(Afar, Bfar)[0]
    assert ll > -math.inf and abs(far - (ll + 18 * th.FAR_SHIFT)) <= 1e-9 * abs(far)


def test_two_edge_inputs_are_live():
    """test_profile_two_edges_gpu.py: the group rule of mb_profile_twos_counts restated (a workgroup per 2 048 (cell, state) items of
    the largest lattice of a launch) and the shapes on either side of its marks; every transition of the group cases with a
    positive count, so that an item left out cannot hide in a zero; the chunking of the budgets restated, with the dead pair and
    (0, 0) inside a chunk; and nine in ten of the 126 live pairs of the traceback case with a path."""
    S = th.GROUP_S
    items = [S * (K + 1) * (L + 1) for K, L in th.GROUP_SHAPES]
    assert items == [2040, 2050, 2050, 4205, 10240, 10400, 10400, 20800] and S % 2 == 1
    assert [th.count_groups(S, [s]) for s in th.GROUP_SHAPES] == list(th.GROUP_COUNTS) and th.GROUP_COUNTS[:4] == (1, 2, 2, 3)
    assert th.GROUP_COUNTS[4:] == (5, 6, 6, 11) and 4205 % (3 * 256) == 256 + 109          # the last stride: group 0, a part of group 1
    assert th.count_groups(S, th.GROUP_RAGGED) == 11 and all(th.count_groups(S, [s]) == 1 for s in th.GROUP_RAGGED[1:])
    assert th.count_groups(1, [(0, 0)]) == 1 and th.count_groups(700, [(3, 4)]) == 7 and th.count_groups(8, [(999, 999)]) == 256
    em, singles, ragged, dead = th.group_case()
    dp = TwoProfileDP(em)
    assert np.array_equal(ragged[0][0], singles[-1][0]) and np.array_equal(ragged[0][1], singles[-1][1])
    for A, B in singles:
        c, ll = dp.counts(A, B)
        assert ll > -math.inf and (c > 0).all(), (len(A), len(B), ll, c.min())
    assert all(dp.forward(A, B)[0] > -math.inf for A, B in ragged[1:]) and dp.forward(*dead)[0] == -math.inf
    em, pairs = th.split_case()
    dp = TwoProfileDP(em)
    lls = [dp.forward(A, B)[0] > -math.inf for A, B in pairs]
    assert [(len(A), len(B)) for A, B in pairs] == list(th.SPLIT_SHAPES) and lls == [k != th.SPLIT_DEAD for k in range(len(pairs))], lls
    assert all(len(dp.viterbi(A, B)[1]) > 0 for k, (A, B) in enumerate(pairs) if k != th.SPLIT_DEAD)
    bounds = [th.path_bound(len(dp.fLevels), K, L) for K, L in th.SPLIT_SHAPES]
    for sizes, slack in (([th.count_bytes(th.SPLIT_S, K, L) for K, L in th.SPLIT_SHAPES], 4096),
                         ([th.path_bytes(th.SPLIT_S, K, L, b) for (K, L), b in zip(th.SPLIT_SHAPES, bounds)], 1024)):
        chunks = th.lattice_chunks(sizes, 2 * max(sizes) + slack)
        assert len(chunks) >= 3 and chunks[0][0] == 0 and chunks[-1][1] == len(sizes) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(sum(sizes[p0:p1]) <= 2 * max(sizes) + slack for p0, p1 in chunks)
        for inside in (th.SPLIT_DEAD, th.SPLIT_SHAPES.index((0, 0))):
            assert any(p0 < inside < p1 - 1 for p0, p1 in chunks), (inside, chunks)
    em, pairs = th.chain_case()
    sizes = [th.path_bytes(th.CHAIN_S, len(A), len(B), th.path_bound(th.CHAIN_S - 1, len(A), len(B))) for A, B in pairs] * 2
    assert len(th.lattice_chunks(sizes, 2 * max(sizes) + 1024)) >= 3
    em, pairs = th.seam_case()
    dp = TwoProfileDP(em)
    lls = [dp.forward(A, B, "max")[0] > -math.inf for A, B in pairs]
    assert len(pairs) == 129 and th.SEAM_DEAD == (63, 64, 128) and not any(lls[k] for k in th.SEAM_DEAD)
    assert np.mean(np.delete(lls, th.SEAM_DEAD)) >= 0.9, np.mean(np.delete(lls, th.SEAM_DEAD))
    assert [(len(A), len(B)) for k, (A, B) in enumerate(pairs) if k not in th.SEAM_DEAD][:6] == list(th.SEAM_SHAPES)
