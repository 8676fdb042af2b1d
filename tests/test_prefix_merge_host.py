"""Decoding against a CTC-merged profile on the host (prefixtree.MergedProfilePrefixDP, docs/decoding.md, "Decoding against a merged
profile"), all through the numpy backend.  The definition is the existing token search (PrefixDP, unchanged) on
algebra.compose(M, profile.mergingRecogniserMachine()) with an EMPTY output; mergeprefixhelpers.merged_composite maps the states of
that composite to the cells of the native lattice."""
import io

import numpy as np
import pytest

from conftest import golden_path
import mergeprefixhelpers as mph
from mergehelpers import one_hot_runs, random_merge_profile, run_heads
from mergeprefixhelpers import worst
from prefixhelpers import family_paths, populated_machine
from randmachine import random_seq
from machineboss_amd import boss, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import Profile, _red_planes

RTOL = 1e-9          # relative with a floor of 1: the bound of tests/test_prefix_profile_host.py


def _compare(M, em, prof, paths, params=None):
    """MergedProfilePrefixDP against PrefixDP on the composite: both probabilities of every node, every W cell whose state the
    composite kept (rows 0..L-1 plane by plane, row L summed over the planes: the recogniser has one end state).  Returns the
    composite's probabilities in one list and the number of cells compared."""
    P, colTok = prof.mergeRows(em)
    L, S, PL = len(P), em.nStates, len(colTok) + 1
    C, cellOf = mph.merged_composite(M, em, prof, params)
    ref = mph.composite_fills(C, em, paths)
    got = mph.merged_fills(em, P, colTok, paths)
    values, cells = [], 0
    for p in paths:
        assert worst([got[p][1], got[p][2]], [ref[p][1], ref[p][2]]) <= RTOL, (p, got[p][1:], ref[p][1:])
        values += [ref[p][1], ref[p][2]]
        assert got[p][0].shape == (L + 1, 2, PL, S)
        if ref[p][0].shape[2] != C.nStates:
            continue                                  # an input symbol the composite lost: the node is impossible
        want, have, last, haveLast = mph.composite_w_cells(ref[p][0], cellOf, L, PL, S)
        W = got[p][0][:, 0]
        assert worst(W[:L][have[:L]], want[:L][have[:L]]) <= RTOL, p
        assert worst(_red_planes(W[L], False)[haveLast], last[haveLast]) <= RTOL, p
        cells += int(have[:L].sum()) + int(haveLast.sum())
    return values, cells


# Seeds per (S, levels), searched on the CPU under the restatement alone: without silent levels the end state is out of reach of
# the shortest profiles, and these are the machines on which most of the twenty values of a seed are finite all the same.
SEEDS = {(5, True): range(8), (8, True): range(8), (5, False): (0, 1, 7, 9, 11, 12, 15, 16), (8, False): (1, 4, 8, 11, 14, 16, 19, 22)}


@pytest.fixture(scope="module")
def restatement():
    """Per (S, levels): (the composite's probabilities, W cells compared), or the AssertionError of the first node that differs."""
    out = {}
    for (S, levels), seeds in SEEDS.items():
        values, cells = [], 0
        try:
            for L in (0, 1, 2, 6):
                for seed in seeds:
                    M, em = mph.named_machine(populated_machine(S, seed, levels))
                    assert (int(em.silentLevels().max()) > 0) == levels
                    prof = random_merge_profile(np.random.RandomState(100 + seed), em, L)
                    assert len(set(prof.header)) < len(prof.header) and "zz" in prof.header
                    v, c = _compare(M, em, prof, family_paths(em.nInTok))
                    values += v; cells += c
            out[(S, levels)] = (values, cells)
        except AssertionError as e:
            out[(S, levels)] = e
    return out


@pytest.mark.parametrize("levels", [True, False])
@pytest.mark.parametrize("S", [5, 8])
def test_fill_equals_token_search_on_the_composite(restatement, S, levels):
    """The root, all children and one grandchild each over L in {0, 1, 2, 6} and 8 seeds; the profiles have a duplicated header
    symbol and a foreign one."""
    if isinstance(restatement[(S, levels)], AssertionError):
        raise restatement[(S, levels)]
    values, cells = restatement[(S, levels)]
    print("merged prefix restatement S=%d levels=%d: %d of %d probabilities finite, %d W cells compared" % (
        S, levels, sum(np.isfinite(values)), len(values), cells))
    assert len(values) == 4 * 8 * 5 * 2 and cells > 1000


def test_most_compared_values_are_finite(restatement):
    """At least three quarters of the compared logSeqProb and logPrefixProb values are finite: nothing passes on -inf = -inf."""
    values = [v for r in restatement.values() if not isinstance(r, AssertionError) for v in r[0]]
    assert len(values) == 4 * 320
    assert 4 * sum(np.isfinite(values)) >= 3 * len(values), (sum(np.isfinite(values)), len(values))


def test_dnastore4_against_golden_csv():
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    par = m.getParamDefs(True)
    for k, ms in enumerate(m.state):
        ms.name = k
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(golden_path("csv", "tiny_uc.csv"))
    values, cells = _compare(m, em, prof, family_paths(em.nInTok), par)
    assert sum(np.isfinite(values)) >= 2 and cells > 0


@pytest.mark.parametrize("levels", [True, False])
def test_one_hot_profile_equals_token_fill(levels):
    """A merged profile that is one-hot on the run heads of a token string, doubled by blanks, is that string: the token search
    gives the same two probabilities."""
    finite = 0
    for seed in range(6):
        em = populated_machine(8, seed, levels)
        rng = np.random.RandomState(seed)
        y = random_seq(rng, 9, em.nOutTok)
        colTok = [1, 2, 1]
        P = one_hot_runs(rng, colTok, y)
        assert run_heads(P, colTok) == [int(t) for t in y] and len(P) > len(y)
        tok = prefixtree.PrefixDP(em)
        got = mph.merged_fills(em, P, colTok, family_paths(2))
        ref = {}
        for p in family_paths(2):
            ref[p] = tok.fill(y) if not p else tok.fill(y, ref[p[:-1]][0], p[-1])
            assert worst([got[p][1], got[p][2]], [ref[p][1], ref[p][2]]) <= RTOL, (p, got[p][1:], ref[p][1:])
            finite += int(np.isfinite(ref[p][1])) + int(np.isfinite(ref[p][2]))
    assert finite >= 6 * 5


def test_whole_searches_on_sharp_profiles():
    m, em, colTok, ins, profs = mph.dnastore_merged_profiles()
    got, trees = prefixtree.decodeBatch(em, None, backend="numpy", profiles=profs, colTok=colTok)
    assert sum(a == b for a, b in zip(got, ins)) >= 6, (got, ins)
    for k in (0, 3, 7):
        t = prefixtree.PrefixTree.forProfile(em, profs[k], backend="numpy", colTok=colTok)
        assert t.doPrefixSearch() == got[k] and t.nFills == trees[k].nFills
        t.close()
    assert boss.prefixDecodeProfile(m, (profs[2], colTok), "numpy", merge=True) == got[2]


def test_plain_helper_equals_decode_batch():
    """boss.prefixDecodeProfile without merge is the existing search against a plain profile."""
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, None, useDefaults=True)
    prof = Profile.fromCsv(golden_path("csv", "tiny_uc.csv"))
    want = prefixtree.decodeBatch(em, None, backend="numpy", profiles=[prof])[0][0]
    assert boss.prefixDecodeProfile(m, prof, "numpy") == want
    merged = boss.prefixDecodeProfile(m, prof, "numpy", merge=True)
    t = prefixtree.PrefixTree.forProfile(em, prof, backend="numpy", colTok=prof.mergeRows(em)[1])
    assert t.doPrefixSearch() == merged
    t.close()


def test_rejections():
    em = populated_machine(5, 1, True)
    for bad in ([0, 1], [1, em.nOutTok + 1]):
        with pytest.raises(MachineError, match="column token outside"):
            prefixtree.MergedProfilePrefixDP(em, bad)
    dp = prefixtree.MergedProfilePrefixDP(em, [1, 2, 1])
    for bad in (np.nan, np.inf):
        P = np.zeros((3, 4)); P[1, 2] = bad
        with pytest.raises(MachineError, match="NaN or \\+infinity"):
            dp.fill(P)
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    with pytest.raises(MachineError, match="Need header"):
        boss.prefixDecodeProfile(m, Profile([], [[1.0], [1.0]]), "numpy", merge=True)
    with pytest.raises(MachineError, match="column map needs profiles"):
        prefixtree.makeNodes(em, [[1]], "numpy", colTok=[1])
    em4 = EvaluatedMachine.fromMachine(m, None, useDefaults=True)
    prof = Profile.fromCsv(golden_path("csv", "tiny_uc.csv"))
    with pytest.raises(MachineError, match="not the column map"):
        prefixtree.decodeBatch(em4, None, backend="numpy", profiles=[prof], colTok=[1])


def test_cli_spelling_is_still_rejected():
    with pytest.raises(MachineError, match="cannot be prefix-decoded"):
        boss.run(["tests/golden/machine/dnastore4.json", "--use-defaults", "--recognize-merge-csv", "tests/golden/csv/tiny_uc.csv",
                  "--prefix-decode", "--decode-backend", "numpy"], io.StringIO())


def _live(ref, floor, tag):
    """Every result finite, at least ``floor`` of each layer finite."""
    for p, (cells, lsp, lpp) in ref.items():
        assert np.isfinite(lsp) and np.isfinite(lpp), (tag, p, lsp, lpp)
    for layer in (0, 1):
        fin = sum(int(np.isfinite(c[:, layer]).sum()) for c, _, _ in ref.values())
        assert fin >= floor * sum(c[:, layer].size for c, _, _ in ref.values()), (tag, layer, fin)


def test_edge_suite_inputs_are_live():
    """tests/test_prefix_merge_edges_gpu.py asserts, from the yardstick, that its inputs are finite, dead, far down or tied where its
    cases need them to be; the same builders of mergeprefixhelpers.py are held to the same conditions here, so the seeds are
    verified without a GPU and nothing there passes on -inf = -inf."""
    import math
    import prefixhelpers as ph
    # 1. many planes: every result finite, half of each layer
    assert [c[0] + 1 for c in mph.PLANE_CASES] == [601, 1024, 1025, 1031, 1501]
    for nCols, S, L in mph.PLANE_CASES:
        em, colTok, P = mph.lane_case(nCols, S, L)
        assert em.nStates == S and P.shape == (L, nCols + 1) and colTok == [1 + c % 3 for c in range(nCols)]
        paths = mph.plane_paths(nCols)
        assert len(paths) == (5 if nCols < 1024 else 3) and max(len(p) for p in paths) == 2
        _live(mph.merged_fills(em, P, colTok, paths), 0.5, ("planes", nCols, S, L))
    # 2. alphabets: every result finite, three quarters of each layer
    for S, nIn, nOut, lv in mph.ALPHABET_CASES:
        em, colTok, P = mph.alphabet_case(S, nIn, nOut, lv)
        assert (em.nStates, em.nInTok, em.nOutTok) == (S, nIn, nOut) and (int(em.silentLevels().max()) > 0) == lv
        assert colTok == [1 + c % nOut for c in range(2 * nOut - 1)] and P.shape == (33, 2 * nOut) and np.isfinite(P).all()
        _live(mph.merged_fills(em, P, colTok, family_paths(nIn)), 0.75, ("alphabets", S, nIn, nOut, lv))
    # 3. dead weights
    em = mph.batch_machine()
    assert (em.nStates, em.nInTok, em.nOutTok) == (40, 3, 5) and int(em.silentLevels().max()) > 0
    P = mph.sparse_rows()
    dead = np.isneginf(P[:, 0])
    assert dead.sum() == 12 and (dead[:-1] & ~dead[1:]).any() and not np.isneginf(P).all(axis=1).any()
    assert 0.3 <= np.isneginf(P).mean() <= 0.4
    _live(mph.merged_fills(em, P, mph.DEAD_COLTOK, family_paths(3)), 0.5, "a third dead")
    P = mph.dead_row_rows()
    assert np.isneginf(P[mph.DEAD_ROW]).all() and np.isfinite(np.delete(P, mph.DEAD_ROW, 0)).all()
    for p, (cells, lsp, lpp) in mph.merged_fills(em, P, mph.DEAD_COLTOK, family_paths(3)).items():
        assert lsp == -math.inf and lpp == -math.inf and np.isneginf(cells[mph.DEAD_ROW + 1:]).all(), p
        assert np.isfinite(cells[:mph.DEAD_ROW + 1]).mean() >= 0.5 and np.isfinite(cells[mph.DEAD_ROW]).mean() >= 0.5, p
    em, colTok, P = mph.dead_blank_case()
    assert P.shape == (6, 66) and em.nStates == 2 and np.isneginf(P[:, 0]).all()
    _live(mph.merged_fills(em, P, colTok, family_paths(2)), 0.5, "every blank dead")
    # 4. the far column: every prefix probability is finite, and below what a linear product under the row maximum can hold
    em, R, _ = ph.far_column_case()
    ref = mph.merged_fills(em, mph.far_column_rows(), [1, 2], family_paths(2), R)
    assert all(np.isfinite(v[2]) and v[2] < -850 for v in ref.values()), [v[2] for v in ref.values()]
    assert ref[()][2] == pytest.approx(-851.127, abs=1e-3)
    # 5. twins and ties: the yardstick's twins are the same bits, every best input holds a twin symbol, the searches are short
    for quantised in (False, True):
        em = ph.twin_machine(ph.TWIN_STATES, ph.TWIN_SEED, quantised)
        profs = mph.twin_merged_profiles(em, quantised)
        assert len(profs) == 4
        if quantised:
            for k in [em.logWeight / math.log(0.5)] + [P / math.log(0.5) for P in profs]:
                assert np.abs(k - np.round(k)).max() < 1e-12
        ref = mph.merged_fills(em, profs[0], mph.TWIN_COLTOK, [(), (1,), (2,), (3,), (2, 1), (2, 2), (2, 3)])
        for a, b, c in (((1,), (2,), (3,)), ((2, 1), (2, 2), (2, 3))):
            assert ref[a][0].tobytes() == ref[b][0].tobytes() and ref[a][1:] == ref[b][1:]
            assert ref[a][0].tobytes() != ref[c][0].tobytes() and np.isfinite(ref[a][2])
        seqs, trees = prefixtree.decodeBatch(em, None, backend="numpy", profiles=profs, colTok=mph.TWIN_COLTOK)
        assert all(set(sq) & {"A", "B"} for sq in seqs), seqs
        print("merged twin searches", quantised, seqs, [t.nFills for t in trees])
        assert max(t.nFills for t in trees) < 300
    # 6. the silent self-loop
    em, _ = ph.self_loop_case()
    loops = [t for t in ph.machine_edges(em) if t[2] == 0 and t[3] == 0 and t[0] == t[1]]
    assert len(loops) == 1 and loops[0][0] == 0 and int(em.silentLevels().max()) > 0
    P = mph.self_loop_rows()
    assert P.shape == (12, len(mph.SELF_LOOP_COLTOK) + 1)
    _live(mph.merged_fills(em, P, mph.SELF_LOOP_COLTOK, family_paths(3)), 0.5, "self-loop")
    # 7. lengths 0 to 9: the root and the three children of every search are finite
    em, profs = mph.batch_machine(), mph.batch_rows()
    assert [P.shape for P in profs] == [(L, len(mph.BATCH_COLTOK) + 1) for L in range(10)]
    for P in profs:
        ref = mph.merged_fills(em, P, mph.BATCH_COLTOK, [(), (1,), (2,), (3,)])
        assert all(np.isfinite(v[1]) and np.isfinite(v[2]) for v in ref.values()), len(P)
    # 8. and 9. the many fills and the LDS marks: the root and the children compared are finite
    for S, toks in [(mph.MANY_FILLS[0], (1, 2))] + [(S, (1,)) for S in mph.LDS_MARK_STATES]:
        em, colTok, P = mph.lds_case(S)
        assert em.nStates == S and len(colTok) == 4 and len(P) == 3
        ref = mph.merged_fills(em, P, colTok, [()] + [(t,) for t in toks])
        assert all(np.isfinite(v[1]) and np.isfinite(v[2]) for v in ref.values()), S
