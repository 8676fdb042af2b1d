"""Decoding against a profile on the host (prefixtree.ProfilePrefixDP, docs/decoding.md), all through the numpy backend.  The
yardstick is the existing token search (PrefixDP / PrefixTree, unchanged) on compose(M, profile recogniser) with an EMPTY output:
the composite is built directly as an EvaluatedMachine (profileprefixhelpers.composite_machine) and also through
algebra.compose, which is what decides: dnastore4 has output-less moves, and there the order that the composition gives a blank
and such a move (the recogniser waits) changes the likelihood."""
import json
import math
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_path, load_json
from prefixhelpers import family_paths, populated_machine
from profileprefixhelpers import all_paths, composite_fills, composite_machine, composite_seq_cells, hard_profile, profile_fills, random_profile
from randmachine import random_seq
from machineboss_amd import algebra, boss, dp, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import Profile

RTOL = 1e-9          # relative with a floor of 1: the bound of tests/test_prefix_host.py


def _worst(got, ref):
    """Worst |got - ref| / max(1, |ref|) over the finite entries; -inf (and nothing else) must sit where the reference has it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (got, ref)
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))) if fin.any() else 0.0


def _compare(em, P, paths):
    """ProfilePrefixDP against PrefixDP on the composite: both probabilities of every node and every W cell.  Returns the
    composite's (logSeqProb, logPrefixProb) per node."""
    L, S = len(P), em.nStates
    ref = composite_fills(composite_machine(em, P), paths)
    got = profile_fills(em, P, paths)
    for p in paths:
        assert _worst([got[p][1], got[p][2]], [ref[p][1], ref[p][2]]) <= RTOL, (p, got[p][1:], ref[p][1:])
        assert got[p][0].shape == (L + 1, 2, S)
        assert _worst(got[p][0][:, 0], composite_seq_cells(ref[p][0], L, S)) <= RTOL, p      # W[r][q] is C's seq cell (q, r)
    return {p: ref[p][1:] for p in paths}


@pytest.mark.parametrize("levels", [True, False])
@pytest.mark.parametrize("L", [0, 1, 6, 12])
@pytest.mark.parametrize("S", [5, 8])
def test_fill_equals_token_search_on_the_composite(S, L, levels):
    """Root, children and all grandchildren (a superset of prefixhelpers.family_paths) over 12 seeds.  At S = 8, L = 12 the
    composite alone gives a finite logSeqProb and logPrefixProb on all 14 values of every seed, so nothing passes on -inf."""
    paths = all_paths(2)
    assert set(family_paths(2)) <= set(paths)
    for seed in range(12):
        em = populated_machine(S, seed, levels)
        assert (int(em.silentLevels().max()) > 0) == levels
        P = random_profile(np.random.RandomState(1000 + seed), L, em.nOutTok)
        assert np.isfinite(P[:, 0]).all()
        ref = _compare(em, P, paths)
        if S == 8 and L == 12:
            assert all(np.isfinite(v) for p in paths for v in ref[p]), (seed, ref)


def test_rows_without_a_blank():
    """The blank of some rows is zero: those rows must be crossed by an emission.  The -inf pattern is the composite's, and a
    profile whose symbols AND blank are zero in one row makes every node impossible."""
    paths = all_paths(2)
    some_inf = 0
    for seed in range(6):
        em = populated_machine(8, seed, seed % 2 == 0)
        rng = np.random.RandomState(2000 + seed)
        P = random_profile(rng, 12, em.nOutTok, pZero=0.4)
        P[rng.rand(12) < 0.5, 0] = -np.inf
        ref = _compare(em, P, paths)
        some_inf += sum(not np.isfinite(v) for p in paths for v in ref[p])
        P[5, :] = -np.inf
        dead = _compare(em, P, paths)
        assert all(v == -math.inf for p in paths for v in dead[p])
    print("nodes values at -inf with blank-less rows:", some_inf)


@pytest.mark.parametrize("name,params,csv", [("bitnoise", "params.json", "prof001.csv"), ("dnastore4", None, "tiny_uc.csv"),
                                             ("bitecho", None, "prof001.csv")])
def test_fill_equals_token_search_on_algebra_compose(name, params, csv):
    """The composite once through the algebra: compose(M, recogniser) as the command line of the reference would build it."""
    m = Machine.fromFile(golden_path("machine", name + ".json"))
    par = load_json("io", params) if params else m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(golden_path("csv", csv))
    C = EvaluatedMachine.fromMachine(algebra.compose(m, prof.recogniserMachine(), True, False), par)
    assert C.nOutTok == 0 and C.nInTok == em.nInTok
    paths = all_paths(em.nInTok)
    ref = composite_fills(C, paths)
    got = profile_fills(em, prof.logRows(em), paths)
    finite = 0
    for p in paths:
        assert _worst([got[p][1], got[p][2]], [ref[p][1], ref[p][2]]) <= RTOL, (p, got[p][1:], ref[p][1:])
        finite += int(np.isfinite(ref[p][1])) + int(np.isfinite(ref[p][2]))
    assert finite >= 2


@pytest.mark.parametrize("levels", [True, False])
def test_hard_profile_equals_token_fill(levels):
    """One symbol of weight 1 per row and no blank is the token string: the two searches give the same probabilities."""
    finite = 0
    for seed in range(6):
        em = populated_machine(8, seed, levels)
        y = random_seq(np.random.RandomState(seed), 12, em.nOutTok)
        tok = prefixtree.PrefixDP(em)
        got = profile_fills(em, hard_profile(y, em.nOutTok), all_paths(2))
        ref = {}
        for p in all_paths(2):
            ref[p] = tok.fill(y) if not p else tok.fill(y, ref[p[:-1]][0], p[-1])
            assert _worst([got[p][1], got[p][2]], [ref[p][1], ref[p][2]]) <= RTOL, (p, got[p][1:], ref[p][1:])
            assert _worst(got[p][0][:, 0], ref[p][0][:, 0]) <= RTOL
            finite += int(np.isfinite(ref[p][1])) + int(np.isfinite(ref[p][2]))
    assert finite >= 6 * 12


def _composite_search(C, maxBacktrack=prefixtree.NO_BACKTRACK_LIMIT):
    t = prefixtree.PrefixTree(C, prefixtree.makeNodes(C, [[]], "numpy"), 0, maxBacktrack, owner=True)
    t.start()
    seq = t.doPrefixSearch()
    n = t.nFills
    t.close()
    return seq, n, t.bestLogSeqProb


GOLDEN_SEARCHES = [("bitnoise", "params.json", "prof001.csv"), ("bitnoise", "params.json", "tiny_uc.csv"), ("bitecho", None, "prof001.csv"),
                   ("dnastore4", None, "tiny_uc.csv")]


@pytest.mark.parametrize("name,params,csv", GOLDEN_SEARCHES)
def test_whole_search_on_goldens(name, params, csv):
    m = Machine.fromFile(golden_path("machine", name + ".json"))
    par = load_json("io", params) if params else m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(golden_path("csv", csv))
    want, fills, ll = _composite_search(composite_machine(em, prof.logRows(em)))
    t = prefixtree.PrefixTree.forProfile(em, prof, backend="numpy")
    assert t.doPrefixSearch() == want and t.nFills == fills
    assert abs(t.bestLogSeqProb - ll) <= RTOL * max(1.0, abs(ll))
    t.close()
    seqs, trees = prefixtree.decodeBatch(em, None, backend="numpy", profiles=[prof, prof.logRows(em)])
    assert seqs == [want, want] and [x.nFills for x in trees] == [fills, fills]


@pytest.mark.parametrize("levels", [True, False])
def test_whole_search_with_backtrack_limit(levels):
    """populated_machine has many near-equal answers; with --prefix-backtrack the search ends, and it makes the same nodes in
    the same order as the token search on the composite."""
    decoded = 0
    for seed in range(4):
        em = populated_machine(5, seed, levels)
        P = random_profile(np.random.RandomState(3000 + seed), 6, em.nOutTok)
        want, fills, ll = _composite_search(composite_machine(em, P), 2)
        t = prefixtree.PrefixTree.forProfile(em, P, maxBacktrack=2, backend="numpy")
        assert t.doPrefixSearch() == want and t.nFills == fills, (seed, t.nFills, fills)
        t.close()
        decoded += len(want)
    assert decoded > 0


def _viterbi_on_composite(oracle_mod, m, par, prof):
    """decodePath of the oracle's Viterbi path through the composite of the input-silenced machine and the profile."""
    silent = algebra.silenceInput(m)
    ev = EvaluatedMachine.fromMachine(silent, par)
    P = prof.logRows(ev)
    C, origin = composite_machine(ev, P, origins=True)
    om = oracle_mod.OracleMachine(C)
    none = np.zeros(0, np.int32)
    V = om.viterbi(none, none)
    assert np.isfinite(V[-1, -1, -1])
    edges = [int(origin[e]) for e in om.traceback(none, none, V) if origin[e] >= 0]      # the blanks are no edges of the machine
    return algebra.decodePath(dp.edgesToPath(ev, silent, edges), m, par)


@pytest.mark.parametrize("name,params,csv", [("bitnoise", "params.json", "prof001.csv"), ("bitecho", None, "prof001.csv"),
                                             ("dnastore4", None, "nanopore_test.csv")])
def test_viterbi_decode_against_profile(oracle_mod, name, params, csv):
    m = Machine.fromFile(golden_path("machine", name + ".json"))
    par = load_json("io", params) if params else m.getParamDefs(True)
    prof = Profile.fromCsv(golden_path("csv", csv))
    if csv == "nanopore_test.csv":
        prof = Profile(prof.header, prof.row[:40])
    got = boss.viterbiDecodeProfile(m, prof, "numpy", par)
    assert got == _viterbi_on_composite(oracle_mod, m, par, prof)


def _boss(*args):
    r = subprocess.run([sys.executable, "-m", "machineboss_amd.boss", "--decode-backend", "numpy"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


M = "tests/golden/machine/"
CSV = "tests/golden/csv/"
CLI = [([M + "dnastore4.json", "--use-defaults"], "dnastore4", None, "tiny_uc.csv"),
       ([M + "bitnoise.json", "-P", "tests/golden/io/params.json"], "bitnoise", "params.json", "prof001.csv"),
       ([M + "bitecho.json"], "bitecho", None, "prof001.csv")]


@pytest.mark.parametrize("args,name,params,csv", CLI, ids=[c[1] + "-" + c[3] for c in CLI])
def test_cli_prefix_and_viterbi_decode(oracle_mod, args, name, params, csv):
    m = Machine.fromFile(golden_path("machine", name + ".json"))
    par = load_json("io", params) if params else m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(golden_path("csv", csv))
    want, _, _ = _composite_search(composite_machine(em, prof.logRows(em)))
    rc, out, err = _boss(*args, "--recognize-csv", CSV + csv, "--prefix-decode")
    assert rc == 0, err
    assert json.loads(out) == [{"input": {"name": "input", "sequence": want}, "output": {"name": "", "sequence": []}}]
    rc, out, err = _boss(*args, "--recognize-csv", CSV + csv, "--viterbi-decode")
    assert rc == 0, err
    assert json.loads(out)[0]["input"]["sequence"] == _viterbi_on_composite(oracle_mod, m, par, prof)
    assert json.loads(out)[0]["output"] == {"name": "", "sequence": []}


def test_cli_rejections():
    base = [M + "bitecho.json", "--recognize-csv", CSV + "prof001.csv"]
    for flag in ("--prefix-encode", "--viterbi-encode", "--random-encode"):
        rc, _, err = _boss(*base, flag)
        assert rc == 1 and "cannot be encoded" in err, (flag, err)
    for extra in (["--output-chars", "001"], ["--input-chars", "1"], ["-D", "tests/golden/io/seqpairlist.json"]):
        rc, _, err = _boss(*base, "--prefix-decode", *extra)
        assert rc == 1 and "takes no other sequence data" in err, (extra, err)
    rc, _, err = _boss(*base, "--viterbi-decode", "-L")
    assert rc == 1 and "not both" in err
    for flag in ("-L", "-V", "-C"):                     # scoring keeps its check for machines with inputs
        rc, _, err = _boss(*base, flag)
        assert rc == 1 and "needs a machine with an empty input alphabet" in err
    rc, _, err = _boss(M + "dnastore4.json", "--use-defaults", "--recognize-csv", CSV + "nanopore_test.csv", "--prefix-decode",
                       "--decode-nodes", "3")
    assert rc == 1 and "node pool is full" in err
    em = populated_machine(5, 1, True)
    with pytest.raises(MachineError, match="NaN or \\+infinity"):
        prefixtree.ProfilePrefixDP(em).fill(np.full((2, em.nOutTok + 1), np.nan))
