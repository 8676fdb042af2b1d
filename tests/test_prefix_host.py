"""Prefix search on the host (machineboss_amd/prefixtree.py, docs/decoding.md), all through the numpy backend: the restated node
fill against the oracle's Forward and against brute force, the search against the reference's expected outputs through the
command line, the sampler, the rejections."""
import itertools
import json
import math
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_path, load_json
from randmachine import random_machine, random_seq
from machineboss_amd import algebra, prefixtree
from machineboss_amd.dp import Mt19937
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError


def _strings(nIn, maxLen):
    for n in range(maxLen + 1):
        yield from itertools.product(range(1, nIn + 1), repeat=n)


def _fills(dp, y, strings, monotone=True):
    """{x: (cells, logSeqProb, logPrefixProb)} for every x in ``strings`` (prefix-closed, shortest first)."""
    out = {}
    for x in strings:
        out[x] = dp.fill(y) if not x else dp.fill(y, out[x[:-1]][0], x[-1])
        if x and monotone:
            assert out[x][2] <= out[x[:-1]][2] + 1e-12, (x, out[x][2], out[x[:-1]][2])     # a longer prefix is no likelier
    return out


def _close(a, b, rtol=1e-9):
    return a == b if not (np.isfinite(a) and np.isfinite(b)) else abs(a - b) <= rtol * max(abs(a), abs(b))


@pytest.mark.parametrize("S,seed,L", [(3, 3, 4), (6, 4, 4), (9, 2, 4), (12, 4, 2), (12, 5, 0), (20, 6, 4)])
def test_seq_layer_is_the_oracle_forward(oracle_mod, S, seed, L):
    """seq[L][S-1] of the node of x is the Forward log-likelihood of (x, y): 1e-9 relative, the README's Forward figure."""
    em = random_machine(S, 2, 2, seed)
    om = oracle_mod.OracleMachine(em)
    y = random_seq(np.random.RandomState(seed), L, em.nOutTok)
    # (these machines have input-reading cycles heavier than 1: (I - N)^-1 is no convergent sum there, the prefix layer means
    # nothing and is not looked at -- the seq layer does not read it)
    nodes = _fills(prefixtree.PrefixDP(em), y, list(_strings(2, 3)), monotone=False)
    finite = 0
    for x, (_, lsp, _) in nodes.items():
        ref = om.loglike(np.array(x, np.int32), y, oracle_mod.SUM_EXACT)
        assert _close(lsp, ref), (x, lsp, ref)
        finite += np.isfinite(ref)
    assert finite >= 4


def _acyclic_machine(S, seed):
    """A random machine whose transitions all go forward, so that no input is longer than S - 1."""
    em = random_machine(S, 2, 2, seed)
    keep = em.dst > em.src
    src = em.src[keep]
    off = np.zeros(S + 1, np.int64)
    np.add.at(off, src.astype(np.int64) + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(len(src)) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, em.inputTokenizer, em.outputTokenizer, src, em.dst[keep], em.inTok[keep], em.outTok[keep], tidx,
                            em.logWeight[keep], off, em.stateNames)


def _brute_force_prefix(oracle_mod, em, y, maxIn, upTo):
    om = oracle_mod.OracleMachine(em)
    full = {x: om.loglike(np.array(x, np.int32), y, oracle_mod.SUM_EXACT) for x in _strings(em.nInTok, maxIn)}
    assert all(v == -math.inf for x, v in full.items() if len(x) == maxIn), "inputs of the longest length must be impossible"
    nodes = _fills(prefixtree.PrefixDP(em), y, list(_strings(em.nInTok, upTo)))
    some = 0
    for x, (_, lsp, lpp) in nodes.items():
        total = sum(math.exp(v) for w, v in full.items() if w[:len(x)] == x)
        assert abs(math.exp(lpp) - total) <= 1e-9 * total, (x, lpp, total)
        some += total > 0
    assert some > 1


@pytest.mark.parametrize("S,seed,L", [(6, 6, 2), (7, 40, 2), (8, 23, 2), (8, 13, 2)])
def test_prefix_layer_is_the_sum_over_continuations_random(oracle_mod, S, seed, L):
    em = _acyclic_machine(S, seed)
    _brute_force_prefix(oracle_mod, em, random_seq(np.random.RandomState(seed), L, em.nOutTok), S, 3)


def test_prefix_layer_is_the_sum_over_continuations_bintern(oracle_mod, machines):
    m, em = machines("bintern")
    # three input bits give two trits and the tail of up to two more: no input of 6 bits emits 12222
    _brute_force_prefix(oracle_mod, em, em.outputTokenizer.tokenize(list("12222")), 6, 3)


def test_prefix_layer_is_the_sum_over_continuations_hamming_block(oracle_mod, machines):
    m, em = machines("hamming74", preset=True)
    # one block: four input bits give seven output bits, so no input of 5 bits emits 7
    _brute_force_prefix(oracle_mod, em, em.outputTokenizer.tokenize(list("0110011")), 5, 3)


def _boss(*args):
    r = subprocess.run([sys.executable, "-m", "machineboss_amd.boss", "--decode-backend", "numpy"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


HAMMING_IN = "0000000100100011010001010110011110001001101010111100110111101111"
M = "tests/golden/machine/"
CLI = [
    ([M + "bitecho.json", "--recognize-chars", "101", "--prefix-decode"], "decode-bitecho-101.json"),        # test-decode-bitecho-101
    (["--generate-chars", "101", M + "bintern.json", "--prefix-encode"], "encode-g101-bintern.json"),        # test-bintern
    (["--input-chars", "101", M + "bintern.json", "--prefix-encode"], "encode-i101-bintern.json"),
    ([M + "bintern.json", "--recognize-chars", "12222", "--prefix-decode"], "decode-a12222-bintern.json"),
    ([M + "bintern.json", "--output-chars", "12222", "--prefix-decode"], "decode-o12222-bintern.json"),
    (["--preset", "hamming74", "--viterbi-encode", "--input-chars", HAMMING_IN], "hamming74.json"),          # test-hamming
    (["--preset", "hamming74", "--prefix-encode", "--input-chars", HAMMING_IN], "hamming74.json"),
    ([M + "bitecho.json", "--recognize-chars", "101", "--viterbi-decode"], "decode-bitecho-101.json"),       # test-viterbi-decode-bitecho
    # dnastore-decode.json: the reference tests it under --beam-decode only.  What backs it for these two options: the numpy search
    # below finds it in 25 node fills at log-likelihood 4.394449 (test_node_counts_of_small_searches), and --viterbi-decode, whose
    # Viterbi restatement is checked against the oracle elsewhere in this suite, reads the same symbols off its path.
    ([M + "dnastore4.json", "--output-chars", "AGTAGTAG", "--prefix-decode"], "dnastore-decode.json"),
    ([M + "dnastore4.json", "--output-chars", "AGTAGTAG", "--viterbi-decode"], "dnastore-decode.json"),
]


@pytest.mark.parametrize("args,expect", CLI, ids=["%s %s" % (e[:-5], [a for a in args if a.startswith("--") and a.endswith("code")][0]) for args, e in CLI])
def test_cli_goldens(args, expect):
    rc, out, err = _boss(*args)
    assert rc == 0, err
    assert json.loads(out) == load_json("expect", expect)


def test_node_counts_of_small_searches(machines):
    """Node counts pin the search order: bitecho / 101 and bintern / 12222 take 7 fills (the root and two children per symbol of
    the answer), dnastore4 / AGTAGTAG 25 (the root and three per symbol); no fill is spent off the winning path."""
    for name, out, want, fills, ll in (("bitecho", "101", ["1", "0", "1"], 7, None), ("bintern", "12222", ["1", "0", "1"], 7, None),
                                       ("dnastore4", "AGTAGTAG", ["0_3", "1_3", "2_3", "0_3", "1_3", "2_3", "0_3", "1_3"], 25, 4.394449)):
        m, em = machines(name, useDefaults=True)
        t = prefixtree.PrefixTree.forOutput(em, list(out), backend="numpy")
        assert t.doPrefixSearch() == want and t.nFills == fills, (name, t.nFills)
        assert ll is None or abs(t.bestLogSeqProb - ll) < 1e-6
        assert t.monotone
        t.close()


def test_lock_step_batch_equals_single_searches(machines):
    m, em = machines("bintern")
    enc = EvaluatedMachine.fromMachine(algebra.advancingMachine(algebra.advanceSort(algebra.transpose(m))), None)
    outs, _ = prefixtree.decodeBatch(enc, [list(i) for i in ("101", "000", "110", "0110", "1", "")], backend="numpy")
    assert len({tuple(o) for o in outs}) == 6
    seqs, trees = prefixtree.decodeBatch(em, outs, backend="numpy")
    for o, s, bt in zip(outs, seqs, trees):
        t = prefixtree.PrefixTree.forOutput(em, o, backend="numpy")
        assert t.doPrefixSearch() == s and t.nFills == bt.nFills and t.bestLogSeqProb == bt.bestLogSeqProb
        assert t.monotone and bt.monotone
        t.close()


def test_backtrack_limit_purges_and_frees(machines):
    m, em = machines("dnastore4", useDefaults=True)
    full = prefixtree.PrefixTree.forOutput(em, list("AGTAGTAG"), backend="numpy")
    want = full.doPrefixSearch()
    t = prefixtree.PrefixTree.forOutput(em, list("AGTAGTAG"), maxBacktrack=1, backend="numpy", maxNodes=64)
    assert t.doPrefixSearch() == want
    def alive(n):
        return 1 + sum(alive(c) for c in n.child)
    assert t.nFills <= full.nFills
    assert t.nodes.free_nodes() == 64 - alive(t.root) and full.nodes.free_nodes() == prefixtree.DEFAULT_MAX_NODES - alive(full.root)
    assert t.logSeqProb(em.inputTokenizer.tokenize(want)) == t.bestLogSeqProb
    full.close(); t.close()


def test_random_encode_same_seed_same_answer():
    a = _boss(M + "bitecho.json", "--input-chars", "101", "--random-encode", "--seed", "42")
    b = _boss(M + "bitecho.json", "--input-chars", "101", "--random-encode", "--seed", "42")
    assert a[0] == 0 and a == b, a[2]
    assert json.loads(a[1])[0]["input"] == {"name": "101", "sequence": ["1", "0", "1"]}


def _sample_counts(em, out, seeds):
    counts = {}
    t = prefixtree.PrefixTree.forOutput(em, out, backend="numpy")
    for seed in range(seeds):
        mt = Mt19937(seed)
        x = tuple(t.sampleTokSeq(lambda: (mt() + mt() * 4294967296.0) / 18446744073709551616.0))
        counts[x] = counts.get(x, 0) + 1
    return t, counts


def test_random_encode_distribution_bitecho(machines):
    """2 000 seeds on bitecho with input 101: every output within 4 standard errors of exp(logSeqProb) (the machine is normalised)."""
    m, em0 = machines("bitecho")
    em = EvaluatedMachine.fromMachine(algebra.advancingMachine(algebra.advanceSort(algebra.transpose(m))), None)
    t, counts = _sample_counts(em, list("101"), 2000)
    for x in set(counts) | {tuple(em.inputTokenizer.tokenize(list("101")))}:
        p = math.exp(t.logSeqProb(x))
        assert abs(counts.get(x, 0) / 2000 - p) <= 4 * math.sqrt(p * (1 - p) / 2000), (x, counts.get(x, 0), p)
    t.close()


def test_sampler_distribution_random_machine():
    """The same on a machine with many answers: x is drawn with probability P(x, y) / P(y | any input)."""
    em = _acyclic_machine(8, 23)
    y = random_seq(np.random.RandomState(23), 2, em.nOutTok)
    t, counts = _sample_counts(em, em.outputTokenizer.detokenize(y), 2000)
    assert len(counts) > 2
    for x in _strings(2, 7):
        p = math.exp(t.logSeqProb(x) - t.root.logPrefixProb)
        assert abs(counts.get(x, 0) / 2000 - p) <= 4 * math.sqrt(p * (1 - p) / 2000) + 1e-12, (x, counts.get(x, 0), p)
    t.close()


def test_rejections():
    rc, _, err = _boss(M + "bitecho.json", "--input-chars", "101", "--output-chars", "101", "--prefix-decode")
    assert rc == 1 and "cannot specify input sequences when decoding" in err
    rc, _, err = _boss(M + "bitecho.json", "--input-chars", "101", "--output-chars", "101", "--viterbi-encode")
    assert rc == 1 and "cannot specify output sequences when encoding" in err
    rc, _, err = _boss(M + "dnastore4.json", "--output-chars", "AGTAGTAG", "--prefix-decode", "--decode-nodes", "12")
    assert rc == 1 and "node pool is full" in err
    m = Machine.fromFile(golden_path("machine", "bitecho.json"))
    em = EvaluatedMachine.fromMachine(m, None)
    with pytest.raises(MachineError, match="unknown prefix search backend"):
        prefixtree.makeNodes(em, [[1]], backend="cuda")


def test_decode_helpers_of_the_algebra(machines):
    m, _ = machines("bintern")
    t = algebra.transpose(m)
    assert t.inputAlphabet() == m.outputAlphabet() and t.outputAlphabet() == m.inputAlphabet()
    assert algebra.transpose(t).inputAlphabet() == m.inputAlphabet()
    s = algebra.silenceInput(m)
    assert not s.inputAlphabet() and s.outputAlphabet() == m.outputAlphabet() and m.inputAlphabet()
    d = algebra.decodeSort(algebra.advancingMachine(algebra.advanceSort(t)))
    assert d.nStates() >= m.nStates() and algebra.nEmptyOutputBackTransitions(d) <= algebra.nEmptyOutputBackTransitions(t)


def _family_refs(dp, y, nIn):
    from prefixhelpers import family_paths
    out = {}
    for p in family_paths(nIn):
        out[p] = dp.fill(y) if not p else dp.fill(y, out[p[:-1]][0], p[-1])
    return out


def _live_family(ref, floor, tag):
    """Every result finite, at least ``floor`` of each layer finite."""
    for p, (cells, lsp, lpp) in ref.items():
        assert np.isfinite(lsp) and np.isfinite(lpp), (tag, p, lsp, lpp)
    for layer in (0, 1):
        fin = sum(int(np.isfinite(c[:, layer]).sum()) for c, _, _ in ref.values())
        assert fin >= floor * sum(c[:, layer].size for c, _, _ in ref.values()), (tag, layer, fin)


def test_edge_suite_inputs_are_live():
    """tests/test_prefix_edges_gpu.py asserts, from the yardsticks, that its inputs are finite, dead, far down or tied where its cases
    need them to be; the same builders of prefixhelpers.py and profileprefixhelpers.py are held to the same conditions here, so the
    seeds are verified without a GPU."""
    import prefixhelpers as ph
    import profileprefixhelpers as pph
    # 1. alphabets and lanes: every result finite, half of each layer finite, with both yardsticks
    for S, nIn, nOut, lv in ph.EDGE_CASES:
        em, y = ph.edge_case(S, nIn, nOut, lv)
        assert em.nStates == S and em.nInTok == nIn and em.nOutTok == nOut and len(y) == ph.EDGE_L
        assert (int(em.silentLevels().max()) > 0) == lv
        R = prefixtree.logSumInTrans(em)
        _live_family(_family_refs(prefixtree.PrefixDP(em, R), y, nIn), 0.5, ("token", S, nIn, nOut, lv))
        _live_family(_family_refs(prefixtree.ProfilePrefixDP(em, R), pph.edge_profile(S, nOut), nIn), 0.5, ("profile", S, nIn, nOut, lv))
    assert {c[0] for c in ph.EDGE_CASES} == {1, 2, 63, 64, 65, 1024, 1025}
    for S in (1, 2, 63, 64, 65, 1025):
        here = [c for c in ph.EDGE_CASES if c[0] == S]
        assert {c[3] for c in here} == ({False} if S == 1 else {True, False}), S
    for ab in ph.EDGE_ALPHABETS:
        assert {c[3] for c in ph.EDGE_CASES if c[1:3] == ab} == {True, False}
    assert all(c in ph.EDGE_CASES for c in ph.WITNESS_CASES)
    # 2. the LDS marks: the child's two results are finite
    for S in ph.LDS_TOKEN_STATES:
        em, R, y = ph.lds_token_case(S)
        dp = prefixtree.PrefixDP(em, R)
        root = dp.fill(y)
        child = dp.fill(y, root[0], 1)
        assert all(np.isfinite(v) for v in root[1:] + child[1:]), (S, root[1:], child[1:])
    assert ph.LDS_TOKEN_STATES == (64 * 1024 // 8, 64 * 1024 // 8 + 1)
    for lds in (64 * 1024, 160 * 1024):
        S0 = pph.lds_profile_states(2, lds)
        assert (3 * S0 + 3) * 8 <= lds < (3 * (S0 + 1) + 3) * 8
        for S in (S0, S0 + 1)[:2 if lds == 64 * 1024 else 1]:
            em = ph.lds_machine(S)
            dp = prefixtree.ProfilePrefixDP(em, ph.banded_R(S))
            P = pph.lds_profile(S, 2)
            root = dp.fill(P)
            child = dp.fill(P, root[0], 1)
            assert all(np.isfinite(v) for v in root[1:] + child[1:]), (S, root[1:], child[1:])
    # 3. batches: every root of two symbols or rows and more is finite
    em, ys = ph.batch_case()
    assert (em.nStates, em.nInTok, em.nOutTok) == (40, 3, 5) and [len(y) for y in ys] == list(range(10)) and int(em.silentLevels().max()) > 0
    R = prefixtree.logSumInTrans(em)
    dp, pdp = prefixtree.PrefixDP(em, R), prefixtree.ProfilePrefixDP(em, R)
    profs = pph.batch_profiles()
    assert [len(P) for P in profs] == list(range(10))
    for y, P in zip(ys, profs):
        assert len(y) < 2 or (np.isfinite(dp.fill(y)[1]) and np.isfinite(pdp.fill(P)[1])), len(y)
    # 4. the far column
    em, R, y = ph.far_column_case()
    s, fed = ph.COLUMN_STATE, ph.COLUMN_FED
    for kind, dp, out in (("token", prefixtree.PrefixDP(em, R), y), ("profile", prefixtree.ProfilePrefixDP(em, R), pph.far_column_profile())):
        for p, (cells, lsp, lpp) in _family_refs(dp, out, em.nInTok).items():
            row = cells[1, 1]
            V = dp.columnSums(row)
            terms = row[:, None] + R
            assert np.isfinite(V[s]) and np.isfinite(terms.max()) and terms[:, s].max() <= terms.max() - 800, (kind, p)
            assert math.exp(V[s] - terms.max()) == 0.0                          # what a linear product under one maximum would keep of it
            assert np.isfinite(cells[2, 1, fed]) and np.isfinite(lpp), (kind, p)
            # the cell is fed through V[s] alone: one edge on b, times the row's weight of b against a profile
            into = [(int(q), float(w)) for q, d, o, w in zip(em.src, em.dst, em.outTok, em.logWeight) if d == fed and o == 2]
            assert {q for q, _ in into} == {s}
            extra = 0.0 if kind == "token" else float(out[1][2])
            want = np.logaddexp.reduce([V[s] + w + extra for _, w in into])
            assert abs(cells[2, 1, fed] - want) <= 1e-12 * abs(want), (kind, p, cells[2, 1, fed], want)
            assert lpp == pytest.approx(cells[2, 1, fed], rel=1e-12)          # and the node's prefix probability reads nothing else
    # 5. sparse profiles
    em, _ = ph.edge_case(65, 3, 5, True)
    R = prefixtree.logSumInTrans(em)
    pdp = prefixtree.ProfilePrefixDP(em, R)
    P = pph.sparse_profile(ph.EDGE_L, 5)
    assert 0.25 <= np.isneginf(P[:, 1:]).mean() <= 0.42 and 0.2 <= np.isneginf(P[:, 0]).mean() <= 0.45
    _live_family(_family_refs(pdp, P, 3), 0.5, "sparse")
    P = pph.dead_row_profile(ph.EDGE_L, 5)
    assert np.isneginf(P[pph.DEAD_ROW]).all() and np.isfinite(np.delete(P, pph.DEAD_ROW, 0)).all()
    for p, (cells, lsp, lpp) in _family_refs(pdp, P, 3).items():
        assert lsp == -math.inf and lpp == -math.inf and np.isneginf(cells[pph.DEAD_ROW + 1:]).all(), p
        assert np.isfinite(cells[pph.DEAD_ROW]).mean() >= 0.5, p
    y = ph.edge_case(65, 3, 5, True)[1]
    hot = pph.hard_profile(y, 5)
    assert np.isneginf(hot[:, 0]).all() and (np.isfinite(hot).sum(axis=1) == 1).all()
    _live_family(_family_refs(pdp, hot, 3), 0.5, "one-hot")
    # 6. twins and ties: the best input of every search holds a twin symbol, and on the quantised machine children tie exactly
    for quantised in (False, True):
        em = ph.twin_machine(ph.TWIN_STATES, ph.TWIN_SEED, quantised)
        e = [t for t in ph.machine_edges(em) if t[2] in (1, 2)]
        assert e and [t[:2] + t[3:] for t in e if t[2] == 1] == [t[:2] + t[3:] for t in e if t[2] == 2]
        assert [t[:2] + t[3:] for t in ph.machine_edges(em) if t[2] == 3] != [t[:2] + t[3:] for t in e if t[2] == 1]
        assert int(em.silentLevels().max()) > 0
        if quantised:
            k = em.logWeight / math.log(0.5)
            assert np.abs(k - np.round(k)).max() < 1e-12
        outs = ph.twin_outputs(em, ph.TWIN_SEARCHES, ph.TWIN_L, ph.TWIN_SEED)
        for kw in (dict(outputs=outs), dict(outputs=None, profiles=pph.twin_profiles(em, outs, 0.5 if quantised else 0.8))):
            seqs, trees = prefixtree.decodeBatch(em, kw["outputs"], backend="numpy", profiles=kw.get("profiles"))
            assert all(set(sq) & {"A", "B"} for sq in seqs), seqs
            print("twin searches", quantised, seqs, [t.nFills for t in trees])
            assert max(t.nFills for t in trees) <= 2000
    # 7. the silent self-loop
    em, y = ph.self_loop_case()
    loops = [t for t in ph.machine_edges(em) if t[2] == 0 and t[3] == 0 and t[0] == t[1]]
    assert len(loops) == 1 and loops[0][0] == 0 and int(em.silentLevels().max()) > 0
    _live_family(_family_refs(prefixtree.PrefixDP(em), y, 3), 0.5, "self-loop")
