"""Prefix search on the device (mb_prefix.hip, docs/decoding.md): node lattices against the numpy restatement, seq cells against
the library's own Forward, the command-line goldens and the lock-step driver on the device backend, determinism, pool hygiene."""
import io
import json
import math

import numpy as np
import pytest

from conftest import golden_path, load_json
from prefixhelpers import family_paths, populated_machine
from randmachine import random_seq
from machineboss_amd import algebra, boss, capi, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine

pytestmark = pytest.mark.gpu

# Bound on |device - PrefixDP| / max(1, |PrefixDP|) over the finite cells.  Measured once per case on an MI355X (the table in
# docs/decoding.md): the worst of the eighteen cases deviates by 4.71e-15 (S = 2000, silent levels, L = 257).  The bound is ten times
# that, far inside the 1e-9 this project publishes for Forward.
CELL_RTOL = 4.71e-14


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_kernel(capi.KERNEL_AUTO)


def _family(em, y):
    """(device machine, device store, R, {path: (node, lsp, lpp)}) for the root, its children and one grandchild of each."""
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, [y], R, 16)
    nodes = {(): dev.root(0)}
    paths = family_paths(em.nInTok)
    for depth in (1, 2):
        ps = [p for p in paths if len(p) == depth]
        ch, a, b = dev.extend([0] * len(ps), [nodes[p[:-1]][0] for p in ps], [p[-1] for p in ps])
        for p, c, x, z in zip(ps, ch, a, b):
            nodes[p] = (int(c), float(x), float(z))
    return dm, dev, R, nodes


def _reference(em, R, y, paths):
    dp = prefixtree.PrefixDP(em, R)
    out = {}
    for p in sorted(paths, key=len):
        out[p] = dp.fill(y) if not p else dp.fill(y, out[p[:-1]][0], p[-1])
    return out


def _worst(got, ref):
    """Worst relative deviation over the finite cells; -inf (and nothing else) must sit where the reference has it."""
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))) if fin.any() else 0.0


@pytest.mark.parametrize("L", [0, 1, 257])
@pytest.mark.parametrize("levels", [True, False])
@pytest.mark.parametrize("S", [8, 300, 2000])
def test_node_cells_against_restatement(S, levels, L):
    """Every cell of a root, its children and one grandchild each.  The machines (prefixhelpers.populated_machine) fill their
    lattices and have a convergent (I - N)^-1, so the prefix layer is a probability mass and must not grow from parent to child.
    Floors on what is compared: at L = 257 four fifths of the seq cells and of the prefix cells are finite and every node has a
    finite logSeqProb and logPrefixProb; at L <= 1 a machine without silent edges can only hold what its inserting edges reach
    from the start state, so there the floor is the root's cell and one more per layer."""
    em = populated_machine(S, 100 + S, levels)
    assert (int(em.silentLevels().max()) > 0) == levels
    y = random_seq(np.random.RandomState(S + L), L, em.nOutTok)
    dm, dev, R, nodes = _family(em, y)
    ref = _reference(em, R, y, nodes)
    worst, span = 0.0, 0.0
    for p, (node, lsp, lpp) in nodes.items():
        cells, rs, rp = ref[p]
        got = dev.node_cells(node, 0)
        worst = max(worst, _worst(got, cells), _worst(np.array([lsp, lpp]), np.array([rs, rp])))
        for row in cells[:, 1]:
            if np.isfinite(row).any():
                span = max(span, float(np.ptp(row[np.isfinite(row)])))
        if p:
            assert lpp <= nodes[p[:-1]][2] + 1e-12, (p, lpp, nodes[p[:-1]][2])
    total = sum(ref[p][0][:, 0].size for p in nodes)
    fseq = sum(int(np.isfinite(ref[p][0][:, 0]).sum()) for p in nodes)
    fpre = sum(int(np.isfinite(ref[p][0][:, 1]).sum()) for p in nodes)
    print("prefix cells S=%d levels=%d L=%d cells/layer=%d finite seq=%d prefix=%d widest prefix row %.0f nats worst relative deviation %.3g" % (
        S, levels, L, total, fseq, fpre, span, worst))
    dev.close(); dm.close()
    if L == 257:
        assert fseq >= 0.8 * total and fpre >= 0.8 * total
        assert all(np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]) for p in nodes)
    else:
        assert fseq >= 2 and fpre >= 2
    assert worst <= CELL_RTOL


def test_seq_cells_equal_forward_batch():
    """seq[L][S-1] of a node is the Forward likelihood of (its input prefix, y): the prefix kernel against the generic Forward
    kernel, both exact log-sum-exp in fp64 -- 1e-9 relative, the Forward figure of the README.  With and without silent levels;
    every one of the twenty likelihoods compared must be finite."""
    capi.set_kernel(capi.KERNEL_GENERIC)
    finite = 0
    try:
        for S, L, levels in ((8, 5, True), (300, 40, True), (8, 12, False), (300, 40, False)):
            em = populated_machine(S, 7 + S, levels)
            y = random_seq(np.random.RandomState(L), L, em.nOutTok)
            dm, dev, R, nodes = _family(em, y)
            paths = list(nodes)
            ll = capi.DeviceBatch.from_pairs(dm, [(np.array(p, np.int32), y) for p in paths]).forward(capi.MB_MATERIALISE)
            for p, f in zip(paths, ll):
                lsp = nodes[p][1]
                assert (lsp == f) if not np.isfinite(f) else abs(lsp - f) <= 1e-9 * max(1.0, abs(f)), (p, lsp, f)
                finite += bool(np.isfinite(f))
            dev.close(); dm.close()
    finally:
        capi.set_kernel(capi.KERNEL_AUTO)
    assert finite == 20


def _boss(*args):
    out = io.StringIO()
    assert boss.run(list(args) + ["--decode-backend", "device"], out) == 0
    return json.loads(out.getvalue())


HAMMING_IN = "0000000100100011010001010110011110001001101010111100110111101111"
CLI = [
    (["M:bitecho", "--recognize-chars", "101", "--prefix-decode"], "decode-bitecho-101.json"),
    (["M:bitecho", "--recognize-chars", "101", "--viterbi-decode"], "decode-bitecho-101.json"),
    (["--generate-chars", "101", "M:bintern", "--prefix-encode"], "encode-g101-bintern.json"),
    (["--input-chars", "101", "M:bintern", "--prefix-encode"], "encode-i101-bintern.json"),
    (["M:bintern", "--recognize-chars", "12222", "--prefix-decode"], "decode-a12222-bintern.json"),
    (["M:bintern", "--output-chars", "12222", "--prefix-decode"], "decode-o12222-bintern.json"),
    (["--preset", "hamming74", "--viterbi-encode", "--input-chars", HAMMING_IN], "hamming74.json"),
    (["--preset", "hamming74", "--prefix-encode", "--input-chars", HAMMING_IN], "hamming74.json"),
    # the reference tests this file under --beam-decode only.  What backs it here: the numpy search (tests/test_prefix_host.py)
    # and the Viterbi path through the existing, oracle-checked Viterbi read the same symbols
    (["M:dnastore4", "--output-chars", "AGTAGTAG", "--prefix-decode"], "dnastore-decode.json"),
    (["M:dnastore4", "--output-chars", "AGTAGTAG", "--viterbi-decode"], "dnastore-decode.json"),
]


@pytest.mark.parametrize("args,expect", CLI, ids=[" ".join(a[:4])[:60] for a, _ in CLI])
def test_cli_goldens_on_device(args, expect):
    args = [golden_path("machine", a[2:] + ".json") if a.startswith("M:") else a for a in args]
    assert _boss(*args) == load_json("expect", expect)


def _dnastore():
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    return m, EvaluatedMachine.fromMachine(m, None, useDefaults=True)


def _dnastore_outputs(m, n=64, length=8):
    """n DIFFERENT decodable outputs: the Viterbi encodings of random inputs (the numpy route of --viterbi-encode)."""
    rng = np.random.RandomState(11)
    syms = m.inputAlphabet()
    outs = []
    while len(outs) < n:
        ins = [[syms[k] for k in rng.randint(0, len(syms), length)] for _ in range(n)]
        for o in boss.viterbiEncode(m, ins, "numpy"):
            if o not in outs and len(outs) < n:
                outs.append(o)
    assert len({tuple(o) for o in outs}) == n
    return outs


def test_lock_step_batch_equals_single_searches():
    m, em = _dnastore()
    outs = _dnastore_outputs(m)
    seqs, trees = prefixtree.decodeBatch(em, outs, backend="device")
    for k, o in enumerate(outs):
        t = prefixtree.PrefixTree.forOutput(em, o, backend="device")
        assert t.doPrefixSearch() == seqs[k]
        assert t.nFills == trees[k].nFills, (k, t.nFills, trees[k].nFills)     # the same search order, fill for fill
        assert t.bestLogSeqProb == trees[k].bestLogSeqProb
        t.close()
    assert all(t.monotone for t in trees)


def test_same_batch_twice_gives_the_same_bits():
    m, em = _dnastore()
    outs = _dnastore_outputs(m, 16)
    runs = []
    for _ in range(2):
        seqs, trees = prefixtree.decodeBatch(em, outs, backend="device")
        runs.append((seqs, [(t.bestLogSeqProb, t.root.logPrefixProb, t.root.logSeqProb, t.nFills) for t in trees]))
    assert runs[0] == runs[1]
    em2 = populated_machine(300, 5, True)
    y = random_seq(np.random.RandomState(3), 60, em2.nOutTok)
    cells = []
    for _ in range(2):
        dm, dev, R, nodes = _family(em2, y)
        cells.append({p: (dev.node_cells(n[0], 0).tobytes(), n[1], n[2]) for p, n in nodes.items()})
        dev.close(); dm.close()
    assert cells[0] == cells[1]


def test_pool_hygiene():
    m, em = _dnastore()
    outs = _dnastore_outputs(m, 8)
    prefixtree.decodeBatch(em, outs, backend="device")            # the first search sizes the cached pool
    before = capi.alloc_stats()
    for _ in range(10):
        prefixtree.decodeBatch(em, outs, backend="device")
    after = capi.alloc_stats()
    for k in ("pool_allocs", "pool_frees", "evictions", "bytes_allocated"):
        assert after[k] == before[k], (k, before, after)


def test_full_pool_and_bad_handles_are_errors():
    m, em = _dnastore()
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    y = em.outputTokenizer.tokenize(list("AGTAG"))
    dev = capi.DevicePrefix(dm, [y], R, 3)
    r = dev.root(0)
    with pytest.raises(capi.MbError, match="pool is full"):
        dev.extend([0] * 3, [r[0]] * 3, [1, 2, 3])
    assert dev.free_nodes() == 2                                   # a refused call takes nothing
    ch, _, _ = dev.extend([0, 0], [r[0]] * 2, [1, 2])
    dev.release([ch[0]])
    with pytest.raises(capi.MbError, match="not live"):
        dev.release([ch[0]])
    with pytest.raises(capi.MbError, match="not a live node"):
        dev.extend([0], [ch[0]], [1])
    with pytest.raises(capi.MbError, match="input token"):
        dev.extend([0], [r[0]], [em.nInTok + 1])
    dev.close()
    capi.set_memory_budget(1 << 20)
    try:
        with pytest.raises(capi.MbError, match="memory budget"):
            capi.DevicePrefix(dm, [y], R, 100000)
    finally:
        capi.set_memory_budget(0)
    dm.close()
