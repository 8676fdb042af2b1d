"""Decoding against a profile on the device (k_prefix_fill_profile in mb_prefix.hip, docs/decoding.md): node lattices against the
numpy restatement and against the token search on the composite, whole searches and the command line against the numpy backend,
determinism, pool hygiene, rejections."""
import io
import json

import numpy as np
import pytest

from conftest import golden_path
from prefixhelpers import family_paths, populated_machine
from profileprefixhelpers import composite_fills, composite_machine, composite_seq_cells, profile_fills, random_profile
from randmachine import random_seq
from machineboss_amd import boss, capi, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine

pytestmark = pytest.mark.gpu

# Bound on |device - ProfilePrefixDP| / max(1, |ProfilePrefixDP|) over the finite cells.  Measured once per case on an MI355X (the
# table in docs/decoding.md): the worst of the eighteen cases deviates by 4.33e-15 (S = 2000, silent levels, L = 257).  The bound
# is ten times that, the rule of tests/test_prefix_gpu.py.  The deviations are rounding between the device's one-by-one
# log1p(exp()) fold and numpy's max-shifted sum.
CELL_RTOL = 4.33e-14


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_kernel(capi.KERNEL_AUTO)


def _family(em, P, maxNodes=16):
    """(device machine, device store, R, {path: (node, lsp, lpp)}) for the root, its children and one grandchild of each."""
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, maxNodes, profiles=[P])
    nodes = {(): dev.root(0)}
    paths = family_paths(em.nInTok)
    for depth in (1, 2):
        ps = [p for p in paths if len(p) == depth]
        ch, a, b = dev.extend([0] * len(ps), [nodes[p[:-1]][0] for p in ps], [p[-1] for p in ps])
        for p, c, x, z in zip(ps, ch, a, b):
            nodes[p] = (int(c), float(x), float(z))
    return dm, dev, R, nodes


def _worst(got, ref):
    """Worst relative deviation over the finite cells; -inf (and nothing else) must sit where the reference has it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))) if fin.any() else 0.0


@pytest.mark.parametrize("L", [0, 1, 257])
@pytest.mark.parametrize("levels", [True, False])
@pytest.mark.parametrize("S", [8, 300, 2000])
def test_node_cells_against_restatement(S, levels, L):
    """Every cell of both layers of a root, its children and one grandchild each.  At L = 257 every node has a finite logSeqProb
    and logPrefixProb and at least nine tenths of the cells of each layer are finite."""
    em = populated_machine(S, 100 + S, levels)
    assert (int(em.silentLevels().max()) > 0) == levels
    P = random_profile(np.random.RandomState(S + L), L, em.nOutTok)
    dm, dev, R, nodes = _family(em, P)
    ref = profile_fills(em, P, list(nodes), R)
    worst = 0.0
    for p, (node, lsp, lpp) in nodes.items():
        cells, rs, rp = ref[p]
        got = dev.node_cells(node, 0)
        assert got.shape == cells.shape
        worst = max(worst, _worst(got, cells), _worst([lsp, lpp], [rs, rp]))
        if p:
            assert lpp <= nodes[p[:-1]][2] + 1e-12, (p, lpp, nodes[p[:-1]][2])
    total = sum(ref[p][0][:, 0].size for p in nodes)
    fseq = sum(int(np.isfinite(ref[p][0][:, 0]).sum()) for p in nodes)
    fpre = sum(int(np.isfinite(ref[p][0][:, 1]).sum()) for p in nodes)
    print("profile prefix cells S=%d levels=%d L=%d cells/layer=%d finite W=%d X=%d worst relative deviation %.3g" % (
        S, levels, L, total, fseq, fpre, worst))
    dev.close(); dm.close()
    if L == 257:
        assert fseq >= 0.9 * total and fpre >= 0.9 * total
        assert all(np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]) for p in nodes)
    else:
        assert fseq >= 1 and fpre >= 1
    assert worst <= CELL_RTOL


@pytest.mark.parametrize("levels", [True, False])
def test_device_against_token_search_on_the_composite(levels):
    """S = 8, L = 12: the device against PrefixDP on the composite machine with an empty output -- no new numpy code between."""
    finite = 0
    for seed in range(4):
        em = populated_machine(8, seed, levels)
        P = random_profile(np.random.RandomState(1000 + seed), 12, em.nOutTok)
        dm, dev, R, nodes = _family(em, P)
        ref = composite_fills(composite_machine(em, P), list(nodes))
        for p, (node, lsp, lpp) in nodes.items():
            assert _worst([lsp, lpp], ref[p][1:]) <= 1e-9, (p, lsp, lpp, ref[p][1:])
            assert _worst(dev.node_cells(node, 0)[:, 0], composite_seq_cells(ref[p][0], 12, 8)) <= 1e-9
            finite += int(np.isfinite(ref[p][1])) + int(np.isfinite(ref[p][2]))
        dev.close(); dm.close()
    assert finite == 4 * 5 * 2


def test_same_batch_twice_gives_the_same_bits():
    em = populated_machine(300, 5, True)
    P = random_profile(np.random.RandomState(3), 60, em.nOutTok)
    cells = []
    for _ in range(2):
        dm, dev, R, nodes = _family(em, P)
        cells.append({p: (dev.node_cells(n[0], 0).tobytes(), n[1], n[2]) for p, n in nodes.items()})
        dev.close(); dm.close()
    assert cells[0] == cells[1]


def test_profile_and_token_searches_alive_together():
    """A token search and a profile search of the same machine, interleaved: each gives what it gives alone."""
    em = populated_machine(300, 9, True)
    R = prefixtree.logSumInTrans(em)
    y = random_seq(np.random.RandomState(4), 40, em.nOutTok)
    P = random_profile(np.random.RandomState(4), 40, em.nOutTok)
    dm = capi.DeviceMachine(em)

    def family(dev):
        r = dev.root(0)
        ch, a, b = dev.extend([0, 0], [r[0]] * 2, [1, 2])
        return [r[1:]] + list(zip(a.tolist(), b.tolist())), [dev.node_cells(n, 0).tobytes() for n in [r[0]] + list(ch)]

    alone = []
    for kw in ({"outputs": [y]}, {"outputs": None, "profiles": [P]}):
        dev = capi.DevicePrefix(dm, kw["outputs"], R, 8, kw.get("profiles"))
        alone.append(family(dev))
        dev.close()
    tok = capi.DevicePrefix(dm, [y], R, 8)
    pro = capi.DevicePrefix(dm, None, R, 8, [P])
    rt, rp = tok.root(0), pro.root(0)
    ct = tok.extend([0], [rt[0]], [1]); cp = pro.extend([0, 0], [rp[0]] * 2, [1, 2]); ct2 = tok.extend([0], [rt[0]], [2])
    got_t = [dev_cells for dev_cells in (tok.node_cells(n, 0).tobytes() for n in (rt[0], ct[0][0], ct2[0][0]))]
    got_p = [pro.node_cells(n, 0).tobytes() for n in (rp[0], cp[0][0], cp[0][1])]
    assert got_t == alone[0][1] and got_p == alone[1][1]
    assert [rt[1:], (ct[1][0], ct[2][0]), (ct2[1][0], ct2[2][0])] == alone[0][0]
    assert [rp[1:]] + list(zip(cp[1].tolist(), cp[2].tolist())) == alone[1][0]
    assert alone[0][0] != alone[1][0]
    tok.close(); pro.close(); dm.close()


def _dnastore():
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    return m, EvaluatedMachine.fromMachine(m, None, useDefaults=True)


def _dnastore_profiles(m, em, lengths=(2, 3, 4, 5, 6, 7, 8, 9)):
    """Soft versions of the Viterbi encodings of random inputs: 0.86 on the encoded symbol, 0.04 on the others, 0.02 on the
    blank, each jittered by up to a tenth.  One profile per input length, so their row counts differ."""
    rng = np.random.RandomState(5)
    syms = m.inputAlphabet()
    ins = [[syms[k] for k in rng.randint(0, len(syms), n)] for n in lengths]
    profs = []
    for o in boss.viterbiEncode(m, ins, "numpy"):
        y = em.outputTokenizer.tokenize(o)
        W = np.full((len(y), em.nOutTok + 1), 0.04)
        W[:, 0] = 0.02
        W[np.arange(len(y)), y] = 0.86
        profs.append(np.log(W * rng.uniform(0.9, 1.1, W.shape)))
    assert len({len(p) for p in profs}) == len(profs)
    return ins, profs


def test_decode_batch_equals_numpy_backend():
    m, em = _dnastore()
    ins, profs = _dnastore_profiles(m, em)
    want, wt = prefixtree.decodeBatch(em, None, backend="numpy", profiles=profs)
    got, gt = prefixtree.decodeBatch(em, None, backend="device", profiles=profs)
    assert got == want and [t.nFills for t in gt] == [t.nFills for t in wt]
    assert sum(a == b for a, b in zip(got, ins)) >= 6            # the profiles are sharp: most inputs come back
    for a, b in zip(gt, wt):
        assert abs(a.bestLogSeqProb - b.bestLogSeqProb) <= 1e-9 * max(1.0, abs(b.bestLogSeqProb))
    assert all(t.monotone for t in gt)


def test_pool_hygiene():
    m, em = _dnastore()
    _, profs = _dnastore_profiles(m, em)
    prefixtree.decodeBatch(em, None, backend="device", profiles=profs)            # the first search sizes the cached pool
    before = capi.alloc_stats()
    for _ in range(10):
        prefixtree.decodeBatch(em, None, backend="device", profiles=profs)
    after = capi.alloc_stats()
    for k in ("pool_allocs", "pool_frees", "evictions", "bytes_allocated"):
        assert after[k] == before[k], (k, before, after)


def test_full_pool_and_bad_arguments_are_errors():
    m, em = _dnastore()
    _, profs = _dnastore_profiles(m, em)
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, 3, profs[:1])
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
    with pytest.raises(capi.MbError, match="no such search"):
        dev.root(1)
    dev.close()
    for bad in (np.nan, np.inf):
        P = profs[0].copy()
        P[1, 2] = bad
        with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
            capi.DevicePrefix(dm, None, R, 3, [P])
    capi.set_memory_budget(1 << 20)
    try:
        with pytest.raises(capi.MbError, match="memory budget"):
            capi.DevicePrefix(dm, None, R, 100000, profs[:1])
    finally:
        capi.set_memory_budget(0)
    dm.close()


CLI = [(["tests/golden/machine/dnastore4.json", "--use-defaults"], "tiny_uc.csv"),
       (["tests/golden/machine/bitnoise.json", "-P", "tests/golden/io/params.json"], "prof001.csv"),
       (["tests/golden/machine/bitecho.json"], "prof001.csv")]


@pytest.mark.parametrize("mode", ["--prefix-decode", "--viterbi-decode"])
@pytest.mark.parametrize("args,csv", CLI, ids=[c[0][0].split("/")[-1][:-5] + "-" + c[1] for c in CLI])
def test_cli_device_equals_numpy(args, csv, mode):
    outs = []
    for backend in ("device", "numpy"):
        out = io.StringIO()
        assert boss.run(args + ["--recognize-csv", "tests/golden/csv/" + csv, mode, "--decode-backend", backend], out) == 0
        outs.append(json.loads(out.getvalue()))
    assert outs[0] == outs[1]
    assert outs[0][0]["output"] == {"name": "", "sequence": []}
