"""Decoding against a CTC-merged profile on the device (k_prefix_fill_merged in mb_prefix_merge.hip, docs/decoding.md): node lattices
against the numpy restatement at the edges of the lane grouping, the planes and the rows, and against the token search on the
composite; column maps, determinism, batches of different lengths, the three kinds of search alive together, whole searches against
the numpy backend, pool hygiene and the LDS limit."""
import numpy as np
import pytest

import mergeprefixhelpers as mph
from mergeprefixhelpers import family_fills, worst
from prefixhelpers import populated_machine
from profileprefixhelpers import random_profile
from randmachine import random_seq
from machineboss_amd import boss, capi, prefixtree

pytestmark = pytest.mark.gpu

# Bound on |device - MergedProfilePrefixDP| / max(1, |MergedProfilePrefixDP|) over the finite cells and the two results of a node.
# Measured once per case on an MI355X (the table in docs/decoding.md): the worst case deviates by CELL_WORST.  The bound is ten times
# that, the rule of tests/test_prefix_gpu.py and tests/test_prefix_profile_gpu.py.  The deviations are rounding between the device's
# one-by-one log1p(exp()) folds and numpy's max-shifted sums.
CELL_WORST = 3.5e-15          # nCols = 65, S = 2, L = 33
CELL_RTOL = 10 * CELL_WORST

LDS_BYTES = 160 * 1024          # PREFIX_PROFILE_MAX_LDS (mb_prefix.h)


def lds_doubles(S, nCols):
    """merged_prefix_lds_doubles (mb_prefix.h): Y, N, Xn (nCols + 1 planes), three exclusion vectors (nCols planes), two blank
    sums, the row's weights."""
    return (6 * nCols + 5) * S + nCols + 1


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_kernel(capi.KERNEL_AUTO)


def _family(em, P, colTok, maxNodes=16):
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, maxNodes, profiles=[P], colTok=colTok)
    return dm, dev, R, family_fills(dev, em.nInTok)


def _check_family(em, P, colTok, tag, populated):
    """Both layers of the root, its children and one grandchild each against the restatement."""
    dm, dev, R, nodes = _family(em, P, colTok)
    ref = mph.merged_fills(em, P, colTok, list(nodes), R)
    dev_worst = 0.0
    for p, (node, lsp, lpp) in nodes.items():
        cells, rs, rp = ref[p]
        got = dev.node_cells(node, 0)
        assert got.shape == cells.shape == (len(P) + 1, 2, len(colTok) + 1, em.nStates)
        dev_worst = max(dev_worst, worst(got, cells), worst([lsp, lpp], [rs, rp]))
        if p:
            assert lpp <= nodes[p[:-1]][2] + 1e-12, (p, lpp, nodes[p[:-1]][2])
    total = sum(ref[p][0][:, 0].size for p in nodes)
    fW = sum(int(np.isfinite(ref[p][0][:, 0]).sum()) for p in nodes)
    fX = sum(int(np.isfinite(ref[p][0][:, 1]).sum()) for p in nodes)
    print("merged prefix cells %s cells/layer=%d finite W=%d X=%d worst relative deviation %.3g" % (tag, total, fW, fX, dev_worst))
    dev.close(); dm.close()
    if populated:
        assert 10 * fW >= 9 * total and 10 * fX >= 9 * total, (fW, fX, total)
        assert all(np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]) for p in nodes)
    else:
        assert fW >= 1 and fX >= 1
    assert dev_worst <= CELL_RTOL, dev_worst


@pytest.mark.parametrize("L", mph.LANE_ROWS)
@pytest.mark.parametrize("nCols,S", mph.LANE_CASES)
def test_node_cells_against_restatement(nCols, S, L):
    """Idle lanes (1, 1), (2, 1); the first state stride within a plane group (4, 204) / (4, 205); 64, 65 and 66 planes across
    wavefront boundaries.  L = 1: the first and last row coincide; L = 2: the first repeat."""
    em, colTok, P = mph.lane_case(nCols, S, L)
    _check_family(em, P, colTok, "nCols=%d S=%d L=%d" % (nCols, S, L), populated=L >= 33)


@pytest.mark.parametrize("levels", [True, False])
def test_node_cells_with_and_without_silent_levels(levels):
    em, colTok, P = mph.levels_case(levels)
    assert (int(em.silentLevels().max()) > 0) == levels and em.nStates == 300 and len(P) == 65
    _check_family(em, P, colTok, "nCols=4 S=300 L=65 levels=%d" % levels, populated=True)


@pytest.mark.parametrize("name", ["two", "same", "unused", "one"])
def test_column_maps(name):
    em, colTok, P = mph.column_map_cases()[name]
    assert em.nStates == 40 and len(P) == 20
    _check_family(em, P, colTok, "column map %s" % name, populated=False)


def test_device_against_token_search_on_the_composite():
    """S = 8, nCols = 2, L = 6: the device against PrefixDP on algebra.compose(M, merging recogniser) with an empty output -- no new
    numpy code between."""
    finite = total = 0
    for seed in range(4):
        M, em = mph.named_machine(populated_machine(8, seed, True))
        prof = mph.two_column_profile(np.random.RandomState(500 + seed), em, 6)
        P, colTok = prof.mergeRows(em)
        assert len(colTok) == 2 and len(P) == 6
        C, cellOf = mph.merged_composite(M, em, prof)
        dm, dev, R, nodes = _family(em, P, colTok)
        ref = mph.composite_fills(C, em, list(nodes))
        for p, (node, lsp, lpp) in nodes.items():
            assert worst([lsp, lpp], ref[p][1:]) <= 1e-9, (p, lsp, lpp, ref[p][1:])
            want, have, last, haveLast = mph.composite_w_cells(ref[p][0], cellOf, 6, 3, 8)
            W = dev.node_cells(node, 0)[:, 0]
            assert worst(W[:6][have[:6]], want[:6][have[:6]]) <= 1e-9
            assert worst(np.logaddexp.reduce(W[6], axis=0)[haveLast], last[haveLast]) <= 1e-9
            finite += int(np.isfinite(ref[p][1])) + int(np.isfinite(ref[p][2])); total += 2
        dev.close(); dm.close()
    assert finite == total == 4 * 5 * 2


def test_same_batch_twice_gives_the_same_bits():
    em = populated_machine(300, 5, True)
    P = mph.live_rows(np.random.RandomState(3), 4, 60, zeros=0.05)
    cells = []
    for _ in range(2):
        dm, dev, R, nodes = _family(em, P, [1, 2, 1, 2])
        cells.append({p: (dev.node_cells(n[0], 0).tobytes(), n[1], n[2]) for p, n in nodes.items()})
        dev.close(); dm.close()
    assert cells[0] == cells[1]
    assert all(np.isfinite(v[1]) and np.isfinite(v[2]) for v in cells[0].values())


def test_one_extend_over_searches_of_different_lengths():
    """Searches of 2..9 rows in one store: one extend over all of them gives, bit for bit, what each search gives alone."""
    em = populated_machine(40, 7, True)
    colTok = [1, 2, 2]
    profs = [mph.live_rows(np.random.RandomState(20 + L), 3, L, zeros=0.05) for L in range(2, 10)]
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    alone = []
    for P in profs:
        dev = capi.DevicePrefix(dm, None, R, 4, profiles=[P], colTok=colTok)
        r = dev.root(0)
        ch, a, b = dev.extend([0, 0], [r[0]] * 2, [1, 2])
        alone.append((r[1:], a.tolist(), b.tolist(), [dev.node_cells(n, 0).tobytes() for n in [r[0]] + list(ch)]))
        dev.close()
    dev = capi.DevicePrefix(dm, None, R, 3 * len(profs), profiles=profs, colTok=colTok)
    roots = [dev.root(k) for k in range(len(profs))]
    seq = [k for k in range(len(profs)) for _ in (1, 2)]
    ch, a, b = dev.extend(seq, [roots[k][0] for k in seq], [1, 2] * len(profs))
    for k in range(len(profs)):
        got = (roots[k][1:], a[2 * k:2 * k + 2].tolist(), b[2 * k:2 * k + 2].tolist(),
               [dev.node_cells(n, k).tobytes() for n in [roots[k][0]] + list(ch[2 * k:2 * k + 2])])
        assert got == alone[k], k
    assert all(np.isfinite(x[0][1]) for x in alone)
    dev.close(); dm.close()


def test_three_kinds_of_search_alive_together():
    """A token search, a plain-profile search and a merged search on one machine, interleaved: each gives what it gives alone."""
    em = populated_machine(300, 9, True)
    R = prefixtree.logSumInTrans(em)
    y = random_seq(np.random.RandomState(4), 40, em.nOutTok)
    P = random_profile(np.random.RandomState(4), 40, em.nOutTok)
    Pm = mph.live_rows(np.random.RandomState(4), 3, 40, zeros=0.05)
    kinds = [dict(outputs=[y]), dict(outputs=None, profiles=[P]), dict(outputs=None, profiles=[Pm], colTok=[1, 2, 1])]
    dm = capi.DeviceMachine(em)

    def make(kw):
        return capi.DevicePrefix(dm, kw["outputs"], R, 8, kw.get("profiles"), kw.get("colTok"))

    def snapshot(dev, nodes, results):
        return [dev.node_cells(n, 0).tobytes() for n in nodes], results

    alone = []
    for kw in kinds:
        dev = make(kw)
        r = dev.root(0)
        c1 = dev.extend([0], [r[0]], [1]); c2 = dev.extend([0], [r[0]], [2])
        alone.append(snapshot(dev, [r[0], c1[0][0], c2[0][0]], [r[1:], (c1[1][0], c1[2][0]), (c2[1][0], c2[2][0])]))
        dev.close()
    devs = [make(kw) for kw in kinds]
    roots = [d.root(0) for d in devs]
    first = [d.extend([0], [r[0]], [1]) for d, r in zip(devs, roots)]
    second = [d.extend([0], [r[0]], [2]) for d, r in reversed(list(zip(devs, roots)))][::-1]
    for k, d in enumerate(devs):
        got = snapshot(d, [roots[k][0], first[k][0][0], second[k][0][0]],
                       [roots[k][1:], (first[k][1][0], first[k][2][0]), (second[k][1][0], second[k][2][0])])
        assert got == alone[k], k
        d.close()
    assert alone[0][1] != alone[1][1] and alone[1][1] != alone[2][1]
    dm.close()


def test_decode_batch_equals_numpy_backend():
    m, em, colTok, ins, profs = mph.dnastore_merged_profiles()
    want, wt = prefixtree.decodeBatch(em, None, backend="numpy", profiles=profs, colTok=colTok)
    got, gt = prefixtree.decodeBatch(em, None, backend="device", profiles=profs, colTok=colTok)
    assert got == want and [t.nFills for t in gt] == [t.nFills for t in wt]
    assert sum(a == b for a, b in zip(got, ins)) >= 6
    for a, b in zip(gt, wt):
        assert abs(a.bestLogSeqProb - b.bestLogSeqProb) <= 1e-9 * max(1.0, abs(b.bestLogSeqProb))
    assert all(t.monotone for t in gt)
    assert boss.prefixDecodeProfile(m, (profs[3], colTok), "device", merge=True) == boss.prefixDecodeProfile(m, (profs[3], colTok), "numpy", merge=True)


def test_pool_hygiene():
    m, em, colTok, _, profs = mph.dnastore_merged_profiles()
    prefixtree.decodeBatch(em, None, backend="device", profiles=profs, colTok=colTok)            # the first search sizes the cached pool
    before = capi.alloc_stats()
    for _ in range(10):
        prefixtree.decodeBatch(em, None, backend="device", profiles=profs, colTok=colTok)
    after = capi.alloc_stats()
    for k in ("pool_allocs", "pool_frees", "evictions", "bytes_allocated"):
        assert after[k] == before[k], (k, before, after)


def test_full_pool_and_bad_arguments_are_errors():
    m, em, colTok, _, profs = mph.dnastore_merged_profiles()
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, 3, profs[:1], colTok)
    r = dev.root(0)
    with pytest.raises(capi.MbError, match="pool is full"):
        dev.extend([0] * 3, [r[0]] * 3, [1, 2, 3])
    assert dev.free_nodes() == 2                                   # a refused call takes nothing
    dev.close()
    for bad in (np.nan, np.inf):
        P = profs[0].copy()
        P[1, 2] = bad
        with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
            capi.DevicePrefix(dm, None, R, 3, [P], colTok)
    for bad in ([0, 1, 2, 3], [1, 2, 3, em.nOutTok + 1]):
        with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
            capi.DevicePrefix(dm, None, R, 3, profs[:1], bad)
    with pytest.raises(capi.MbError, match="columns"):
        capi.DevicePrefix(dm, None, R, 3, [np.zeros((2, 1))], [])
    capi.set_memory_budget(1 << 20)
    try:
        with pytest.raises(capi.MbError, match="memory budget"):
            capi.DevicePrefix(dm, None, R, 100000, profs[:1], colTok)
    finally:
        capi.set_memory_budget(0)
    dm.close()


def test_lds_limit():
    """The largest machine the documented formula admits at nCols = 4 fills correctly (the root and one child, L = 3); one state
    more is the error, and nothing is launched."""
    nCols = 4
    S = (LDS_BYTES // 8 - (nCols + 1)) // (6 * nCols + 5)
    assert lds_doubles(S, nCols) * 8 <= LDS_BYTES < lds_doubles(S + 1, nCols) * 8
    em, colTok, P = mph.lds_case(S)
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, 2, profiles=[P], colTok=colTok)
    root = dev.root(0)
    ch, a, b = dev.extend([0], [root[0]], [1])
    ref = mph.merged_fills(em, P, colTok, [(), (1,)], R)
    dev_worst = max(worst(dev.node_cells(root[0], 0), ref[()][0]), worst(root[1:], ref[()][1:]),
                    worst(dev.node_cells(int(ch[0]), 0), ref[(1,)][0]), worst([a[0], b[0]], ref[(1,)][1:]))
    print("merged prefix cells at the LDS limit S=%d worst relative deviation %.3g" % (S, dev_worst))
    assert np.isfinite(ref[(1,)][1]) and np.isfinite(ref[(1,)][2])
    dev.close(); dm.close()
    em1, colTok, P = mph.lds_case(S + 1)
    dm = capi.DeviceMachine(em1)
    before = capi.alloc_stats()
    with pytest.raises(capi.MbError, match="\\(6 nCols \\+ 5\\) x states \\+ nCols \\+ 1"):          # no object, so nothing to launch on
        capi.DevicePrefix(dm, None, prefixtree.logSumInTrans(em1), 2, profiles=[P], colTok=colTok)
    assert capi.alloc_stats() == before
    dm.close()
    assert dev_worst <= CELL_RTOL, dev_worst
