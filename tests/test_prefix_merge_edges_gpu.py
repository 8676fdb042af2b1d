"""The merged node fill of the prefix search (k_prefix_fill_merged in mb_prefix_merge.hip, docs/decoding.md) at its edges: the LDS
marks, 601 to 1 501 planes (a lane alone on a plane, idle lanes, several planes per lane in every phase), alphabets of different
sizes, dead blanks, dead columns and a dead row, a column of the Y product 850 nats below its row, twin symbols and exact ties, a
silent self-loop, searches of 0 to 9 rows in one store, slot reuse, and one extend of more fills than workgroups can be resident.
The yardstick is prefixtree.MergedProfilePrefixDP (mergeprefixhelpers.merged_fills); the inputs come from mergeprefixhelpers.py, and
tests/test_prefix_merge_host.py::test_edge_suite_inputs_are_live holds them to the liveness conditions asserted here without a
GPU."""
import math

import numpy as np
import pytest

import mergeprefixhelpers as mph
import prefixhelpers as ph
from mergeprefixhelpers import worst
from prefixhelpers import family_paths
from machineboss_amd import capi, prefixtree

pytestmark = pytest.mark.gpu

# Bound on |device - MergedProfilePrefixDP| / max(1, |MergedProfilePrefixDP|) over the finite cells and the two results of a node.
# Measured once per case on an MI355X (the table in docs/decoding.md, "Edges of the merged fill"): the worst case deviates by
# CELL_WORST.  The bound is ten times that, the rule of tests/test_prefix_merge_gpu.py and tests/test_prefix_edges_gpu.py; no bound
# here may exceed the 1e-9 this project publishes.  The worst case is a fold over 1 024 planes: the exclusion vectors and the blank
# sums take one log1p(exp()) per plane, where numpy shifts by the maximum and takes one logarithm; up to 66 planes the figure is 3.5e-15.
CELL_WORST = 1.30e-14          # nCols = 1 024, S = 1, L = 3
CELL_RTOL = 10 * CELL_WORST

LDS_DEFAULT, LDS_BYTES = 64 * 1024, 160 * 1024          # what a kernel may use unasked, and PREFIX_PROFILE_MAX_LDS (mb_prefix.h)


def lds_bytes(S, nCols):
    """merged_prefix_lds_doubles (mb_prefix.h), in bytes."""
    return 8 * ((6 * nCols + 5) * S + nCols + 1)


def test_bound_stays_inside_the_published_figure():
    assert CELL_RTOL <= 1e-9


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_kernel(capi.KERNEL_AUTO)


def _device_family(dev, paths, seq=0):
    """{path: (node, lsp, lpp)}: the root, then one extend per depth."""
    nodes = {(): dev.root(seq)}
    for depth in sorted({len(p) for p in paths if p}):
        ps = [p for p in paths if len(p) == depth]
        ch, a, b = dev.extend([seq] * len(ps), [nodes[p[:-1]][0] for p in ps], [p[-1] for p in ps])
        for p, c, x, z in zip(ps, ch, a, b):
            nodes[p] = (int(c), float(x), float(z))
    return nodes


def _compare_family(em, P, colTok, tag, R=None, paths=None, floor=0.5, live=True):
    """Every cell of both layers and both results of the family (family_paths unless ``paths``) against the yardstick, -inf exactly
    where the yardstick has it.  Returns (worst deviation, device family as {path: (cells, lsp, lpp)}, yardstick family)."""
    R = prefixtree.logSumInTrans(em) if R is None else R
    paths = family_paths(em.nInTok) if paths is None else paths
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, len(paths), profiles=[P], colTok=colTok)
    nodes = _device_family(dev, paths)
    ref = mph.merged_fills(em, P, colTok, paths, R)
    dev_worst, got = 0.0, {}
    for p, (node, lsp, lpp) in nodes.items():
        cells = dev.node_cells(node, 0)
        assert cells.shape == ref[p][0].shape == (len(P) + 1, 2, len(colTok) + 1, em.nStates)
        got[p] = (cells, lsp, lpp)
        dev_worst = max(dev_worst, worst(cells, ref[p][0]), worst([lsp, lpp], ref[p][1:]))
    dev.close(); dm.close()
    total = sum(ref[p][0][:, 0].size for p in ref)
    fin = [sum(int(np.isfinite(ref[p][0][:, k]).sum()) for p in ref) for k in (0, 1)]
    print("merged prefix edges %s cells/layer=%d finite W=%d X=%d worst relative deviation %.3g" % (tag, total, fin[0], fin[1], dev_worst))
    if live:
        assert all(np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]) for p in ref), tag
        assert fin[0] >= floor * total and fin[1] >= floor * total, (tag, fin, total)
    return dev_worst, got, ref


# ---- 9. the LDS marks (first in the module: a process that has opted in cannot be told from one that has not) ---------------------
@pytest.mark.parametrize("S", list(mph.LDS_MARK_STATES) + [mph.LDS_MARK_STATES[0]], ids=["below", "above", "limit", "below-again"])
def test_fill_at_the_lds_marks(S):
    """nCols = 4, 29 S + 5 doubles of LDS: the last machine within 64 KiB, the first past it (the launcher asks once for more), the
    last within 160 KiB, and the first again once the launcher has asked.  The root and the child by symbol 1; correctness only,
    since no output depends on the call itself (docs/decoding.md)."""
    lo, hi, top = mph.LDS_MARK_STATES
    assert lds_bytes(lo, 4) == 65464 <= LDS_DEFAULT < lds_bytes(hi, 4) == 65696 and hi == lo + 1
    assert lds_bytes(top, 4) <= LDS_BYTES < lds_bytes(top + 1, 4)
    em, colTok, P = mph.lds_case(S)
    dev_worst, _, ref = _compare_family(em, P, colTok, "LDS S=%d" % S, paths=[(), (1,)], live=False)
    assert all(np.isfinite(v) for p in ref for v in ref[p][1:])
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 1. many planes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S,L", mph.PLANE_CASES)
def test_many_planes(nCols, S, L):
    """601 planes: LPP = 1 and the lanes from 601 to 639 idle; 1 024 and 1 025: the workgroup exactly full, and the first lane with
    a second plane; 1 031 and 1 501 planes: several planes per lane in the Y product, the exclusion vectors, the middle phase and
    the silent levels, with 104.7 and 152.4 KiB of LDS.  Columns on three tokens in turn, a tenth of the weights -inf; every result
    finite and at least half of each layer.  From 1 024 columns on the root, one child and one grandchild only: the yardstick
    takes a second per node per 1 000 planes."""
    em, colTok, P = mph.lane_case(nCols, S, L)
    assert colTok == [1 + c % 3 for c in range(nCols)] and em.nOutTok == 3 and len(P) == L
    if nCols >= 1030:
        assert LDS_DEFAULT < lds_bytes(S, nCols) <= LDS_BYTES
    dev_worst, _, _ = _compare_family(em, P, colTok, "planes nCols=%d S=%d L=%d" % (nCols, S, L), paths=mph.plane_paths(nCols))
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 2. alphabets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,nIn,nOut,levels", mph.ALPHABET_CASES)
def test_alphabets_of_different_sizes(S, nIn, nOut, levels):
    """nIn != nOut: the strides C = nOut + 1 and K = (nIn + 1)(nOut + 1) come from different alphabets.  2 nOut - 1 columns, 33
    rows without -inf; every result finite and three quarters of each layer."""
    em, colTok, P = mph.alphabet_case(S, nIn, nOut, levels)
    assert (em.nStates, em.nInTok, em.nOutTok) == (S, nIn, nOut) and (int(em.silentLevels().max()) > 0) == levels
    assert len(colTok) == 2 * nOut - 1 and P.shape == (33, 2 * nOut) and np.isfinite(P).all()
    dev_worst, _, _ = _compare_family(em, P, colTok, "alphabets S=%d nIn=%d nOut=%d levels=%d" % (S, nIn, nOut, levels), floor=0.75)
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 3. dead weights --------------------------------------------------------------------------------------------------------------
def test_a_third_of_the_weights_dead_the_blank_included():
    """Rows whose blank is -inf skip the blank sums (the p == 0 branch of the exclusion phase) and leave bN / bXn from an earlier
    row behind; a dead column leaves its eP / eW / eY behind.  A live blank after a dead one must not read them."""
    em, P = mph.batch_machine(), mph.sparse_rows()
    dead = np.isneginf(P[:, 0])
    assert dead.any() and (dead[:-1] & ~dead[1:]).any() and not np.isneginf(P).all(axis=1).any()
    dev_worst, _, _ = _compare_family(em, P, mph.DEAD_COLTOK, "a third of the weights dead")
    assert dev_worst <= CELL_RTOL, dev_worst


def test_a_dead_row():
    """Row 16 is -inf throughout: every cell past it and both results of every node are -inf exactly, the rows up to it are
    not."""
    em, P = mph.batch_machine(), mph.dead_row_rows()
    dev_worst, got, ref = _compare_family(em, P, mph.DEAD_COLTOK, "dead row", live=False)
    for p, (cells, lsp, lpp) in got.items():
        assert lsp == -math.inf and lpp == -math.inf and np.isneginf(cells[mph.DEAD_ROW + 1:]).all(), p
        assert np.isfinite(ref[p][0][:mph.DEAD_ROW + 1]).mean() >= 0.5 and np.isfinite(ref[p][0][mph.DEAD_ROW]).mean() >= 0.5
    assert dev_worst <= CELL_RTOL, dev_worst


def test_every_blank_dead():
    """66 planes, S = 2, 6 rows, the blank of every row -inf: the blank sums are never formed and never read."""
    em, colTok, P = mph.dead_blank_case()
    assert np.isneginf(P[:, 0]).all() and len(P) == 6
    dev_worst, _, _ = _compare_family(em, P, colTok, "every blank dead")
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 4. the column 850 nats down --------------------------------------------------------------------------------------------------
def test_a_column_fed_only_from_far_below_the_row_maximum():
    """pxm_column stays in log space: in prefixhelpers.far_column_case column 3 of the product receives terms 850 nats and more
    below the row's largest, the only way into the end state runs through it, and logPrefixProb reads that one cell.  A linear
    product under the row maximum returns -inf here."""
    em, R, _ = ph.far_column_case()
    dev_worst, got, ref = _compare_family(em, mph.far_column_rows(), [1, 2], "far column", R=R, live=False)
    for p, (cells, lsp, lpp) in got.items():
        assert np.isfinite(ref[p][2]) and ref[p][2] < -850, (p, ref[p][2])
        assert np.isfinite(lpp) and lpp < -850, (p, lpp)
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 5. twins and ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [False, True])
def test_twin_symbols_give_identical_children(quantised):
    """Input symbols 1 and 2 have the same edges with the same weights in the same order: their children of the root and of a
    child are the same bits, cells and results, as the yardstick's are; symbol 3's are not.  All against the yardstick."""
    em = ph.twin_machine(ph.TWIN_STATES, ph.TWIN_SEED, quantised)
    P = mph.twin_merged_profiles(em, quantised)[0]
    paths = [(), (1,), (2,), (3,), (2, 1), (2, 2), (2, 3)]
    dev_worst, got, ref = _compare_family(em, P, mph.TWIN_COLTOK, "twins quantised=%d" % quantised, paths=paths, live=False)
    for fam in (got, ref):
        for a, b, c in (((1,), (2,), (3,)), ((2, 1), (2, 2), (2, 3))):
            assert fam[a][0].tobytes() == fam[b][0].tobytes() and fam[a][1:] == fam[b][1:], (a, b)
            assert fam[a][0].tobytes() != fam[c][0].tobytes() and np.isfinite(fam[a][2])
    assert dev_worst <= CELL_RTOL, dev_worst


@pytest.mark.parametrize("quantised", [False, True])
def test_searches_break_ties_as_the_numpy_backend_does(quantised):
    """Whole searches on the twin machine, whose best inputs hold a twin symbol, and on its quantised version against profiles
    whose weights are multiples of log 0.5 too, where different paths tie exactly: the device backend returns the strings and the
    fill counts of the numpy backend."""
    em = ph.twin_machine(ph.TWIN_STATES, ph.TWIN_SEED, quantised)
    profs = mph.twin_merged_profiles(em, quantised)
    want, wt = prefixtree.decodeBatch(em, None, backend="numpy", profiles=profs, colTok=mph.TWIN_COLTOK)
    got, gt = prefixtree.decodeBatch(em, None, backend="device", profiles=profs, colTok=mph.TWIN_COLTOK)
    assert all(set(s) & {"A", "B"} for s in want)
    for k, (a, b) in enumerate(zip(gt, wt)):
        print("merged prefix edges ties quantised=%d search %d: device %s %d fills %.17g, numpy %s %d fills %.17g" % (
            quantised, k, "".join(got[k]), a.nFills, a.bestLogSeqProb, "".join(want[k]), b.nFills, b.bestLogSeqProb))
    assert got == want and [t.nFills for t in gt] == [t.nFills for t in wt]
    assert max(t.nFills for t in wt) < 300
    for a, b in zip(gt, wt):
        assert abs(a.bestLogSeqProb - b.bestLogSeqProb) <= 1e-9 * max(1.0, abs(b.bestLogSeqProb))


# ---- 6. a silent self-loop --------------------------------------------------------------------------------------------------------
def test_silent_self_loop_on_the_start_state_is_skipped():
    """The machine compiler lets a silent self-loop through on the start state only; the level loop skips it (s >= q) as the
    yardstick drops it."""
    em, _ = ph.self_loop_case()
    dev_worst, _, _ = _compare_family(em, mph.self_loop_rows(), mph.SELF_LOOP_COLTOK, "silent self-loop")
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 7. lengths 0 to 9 in one store, slot reuse -----------------------------------------------------------------------------------
def test_one_extend_over_searches_of_0_to_9_rows():
    """Ten searches of 0, 1, ..., 9 rows in one store, so nine of them start past the first row of the weights and fill slots sized
    for the longest: the roots, then ONE extend over all thirty children, give bit for bit what each search gives in a store of its
    own, and agree with the yardstick.  Then the children of the 9-row search are released and children of the 0-row and 1-row
    searches are filled again: they land in the released slots, over the rows of the longer lattices, and have the short shape and
    the bits they had."""
    em, colTok, profs = mph.batch_machine(), mph.BATCH_COLTOK, mph.batch_rows()
    n, PL, S = len(profs), len(colTok) + 1, em.nStates
    assert [len(P) for P in profs] == list(range(10)) and em.nInTok == 3
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    alone, dev_worst = [], 0.0
    for P in profs:
        dev = capi.DevicePrefix(dm, None, R, 4, profiles=[P], colTok=colTok)
        r = dev.root(0)
        ch, a, b = dev.extend([0] * 3, [r[0]] * 3, [1, 2, 3])
        cells = [dev.node_cells(x, 0) for x in [r[0]] + list(ch)]
        ref = mph.merged_fills(em, P, colTok, [(), (1,), (2,), (3,)], R)
        for k, p in enumerate(ref):
            res = r[1:] if k == 0 else (a[k - 1], b[k - 1])
            assert np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]), (len(P), p)
            dev_worst = max(dev_worst, worst(cells[k], ref[p][0]), worst(res, ref[p][1:]))
        alone.append((r[1:], a.tolist(), b.tolist(), [c.tobytes() for c in cells]))
        dev.close()
    print("merged prefix edges lengths 0 to 9 worst relative deviation %.3g" % dev_worst)
    dev = capi.DevicePrefix(dm, None, R, 4 * n, profiles=profs, colTok=colTok)
    roots = [dev.root(k) for k in range(n)]
    seq = [k for k in range(n) for _ in range(3)]
    ch, a, b = dev.extend(seq, [roots[k][0] for k in seq], [1, 2, 3] * n)
    assert capi.last_launch_count() == 1 and dev.free_nodes() == 0
    for k in range(n):
        sl = slice(3 * k, 3 * k + 3)
        got = (roots[k][1:], a[sl].tolist(), b[sl].tolist(), [dev.node_cells(x, k).tobytes() for x in [roots[k][0]] + list(ch[sl])])
        assert got == alone[k], k
    gone = [int(x) for x in ch[27:30]]
    dev.release(gone)
    back = [(0, 1), (1, 1), (1, 2)]                                   # (search, symbol)
    c2, a2, b2 = dev.extend([k for k, _ in back], [roots[k][0] for k, _ in back], [t for _, t in back])
    assert sorted(int(x) for x in c2) == sorted(gone) and dev.free_nodes() == 0
    for (k, t), x, lsp, lpp in zip(back, c2, a2, b2):
        cells = dev.node_cells(int(x), k)
        assert cells.shape == (k + 1, 2, PL, S)
        assert (float(lsp), float(lpp), cells.tobytes()) == (alone[k][1][t - 1], alone[k][2][t - 1], alone[k][3][t]), (k, t)
    dev.close(); dm.close()
    assert dev_worst <= CELL_RTOL, dev_worst


# ---- 8. more fills than resident workgroups ---------------------------------------------------------------------------------------
def test_one_extend_of_more_fills_than_workgroups_are_resident():
    """S = 300, nCols = 4, L = 3 takes 69 640 B of LDS, so at most two workgroups share the 160 KiB of a CU and 600 fills outnumber
    what 256 CUs hold at once: one launch, 600 children of one root by symbols 1 and 2 in turn.  All 300 of a symbol are the same
    bits, and both agree with the yardstick."""
    S, n = mph.MANY_FILLS
    em, colTok, P = mph.lds_case(S)
    assert lds_bytes(S, 4) == 69640 and 2 * lds_bytes(S, 4) <= LDS_BYTES < 3 * lds_bytes(S, 4) and n > 2 * 256
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, None, R, n + 1, profiles=[P], colTok=colTok)
    root = dev.root(0)
    ch, a, b = dev.extend([0] * n, [root[0]] * n, [1, 2] * (n // 2))
    assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_prefix_fill_merged"
    ref = mph.merged_fills(em, P, colTok, [(), (1,), (2,)], R)
    dev_worst = max(worst(dev.node_cells(root[0], 0), ref[()][0]), worst(root[1:], ref[()][1:]))
    for t in (1, 2):
        first = dev.node_cells(int(ch[t - 1]), 0)
        assert np.isfinite(ref[(t,)][1]) and np.isfinite(ref[(t,)][2])
        dev_worst = max(dev_worst, worst(first, ref[(t,)][0]), worst([a[t - 1], b[t - 1]], ref[(t,)][1:]))
        for k in range(t - 1, n, 2):
            assert a[k] == a[t - 1] and b[k] == b[t - 1] and dev.node_cells(int(ch[k]), 0).tobytes() == first.tobytes(), k
    assert a[0] != a[1]
    print("merged prefix edges %d fills in one extend worst relative deviation %.3g" % (n, dev_worst))
    dev.close(); dm.close()
    assert dev_worst <= CELL_RTOL, dev_worst
