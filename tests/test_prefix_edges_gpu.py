"""The token and profile node fills of the prefix search (k_prefix_fill and k_prefix_fill_profile in mb_prefix.hip, docs/decoding.md)
at their edges: alphabets of different sizes, lane counts around a wavefront and around the second stride, both LDS marks of both
launchers, searches of different lengths in one store, slot reuse, a column of the V product 850 nats below its row, -inf profile
weights, twin symbols and exact ties, a silent self-loop.  The yardsticks are prefixtree.PrefixDP and prefixtree.ProfilePrefixDP;
the inputs come from prefixhelpers.py and profileprefixhelpers.py, and tests/test_prefix_host.py::test_edge_suite_inputs_are_live
holds them to the liveness conditions asserted here without a GPU."""
import functools
import math

import numpy as np
import pytest

import prefixhelpers as ph
import profileprefixhelpers as pph
from prefixhelpers import family_paths
from machineboss_amd import capi, prefixtree

pytestmark = pytest.mark.gpu

# Bound on |device - yardstick| / max(1, |yardstick|) over the finite cells and the two results of a node.  Measured once per case on
# an MI355X (the table in docs/decoding.md): the worst case deviates by CELL_WORST.  The bound is ten times that, the rule of
# tests/test_prefix_gpu.py; no bound here may exceed the 1e-9 this project publishes.
CELL_WORST = 3.18e-15          # k_prefix_fill, S = 1, nIn = nOut = 1, no silent levels, L = 33
CELL_RTOL = 10 * CELL_WORST
# The same for layer 0 / layer 1 of k_prefix_fill_profile on a one-hot profile against seq / prefix of k_prefix_fill on the string:
# the same terms folded in another order (the token kernel's own deviation from numpy is in the table of docs/decoding.md).
ONE_HOT_WORST = 9.99e-16       # S = 65, nIn = 3, nOut = 5, no silent levels, L = 33
ONE_HOT_RTOL = 10 * ONE_HOT_WORST

LDS_DEFAULT, LDS_BYTES = 64 * 1024, 160 * 1024          # what a kernel may use unasked, and PREFIX_PROFILE_MAX_LDS (mb_prefix.h)
KINDS = ["token", "profile"]


def test_bounds_stay_inside_the_published_figure():
    assert CELL_RTOL <= 1e-9 and ONE_HOT_RTOL <= 1e-9


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_kernel(capi.KERNEL_AUTO)


def _worst(got, ref):
    """Worst relative deviation over the finite cells; -inf (and nothing else) must sit where the reference has it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))) if fin.any() else 0.0


def _store(kind, dm, outs, R, maxNodes):
    return capi.DevicePrefix(dm, outs, R, maxNodes) if kind == "token" else capi.DevicePrefix(dm, None, R, maxNodes, profiles=outs)


def _yardstick(kind, em, R):
    return prefixtree.PrefixDP(em, R) if kind == "token" else prefixtree.ProfilePrefixDP(em, R)


def _device_family(dev, nIn, seq=0):
    """{path: (node, lsp, lpp)} for the root, its children (one extend) and one grandchild of each (one extend)."""
    nodes = {(): dev.root(seq)}
    paths = family_paths(nIn)
    for depth in (1, 2):
        ps = [p for p in paths if len(p) == depth]
        ch, a, b = dev.extend([seq] * len(ps), [nodes[p[:-1]][0] for p in ps], [p[-1] for p in ps])
        for p, c, x, z in zip(ps, ch, a, b):
            nodes[p] = (int(c), float(x), float(z))
    return nodes


def _reference(dp, out, paths):
    ref = {}
    for p in sorted(paths, key=len):
        ref[p] = dp.fill(out) if not p else dp.fill(out, ref[p[:-1]][0], p[-1])
    return ref


def _compare_family(kind, em, R, out, tag, floor=0.5, live=True):
    """Every cell of both layers and both results of the family against the yardstick; returns (worst deviation, device family as
    {path: (cells, lsp, lpp)}, yardstick family)."""
    dm = capi.DeviceMachine(em)
    dev = _store(kind, dm, [out], R, 2 * em.nInTok + 1)
    nodes = _device_family(dev, em.nInTok)
    ref = _reference(_yardstick(kind, em, R), out, list(nodes))
    worst, got = 0.0, {}
    for p, (node, lsp, lpp) in nodes.items():
        cells = dev.node_cells(node, 0)
        got[p] = (cells, lsp, lpp)
        worst = max(worst, _worst(cells, ref[p][0]), _worst([lsp, lpp], ref[p][1:]))
    dev.close(); dm.close()
    total = sum(ref[p][0][:, 0].size for p in ref)
    fin = [sum(int(np.isfinite(ref[p][0][:, k]).sum()) for p in ref) for k in (0, 1)]
    print("prefix edges %s %s cells/layer=%d finite layer0=%d layer1=%d worst relative deviation %.3g" % (kind, tag, total, fin[0], fin[1], worst))
    if live:
        assert all(np.isfinite(ref[p][1]) and np.isfinite(ref[p][2]) for p in ref), tag
        assert fin[0] >= floor * total and fin[1] >= floor * total, (tag, fin, total)
    return worst, got, ref


# ---- 1. alphabets and lanes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_inputs(S, nIn, nOut, levels):
    em, y = ph.edge_case(S, nIn, nOut, levels)
    return em, prefixtree.logSumInTrans(em), y, pph.edge_profile(S, nOut)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,nIn,nOut,levels", ph.EDGE_CASES)
def test_alphabets_and_lanes(S, nIn, nOut, levels, kind):
    """nIn != nOut (the strides C = nOut + 1 and K = (nIn + 1)(nOut + 1) come from different alphabets), S = 1 (one live lane), 63,
    64, 65, and 1024 / 1025: the first state a lane meets on its second stride, in the product, the middle phase and the silent
    levels.  L = 33; every result finite and at least half of each layer."""
    em, R, y, P = _edge_inputs(S, nIn, nOut, levels)
    assert (int(em.silentLevels().max()) > 0) == levels
    worst, _, _ = _compare_family(kind, em, R, y if kind == "token" else P, "S=%d nIn=%d nOut=%d levels=%d" % (S, nIn, nOut, levels))
    assert worst <= CELL_RTOL, worst


@pytest.mark.parametrize("S,nIn,nOut,levels", ph.WITNESS_CASES)
def test_seq_results_equal_the_generic_forward(S, nIn, nOut, levels):
    """A second witness where the alphabets differ: logSeqProb of every family node is the Forward likelihood of (its input
    prefix, y) under the generic kernel -- 1e-9 relative, the README's Forward figure; every likelihood finite."""
    em, R, y, _ = _edge_inputs(S, nIn, nOut, levels)
    dm = capi.DeviceMachine(em)
    dev = capi.DevicePrefix(dm, [y], R, 2 * nIn + 1)
    nodes = _device_family(dev, nIn)
    paths = list(nodes)
    capi.set_kernel(capi.KERNEL_GENERIC)
    try:
        ll = capi.DeviceBatch.from_pairs(dm, [(np.array(p, np.int32), y) for p in paths]).forward(capi.MB_MATERIALISE)
    finally:
        capi.set_kernel(capi.KERNEL_AUTO)
    for p, f in zip(paths, ll):
        assert np.isfinite(f) and abs(nodes[p][1] - f) <= 1e-9 * max(1.0, abs(f)), (p, nodes[p][1], f)
    dev.close(); dm.close()


# ---- 2. the LDS marks ---------------------------------------------------------------------------------------------------------------
def _root_and_child(kind, em, R, out):
    """Worst deviation of the root and its child by symbol 1, whose results must be finite."""
    dm = capi.DeviceMachine(em)
    dev = _store(kind, dm, [out], R, 2)
    root = dev.root(0)
    ch, a, b = dev.extend([0], [root[0]], [1])
    ref = _reference(_yardstick(kind, em, R), out, [(), (1,)])
    worst = max(_worst(dev.node_cells(root[0], 0), ref[()][0]), _worst(root[1:], ref[()][1:]),
                _worst(dev.node_cells(int(ch[0]), 0), ref[(1,)][0]), _worst([a[0], b[0]], ref[(1,)][1:]))
    dev.close(); dm.close()
    assert all(np.isfinite(v) for v in ref[()][1:] + ref[(1,)][1:])
    return worst


@pytest.mark.parametrize("S", [ph.LDS_TOKEN_STATES[0], ph.LDS_TOKEN_STATES[1], ph.LDS_TOKEN_STATES[0]], ids=["below", "above", "below-again"])
def test_token_fill_at_the_lds_opt_in(S):
    """k_prefix_fill keeps V (S doubles) in LDS and must ask once for more than 64 KiB: 8192 states before the launcher has asked,
    8193, and 8192 again afterwards (the launcher remembers in a static).  R is banded and built by hand (prefixhelpers.banded_R).
    These cases pin the results on both sides of the mark; the runtime this was measured on also launches more than 64 KiB without
    having been asked, so no output depends on the call itself (docs/decoding.md).  Not tested: the 20480-state ceiling from below,
    whose dense R takes 3.4 GB."""
    assert ph.LDS_TOKEN_STATES == (LDS_DEFAULT // 8, LDS_DEFAULT // 8 + 1)
    em, R, y = ph.lds_token_case(S)
    worst = _root_and_child("token", em, R, y)
    print("prefix edges token LDS S=%d worst relative deviation %.3g" % (S, worst))
    assert worst <= CELL_RTOL, worst


def test_token_search_refuses_past_the_ceiling():
    """20481 states: the object is refused on the state count, before R is read -- so the library is called with a one-entry R
    here, not with the 3.4 GB the wrapper would want."""
    import ctypes as C
    S = LDS_BYTES // 8 + 1
    em = ph.populated_machine(S, 1, False)
    dm = capi.DeviceMachine(em)
    before = capi.alloc_stats()
    outTok, outOff, R = np.array([1, 0], np.int32), np.array([0, 1], np.int64), np.zeros(1)
    h = capi.load().mb_prefix_create(dm.h, 1, outTok.ctypes.data_as(C.POINTER(C.c_int32)), outOff.ctypes.data_as(C.POINTER(C.c_int64)),
                                     R.ctypes.data_as(C.POINTER(C.c_double)), 2)
    assert not h and "more than %d states" % (LDS_BYTES // 8) in capi.load().mb_last_error().decode()
    assert capi.alloc_stats() == before
    dm.close()


def _profile_marks():
    lo, hi = pph.lds_profile_states(2, LDS_DEFAULT), pph.lds_profile_states(2, LDS_BYTES)
    return [lo, lo + 1, hi]


@pytest.mark.parametrize("S", _profile_marks() + _profile_marks()[:1], ids=["below", "above", "limit", "below-again"])
def test_profile_fill_at_the_lds_marks(S):
    """k_prefix_fill_profile keeps 3 S + nOut + 1 doubles in LDS: the last machine within 64 KiB, the first past it (the opt-in),
    the last within 160 KiB, and the first again once the launcher has asked."""
    nOut = 2
    assert (3 * S + nOut + 1) * 8 <= LDS_BYTES
    assert _profile_marks() == [2729, 2730, 6825]
    worst = _root_and_child("profile", ph.lds_machine(S, nOut), ph.banded_R(S), pph.lds_profile(S, nOut))
    print("prefix edges profile LDS S=%d worst relative deviation %.3g" % (S, worst))
    assert worst <= CELL_RTOL, worst


def test_profile_fill_refuses_past_the_lds_limit():
    """One state more than 160 KiB holds: the object is created, the first fill is the error, it takes no slot and allocates
    nothing."""
    nOut = 2
    S = pph.lds_profile_states(nOut, LDS_BYTES) + 1
    assert (3 * (S - 1) + nOut + 1) * 8 <= LDS_BYTES < (3 * S + nOut + 1) * 8
    dm = capi.DeviceMachine(ph.lds_machine(S, nOut))
    dev = capi.DevicePrefix(dm, None, ph.banded_R(S), 3, profiles=[pph.lds_profile(S, nOut)])
    before = capi.alloc_stats()
    assert dev.free_nodes() == 3
    with pytest.raises(capi.MbError, match="3 x states"):
        dev.root(0)
    assert dev.free_nodes() == 3
    assert capi.alloc_stats() == before
    dev.close(); dm.close()


# ---- 3. batches and slot reuse ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_extend_over_searches_of_lengths_0_to_9(kind):
    """Ten searches of 0, 1, ..., 9 symbols (rows) in one store, so nine of them start past the first token (row) and fill slots
    sized for the longest: the roots, then ONE extend that makes two children of each, give bit for bit what each search gives in
    a store of its own.  Then a child of the 9-long search is released and a third child of the 2-long search is filled: it lands
    in the released slot, over the rows of the longer lattice, and still equals the lone store's."""
    em, ys = ph.batch_case()
    outs = ys if kind == "token" else pph.batch_profiles(em.nOutTok, ph.BATCH_LENGTHS)
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    alone, third = [], None
    for k, o in enumerate(outs):
        dev = _store(kind, dm, [o], R, 4)
        r = dev.root(0)
        ch, a, b = dev.extend([0, 0], [r[0]] * 2, [1, 2])
        alone.append((r[1:], a.tolist(), b.tolist(), [dev.node_cells(n, 0).tobytes() for n in [r[0]] + list(ch)]))
        if k == 2:
            c3, a3, b3 = dev.extend([0], [r[0]], [3])
            third = (float(a3[0]), float(b3[0]), dev.node_cells(int(c3[0]), 0).tobytes())
        dev.close()
    n = len(outs)
    dev = _store(kind, dm, outs, R, 3 * n)
    roots = [dev.root(k) for k in range(n)]
    seq = [k for k in range(n) for _ in (1, 2)]
    ch, a, b = dev.extend(seq, [roots[k][0] for k in seq], [1, 2] * n)
    for k in range(n):
        got = (roots[k][1:], a[2 * k:2 * k + 2].tolist(), b[2 * k:2 * k + 2].tolist(),
               [dev.node_cells(x, k).tobytes() for x in [roots[k][0]] + list(ch[2 * k:2 * k + 2])])
        assert got == alone[k], k
    assert all(np.isfinite(alone[k][0][0]) for k in range(2, n))
    assert not any(math.isnan(v) or v == math.inf for x in alone for v in list(x[0]) + x[1] + x[2])
    assert dev.free_nodes() == 0
    gone = int(ch[2 * 9])
    dev.release([gone])
    c3, a3, b3 = dev.extend([2], [roots[2][0]], [3])
    assert int(c3[0]) == gone
    assert (float(a3[0]), float(b3[0]), dev.node_cells(gone, 2).tobytes()) == third
    assert len(third[2]) == 3 * 2 * em.nStates * 8 and np.isfinite(third[1])
    dev.close(); dm.close()


# ---- 4. the column 850 nats down ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_column_fed_only_from_far_below_the_row_maximum(kind):
    """The claim in the header of mb_prefix.hip: the V product stays in log space, because a linear product under one row maximum
    drops a column fed only by entries 745 nats down, and a prefix probability that turns -inf prunes the search.  In this machine
    (prefixhelpers.far_column_case) column 3 of row 1 receives terms 850 nats and more below the row's largest, the only way into
    the end state runs through it, and logPrefixProb reads that one cell."""
    em, R, y = ph.far_column_case()
    out = y if kind == "token" else pph.far_column_profile()
    worst, got, ref = _compare_family(kind, em, R, out, "far column", live=False)
    dp = _yardstick(kind, em, R)
    for p, (cells, lsp, lpp) in ref.items():
        V = dp.columnSums(cells[1, 1])
        top = (cells[1, 1][:, None] + R).max()
        assert np.isfinite(V[ph.COLUMN_STATE]) and math.exp(V[ph.COLUMN_STATE] - top) == 0.0
        assert np.isfinite(cells[2, 1, ph.COLUMN_FED]) and np.isfinite(lpp)
        assert np.isfinite(got[p][0][2, 1, ph.COLUMN_FED]) and np.isfinite(got[p][2]) and got[p][2] < -800
    assert worst <= CELL_RTOL, worst


# ---- 5. sparse profiles -------------------------------------------------------------------------------------------------------------
def test_profile_with_a_third_of_its_weights_at_minus_infinity():
    """Symbols of weight -inf (skipped as a whole) and blanks of weight -inf; every result of the family is finite."""
    em, R, _, _ = _edge_inputs(65, 3, 5, True)
    P = pph.sparse_profile(ph.EDGE_L, 5)
    assert np.isneginf(P[:, 1:]).mean() >= 0.25 and np.isneginf(P[:, 0]).mean() >= 0.2
    worst, _, _ = _compare_family("profile", em, R, P, "sparse profile")
    assert worst <= CELL_RTOL, worst


def test_profile_with_a_dead_row():
    """Row 16 is -inf throughout: every cell past it and both results of every node are -inf exactly, the rows before it are not."""
    em, R, _, _ = _edge_inputs(65, 3, 5, True)
    worst, got, ref = _compare_family("profile", em, R, pph.dead_row_profile(ph.EDGE_L, 5), "dead row", live=False)
    for p, (cells, lsp, lpp) in got.items():
        assert lsp == -math.inf and lpp == -math.inf and np.isneginf(cells[pph.DEAD_ROW + 1:]).all(), p
        assert np.isfinite(ref[p][0][pph.DEAD_ROW]).mean() >= 0.5
    assert worst <= CELL_RTOL, worst


@pytest.mark.parametrize("levels", [True, False])
def test_one_hot_profile_reproduces_the_token_fill(levels):
    """Blank -inf, the symbol y[r] at 0, all others -inf: layer 0 and 1 of k_prefix_fill_profile are seq and prefix of
    k_prefix_fill on y, and so are the results -- the same terms in another order, so within a measured tolerance, no numpy
    between."""
    em, R, y, _ = _edge_inputs(65, 3, 5, levels)
    dm = capi.DeviceMachine(em)
    fam = []
    for kind, out in (("token", y), ("profile", pph.hard_profile(y, 5))):
        dev = _store(kind, dm, [out], R, 7)
        nodes = _device_family(dev, 3)
        fam.append({p: (dev.node_cells(n[0], 0), n[1], n[2]) for p, n in nodes.items()})
        dev.close()
    dm.close()
    worst = 0.0
    for p in fam[0]:
        worst = max(worst, _worst(fam[1][p][0], fam[0][p][0]), _worst(fam[1][p][1:], fam[0][p][1:]))
        assert np.isfinite(fam[0][p][1]) and np.isfinite(fam[0][p][2])
        assert np.isfinite(fam[0][p][0]).mean() >= 0.5
    print("prefix edges one-hot profile against the token fill levels=%d worst relative deviation %.3g" % (levels, worst))
    assert worst <= ONE_HOT_RTOL, worst


# ---- 6. twins and ties --------------------------------------------------------------------------------------------------------------
def _twin_inputs(quantised):
    em = ph.twin_machine(ph.TWIN_STATES, ph.TWIN_SEED, quantised)
    outs = ph.twin_outputs(em, ph.TWIN_SEARCHES, ph.TWIN_L, ph.TWIN_SEED)
    return em, outs, pph.twin_profiles(em, outs, 0.5 if quantised else 0.8)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("quantised", [False, True])
def test_twin_symbols_give_identical_children(quantised, kind):
    """Input symbols 1 and 2 have the same edges with the same weights in the same order: their children of the root and of a
    child are the same bits, cells and results; symbol 3's are not."""
    em, outs, profs = _twin_inputs(quantised)
    out = em.outputTokenizer.tokenize(outs[0]) if kind == "token" else profs[0]
    dm = capi.DeviceMachine(em)
    dev = _store(kind, dm, [out], prefixtree.logSumInTrans(em), 8)
    parent = dev.root(0)
    for _ in (0, 1):
        ch, a, b = dev.extend([0] * 3, [parent[0]] * 3, [1, 2, 3])
        cells = [dev.node_cells(int(c), 0).tobytes() for c in ch]
        assert cells[0] == cells[1] and a[0] == a[1] and b[0] == b[1]
        assert cells[0] != cells[2] and np.isfinite(b[0])
        parent = (int(ch[1]),)
    dev.close(); dm.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("quantised", [False, True])
def test_searches_break_ties_as_the_numpy_backend_does(quantised, kind):
    """Whole searches on the twin machine, whose best inputs hold a twin symbol, and on its quantised version, where different
    paths tie exactly: the device backend returns the strings and the node counts of the numpy backend."""
    em, outs, profs = _twin_inputs(quantised)
    kw = dict(outputs=outs) if kind == "token" else dict(outputs=None, profiles=profs)
    want, wt = prefixtree.decodeBatch(em, kw["outputs"], backend="numpy", profiles=kw.get("profiles"))
    got, gt = prefixtree.decodeBatch(em, kw["outputs"], backend="device", profiles=kw.get("profiles"))
    assert all(set(s) & {"A", "B"} for s in want)
    for k, (a, b) in enumerate(zip(gt, wt)):
        print("prefix edges ties %s quantised=%d search %d: device %s %d fills %.17g, numpy %s %d fills %.17g" % (
            kind, quantised, k, "".join(got[k]), a.nFills, a.bestLogSeqProb, "".join(want[k]), b.nFills, b.bestLogSeqProb))
    assert got == want and [t.nFills for t in gt] == [t.nFills for t in wt]
    for a, b in zip(gt, wt):
        assert abs(a.bestLogSeqProb - b.bestLogSeqProb) <= 1e-9 * max(1.0, abs(b.bestLogSeqProb))


# ---- 7. a silent self-loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_silent_self_loop_on_the_start_state_is_skipped(kind):
    """The machine compiler lets a silent self-loop through on the start state only; the fills skip it (s >= q) as PrefixDP drops
    it."""
    em, y = ph.self_loop_case()
    out = y if kind == "token" else pph.random_profile(np.random.RandomState(8), len(y), em.nOutTok)
    worst, _, _ = _compare_family(kind, em, prefixtree.logSumInTrans(em), out, "silent self-loop")
    assert worst <= CELL_RTOL, worst
