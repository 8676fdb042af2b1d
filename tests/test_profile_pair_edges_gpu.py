"""GPU tests of the two-tape profile sweeps (mb_profile_pair.hip) at the places where they change form: the rolling ring in LDS below
and above 64 KiB and in global scratch, found by i and by r, several of them packed in one launch and in chunks; the counts kernel
past the 8 192 transitions it keeps in LDS, in floating point and in fixed point; Viterbi ties decided by candidate order alone;
traceback slots filled to their bound; diagonals wider than the workgroup away from i = 0; other alphabets, a silent self-loop, a
lattice far below 0, stale workspaces.  The reference is profile.PairProfileDP throughout and the bounds are those of
test_profile_pair_gpu.py (pairprofilehelpers: log values 1e-9 relative to max(1, |value|) with -inf exact; counts >= 1e-3 at 1e-6
relative, smaller ones at 1e-9 + 1e-6 x count absolute; Viterbi scores and cells at 1e-12, paths and rows equal).  Every case that
compares likelihoods asserts that nine in ten of them are finite, every case that compares cells that half of them are
(test_profile_pair_host.py::test_pair_edge_suite_inputs_are_live holds the same builders to that on the CPU)."""
import math

import numpy as np
import pytest

import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close
from machineboss_amd import capi
from machineboss_amd.profile import PairProfileDP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


WORST = {}
_SCORES = {}      # (builder, arguments) -> (Forward likelihood, Viterbi score) of the restatement: computed once, shared, never changed


def _scores(key, em, x, P):
    if key not in _SCORES:
        dp = PairProfileDP(em)
        _SCORES[key] = (dp.forward(x, P)[0], dp.forward(x, P, "max")[0])
    return _SCORES[key]


def _full(em, pairs):
    live = dict(ll=[], cells=0, all=0)
    refs = ph.check_machine(em, pairs, live=live, worst=WORST)
    ph.assert_live(live)
    return refs


# ---- 1. where the ring lives ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", (True, False))
@pytest.mark.parametrize("I,L", ph.RING_SHAPES)
def test_ring_placement_by_shape(I, L, levels):
    """S = 300, a ring of 48 (min(I, L) + 1) S bytes.  (10, 30): 158 400 bytes, the last ring in LDS and past 64 KiB; (11, 30) and
    (30, 11): 172 800 bytes, global scratch, the cell found by i and by r -- the 160 KiB mark crossed by the short side, not by S.
    With silent levels (their phase on a scratch ring) and without.  Rolling Forward and Viterbi score against the restatement;
    rolling Forward has the bits of materialised Forward (the two run the same sums in the same order; only the cells' homes differ)."""
    assert (ph.ring_bytes(ph.RING_S, I, L) <= ph.RING_LDS_MAX) == ((I, L) == (10, 30)) and ph.ring_bytes(ph.RING_S, I, L) > 64 * 1024
    em, x, P = ph.ring_case(I, L, levels)
    want, wv = _scores(("ring", I, L, levels), em, x, P)
    assert want > -math.inf and wv > -math.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x], [P])
    try:
        got = dev.forward(capi.MB_ROLLING)
        ph.note("forward", got, [want], WORST)
        assert logs_close(got, [want]), (got, want)
        assert logs_close(dev.viterbi(paths=False)[0], [wv], 1e-12)
        mat = dev.forward(capi.MB_MATERIALISE)
        assert logs_close(mat, [want]) and np.array_equal(got, mat), (got, mat)
    finally:
        dev.close(); dm.close()


# ---- 2. LDS rings and scratch rings in one launch, in single launches over stale workspace, in chunks ------------------------------
def _rolling(dev):
    return dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]


def test_mixed_batch_of_lds_and_scratch_rings():
    """Eight pairs, four of them with rings in scratch (ringBase 0, 21 600, 43 200, 64 800 doubles) between pairs with rings in LDS.
    Against the restatement; the same bits from a second call, from every pair alone -- largest ring first, so that each later ring
    and lattice lies in workspace an earlier call left full -- and from the batch cut into chunks of one scratch ring each, where
    ringBase starts again at 0."""
    em, pairs = ph.mixed_case()
    refs = [_scores(("ring", I, L, True) if k < 3 else ("mixed", k), em, x, P) for k, ((I, L), (x, P)) in enumerate(zip(ph.MIXED_SHAPES, pairs))]
    want, wv = np.array([r[0] for r in refs]), np.array([r[1] for r in refs])
    assert np.mean(want > -math.inf) >= 0.9
    scratch = [ph.ring_bytes(ph.RING_S, I, L) > ph.RING_LDS_MAX for I, L in ph.MIXED_SHAPES]
    assert sum(scratch) == 4 and not scratch[0] and not scratch[3]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        f0, v0 = _rolling(dev)
        ph.note("forward", f0, want, WORST)
        assert logs_close(f0, want), (f0, want)
        assert logs_close(v0, wv, 1e-12), (v0, wv)
        assert capi.last_launch_count() == 1
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        order = sorted(range(len(pairs)), key=lambda k: (ph.MIXED_SHAPES[k] == (2, 3), -ph.ring_bytes(ph.RING_S, *ph.MIXED_SHAPES[k])))
        assert ph.MIXED_SHAPES[order[-1]] == (2, 3) and scratch[order[0]]
        for k in order:
            one = capi.DeviceProfilePairs(dm, [pairs[k][0]], [pairs[k][1]])
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
        capi.set_memory_budget(3 * 172800 // 2 + 4096)          # one scratch ring and a half: no two of the four fit one chunk
        try:
            f2 = dev.forward(capi.MB_ROLLING)
            n2 = capi.last_launch_count()
            v2 = dev.viterbi(paths=False)[0]
            assert n2 >= 3 and capi.last_launch_count() >= 3
        finally:
            capi.set_memory_budget(0)
        assert np.array_equal(f0, f2) and np.array_equal(v0, v2), (f0, f2, v0, v2)
    finally:
        dev.close(); dm.close()


def test_many_scratch_rings_packed_in_one_launch():
    """Twenty-four workgroups, eighteen with a ring of their own in the scratch buffer (S = 854 with levels, shapes around (3, 3)).
    The eight pairs of the mixed batch land on eight dies, each with an L2 of its own that keeps a workgroup's writes to itself
    until the kernel ends: rings packed on top of each other went unnoticed there (docs/profile_tapes.md, "Edges").  Here pairs k,
    k + 8 and k + 16 share a die.  Against the restatement, and every pair alone returns the bits it had in the batch."""
    em, pairs = ph.packed_case()
    dp = PairProfileDP(em)
    want = np.array([dp.forward(x, P)[0] for x, P in pairs]); wv = np.array([dp.forward(x, P, "max")[0] for x, P in pairs])
    assert np.mean(want > -math.inf) >= 0.9
    scratch = [ph.ring_bytes(ph.PACKED_S, I, L) > ph.RING_LDS_MAX for I, L in ph.PACKED_SHAPES]
    assert sum(scratch) == 18 and all(scratch[k] == scratch[k + 8] for k in range(16))
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        f0, v0 = _rolling(dev)
        ph.note("forward", f0, want, WORST)
        assert logs_close(f0, want), (f0, want)
        assert logs_close(v0, wv, 1e-12), (v0, wv)
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        for k, (x, P) in enumerate(pairs):
            one = capi.DeviceProfilePairs(dm, [x], [P])
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
    finally:
        dev.close(); dm.close()


# ---- 3. counts past the LDS table ---------------------------------------------------------------------------------------------------
def _counts_reference(em, pairs):
    dp = PairProfileDP(em)
    res = [dp.counts(x, P) for x, P in pairs]
    return np.sum([c for c, _ in res], axis=0), np.array([ll for _, ll in res])


def _check_counts(got, wc, want, what="counts"):
    c, s, ll = got
    ph.note_counts(c, wc, WORST, what)
    assert counts_close(c, wc), np.abs(c - wc).max()
    assert logs_close(ll, want) and abs(s - want.sum()) <= 1e-9 * max(1.0, abs(want.sum())), (ll, want, s)


def test_counts_past_the_lds_table():
    """11 204 transitions (S = 700 with levels) and 8 634 (S = 1 200 without): beyond PP_COUNTS_LDS_MAX every posterior goes into the
    global table with an atomic of its own.  Three pairs at (5, 6), (6, 5) and (0, 3): 15 groups of 256 lanes per pair, of which the short
    pair (2 800 items) leaves four idle.  With MB_DETERMINISTIC=1 the adds are 64-bit fixed point at 2^-36, each rounded to the nearest: a transition
    receives at most (I + 1)(L + 1) = 42 adds per pair, so at most 42 x 2^-37 = 3.1e-10 of error per pair and 9.2e-10 for the three,
    under the 1e-9 floor of counts_close -- the project's bound holds for the fixed point as it stands.  A dead pair (a profile row
    all -inf) adds nothing in either mode."""
    assert all((I + 1) * (L + 1) <= 45 for I, L in ph.COUNT_SHAPES)
    em, pairs, dead = ph.big_counts_case()
    assert em.nTransitions > 8192
    wc, want = _counts_reference(em, pairs)
    assert (want > -math.inf).all() and (wc > 0).sum() > 8192 and PairProfileDP(em).forward(*dead)[0] == -math.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    both = capi.DeviceProfilePairs(dm, [x for x, _ in pairs[:1] + [dead] + pairs[1:]], [P for _, P in pairs[:1] + [dead] + pairs[1:]])
    try:
        _check_counts(dev.counts(), wc, want)
        c, s, ll = both.counts()
        assert counts_close(c, wc) and ll[1] == -math.inf and s == -math.inf and logs_close(np.delete(ll, 1), want)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            d1 = dev.counts(); d2 = dev.counts(); d3 = both.counts()
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d1[2], d2[2])
        _check_counts(d1, wc, want, "fixed-point counts")
        assert np.array_equal(d3[0], d1[0])                  # integer adds: the dead pair's nothing leaves the same bits
    finally:
        both.close(); dev.close(); dm.close()
    em, pairs = ph.flat_counts_case()
    assert em.nTransitions > 8192 and em.silentLevels().max() == 0
    wc, want = _counts_reference(em, pairs)
    assert (want > -math.inf).all() and wc.any()
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        _check_counts(dev.counts(), wc, want)
    finally:
        dev.close(); dm.close()


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------------
def _equal_paths(dm, em, pairs, census=None):
    """Scores, edges, rows and every Viterbi cell equal (==) to the restatement's, for sums that are exact."""
    dp = PairProfileDP(em)
    refs = [dp.viterbi(x, P, census) for x, P in pairs]
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        v, off, edges, rows = dev.viterbi()
        assert np.array_equal(dev.viterbi(paths=False)[0], v)
    finally:
        dev.close()
    for k, ((x, P), (wv, we, wr)) in enumerate(zip(pairs, refs)):
        assert wv > -math.inf and v[k] == wv, (k, v[k], wv)
        assert np.array_equal(edges[off[k]:off[k + 1]], we) and np.array_equal(rows[off[k]:off[k + 1]], wr), (k, edges[off[k]:off[k + 1]], we)
        _, N, W = dp.forward(x, P, "max")
        assert np.array_equal(capi.profile_pair_fill(dm, capi.MB_VITERBI, x, P), np.stack([N, W], axis=2)), k
    return refs


def test_ties_are_decided_by_candidate_order():
    """The machine of test_profile_pair_host.py::test_tie_census, I, L in 1..4, as one batch of sixteen pairs: the weights are
    multiples of log 0.5 and the profile's are 0, so every sum is exact and equal candidates are equal on the device too.  The
    census of what was just compared holds every kind of tie -- N: blank / match, match / output-only; W: stay / input-only,
    input-only / silent -- so equal paths mean the device took the first candidate at each.  Then the two machines worked by hand
    there, and the quantised twin machine, whose twin symbols must score the same and walk twin edges."""
    em = ph.tie_machine()
    dm = capi.DeviceMachine(em)
    census = {}
    try:
        refs = _equal_paths(dm, em, ph.tie_pairs(), census)
    finally:
        dm.close()
    assert len(refs) == 16 and all(r[0] == 2 * ph.HALF for r in refs)
    met = {(a, b) for kinds in census for a in kinds for b in kinds if a != b}
    for a, b in (("blank", "match"), ("match", "emit"), ("stay", "ins"), ("ins", "silent")):
        assert (a, b) in met, (a, b, census)
    for em, x, P in ph.hand_tie_cases():
        dm = capi.DeviceMachine(em)
        census = {}
        try:
            (v, edges, rows), = _equal_paths(dm, em, [(x, P)], census)
        finally:
            dm.close()
        assert v == 0.0 and len(edges) == 1 and int(em.inTok[edges[0]]) == 1 and list(rows) == [0] and census, (edges, census)
    em, pairs = ph.twin_case()
    dm = capi.DeviceMachine(em)
    try:
        (v1, e1, r1), (v2, e2, r2) = _equal_paths(dm, em, pairs)
    finally:
        dm.close()
    assert v1 == v2 and np.array_equal(r1, r2) and len(e1) == len(e2) and not np.array_equal(e1, e2)
    for a, b in zip(e1, e2):
        twins = {int(em.inTok[a]), int(em.inTok[b])} == {1, 2} and all(f[a] == f[b] for f in (em.src, em.dst, em.outTok, em.logWeight))
        assert a == b or twins, (a, b)


# ---- 5. traceback slots filled to the bound -----------------------------------------------------------------------------------------
def test_full_traceback_slots():
    """The chain machine (pairprofilehelpers.chain_machine, S = 5) against profiles without blanks: every path has exactly
    I + L + (I + L + 1)(nLevF - 1) edges, the size of its slot, so six slots lie end to end without a free entry between them and a
    slot base, a bound or a reversal that is off by one lands in a neighbour.  The paths tie over the order of input-only and
    output-only edges, too.  Counts: every silent edge is used I + L + 1 times per pair."""
    em, pairs = ph.chain_case()
    dp = PairProfileDP(em)
    refs = [dp.viterbi(x, P) for x, P in pairs]
    bounds = [len(x) + len(P) + (len(x) + len(P) + 1) * (ph.CHAIN_S - 1) for x, P in pairs]
    assert [len(r[1]) for r in refs] == bounds and bounds[0] == 39 and all(r[0] > -math.inf for r in refs)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        L_ = capi.load()
        assert [int(L_.mb_profile_pair_path_bound(dm.h, len(x), len(P))) for x, P in pairs] == bounds and dev.path_cap() == sum(bounds)
        v, off, edges, rows = dev.viterbi(cap=dev.path_cap())
        assert list(np.diff(off)) == bounds and len(edges) == sum(bounds)
        for k, (wv, we, wr) in enumerate(refs):
            assert abs(v[k] - wv) <= 1e-12 * max(1.0, abs(wv)), (k, v[k], wv)
            assert np.array_equal(edges[off[k]:off[k + 1]], we) and np.array_equal(rows[off[k]:off[k + 1]], wr), k
        with pytest.raises(capi.MbError, match="pathCap too small"):
            dev.viterbi(cap=dev.path_cap() - 1)
        wc, want = _counts_reference(em, pairs)
        silent = (em.inTok == 0) & (em.outTok == 0)
        assert silent.sum() == ph.CHAIN_S - 1 and np.allclose(wc[silent], sum(len(x) + len(P) + 1 for x, P in pairs), rtol=1e-9, atol=0)
        _check_counts(dev.counts(), wc, want)
        got = dev.forward(capi.MB_ROLLING)
        ph.note("forward", got, want, WORST)
        assert logs_close(got, want)
    finally:
        dev.close(); dm.close()


# ---- 6. a long run of diagonals wider than the workgroup ----------------------------------------------------------------------------
@pytest.mark.parametrize("I,L", ph.FLAT_SHAPES)
def test_flat_run_of_wide_diagonals(I, L):
    """S = 300 at (5, 60) and (60, 5): 1 800 items on each of 55 diagonals in a row against 1 024 lanes, so every lane strides and
    some stride twice; at (60, 5) the diagonals start at i = d - 5 > 0.  Everything the device computes, against the restatement."""
    em, pairs = ph.flat_diagonals_case(I, L)
    assert (min(I, L) + 1) * em.nStates > 1024
    _full(em, pairs)


# ---- 7. small edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nIn,nOut", ph.SMALL_ALPHABETS)
def test_other_alphabets(nIn, nOut):
    """One input symbol against four output symbols, four against one, five against three: S = 65 with silent levels and without,
    at (4, 6) and (6, 4)."""
    live = dict(ll=[], cells=0, all=0)
    for em, pairs in ph.alphabet_case(nIn, nOut):
        assert (em.nInTok, em.nOutTok) == (nIn, nOut)
        ph.check_machine(em, pairs, live=live, worst=WORST)
    ph.assert_live(live)


def test_silent_self_loop_never_fires():
    em, pairs = ph.pair_self_loop_case()
    loop = ph.self_loop_edge(em)
    refs = _full(em, pairs)
    assert all(r["counts"][loop] == 0.0 for r in refs) and all(loop not in r["path"][0] for r in refs)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [P for _, P in pairs])
    try:
        c = dev.counts()[0]
        assert c[loop] == 0.0 and c.any()
    finally:
        dev.close(); dm.close()


def test_lattice_far_below_zero():
    """Every profile entry 700 lower: likelihoods near -6 300, where exp() of a cell is 0 and only differences survive.  The counts
    are those of the unshifted profile: a constant per row cancels in the posterior."""
    em, x, P, Pfar = ph.far_case()
    refs = _full(em, [(x, Pfar)])
    assert refs[0]["ll"] < -6000.0
    near = PairProfileDP(em).counts(x, P)[0]
    assert counts_close(refs[0]["counts"], near)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [x, x], [Pfar, P])
    one = capi.DeviceProfilePairs(dm, [x], [Pfar])
    try:
        c = one.counts()[0]
        assert counts_close(c, near), np.abs(c - near).max()
        assert counts_close(dev.counts()[0], 2.0 * near)
        ll = dev.forward(capi.MB_ROLLING)
        assert abs((ll[1] - ll[0]) + len(P) * ph.FAR_SHIFT) <= 1e-9 * abs(ll[0])
    finally:
        one.close(); dev.close(); dm.close()
