"""GPU tests of the two-profile sweeps where the host splits one call (mb_profile_api.hip: mb_profile_twos_counts, mb_profile_twos_viterbi,
two_profile_descs; docs/profile_tapes.md, "Pairs of profiles"): several count workgroups to a pair around the marks of the group
rule, counts and Viterbi paths in chunks under a memory budget, and a traceback of more pairs than one block of 64 lanes.  The
recurrence is pinned by test_profile_two_gpu.py; here it is the strides, the bases and the seams.  The reference is
profile.TwoProfileDP throughout; the bounds are those of twoprofilehelpers, unchanged: log values 1e-9 relative to max(1, |value|)
with -inf exact; counts >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x count absolute; Viterbi scores at 1e-12; paths,
output rows and input rows equal.  test_profile_two_host.py::test_two_edge_inputs_are_live holds the builders to their liveness
conditions, the group rule and the chunking without a GPU."""
import math

import numpy as np
import pytest

import twoprofilehelpers as th
from twoprofilehelpers import counts_close, logs_close
from machineboss_amd import capi
from machineboss_amd.profile import TwoProfileDP

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    print("worst deviations of the module:", WORST)


def _twos(dm, pairs):
    return capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs])


def _cells(pairs):
    return sum((len(A) + 1) * (len(B) + 1) for A, B in pairs)


def _deterministic(*calls):
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        return [call() for call in calls]
    finally:
        capi.set_option("MB_DETERMINISTIC", None)


# ---- 1. more than one count workgroup to a pair -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    """The pairs of group_case and the restatement's counts and likelihoods of each, computed once, shared, never changed."""
    em, singles, ragged, dead = th.group_case()
    dp = TwoProfileDP(em)
    one = [dp.counts(A, B) for A, B in singles]
    return em, singles, ragged, dead, one, one[-1:] + [dp.counts(A, B) for A, B in ragged[1:]]


@pytest.mark.parametrize("n", range(len(th.GROUP_SHAPES)), ids=["%dx%d" % s for s in th.GROUP_SHAPES])
def test_counts_of_one_pair_across_groups(groups, n):
    """One pair to a launch at the marks of the group rule -- a workgroup per 2 048 (cell, state) items, restated by
    th.count_groups and asserted here, so that a change of the rule in mb_profile_api.hip shows instead of moving every shape to one side
    of its mark: 2 040 items (one group) against 2 050 (two; the short side found by i, then by r), 4 205 (three; the last stride
    of 768 items is whole for group 0, partial for group 1 and empty for group 2), 10 240 = 5 x 2 048 (five) against 10 400 (six;
    by i, then by r) and 20 800 (eleven).  S = 5 is odd: no stride ends on a cell.  Every transition has a positive count in the
    restatement, so an item left out or taken twice cannot hide in a zero.

    With MB_DETERMINISTIC=1 every add is rounded to the nearest 2^-36, half of 2^-36 of error at most; an edge leaves one state and
    is of one kind, so a transition receives at most one add per cell, (K + 1)(L + 1) per pair, and the LDS table and its flush add
    integers without error.  So the fixed point is held to the project's bound plus (K + 1)(L + 1) x 2^-37 (th.fixed_counts_close):
    1.5e-8 at 2 080 cells, above the 1e-9 floor of counts_close, which therefore stays as it is for the floating-point mode only."""
    em, singles, _, _, one, _ = groups
    K, L = th.GROUP_SHAPES[n]
    assert th.GROUP_COUNTS[:4] == (1, 2, 2, 3) and th.count_groups(th.GROUP_S, [(K, L)]) == th.GROUP_COUNTS[n]
    wc, wl = one[n]
    assert wl > -math.inf and (wc > 0).all()
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, [singles[n]])
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_counts" and capi.last_launch_count() == 1
        th.note("forward", ll, [wl], WORST)
        th.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, [wl]) and abs(s - wl) <= 1e-9 * max(1.0, abs(wl)), (ll, s, wl)
        d1, d2 = _deterministic(dev.counts, dev.counts)
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d1[2], ll) and np.array_equal(d2[2], ll)
        th.note_counts(d1[0], wc, WORST, "fixed-point counts")
        assert th.fixed_counts_close(d1[0], wc, (K + 1) * (L + 1)), np.abs(d1[0] - wc).max()
    finally:
        dev.close(); dm.close()


def test_counts_of_a_ragged_launch_across_groups(groups):
    """(63, 64) beside (2, 3), (0, 0), (0, 5), (5, 0): the large pair sets eleven groups for every pair of the launch, and ten of
    the eleven of a small pair (each alone is served by one) own no item but build and flush an accumulator all the same; then the
    same batch with a dead pair (a row of B all -inf) behind the large one.  Against the sum of the restatements; the dead pair's
    likelihood and the sum are -inf and it adds no count: the fixed point has the same bits with it and without it, and twice."""
    em, _, ragged, dead, _, res = groups
    S = th.GROUP_S
    assert th.count_groups(S, th.GROUP_RAGGED) == 11 and all(th.count_groups(S, [s]) == 1 for s in th.GROUP_RAGGED[1:] + ((5, 6),))
    wc, want = np.sum([c for c, _ in res], axis=0), np.array([ll for _, ll in res])
    assert (want > -math.inf).all() and (wc > 0).all()
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, ragged)
    both = _twos(dm, ragged[:1] + [dead] + ragged[1:])
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_counts" and capi.last_launch_count() == 1
        th.note("forward", ll, want, WORST)
        th.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want) and abs(s - want.sum()) <= 1e-9 * abs(want.sum()), (ll, s, want)
        cb, sb, lb = both.counts()
        assert capi.last_launch_count() == 1
        assert lb[1] == -math.inf and sb == -math.inf and np.array_equal(np.delete(lb, 1), ll)
        assert counts_close(cb, wc) and counts_close(cb, c), np.abs(cb - wc).max()
        d1, d2, d3 = _deterministic(dev.counts, dev.counts, both.counts)
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d1[2], ll)
        assert np.array_equal(d3[0], d1[0]) and d3[2][1] == -math.inf and d3[1] == -math.inf
        th.note_counts(d1[0], wc, WORST, "fixed-point counts")
        assert th.fixed_counts_close(d1[0], wc, _cells(ragged)), np.abs(d1[0] - wc).max()
    finally:
        both.close(); dev.close(); dm.close()


# ---- 2. counts and Viterbi paths in chunks ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split():
    """The ragged batch of split_case and the restatement's counts and Viterbi paths of its pairs, computed once."""
    em, pairs = th.split_case()
    dp = TwoProfileDP(em)
    return em, pairs, [dp.counts(A, B) for A, B in pairs], [dp.viterbi(A, B) for A, B in pairs], len(dp.fLevels)


def test_counts_in_chunks(split):
    """Ten ragged pairs at S = 8, (0, 0), (0, 4), (4, 0) and a dead pair among them, under a budget of two of the largest count
    footprints (the Forward and the Backward lattice of (9, 9)) and 4 096 bytes: three chunks, each with descriptors whose cellBase
    starts at 0 again, a cleared table, a copy to the host and a sum there.  The likelihoods have the bits of the unchunked call.
    The counts need not: the chunks' tables are added in fp64 on the host, in another order than the atomics of one launch; they
    are held to the unchunked call and to the restatement by counts_close.  A preloaded array receives the total once, not once
    per chunk and not its own preload again; and the fixed point gives the same bits twice, chunked as well."""
    em, pairs, res, _, _ = split
    sizes = [th.count_bytes(th.SPLIT_S, len(A), len(B)) for A, B in pairs]
    budget = 2 * max(sizes) + 4096
    chunks = th.lattice_chunks(sizes, budget)
    assert max(sizes) == th.count_bytes(th.SPLIT_S, 9, 9) and len(chunks) >= 3 and any(p0 < th.SPLIT_DEAD < p1 - 1 for p0, p1 in chunks)
    wc, want = np.sum([c for c, _ in res], axis=0), np.array([ll for _, ll in res])
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    try:
        c0, s0, l0 = dev.counts()
        assert capi.last_launch_count() == 1
        assert counts_close(c0, wc) and logs_close(l0, want) and s0 == -math.inf and l0[th.SPLIT_DEAD] == -math.inf
        capi.set_memory_budget(budget)
        try:
            c1, s1, l1 = dev.counts(); n1 = capi.last_launch_count()
            c2 = dev.counts(np.full(em.nTransitions, 0.25))[0]
            d1, d2 = _deterministic(dev.counts, dev.counts); n2 = capi.last_launch_count()
        finally:
            capi.set_memory_budget(0)
        assert capi.last_kernel_name() == "k_profile_two_counts"
        assert n1 == len(chunks) and n1 >= 3 and n2 == n1, (n1, n2, chunks)
        assert np.array_equal(l1, l0) and s1 == -math.inf
        th.note_counts(c1, wc, WORST)
        assert counts_close(c1, c0) and counts_close(c1, wc), (np.abs(c1 - c0).max(), np.abs(c1 - wc).max())
        assert counts_close(c2 - 0.25, c1), np.abs(c2 - 0.25 - c1).max()
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d1[2], l0)
        th.note_counts(d1[0], wc, WORST, "fixed-point counts")
        assert th.fixed_counts_close(d1[0], wc, _cells(pairs)), np.abs(d1[0] - wc).max()
    finally:
        dev.close(); dm.close()


def _paths_in_chunks(em, pairs, refs, nLevels):
    """The Viterbi paths of the batch in one chunk and under a budget of two of the largest footprints (the max lattice and twelve
    bytes per entry of the traceback slot) and 1 024 bytes: the five arrays equal, and the scores and every pair's slice equal to
    the restatement's."""
    S = em.nStates
    bounds = [th.path_bound(nLevels, len(A), len(B)) for A, B in pairs]
    sizes = [th.path_bytes(S, len(A), len(B), b) for (A, B), b in zip(pairs, bounds)]
    budget = 2 * max(sizes) + 1024
    chunks = th.lattice_chunks(sizes, budget)
    assert len(chunks) >= 3, chunks
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    try:
        assert dev.path_cap() == sum(bounds)
        one = dev.viterbi(cap=dev.path_cap())
        assert capi.last_launch_count() == 1
        capi.set_memory_budget(budget)
        try:
            cut = dev.viterbi(cap=dev.path_cap()); n = capi.last_launch_count()
        finally:
            capi.set_memory_budget(0)
        assert capi.last_kernel_name() == "k_profile_two_fwd<max,mat>" and n == len(chunks), (n, chunks)
    finally:
        dev.close(); dm.close()
    for a, b in zip(one, cut):
        assert np.array_equal(a, b), (a, b)
    v, off, edges, rows, ins = cut
    assert off[0] == 0 and off[-1] == len(edges) == len(rows) == len(ins)
    th.note("viterbi", v, [r[0] for r in refs], WORST)
    assert np.array_equal(v, [r[0] for r in refs]), (v, [r[0] for r in refs])      # (the additions are in the restatement's order)
    for k, (wv, we, wr, wi) in enumerate(refs):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr) and np.array_equal(ins[sl], wi), (k, edges[sl], we)
    return chunks, off


def test_full_slots_in_chunks():
    """The chain machine against profiles without blanks, its six pairs twice over: twelve slots, each filled to its bound, in
    three chunks.  pathBase starts at 0 again in every chunk, the lengths go to d_len + p0, the host walks a chunk's three arrays
    by the bounds and writes pathOff[p0 + k + 1]: with no free entry anywhere, a base or an offset that is off by one across a
    seam shows in a neighbour."""
    em, pairs = th.chain_case()
    pairs = pairs + pairs
    dp = TwoProfileDP(em)
    refs = [dp.viterbi(A, B) for A, B in pairs]
    bounds = [th.path_bound(th.CHAIN_S - 1, len(A), len(B)) for A, B in pairs]
    assert [len(r[1]) for r in refs] == bounds and all(r[0] > -math.inf for r in refs)
    chunks, off = _paths_in_chunks(em, pairs, refs, th.CHAIN_S - 1)
    assert list(np.diff(off)) == bounds


def test_ragged_paths_in_chunks(split):
    """The batch of test_counts_in_chunks: the empty paths of the dead pair and the short one of (0, 0) lie inside a chunk, between
    pairs whose paths must not move."""
    em, pairs, _, refs, nLevels = split
    chunks, off = _paths_in_chunks(em, pairs, refs, nLevels)
    assert any(p0 < th.SPLIT_DEAD < p1 - 1 for p0, p1 in chunks) and any(p0 < th.SPLIT_SHAPES.index((0, 0)) < p1 - 1 for p0, p1 in chunks)
    lens = np.diff(off)
    assert lens[th.SPLIT_DEAD] == 0 and refs[th.SPLIT_DEAD][0] == -math.inf and (np.delete(lens, th.SPLIT_DEAD) > 0).all()


# ---- 3. the traceback past one block ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam():
    em, pairs = th.seam_case()
    dp = TwoProfileDP(em)
    return em, pairs, [dp.viterbi(A, B) for A, B in pairs]


def test_traceback_past_one_block(seam):
    """k_profile_two_traceback runs a lane per pair in blocks of 64.  129 pairs: three blocks, the last with one live lane; dead
    pairs at 63, 64 and 128 -- the last lane of block 0, the first of block 1, the only one of block 2 --, whose slots stay empty
    between neighbours that fill theirs.  Batches of 64 (one block, every lane live) and 65 (one lane past it) come from the same
    list, and the longer batches return for their first pairs exactly what the shorter ones return."""
    em, pairs, refs = seam
    assert len(pairs) == th.SEAM_PAIRS == 129 and th.SEAM_DEAD == (63, 64, 128)
    live = [r[0] > -math.inf for k, r in enumerate(refs) if k not in th.SEAM_DEAD]
    assert len(live) == 126 and np.mean(live) >= 0.9 and not any(refs[k][0] > -math.inf for k in th.SEAM_DEAD)
    dm = capi.DeviceMachine(em)
    got = {}
    try:
        for n in (64, 65, 129):
            dev = _twos(dm, pairs[:n])
            try:
                got[n] = dev.viterbi()
                assert capi.last_kernel_name() == "k_profile_two_fwd<max,mat>" and capi.last_launch_count() == 1
            finally:
                dev.close()
    finally:
        dm.close()
    for n, (v, off, edges, rows, ins) in got.items():
        assert len(v) == n and len(off) == n + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows) == len(ins)
        th.note("viterbi", v, [r[0] for r in refs[:n]], WORST)
        for k, (wv, we, wr, wi) in enumerate(refs[:n]):
            sl = slice(off[k], off[k + 1])
            assert logs_close([v[k]], [wv], 1e-12), (n, k, v[k], wv)
            assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr) and np.array_equal(ins[sl], wi), (n, k, edges[sl], we)
        for k in th.SEAM_DEAD:
            assert k >= n or (off[k + 1] == off[k] and v[k] == -math.inf), (n, k)
    for short, long_ in ((64, 65), (64, 129), (65, 129)):
        v, off, edges, rows, ins = got[short]
        w, offl, el, rl, il = got[long_]
        end = off[-1]
        assert np.array_equal(w[:short], v) and np.array_equal(offl[:short + 1], off), (short, long_)
        assert np.array_equal(el[:end], edges) and np.array_equal(rl[:end], rows) and np.array_equal(il[:end], ins), (short, long_)
