"""GPU tests of CTC-merged profile tapes at the edges of mb_profile_merge.hip: plane-group lane counts and the three LDS limits where
the kernels change form, machines with an input alphabet, degenerate column maps and profiles, every kind of Viterbi tie, batch
independence and bit-for-bit self-consistency, chunking under a memory budget, long profiles checked without the restatement, and a
cross-check through the composed machine.  The inputs come from the builders of mergehelpers.py, whose seeds
test_profile_merge_host.py::test_edge_suite_inputs_are_live holds to the conditions asserted here, without a GPU."""
import math

import numpy as np
import pytest

from mergehelpers import (ALPHABET_CASES, BATCH_CASES, LANE_CASES, LDS_CASES, PM_LDS_MAX, TIE_KINDS, all_blank_case, alphabet_case,
                          alphabet_one_hot_case, batch_bytes, batch_case, check_all_merged, column_map_cases, composed_case,
                          degenerate_cases, greedy_chunks, lane_case, lanes_of, lds_case, long_case, long_restatement_case,
                          merged_path_weight, tie_cases)
from profhelpers import _close
from randmachine import random_machine
from machineboss_amd import algebra, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.profile import MergedProfileDP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)


def _flow(em, c, nProf, Ltot):
    """Counts conserve flow per state: in - out = 0 inside, -1 / +1 per profile at the start / end state."""
    S = em.nStates
    fin = np.zeros(S); fout = np.zeros(S)
    np.add.at(fin, em.dst, c); np.add.at(fout, em.src, c)
    tol = 1e-8 * max(Ltot, 1)
    if S == 1:
        assert abs(fin[0] - fout[0]) <= tol
        return
    mid = np.arange(1, S - 1)
    assert np.abs(fin[mid] - fout[mid]).max(initial=0.0) <= tol
    assert abs(fout[0] - fin[0] - nProf) <= tol and abs(fin[S - 1] - fout[S - 1] - nProf) <= tol


def _check_path(em, P, colTok, v, edges, rows):
    """A merged Viterbi path chains from 0 to S-1, fires at non-decreasing rows, emits at most once per row, reads no input and
    weighs its score once its blank and repeat rows are read in the best way."""
    S = em.nStates
    if not len(edges):
        assert v == -np.inf or S == 1
        return
    assert int(em.src[edges[0]]) == 0 and int(em.dst[edges[-1]]) == S - 1
    assert np.array_equal(em.dst[edges[:-1]], em.src[edges[1:]])
    assert np.all(np.diff(rows) >= 0) and rows[0] >= 0 and rows[-1] <= len(P)
    assert np.all(em.inTok[edges] == 0)
    emitted = [int(r) for e, r in zip(edges, rows) if em.outTok[e]]
    assert len(emitted) == len(set(emitted)) and all(r < len(P) for r in emitted)
    w = merged_path_weight(em, P, colTok, edges, rows)
    assert abs(w - v) <= 1e-9 * max(1.0, abs(v)), (w, v)


# ---- A. where the kernels change form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nCols,S", LANE_CASES, ids=["%dx%d" % c for c in LANE_CASES])
def test_lane_grouping(nCols, S):
    """pm_threads / pm_lanes: G = min(planes, lanes) groups of LPP = lanes / G lanes, the rest idle.  (2, 1): 3 planes on 64 lanes,
    LPP = 21, one idle lane; (4, 13): 65 items on 128 lanes, LPP = 25, 3 idle; (4, 204) / (4, 205): 1 024 lanes, LPP = 204, the first
    state stride; 64 / 65 / 66 planes around a wavefront; 1 024 planes: one lane each; 1 025 and 1 031 planes: lanes stride over
    planes.  From 1 024 planes on the restatement's Backward and counts are out of reach (O(planes^2) calls per row), so the Forward
    and Viterbi sweeps and lattices are compared with it and the Backward and the counts are held to identities."""
    PL = nCols + 1
    lanes, G, LPP = lanes_of(nCols, S)
    want = {(1, 1): (64, 2, 32), (2, 1): (64, 3, 21), (4, 13): (128, 5, 25), (4, 204): (1024, 5, 204), (4, 205): (1024, 5, 204),
            (63, 2): (128, 64, 2), (64, 2): (192, 65, 2), (65, 2): (192, 66, 2), (1023, 2): (1024, 1024, 1), (1024, 2): (1024, 1024, 1),
            (1030, 3): (1024, 1024, 1)}[(nCols, S)]
    assert (lanes, G, LPP) == want
    assert (S > LPP) == ((nCols, S) in [(4, 205), (1030, 3), (1023, 2), (1024, 2)]) and (PL > lanes) == (nCols >= 1024)
    em, colTok, profs = lane_case(nCols, S)
    if PL <= 66:
        _, _, ref = check_all_merged(em, colTok, profs)
        assert np.isfinite(ref).sum() >= 3
        return
    assert max(len(P) for P in profs) <= 3
    dm = capi.DeviceMachine(em)
    dp = MergedProfileDP(em, colTok)
    dev = capi.DeviceProfiles(dm, profs, colTok)
    refs = [dp.forward(P) for P in profs]
    ref = np.array([r[0] for r in refs])
    assert np.isfinite(ref).sum() >= 3
    fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
    assert _close(fr, ref, 1e-9) and _close(fm, ref, 1e-9) and np.array_equal(fr, fm)
    v, off, edges, rows = dev.viterbi()
    v0 = dev.viterbi(paths=False)[0]
    for k, P in enumerate(profs):
        rv, re_, rr = dp.viterbi(P)
        assert v[k] == rv and v0[k] == rv, (k, v[k], v0[k], rv)
        assert np.array_equal(edges[off[k]:off[k + 1]], re_) and np.array_equal(rows[off[k]:off[k + 1]], rr), k
    P, (_, N, W) = profs[-1], refs[-1]
    F = capi.profile_fill_merged(dm, capi.MB_FORWARD, P, colTok)
    assert _close(F[:, 0], N, 1e-9) and _close(F[:, 1], W, 1e-9)
    _, Nv, Wv = dp.forward(P, "max")
    V = capi.profile_fill_merged(dm, capi.MB_VITERBI, P, colTok)
    assert np.array_equal(V[:, 0], Nv) and np.array_equal(V[:, 1], Wv)
    B = capi.profile_fill_merged(dm, capi.MB_BACKWARD, P, colTok)
    assert _close([B[0, 0, 0, 0]], [ref[-1]], 1e-9), (B[0, 0, 0, 0], ref[-1])
    c, s, ll = dev.counts()
    assert _close(ll, ref, 1e-9) and np.array_equal(ll, fm)
    assert np.all(c >= 0.0)
    _flow(em, c, int(np.isfinite(ref).sum()), sum(len(q) for q in profs))
    assert np.array_equal(dev.counts()[0], c)


@pytest.mark.parametrize("S", LDS_CASES)
def test_lds_boundaries(S):
    """nCols = 4, both sides of: 64 KiB of the rolling ring (19 S doubles: 431 / 432 states, where the dynamic-LDS attribute starts
    to matter), the ring at PM_LDS_MAX (1 077 in LDS / 1 078 in global scratch), the rolling Backward's 15 S doubles (1 365 / 1 366
    -- between the two the Forward rolls in scratch and the Backward in LDS), and X, the 4 S doubles the materialised sweeps keep
    (5 120 / 5 121: from there viterbi() with paths, counts() and profile_fill_merged run MAT with useLds = 0, and the counts'
    two sweeps share one scratch buffer)."""
    ring, bwd, X = 19 * S * 8, 15 * S * 8, 4 * S * 8
    assert 19 * 431 * 8 <= 64 * 1024 < 19 * 432 * 8
    assert 19 * 1077 * 8 <= PM_LDS_MAX < 19 * 1078 * 8 and 15 * 1365 * 8 <= PM_LDS_MAX < 15 * 1366 * 8 and 4 * 5120 * 8 <= PM_LDS_MAX < 4 * 5121 * 8
    assert (ring > 64 * 1024) == (S >= 432) and (ring > PM_LDS_MAX) == (S >= 1078)
    assert (bwd > PM_LDS_MAX) == (S >= 1366) and (X > PM_LDS_MAX) == (S >= 5121)
    em, colTok, profs = lds_case(S)
    assert [len(P) for P in profs] == [0, 9, 24] and profs[-1][:, 0].min() >= math.log(0.02)
    levels = int(em.silentLevels().max(initial=0)) + 1
    assert 1 < levels <= 16
    _, _, ref = check_all_merged(em, colTok, profs, fill=True)
    assert np.isfinite(ref).sum() >= 2


# ---- B. alphabets and column maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nIn,nOut", ALPHABET_CASES)
def test_input_alphabet(nIn, nOut):
    """K = (nIn+1)(nOut+1) > nOut + 1: the CSR rows q K + tok of the emitting edges are no longer adjacent to the next state's.
    Transitions that read input never fire (counts exactly 0, in check_all_merged).  Without the restatement: a one-hot profile
    (one column at 0 per row, runs of equal columns, blank-only rows) has one reading, the token sequence of its run heads, and
    must score as that sequence with an empty input on the plain two-tape kernels."""
    em, colTok, profs = alphabet_case(nIn, nOut)
    assert np.sum(em.inTok != 0) >= 10 and np.sum((em.inTok != 0) & (em.outTok != 0)) >= 1
    dm, _, ref = check_all_merged(em, colTok, profs)
    assert np.isfinite(ref).sum() >= 3
    em, colTok, hot, seqs = alphabet_one_hot_case(nIn, nOut)
    dev = capi.DeviceProfiles(dm, hot, colTok)
    b = capi.DeviceBatch.from_pairs(dm, [([], y) for y in seqs])
    f, fb = dev.forward(capi.MB_ROLLING), b.forward(capi.MB_ROLLING)
    assert _close(f, fb, 1e-6), (f, fb)
    assert np.array_equal(f, dev.forward(capi.MB_MATERIALISE))
    v, vb = dev.viterbi(paths=False)[0], b.viterbi(paths=False)[0]
    assert _close(v, vb, 1e-12), (v, vb)
    assert np.array_equal(f == -np.inf, fb == -np.inf) and np.isfinite(fb[:6]).sum() >= 4
    c = dev.counts()[0]
    assert np.allclose(c, b.counts()[0], rtol=1e-6, atol=1e-9)
    assert np.all(c[em.inTok != 0] == 0.0)
    # (a, a): apart by a blank row, or on the two columns of token 1; the same column twice in a row is the one symbol (a)
    assert seqs[-3:] == [[1, 1], [1, 1], [1]] and np.all(np.isfinite(f[-3:]))
    one = capi.DeviceBatch.from_pairs(dm, [([], [1]), ([], [1, 1])]).forward(capi.MB_ROLLING)
    assert _close(f[-1:], one[:1], 1e-6) and _close(f[-3:-1], [one[1], one[1]], 1e-6)
    assert not _close(one[:1], one[1:], 1e-6)                 # the two readings differ: the merge is visible


def test_column_maps():
    """nCols = 1 (X is plane 0 alone), every column on one token (the planes differ, the edges do not), and a column whose token no
    transition emits (its plane only ever repeats -inf)."""
    for name, (em, colTok, profs) in column_map_cases().items():
        _, _, ref = check_all_merged(em, colTok, profs)
        assert np.isfinite(ref).sum() >= 3, name
    em = random_machine(8, 0, 0, 41)
    assert em.nOutTok == 0
    dm = capi.DeviceMachine(em)
    with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
        capi.DeviceProfiles(dm, [np.zeros((2, 2))], [1])
    with pytest.raises(capi.MbError, match="outside 1..nOutTok"):
        capi.profile_fill_merged(dm, capi.MB_FORWARD, np.zeros((2, 2)), [1])


# ---- C. degenerate profiles ------------------------------------------------------------------------------------------------------
def test_all_blank_profile():
    """Every symbol column -inf, the blank finite: the silent 0 -> S-1 score plus the blank column's sum; the path fires at row L."""
    em, colTok, P = all_blank_case()
    dp = MergedProfileDP(em, colTok)
    E = np.zeros((0, len(colTok) + 1))
    silentF, silentV = dp.forward(E)[0], dp.forward(E, "max")[0]
    assert silentF > -np.inf
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, [P], colTok)
    want = silentF + float(np.sum(P[:, 0]))
    assert _close(dev.forward(capi.MB_ROLLING), [want], 1e-12) and _close(dev.forward(capi.MB_MATERIALISE), [want], 1e-12)
    v, off, edges, rows = dev.viterbi()
    assert _close(v, [silentV + float(np.sum(P[:, 0]))], 1e-12) and _close(dev.viterbi(paths=False)[0], v, 0.0)
    assert len(edges) >= 1 and np.all(rows == len(P)) and np.all(em.outTok[edges] == 0)
    _check_path(em, P, colTok, v[0], edges, rows)
    c = dev.counts()[0]
    assert np.all(c[em.outTok != 0] == 0.0) and c.sum() > 0.0
    check_all_merged(em, colTok, [P, P[:5]])


def test_all_inf_profile_and_empty_batch():
    em = random_machine(30, 0, 2, 502)
    dm = capi.DeviceMachine(em)
    colTok = [1, 2, 1]
    P = np.full((12, 4), -np.inf)
    dev = capi.DeviceProfiles(dm, [P], colTok)
    assert dev.forward(capi.MB_ROLLING)[0] == -np.inf and dev.forward(capi.MB_MATERIALISE)[0] == -np.inf
    v, off, edges, rows = dev.viterbi()
    assert v[0] == -np.inf and off[0] == off[1] and len(edges) == 0 and dev.viterbi(paths=False)[0][0] == -np.inf
    c, s, ll = dev.counts()
    assert not c.any() and s == -np.inf and np.all(ll == -np.inf)
    for mode in (capi.MB_FORWARD, capi.MB_VITERBI, capi.MB_BACKWARD):
        cells = capi.profile_fill_merged(dm, mode, P, colTok)
        assert cells.shape == (13, 2, 4, 30)
        assert np.all(cells[1:] == -np.inf) if mode != capi.MB_BACKWARD else np.all(cells[:12] == -np.inf)
    empty = capi.DeviceProfiles(dm, [], colTok)
    assert empty.forward(capi.MB_ROLLING).shape == (0,) and empty.forward(capi.MB_MATERIALISE).shape == (0,)
    v, off, edges, rows = empty.viterbi()
    assert v.shape == (0,) and list(off) == [0] and len(edges) == 0
    assert empty.viterbi(paths=False)[0].shape == (0,)
    c, s, ll = empty.counts()
    assert not c.any() and s == 0.0 and ll.shape == (0,)


@pytest.mark.parametrize("name", ["noblank", "infrow", "infweights1", "infweights2"])
def test_inf_columns_rows_and_weights(name):
    """The blank -inf in every row (plane 0 dies after row 0); a whole row -inf in two profiles of a batch; machines with an eighth
    of their weights -inf."""
    em, colTok, profs = degenerate_cases()[name]
    if name == "noblank":
        assert all(np.all(P[:, 0] == -np.inf) for P in profs)
    if name.startswith("infweights"):
        assert np.sum(em.logWeight == -np.inf) >= em.nTransitions // 8
    _, _, ref = check_all_merged(em, colTok, profs)
    assert np.isfinite(ref).sum() >= (3 if name != "noblank" else 2)
    if name == "infrow":
        assert ref[1] == -np.inf and ref[4] == -np.inf


# ---- D. ties -------------------------------------------------------------------------------------------------------------------------
def test_viterbi_ties_every_kind():
    """Quantised weights, tokens 1 and 2 on two columns each (colTok = [1, 1, 2, 2, 3]), machines of 6, 12 and 30 states with
    silent edges, 70 profiles each (two traceback blocks): the device traceback must take the documented first maximum at every kind
    of tie.  The restatement's census over the three batches: plane 262, end 121, stay 141, silent 171, repeat 307, blank 155,
    emit 363 -- each kind at least 30 times in every batch."""
    tot = {}
    for n, (em, colTok, profs) in enumerate(tie_cases()):
        assert len(profs) > 64
        dm = capi.DeviceMachine(em)
        dp = MergedProfileDP(em, colTok)
        dev = capi.DeviceProfiles(dm, profs, colTok)
        v, off, edges, rows = dev.viterbi()
        v0 = dev.viterbi(paths=False)[0]
        for k, P in enumerate(profs):
            rv, re_, rr = dp.viterbi(P, tot)
            assert v[k] == rv and v0[k] == rv, (n, k, v[k], v0[k], rv)
            assert np.array_equal(edges[off[k]:off[k + 1]], re_) and np.array_equal(rows[off[k]:off[k + 1]], rr), (n, k)
        check_all_merged(em, colTok, profs[:6], fill=True)
    assert all(tot.get(kind, 0) >= 5 for kind in TIE_KINDS), tot


# ---- E. batch independence, bit-for-bit self-consistency, chunking ---------------------------------------------------------------
@pytest.mark.parametrize("S,n,maxL", BATCH_CASES)
def test_batch_independence_and_chunking(S, n, maxL):
    """nCols = 4.  S = 300: everything in LDS, 120 profiles (two traceback blocks).  S = 1 400: the ring (212 800 bytes) and the
    rolling Backward (168 000 bytes) are both in global scratch, one slice per workgroup."""
    nCols, PL = 4, 5
    assert (19 * S * 8 > PM_LDS_MAX) == (S == 1400) and (15 * S * 8 > PM_LDS_MAX) == (S == 1400) and 4 * S * 8 <= PM_LDS_MAX
    em, colTok, profs = batch_case(S, n, maxL)
    dm = capi.DeviceMachine(em)
    assert dm.n_levels() <= 16 and len(profs) == n and min(len(P) for P in profs) == 0 and max(len(P) for P in profs) == maxL
    dev = capi.DeviceProfiles(dm, profs, colTok)
    fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
    v, off, edges, rows = dev.viterbi()
    vr = dev.viterbi(paths=False)[0]
    capi.set_option("MB_DETERMINISTIC", None)
    c, s, ll = dev.counts()
    assert np.array_equal(c, dev.counts()[0])          # reproducible without MB_DETERMINISTIC
    assert np.array_equal(fr, fm) and np.array_equal(v, vr) and np.array_equal(ll, fm)
    assert np.isfinite(fm).sum() >= n // 2 and (fm == -np.inf).any()
    acc = np.zeros(em.nTransitions)
    for k, P in enumerate(profs):
        one = capi.DeviceProfiles(dm, [P], colTok)
        assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.forward(capi.MB_MATERIALISE)[0] == fm[k], k
        v1, o1, e1, r1 = one.viterbi()
        assert v1[0] == v[k] and np.array_equal(e1, edges[off[k]:off[k + 1]]) and np.array_equal(r1, rows[off[k]:off[k + 1]]), k
        _, _, l1 = one.counts(acc)
        assert l1[0] == ll[k], k
        if k % 40 == 1 and len(P):
            assert capi.profile_fill_merged(dm, capi.MB_VITERBI, P, colTok)[len(P), 1, :, S - 1].max() == v[k]
    assert np.allclose(acc, c, rtol=1e-12, atol=1e-15)  # plane-then-profile sums need not associate as profile-by-profile ones do
    for k in range(n):
        assert v[k] <= fm[k] or not v[k] > -np.inf
        if v[k] > -np.inf:
            _check_path(em, profs[k], colTok, v[k], edges[off[k]:off[k + 1]], rows[off[k]:off[k + 1]])

    # a budget that forces at least 3 chunks of unequal size (the profiles differ in length); outputs unchanged
    cb, vb = batch_bytes(em, nCols, profs, dm.n_levels())
    assert cb[1] == 8 * (maxL + 1) * 2 * PL * S + 8 * em.nTransitions * PL + 8 * (19 * S if S == 1400 else 0)
    budget = int(sum(cb) / 3.5)
    assert budget >= max(cb) * 1.2 and budget >= max(vb) * 1.2
    for b in (cb, vb):
        chunks = greedy_chunks(b, budget)
        assert len(chunks) >= 3 and len({p1 - p0 for p0, p1 in chunks}) >= 2, chunks
    capi.set_memory_budget(budget)
    try:
        fm2 = dev.forward(capi.MB_MATERIALISE); fr2 = dev.forward(capi.MB_ROLLING)
        v2, off2, e2, r2 = dev.viterbi()
        v3 = dev.viterbi(paths=False)[0]
        c2, s2, ll2 = dev.counts()
        # below one profile's lattice: an error, then the normal budget works again
        capi.set_memory_budget(min(max(cb), max(vb)) // 2)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.counts()
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.viterbi()
    finally:
        capi.set_memory_budget(0)
    assert np.array_equal(fm2, fm) and np.array_equal(fr2, fr) and np.array_equal(ll2, ll) and np.array_equal(v3, v)
    assert np.array_equal(v2, v) and np.array_equal(off2, off) and np.array_equal(e2, edges) and np.array_equal(r2, rows)
    assert np.allclose(c2, c, rtol=1e-12, atol=1e-15)
    assert np.array_equal(dev.counts()[0], c)


# ---- F. long profiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_input", [False, True], ids=["noinput", "input"])
def test_long_profiles_flow_paths_and_derivatives(with_input):
    """Three profiles of 1 500 to 3 000 rows at 200 states, without the restatement: finite, Viterbi <= Forward, flow conservation,
    nothing on input-reading transitions, valid paths; on the same profiles cut to 300 rows, six counts against central
    differences of the device's own rolling Forward."""
    em, colTok, profs = long_case(with_input)
    assert [len(P) for P in profs] == [1500, 2200, 3000] and all(np.all(np.isfinite(P)) for P in profs)
    assert (np.sum(em.inTok != 0) > 0) == with_input
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs, colTok)
    c, s, ll = dev.counts()
    assert np.all(np.isfinite(ll)) and np.array_equal(ll, dev.forward(capi.MB_MATERIALISE)) and np.array_equal(ll, dev.forward(capi.MB_ROLLING))
    _flow(em, c, len(profs), sum(len(P) for P in profs))
    assert np.all(c >= 0.0) and np.all(c[em.inTok != 0] == 0.0)
    v, off, edges, rows = dev.viterbi()
    assert np.array_equal(v, dev.viterbi(paths=False)[0])
    for k, P in enumerate(profs):
        assert np.isfinite(v[k]) and v[k] <= ll[k]
        _check_path(em, P, colTok, v[k], edges[off[k]:off[k + 1]], rows[off[k]:off[k + 1]])
    cut = capi.DeviceProfiles(dm, [P[:300] for P in profs], colTok)
    cc = cut.counts()[0]
    fin = np.nonzero((em.logWeight > -np.inf) & (em.inTok == 0))[0]
    used = fin[cc[fin] > 1e-3]
    pick = np.random.RandomState(1).choice(used, 6, replace=False)
    h = 1e-4
    try:
        for t in pick:
            lw = em.logWeight.copy(); lw[t] += h
            dm.set_weights(lw); up = cut.forward(capi.MB_ROLLING).sum()
            lw[t] -= 2 * h
            dm.set_weights(lw); dn = cut.forward(capi.MB_ROLLING).sum()
            d = (up - dn) / (2 * h)
            assert abs(d - cc[t]) <= 1e-5 + 1e-4 * abs(cc[t]), (t, d, cc[t])
    finally:
        dm.set_weights(em.logWeight)
    assert np.array_equal(cut.counts()[0], cc)


def test_long_profile_against_restatement():
    """One profile of 1 200 rows at 100 states, token 1 on two columns: Forward, the Backward lattice, counts, the Viterbi path."""
    em, colTok, P = long_restatement_case()
    assert len(P) == 1200
    dm = capi.DeviceMachine(em)
    dp = MergedProfileDP(em, colTok)
    ll = dp.forward(P)[0]
    assert ll > -np.inf
    dev = capi.DeviceProfiles(dm, [P], colTok)
    assert _close(dev.forward(capi.MB_ROLLING), [ll], 1e-9) and _close(dev.forward(capi.MB_MATERIALISE), [ll], 1e-9)
    _, NB, WB = dp.backward(P)
    B = capi.profile_fill_merged(dm, capi.MB_BACKWARD, P, colTok)
    assert _close(B[:, 0], NB, 1e-9) and _close(B[:, 1], WB, 1e-9)
    rc, _ = dp.counts(P)
    c = dev.counts()[0]
    assert np.allclose(c, rc, rtol=1e-6, atol=1e-9), np.abs(c - rc).max()
    rv, re_, rr = dp.viterbi(P)
    v, off, edges, rows = dev.viterbi()
    assert v[0] == rv and np.array_equal(edges, re_) and np.array_equal(rows, rr)


# ---- G. through the composed machine, on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generator", "random"])
@pytest.mark.parametrize("zeros", [False, True])
def test_merged_sweep_equals_composed_machine(which, zeros):
    """compose(M, merging recogniser) with empty tapes on the two-tape kernels (the route the merged kernels replace) against the
    merged profile sweep."""
    M, em, prof = composed_case(which, zeros)
    P, colTok = prof.mergeRows(em)
    assert len(set(colTok)) < len(colTok) and (P == -np.inf).any() == zeros
    comp = algebra.compose(M, prof.mergingRecogniserMachine(), True, False)   # parallel transitions kept apart: Viterbi is per edge
    ec = EvaluatedMachine.fromMachine(comp, {}, useDefaults=True)
    b = capi.DeviceBatch.from_pairs(capi.DeviceMachine(ec), [([], [])])
    dev = capi.DeviceProfiles(capi.DeviceMachine(em), [P], colTok)
    f, fc = dev.forward(capi.MB_ROLLING)[0], b.forward(capi.MB_ROLLING)[0]
    assert np.isfinite(f) and abs(f - fc) <= 1e-6 * abs(f), (f, fc)
    assert dev.forward(capi.MB_MATERIALISE)[0] == f
    v, vc = dev.viterbi(paths=False)[0][0], b.viterbi(paths=False)[0][0]
    assert np.isfinite(v) and abs(v - vc) <= 1e-12 * abs(v), (v, vc)
