"""GPU tests of the two-profile sweeps (mb_profile_two.hip; docs/profile_tapes.md, "Pairs of profiles"): a machine with an input
alphabet between an input profile and an output profile.  The reference is profile.TwoProfileDP throughout, which
test_profile_two_host.py holds to the composite.  Bounds (twoprofilehelpers): log values 1e-9 relative to max(1, |value|) with -inf
exact; counts >= 1e-3 at 1e-6 relative, smaller ones at 1e-9 + 1e-6 x count absolute; Viterbi scores and cells at 1e-12; paths,
output rows and input rows equal.  The suite cases assert that nine in ten of their likelihoods and half of their cells are finite
(test_profile_two_host.py::test_two_suite_inputs_are_live holds the same builders to that on the CPU)."""
import io
import json
import math

import numpy as np
import pytest

import twoprofilehelpers as th
from twoprofilehelpers import counts_close, logs_close
from machineboss_amd import boss, capi
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine
from machineboss_amd.profile import Profile, TwoProfileDP

pytestmark = pytest.mark.gpu

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    print("worst deviations of the module:", th.WORST)


def _twos(dm, pairs):
    return capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs])


# ---- 1. everything, against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,nIn,nOut", th.SUITE_CASES)
def test_suite(S, nIn, nOut):
    """Every cell of the three fills, rolling and materialised likelihoods (the same bits), Viterbi scores, cells and paths with both
    coordinates, and counts: with and without silent levels, at every shape of SUITE_SHAPES, the pairs of a machine in one batch."""
    live = dict(ll=[], cells=0, all=0)
    cases = th.suite_case(S, nIn, nOut)
    for em in dict.fromkeys(id(c[0]) for c in cases):
        mine = [c for c in cases if id(c[0]) == em]
        th.check_machine(mine[0][0], [c[1:] for c in mine], live=live)
    assert np.mean(live["ll"]) >= 0.9 and live["cells"] >= 0.5 * live["all"], (np.mean(live["ll"]), live["cells"], live["all"])
    assert capi.last_kernel_name().startswith("k_profile_two_fwd<max,mat>")


def test_kernel_names():
    em = th.pair_machine(8, 1, True, 2, 3)
    A, B = th.two_input(np.random.RandomState(1), em, 3, 4, pInf=0.0)
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, [(A, B)])
    try:
        dev.forward(capi.MB_ROLLING); assert capi.last_kernel_name() == "k_profile_two_fwd<sum,rolling>" and capi.last_launch_count() == 1
        dev.forward(capi.MB_MATERIALISE); assert capi.last_kernel_name() == "k_profile_two_fwd<sum,mat>"
        dev.viterbi(paths=False); assert capi.last_kernel_name() == "k_profile_two_fwd<max,rolling>"
        dev.viterbi(); assert capi.last_kernel_name() == "k_profile_two_fwd<max,mat>"
        dev.counts(); assert capi.last_kernel_name() == "k_profile_two_counts"
        capi.profile_two_fill(dm, capi.MB_BACKWARD, A, B); assert capi.last_kernel_name() == "k_profile_two_bwd"
    finally:
        dev.close(); dm.close()


# ---- 2. the reductions, device against device ------------------------------------------------------------------------------------------
def test_one_hot_input_is_the_token_sweep():
    """A one-hot A (row i: 0 at x_i, -inf elsewhere, the blank -inf) against DeviceProfilePairs on x: adding the 0 of A changes no
    bit, so 1e-12 holds with room; the paths are the same edges at the same rows, and the input rows count the input-reading edges."""
    em = th.pair_machine(65, 7, True, 3, 4)
    rng = np.random.RandomState(7)
    pairs = [(rng.randint(1, 4, size=K).astype(np.int32), th.soft_profile(rng, L, 4, 0.1)) for K, L in th.SUITE_SHAPES]
    dm = capi.DeviceMachine(em)
    tok = capi.DeviceProfilePairs(dm, [x for x, _ in pairs], [B for _, B in pairs])
    two = _twos(dm, [(th.one_hot(x, 3), B) for x, B in pairs])
    try:
        ft = tok.forward(capi.MB_ROLLING)
        assert np.mean(ft > -math.inf) >= 0.7
        for flags in (capi.MB_ROLLING, capi.MB_MATERIALISE):
            assert logs_close(two.forward(flags), ft, 1e-12)
        vt, ot, et, rt = tok.viterbi()
        v, off, e, r, i = two.viterbi()
        assert logs_close(v, vt, 1e-12) and np.array_equal(off, ot) and np.array_equal(e, et) and np.array_equal(r, rt)
        for k in range(len(pairs)):
            reads = (em.inTok[e[off[k]:off[k + 1]]] > 0).astype(np.int64)
            assert np.array_equal(i[off[k]:off[k + 1]], np.cumsum(reads) - reads)
        ct, ctk = two.counts()[0], tok.counts()[0]
        assert counts_close(ct, ctk), np.abs(ct - ctk).max()
    finally:
        tok.close(); two.close(); dm.close()


def test_no_input_rows_is_the_one_tape_sweep():
    """K = 0: nothing reads the input, and the sweep is that of DeviceProfiles on the machine with its input edges taken out."""
    from prefixhelpers import machine_edges, machine_from_edges
    em = th.pair_machine(65, 8, True, 2, 3)
    gen = machine_from_edges(65, 0, 3, [e for e in machine_edges(em) if e[2] == 0])
    rng = np.random.RandomState(8)
    Bs = [th.soft_profile(rng, L, 3, 0.1) for L in (0, 1, 3, 9)]
    dm, dg = capi.DeviceMachine(em), capi.DeviceMachine(gen)
    two = _twos(dm, [(np.zeros((0, 3)), B) for B in Bs])
    one = capi.DeviceProfiles(dg, Bs)
    try:
        f1 = one.forward(capi.MB_ROLLING)
        assert (f1 > -math.inf).sum() >= 3
        assert logs_close(two.forward(capi.MB_ROLLING), f1, 1e-12) and logs_close(two.forward(capi.MB_MATERIALISE), f1, 1e-12)
        assert logs_close(two.viterbi(paths=False)[0], one.viterbi(paths=False)[0], 1e-12)
        c2, c1 = two.counts()[0], one.counts()[0]
        keep = np.nonzero(em.inTok == 0)[0]
        assert counts_close(c2[keep], c1) and not c2[em.inTok > 0].any()
    finally:
        two.close(); one.close(); dm.close(); dg.close()


# ---- 3. where the ring lives -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rings():
    """The ring pairs and the restatement's scores of some of them, computed once, shared, never changed: Forward of the two lattices
    around 64 KiB found by i, Forward and Viterbi of the small pairs.  The restatement takes seconds on the others (3 500 cells of 40
    states); they are held to the bits of the materialised sweeps, which the suite holds to the restatement."""
    em, pairs = th.ring_pairs()
    dp = TwoProfileDP(em)
    want = {k: (dp.forward(*pairs[k])[0], dp.forward(*pairs[k], "max")[0] if k >= 8 else None) for k in (0, 1, 8, 9, 10, 11)}
    return em, pairs, want


def _rolling(dev):
    return dev.forward(capi.MB_ROLLING), dev.viterbi(paths=False)[0]


def test_rings_in_lds_and_in_scratch(rings):
    """S = 40, a ring of 72 (min(K, L) + 1) S bytes: min + 1 = 22 / 23 straddle 64 KiB (63 360 / 66 240 bytes, the limit is raised for
    the second), 56 / 57 straddle 160 KiB (161 280 in LDS / 164 160 in global scratch), each found by i (K the short side) and by r.
    One ragged launch of the eight beside (2, 3), (0, 40), (40, 0) and a dead pair; then each pair alone on the workspace the batch
    left behind, largest first; then the batch in chunks under a memory budget, rolling (one scratch ring to a chunk, ringBase from 0
    again) and materialised.  Each pair gets the bits it gets alone, rolling has the bits of materialised Forward, and a chunked batch
    the bits of the unchunked one."""
    em, pairs, want = rings
    shapes = [(len(A), len(B)) for A, B in pairs]
    scratch = [th.ring_bytes(th.RING_S, K, L) > th.RING_LDS_MAX for K, L in shapes]
    assert sum(scratch) == 2 and shapes[3] == (56, 60) and shapes[7] == (60, 56) and scratch[3] and scratch[7]
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    try:
        f0, v0 = _rolling(dev)
        assert capi.last_launch_count() == 1
        for k, (wl, wv) in want.items():
            assert logs_close([f0[k]], [wl]) and (wv is None or logs_close([v0[k]], [wv], 1e-12)), (k, f0[k], wl, v0[k], wv)
        th.note("forward", f0[list(want)], [w[0] for w in want.values()], th.WORST)
        assert f0[-1] == -math.inf and v0[-1] == -math.inf and (f0[:-1] > -math.inf).all()
        m0 = dev.forward(capi.MB_MATERIALISE)
        assert np.array_equal(f0, m0), (f0, m0)
        assert np.array_equal(dev.viterbi()[0], v0)              # (with paths: the materialised max sweep)
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        for k in sorted(range(len(pairs)), key=lambda k: -th.ring_bytes(th.RING_S, *shapes[k])):
            one = _twos(dm, [pairs[k]])
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
        capi.set_memory_budget(3 * 164160 // 2 + 4096)           # a scratch ring and a half: the two do not share a chunk
        try:
            f2 = dev.forward(capi.MB_ROLLING); n2 = capi.last_launch_count()
            v2 = dev.viterbi(paths=False)[0]
            assert n2 >= 2 and capi.last_launch_count() >= 2
        finally:
            capi.set_memory_budget(0)
        assert np.array_equal(f0, f2) and np.array_equal(v0, v2), (f0, f2, v0, v2)
        capi.set_memory_budget(2 * 57 * 61 * 3 * 40 * 8 + 4096)   # two of the largest lattices: three chunks or more
        try:
            m2 = dev.forward(capi.MB_MATERIALISE)
            assert capi.last_launch_count() >= 3
        finally:
            capi.set_memory_budget(0)
        assert np.array_equal(m0, m2)
    finally:
        dev.close(); dm.close()


def test_many_scratch_rings_packed_in_one_launch():
    """Twenty-four workgroups, eighteen with a ring of their own in the scratch buffer (S = 570 with levels, shapes around (3, 3)):
    three workgroups to a die, so rings packed on top of each other meet in one L2 (docs/profile_tapes.md, "Edges").  Against the
    restatement, and every pair alone returns the bits it had in the batch."""
    em, pairs = th.packed_case()
    dp = TwoProfileDP(em)
    want = np.array([dp.forward(A, B)[0] for A, B in pairs]); wv = np.array([dp.forward(A, B, "max")[0] for A, B in pairs])
    assert (want > -math.inf).all()
    scratch = [th.ring_bytes(th.PACKED_S, K, L) > th.RING_LDS_MAX for K, L in th.PACKED_SHAPES]
    assert sum(scratch) == 18 and all(scratch[k] == scratch[k + 8] for k in range(16))
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    try:
        f0, v0 = _rolling(dev)
        th.note("forward", f0, want, th.WORST)
        assert logs_close(f0, want), (f0, want)
        assert logs_close(v0, wv, 1e-12), (v0, wv)
        f1, v1 = _rolling(dev)
        assert np.array_equal(f0, f1) and np.array_equal(v0, v1)
        assert np.array_equal(dev.forward(capi.MB_MATERIALISE), f0)
        for k, pair in enumerate(pairs):
            one = _twos(dm, [pair])
            try:
                f, v = _rolling(one)
            finally:
                one.close()
            assert f[0] == f0[k] and v[0] == v0[k], (k, f, f0[k], v, v0[k])
    finally:
        dev.close(); dm.close()


# ---- 4. counts past the LDS table ----------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table():
    """11 204 transitions (S = 700 with levels): beyond the 8 192 the workgroup keeps in LDS every posterior goes into the global
    table with an atomic of its own.  Three pairs at (3, 4), (4, 3) and (0, 3) and a dead pair (a row of B all -inf), which adds
    nothing in either mode.  With MB_DETERMINISTIC=1 the adds are 64-bit fixed point at 2^-36, each rounded to the nearest: a
    transition receives at most one add per cell, (K + 1)(L + 1) = 20 + 20 + 4 = 44 over the three pairs, so at most 44 x 2^-37 =
    3.2e-10 of error, under the 1e-9 floor of counts_close -- the project's bound holds for the fixed point as it stands; and the
    same bits twice."""
    assert sum((K + 1) * (L + 1) for K, L in th.COUNT_SHAPES) * 2.0 ** -37 < 1e-9
    em, pairs, dead = th.big_counts_case()
    assert em.nTransitions > 8192
    dp = TwoProfileDP(em)
    res = [dp.counts(A, B) for A, B in pairs]
    wc, want = np.sum([c for c, _ in res], axis=0), np.array([ll for _, ll in res])
    assert (want > -math.inf).all() and (wc > 0).sum() > 8192
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    both = _twos(dm, pairs[:1] + [dead] + pairs[1:])
    try:
        c, s, ll = dev.counts()
        th.note_counts(c, wc, th.WORST)
        assert counts_close(c, wc) and logs_close(ll, want) and abs(s - want.sum()) <= 1e-9 * abs(want.sum())
        c, s, ll = both.counts()
        assert counts_close(c, wc) and ll[1] == -math.inf and s == -math.inf and logs_close(np.delete(ll, 1), want)
        capi.set_option("MB_DETERMINISTIC", "1")
        try:
            d1 = dev.counts(); d2 = dev.counts(); d3 = both.counts()
        finally:
            capi.set_option("MB_DETERMINISTIC", None)
        assert np.array_equal(d1[0], d2[0]) and d1[0].any() and np.array_equal(d1[2], d2[2])
        th.note_counts(d1[0], wc, th.WORST, "fixed-point counts")
        assert counts_close(d1[0], wc), np.abs(d1[0] - wc).max()
        assert np.array_equal(d3[0], d1[0])                  # integer adds: the dead pair's nothing leaves the same bits
    finally:
        both.close(); dev.close(); dm.close()


# ---- 5. profiles at their edges --------------------------------------------------------------------------------------------------------
def test_special_profiles():
    """All-blank rows on either tape and on both, a whole -inf row on either tape (a dead pair: -inf, an empty path, no counts), an
    eighth of the weights -inf: one batch, everything against the restatement."""
    em, pairs = th.special_profiles()
    refs = th.check_machine(em, pairs)
    lls = [r["ll"] > -math.inf for r in refs]
    assert lls[:3] == [True] * 3 and lls[3:5] == [False] * 2 and any(lls[5:])
    assert all(len(r["path"][0]) == 0 and not r["counts"].any() for r in refs[3:5])


def test_lattice_far_below_zero():
    """Every entry of both profiles 700 lower: likelihoods near -12 600, where exp() of a cell is 0 and only differences survive.  The
    counts are those of the unshifted profiles: a constant per row cancels in the posterior."""
    em, A, B, Afar, Bfar = th.far_case()
    refs = th.check_machine(em, [(Afar, Bfar)])
    assert refs[0]["ll"] < -12000.0
    near = TwoProfileDP(em).counts(A, B)[0]
    assert counts_close(refs[0]["counts"], near)
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, [(Afar, Bfar), (A, B)])
    try:
        assert counts_close(dev.counts()[0], 2.0 * near)
        ll = dev.forward(capi.MB_ROLLING)
        assert abs((ll[1] - ll[0]) + 18 * th.FAR_SHIFT) <= 1e-9 * abs(ll[0])
    finally:
        dev.close(); dm.close()


# ---- 6. ties and full slots ------------------------------------------------------------------------------------------------------------
def _equal_paths(dm, em, pairs, census=None):
    """Scores, edges, both coordinates and every Viterbi cell equal (==) to the restatement's, for sums that are exact."""
    dp = TwoProfileDP(em)
    refs = [dp.viterbi(A, B, census) for A, B in pairs]
    dev = _twos(dm, pairs)
    try:
        v, off, edges, rows, ins = dev.viterbi()
        assert np.array_equal(dev.viterbi(paths=False)[0], v)
    finally:
        dev.close()
    for k, ((A, B), (wv, we, wr, wi)) in enumerate(zip(pairs, refs)):
        sl = slice(off[k], off[k + 1])
        assert wv > -math.inf and v[k] == wv, (k, v[k], wv)
        assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr) and np.array_equal(ins[sl], wi), (k, edges[sl], we)
        assert np.array_equal(capi.profile_two_fill(dm, capi.MB_VITERBI, A, B), np.stack(dp.forward(A, B, "max")[1:], axis=2)), k
    return refs


def test_ties_are_decided_by_candidate_order():
    """The tie machine, K, L in 1..4, as one batch of sixteen pairs: the weights are multiples of log 0.5 and the profiles' are 0, so
    every sum is exact and equal candidates are equal on the device too.  The census of what was just compared holds every kind of
    tie -- N: output blank / match, match / output-only; W: stay / input-only, input-only / silent; Z: W / input blank -- so equal
    paths mean the device took the first candidate at each.  Then the two machines worked by hand."""
    em = th.tie_machine()
    dm = capi.DeviceMachine(em)
    census = {}
    try:
        refs = _equal_paths(dm, em, th.tie_pairs(), census)
    finally:
        dm.close()
    assert len(refs) == 16
    met = {(a, b) for kinds in census for a in kinds for b in kinds if kinds.index(a) < kinds.index(b)}
    for kinds in th.TIE_KINDS:
        assert kinds in met, (kinds, census)
    for em, A, B, edges, rows, ins in th.hand_tie_cases():
        dm = capi.DeviceMachine(em)
        try:
            (v, e, r, i), = _equal_paths(dm, em, [(A, B)])
        finally:
            dm.close()
        assert v == 0.0 and list(e) == edges and list(r) == rows and list(i) == ins


def test_full_traceback_slots():
    """The chain machine (S = 5) against profiles without blanks on either tape: every path has exactly K + L + (K + L + 1)(nLevF - 1)
    edges, the size of its slot, so six slots lie end to end without a free entry between them and a slot base, a bound or a
    reversal that is off by one lands in a neighbour -- in any of the three arrays."""
    em, pairs = th.chain_case()
    dp = TwoProfileDP(em)
    refs = [dp.viterbi(A, B) for A, B in pairs]
    bounds = [len(A) + len(B) + (len(A) + len(B) + 1) * (th.CHAIN_S - 1) for A, B in pairs]
    assert [len(r[1]) for r in refs] == bounds and bounds[0] == 39 and all(r[0] > -math.inf for r in refs)
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, pairs)
    try:
        assert dev.path_cap() == sum(bounds)
        v, off, edges, rows, ins = dev.viterbi(cap=dev.path_cap())
        assert list(np.diff(off)) == bounds and len(edges) == sum(bounds)
        for k, (wv, we, wr, wi) in enumerate(refs):
            sl = slice(off[k], off[k + 1])
            assert abs(v[k] - wv) <= 1e-12 * max(1.0, abs(wv)), (k, v[k], wv)
            assert np.array_equal(edges[sl], we) and np.array_equal(rows[sl], wr) and np.array_equal(ins[sl], wi), k
        res = [dp.counts(A, B) for A, B in pairs]
        c, s, ll = dev.counts()
        assert counts_close(c, np.sum([r[0] for r in res], axis=0)) and logs_close(ll, [r[1] for r in res])
    finally:
        dev.close(); dm.close()


# ---- 7. errors: raised before anything is launched ---------------------------------------------------------------------------------------
def test_errors_launch_nothing():
    em = th.pair_machine(8, 2, True, 2, 3)
    A, B = th.two_input(np.random.RandomState(2), em, 3, 4, pInf=0.0)
    dm = capi.DeviceMachine(em)
    dev = _twos(dm, [(A, B), (A[:1], B)])
    try:
        assert (dev.forward(capi.MB_ROLLING) > -math.inf).all() and capi.last_launch_count() == 1
        for table in (0, 1):
            for bad in (np.nan, np.inf):
                X, Y = A.copy(), B.copy()
                (X, Y)[table][1, 1] = bad
                n = capi.last_launch_count()
                with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
                    _twos(dm, [(X, Y)])
                assert capi.last_launch_count() == n
                with pytest.raises(capi.MbError, match="NaN or \\+infinity"):
                    capi.profile_two_fill(dm, capi.MB_FORWARD, X, Y)
                assert capi.last_launch_count() == 0
        dev.forward(capi.MB_ROLLING)
        with pytest.raises(capi.MbError, match="pathCap too small"):
            dev.viterbi(cap=dev.path_cap() - 1)
        assert capi.last_launch_count() == 0
        capi.set_memory_budget(1024)
        try:
            for call in (lambda: dev.forward(capi.MB_MATERIALISE), dev.viterbi, dev.counts, lambda: capi.profile_two_fill(dm, capi.MB_FORWARD, A, B)):
                with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
                    call()
                assert capi.last_launch_count() == 0
        finally:
            capi.set_memory_budget(0)
        with pytest.raises(capi.MbError, match="unknown flags"):
            dev.forward(7)
        assert (dev.forward(capi.MB_ROLLING) > -math.inf).all()
    finally:
        dev.close(); dm.close()
    from randmachine import random_machine
    gen = random_machine(8, 0, 2, 41)                       # a generator: no input alphabet
    dg = capi.DeviceMachine(gen)
    try:
        for call in (lambda: capi.DeviceProfileTwos(dg, [np.zeros((0, 1))], [np.zeros((2, 3))]),
                     lambda: capi.profile_two_fill(dg, capi.MB_FORWARD, np.zeros((0, 1)), np.zeros((2, 3)))):
            with pytest.raises(capi.MbError, match="two-profile sweeps need a machine with an input alphabet"):
                call()
    finally:
        dg.close()
    assert not hasattr(capi.DeviceProfileTwos, "set_envelopes")


# ---- 8. the Python entry point and the command line --------------------------------------------------------------------------------------
def _dnastore(tmp_path):
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    return m, par, EvaluatedMachine.fromMachine(m, par), str(a), Profile.fromCsv(str(a)), Profile.fromCsv(CSV)


def test_score_two_profiles_device_equals_numpy(tmp_path):
    m, par, em, _, pa, pb = _dnastore(tmp_path)
    ins = [pa, Profile(pa.header, pa.row[:1]), Profile(pa.header, [])]
    dev, dc = boss.scoreTwoProfiles(m, ins, pb, backend="device", params=par, loglike=True, viterbi=True, counts=True)
    ref, rc = boss.scoreTwoProfiles(m, ins, pb, backend="numpy", params=par, loglike=True, viterbi=True, counts=True)
    assert logs_close(dev["loglike"], ref["loglike"]) and logs_close(dev["viterbi"], ref["viterbi"], 1e-12) and dc == rc
    assert np.mean(np.array(ref["loglike"]) > -math.inf) >= 0.6
    bit = Machine.fromFile("tests/golden/machine/bitnoise.json")          # a machine with parameters
    pb2 = json.load(open("tests/golden/io/params.json"))
    soft = Profile(["0", "1"], [[.6, .3, .1], [.2, .7, .1], [.45, .45, .1]])
    out = Profile.fromCsv("tests/golden/csv/prof001.csv")
    dev, dc = boss.scoreTwoProfiles(bit, [soft], out, backend="device", params=pb2, counts=True)
    ref, rc = boss.scoreTwoProfiles(bit, [soft], out, backend="numpy", params=pb2, counts=True)
    assert ref["loglike"][0] > -math.inf and logs_close(dev["loglike"], ref["loglike"])
    assert dc.keys() == rc.keys() and all(abs(dc[k] - rc[k]) <= 1e-6 * max(1.0, abs(rc[k])) for k in rc), (dc, rc)


def test_cli_on_dnastore(tmp_path):
    m, par, em, a, pa, pb = _dnastore(tmp_path)
    dp = TwoProfileDP(em)
    A, B = pa.logRowsIn(em), pb.logRows(em)

    def run(*flags):
        out = io.StringIO()
        assert boss.run([DNASTORE, "--use-defaults", "--generate-csv", a, "--recognize-csv", CSV] + list(flags), out) == 0
        return out.getvalue()
    for flag, mode in (("-L", "exact"), ("-V", "max")):
        got = json.loads(run(flag))
        want = dp.forward(A, B, mode)[0]
        assert got[0][:2] == [a, ""] and want > -math.inf and abs(got[0][2] - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
        assert run(flag) == run(flag, "--decode-backend", "numpy")
    assert json.loads(run("-C")) == {}
    assert capi.last_kernel_name() == "k_profile_two_counts"
