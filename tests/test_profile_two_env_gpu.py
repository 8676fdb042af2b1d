"""GPU tests of the two-profile sweeps under an envelope (the TwoEnvGeom instantiations of mb_profile_two.hip; docs/profile_tapes.md,
"Pairs of profiles under an envelope"): capi.DeviceProfileTwos(envs=...) against profile.TwoProfileDP(env=...), which
test_profile_two_env_host.py holds to path enumeration, to the pair sweep and to its own identities without a GPU, and which also
holds the inputs built by twoenvhelpers to the conditions named here.

Bounds (pairprofilehelpers): likelihoods and cells 1e-9 relative to max(1, |value|), -inf matching exactly; counts and posteriors
1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; Viterbi scores 1e-12 with paths, output rows and input rows equal."""
import math

import numpy as np
import pytest
import torch

import twoenvhelpers as te
import twoposthelpers as tp
import twoprofilehelpers as th
from pairenvhelpers import full, n_cells, staircase
from pairprofilehelpers import counts_close, logs_close
from twoenvhelpers import WORST, check_env_batch, open_twos
from machineboss_amd import boss, capi
from machineboss_amd.profile import TwoProfileDP
from machineboss_amd.seqpair import Envelope
from machineboss_amd.torchprofile import two_profile_loglike

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() == 0:
        pytest.fail("no GPU visible")
    capi.set_device(0)
    yield
    capi.set_memory_budget(0)
    capi.set_option("MB_DETERMINISTIC", None)
    capi.set_option("MB_ROWPOST_TABLE", None)
    print("worst deviations of the two-profile sweeps under an envelope:", WORST, tp.WORST)


def everything(dev, posteriors=True):
    """Every result of one object, for comparisons bit by bit: Forward in both modes, Viterbi with paths, counts, both tables."""
    out = [dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]]
    out += list(dev.viterbi())
    c, s, ll = dev.counts()
    out += [c, np.array([s]), ll]
    if posteriors:
        out += list(dev.row_posteriors())
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. every cell, every sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", te.CELL_STATES)
def test_every_cell_under_every_envelope(S):
    """The machine with silent levels and without at the seven lattices from (0, 0) to (9, 9) under the full envelope, band(0),
    band(1), a path envelope and a staircase of single cells, each machine's pairs in one batch: scores, paths, counts and both
    posterior tables, then every cell of the Forward, max and Backward fills, all three layers exactly -inf outside."""
    case = te.cell_case(S)
    live = []
    for em in {id(c[0]): c[0] for c in case}.values():
        triples = [(A, B, env) for e, A, B, _, env in case if e is em]
        assert {c[3] for c in case if c[0] is em} == set(te.ENV_KINDS)
        check_env_batch(em, triples, fill=True, live=live)
    assert np.mean(live) >= 0.75, np.mean(live)


# ---- 2. the rings -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def marks():
    """The four band pairs at S = 40, K = L = 72 and the three extras, with the yardstick's likelihood and Viterbi score of each."""
    em = te.mark_machine()
    triples = [te.mark_case(M) for M in te.MARK_M] + list(te.mark_extras())
    dp = TwoProfileDP(em)
    return em, triples, [(dp.forward(A, B, env=env)[0], dp.forward(A, B, "max", env=env)[0]) for A, B, env in triples]


@pytest.mark.parametrize("which", range(len(te.MARK_M)))
def test_ring_marks_alone(marks, which):
    """M = 22 / 23 is 63 360 / 66 240 bytes, either side of the 64 KiB opt-in; M = 56 / 57 is 161 280 / 164 160 bytes, the last ring
    in LDS and the first in scratch.  Rolling Forward, the materialised Forward (the same bits), the rolling Viterbi score and the
    yardstick's."""
    em, triples, want = marks
    assert te.ring_bytes(em.nStates, te.diag_max(triples[which][2])) == (63360, 66240, 161280, 164160)[which]
    dm, dev = open_twos(em, [triples[which]])
    try:
        fr, fm, v = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]
        assert capi.last_kernel_name() == "k_profile_two_env_fwd<max,rolling>" and capi.last_launch_count() == 1
        assert np.array_equal(fr, fm) and logs_close(fr, [want[which][0]]) and logs_close(v, [want[which][1]], 1e-12), (fr, fm, v, want[which])
        assert dev.cells() == 3 * em.nStates * n_cells(triples[which][2])
    finally:
        dev.close(); dm.close()


def test_ring_marks_in_one_ragged_launch(marks):
    """The four beside a pair given None, a (0, 0) pair and a dead pair: LDS and scratch rings in one launch.  Every pair alone
    returns its bits of the batch."""
    em, triples, want = marks
    dm, dev = open_twos(em, triples)
    try:
        fr, fm, v = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE), dev.viterbi(paths=False)[0]
        assert capi.last_launch_count() == 1
        assert np.array_equal(fr, fm) and logs_close(fr, [w[0] for w in want]) and logs_close(v, [w[1] for w in want], 1e-12)
        assert fr[-1] == -math.inf and (fr[:-1] > -math.inf).all()
    finally:
        dev.close(); dm.close()
    for k, t in enumerate(triples):
        dm, one = open_twos(em, [t])
        try:
            assert one.forward(capi.MB_ROLLING)[0] == fr[k] and one.viterbi(paths=False)[0][0] == v[k], k
        finally:
            one.close(); dm.close()


@pytest.mark.parametrize("K,L,w", te.SLOPE_CASES)
def test_i_mod_m_with_k_far_past_m(K, L, w):
    """(200, 40) under band(6) and (40, 200) under band(2) at S = 8: the ring slot i mod M wraps many times."""
    check_env_batch(te.slope_machine(), [te.slope_case(K, L, w)], post=False)


def test_scratch_rings_side_by_side():
    """Twenty-four pairs with rings of 194 400 bytes in scratch at S = 300, in one launch: rings that overlapped would show."""
    em, pairs, env = te.pack_case()
    dp = TwoProfileDP(em)
    want = np.array([dp.forward(A, B, env=env)[0] for A, B in pairs])
    dm, dev = open_twos(em, [(A, B, env) for A, B in pairs])
    try:
        fr = dev.forward(capi.MB_ROLLING)
        assert capi.last_launch_count() == 1 and capi.last_kernel_name() == "k_profile_two_env_fwd<sum,rolling>"
        fm = dev.forward(capi.MB_MATERIALISE)
        assert np.array_equal(fr, fm) and logs_close(fr, want) and (want > -math.inf).all()
        assert np.array_equal(dev.viterbi(paths=False)[0], dev.viterbi()[0])
    finally:
        dev.close(); dm.close()


# ---- 3. the full envelope is no envelope ---------------------------------------------------------------------------------------------------------
def test_full_envelope_returns_the_bits_of_none():
    """On the ragged batch: Forward in both modes, Viterbi with paths, fixed-point counts and both posterior tables.  A batch in
    which one pair alone has an envelope (full) runs every pair through the envelope kernels, and still the same bits."""
    em, pairs = te.ragged_case()
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        dm, dev = open_twos(em, [(A, B, None) for A, B in pairs])
        try:
            plain = everything(dev)
            assert capi.last_kernel_name() == "k_profile_two_rowpost" and dev.cells() == sum(3 * em.nStates * (len(A) + 1) * (len(B) + 1) for A, B in pairs)
            dev.envelopes([full(len(A), len(B)) for A, B in pairs])
            enveloped = everything(dev)
            assert capi.last_kernel_name() == "k_profile_two_env_rowpost" and capi.last_launch_count() == 1
            dev.envelopes([None] * 3 + [full(len(pairs[3][0]), len(pairs[3][1]))] + [None] * (len(pairs) - 4))
            mixed = everything(dev)
            assert capi.last_kernel_name() == "k_profile_two_env_rowpost" and capi.last_launch_count() == 1
        finally:
            dev.close(); dm.close()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
    assert same_bits(plain, enveloped) and same_bits(plain, mixed)
    assert plain[0][te.RAGGED_DEAD] == -math.inf and np.isfinite(np.delete(plain[0], te.RAGGED_DEAD)).all()


# ---- 4. counts ----------------------------------------------------------------------------------------------------------------------------------
def test_counts_past_the_lds_table():
    """11 204 transitions under band(2), beside a dead pair: floating point against the yardstick; fixed point the same bits twice
    and the sum of the pairs run alone."""
    em, triples = te.big_counts_env_case()
    dp = TwoProfileDP(em)
    want = np.sum([dp.counts(A, B, env=env)[0] for A, B, env in triples], axis=0)
    cells = sum(n_cells(env) for _, _, env in triples)
    dm, dev = open_twos(em, triples)
    try:
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_env_counts" and capi.last_launch_count() == 1
        assert counts_close(c, want) and ll[-1] == -math.inf and s == -math.inf
        capi.set_option("MB_DETERMINISTIC", "1")
        d0, _, _ = dev.counts()
        d1, _, _ = dev.counts()
        assert np.array_equal(d0, d1) and th.fixed_counts_close(d0, want, cells)
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()
    capi.set_option("MB_DETERMINISTIC", "1")
    try:
        alone = np.zeros_like(d0)
        for t in triples:
            dm, one = open_twos(em, [t])
            try:
                alone += one.counts()[0]
            finally:
                one.close(); dm.close()
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
    assert np.array_equal(alone, d0)


# ---- 5. row posteriors, both axes ------------------------------------------------------------------------------------------------------------------
def test_posteriors_over_columns_of_one_two_and_many_cells():
    """An envelope whose input rows hold a run of many output rows, of two and of one: the bisection in colOff and the lines of
    unequal length, under the default table and under one of 4 doubles (a line a block)."""
    em, A, B, env = te.post_stairs_case()
    refs = check_env_batch(em, [(A, B, env)], fill=True)
    capi.set_option("MB_ROWPOST_TABLE", "4")
    try:
        check_env_batch(em, [(A, B, env)], refs=refs)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)


@pytest.mark.parametrize("table", te.LONG_TABLES)
@pytest.mark.parametrize("K,L", te.LONG_SHAPES)
def test_more_line_blocks_than_groups(K, L, table):
    """S = 2 at (1, 1 100) and (1 100, 1) under the staircase: with a table of 4 doubles a line is a block, 1 100 blocks against
    1 024 groups on the long axis; with 2 the bins are global; and the default.  Row sums 1 on both tables, column sums the counts
    of the same object, the dead pair's rows exactly zero."""
    em, triples = te.long_case(K, L)
    dp = TwoProfileDP(em)
    refs = [dp.rowPosteriors(A, B, env=env) for A, B, env in triples]
    capi.set_option("MB_ROWPOST_TABLE", table)
    dm, dev = open_twos(em, triples)
    try:
        pa, pb, ll = dev.row_posteriors()
        assert capi.last_kernel_name() == "k_profile_two_env_rowpost" and capi.last_launch_count() == 1
        gotA, gotB = tp.split(dev, pa, pb)
        tp.compare(em, gotA, gotB, ll, refs, "long lines under an envelope")
        assert ll[0] > -math.inf and ll[1] == -math.inf and not gotA[1].any() and not gotB[1].any()
        c, _, _ = dev.counts()
        ga, gb = tp.grouped(em, c)
        assert counts_close(pa[:, 1:].sum(axis=0), ga) and counts_close(pb[:, 1:].sum(axis=0), gb)
    finally:
        capi.set_option("MB_ROWPOST_TABLE", None)
        dev.close(); dm.close()


# ---- 6. chunks ----------------------------------------------------------------------------------------------------------------------------------------
def test_chunks_by_the_compact_lattices():
    """S = 65 at K = L = 100 under band(4) with the budget at a quarter of a rectangle: three pairs in three chunks.  Floating point against
    the yardstick; chunked counts and posteriors in fixed point give the unchunked bits."""
    em, pairs, env = te.chunk_case()
    triples = [(A, B, env) for A, B in pairs]
    dp = TwoProfileDP(em)
    refs = []
    for A, B, env in triples:      # (the two calls the chunks are asked for, and no more: the yardstick is most of this test's time)
        c, ll = dp.counts(A, B, env=env)
        refs.append(dict(counts=c, ll=ll, post=dp.rowPosteriors(A, B, env=env)))
    dm, dev = open_twos(em, triples)
    try:
        capi.set_memory_budget(te.chunk_budget())
        c, s, ll = dev.counts()
        assert capi.last_launch_count() == 3
        assert counts_close(c, np.sum([r["counts"] for r in refs], axis=0)) and logs_close(ll, [r["ll"] for r in refs])
        pa, pb, pl = dev.row_posteriors()
        assert capi.last_launch_count() >= 3
        tp.compare(em, *tp.split(dev, pa, pb), pl, [r["post"] for r in refs], "chunked under an envelope")
        assert logs_close(dev.forward(capi.MB_MATERIALISE), [r["ll"] for r in refs])
        capi.set_option("MB_DETERMINISTIC", "1")
        chunked = [dev.counts()[0]] + list(dev.row_posteriors())
        capi.set_memory_budget(0)
        whole = [dev.counts()[0]] + list(dev.row_posteriors())
        assert capi.last_launch_count() == 1
        assert same_bits(chunked, whole)
        capi.set_memory_budget(te.lattice_bytes(em.nStates, env) - 8)
        with pytest.raises(capi.MbError, match="exceeds the device memory budget"):
            dev.forward(capi.MB_MATERIALISE)
    finally:
        capi.set_memory_budget(0)
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


# ---- 7. ties, the pair family ---------------------------------------------------------------------------------------------------------------------------
def test_ties_under_a_band():
    em = th.tie_machine()
    check_env_batch(em, te.tie_env_pairs(), fill=True)


def test_one_hot_input_is_the_pair_sweep_under_the_same_envelope():
    """A one-hot A (its blank -inf) under band(3) against DeviceProfilePairs under the same envelope: likelihood and Viterbi score
    1e-9 / 1e-12, counts and the output-row posteriors as counts, the same path."""
    em, x, A, B, env = te.onehot_case()
    dm = capi.DeviceMachine(em)
    two = capi.DeviceProfileTwos(dm, [A], [B], envs=[env])
    one = capi.DeviceProfilePairs(dm, [x], [B])
    try:
        one.set_envelopes([env])
        assert logs_close(two.forward(), one.forward()) and logs_close(two.forward(capi.MB_MATERIALISE), one.forward(capi.MB_MATERIALISE))
        v2, _, e2, r2, i2 = two.viterbi()
        v1, _, e1, r1 = one.viterbi()
        assert v2[0] > -math.inf and logs_close(v2, v1, 1e-12) and np.array_equal(e2, e1) and np.array_equal(r2, r1)
        assert counts_close(two.counts()[0], one.counts()[0])
        assert counts_close(two.row_posteriors()[1], one.row_posteriors()[0])
    finally:
        two.close(); one.close(); dm.close()


# ---- 8. state, errors, entry points ------------------------------------------------------------------------------------------------------------------------
def test_envelopes_set_changed_cleared():
    """Envelopes set, changed, cleared, and set_profiles in between: each state equals a fresh object's."""
    em, pairs = te.ragged_case()
    rng = np.random.RandomState(5)
    bands = [te.band_or_full(len(A), len(B), 1) for A, B in pairs]
    stairs = [staircase(len(A), len(B)) if k % 2 else None for k, (A, B) in enumerate(pairs)]
    other = [th.two_input(rng, em, len(A), len(B), pInf=0.0) for A, B in pairs]

    def fresh(ps, envs):
        dm, dev = open_twos(em, [(A, B, e) for (A, B), e in zip(ps, envs)]) if envs is not None else tp.open_pairs(em, ps)
        try:
            return everything(dev), capi.last_kernel_name(), dev.cells()
        finally:
            dev.close(); dm.close()
    capi.set_option("MB_DETERMINISTIC", "1")
    dm, dev = tp.open_pairs(em, pairs)
    try:
        states = []
        for ps, envs in ((pairs, None), (pairs, bands), (other, bands), (other, stairs), (other, None), (pairs, None), (pairs, stairs)):
            if ps is not states[-1][0] if states else False:
                dev.set_profiles([A for A, _ in ps], [B for _, B in ps])
            if envs is not (states[-1][1] if states else None):
                dev.envelopes(envs)
            states.append((ps, envs))
            got = everything(dev), capi.last_kernel_name(), dev.cells()
            want = fresh(ps, envs)
            assert same_bits(got[0], want[0]) and got[1:] == want[1:], len(states)
            assert got[1] == ("k_profile_two_rowpost" if envs is None else "k_profile_two_env_rowpost")
    finally:
        capi.set_option("MB_DETERMINISTIC", None)
        dev.close(); dm.close()


def test_errors_leave_the_object_without_envelopes():
    em = th.split_machine()
    A, B = th.two_input(np.random.RandomState(1), em, 3, 2, pInf=0.0)
    dm, dev = tp.open_pairs(em, [(A, B)])
    try:
        plain = everything(dev)
        launches = capi.last_launch_count()
        bad = (([0, 0], [4, 4], "Envelope/sequence mismatch"), ([0, 0, 0], [4, 4, 5], "Envelope/sequence mismatch"),
               ([0, 0, -1], [4, 4, 4], "Envelope/sequence mismatch"), ([0, 2, 3], [1, 3, 4], "Envelope is not connected"),
               ([1, 0, 0], [4, 4, 4], "Envelope is not connected"), ([0, 0, 0], [4, 4, 3], "Envelope is not connected"),
               ([0, 0, 0], [4, 3, 4], "Envelope is not monotone"))
        for st, en, msg in bad:
            dev.envelopes([Envelope.band(3, 2, 1)])
            assert dev.cells() < 3 * em.nStates * 12
            with pytest.raises(capi.MbError, match=msg):
                dev.envelopes([(st, en)])
            assert capi.last_launch_count() == launches and dev.cells() == 3 * em.nStates * 12
        for st, en, msg in bad:      # (a fill that reaches the library starts a call of its own: it launches nothing and reports no launch)
            with pytest.raises(capi.MbError, match=msg):
                capi.profile_two_fill(dm, capi.MB_FORWARD, A, B, (st, en))
            assert capi.last_launch_count() == (0 if len(st) == len(B) + 1 else launches)
            launches = capi.last_launch_count()
        with pytest.raises(ValueError, match="one envelope"):
            dev.envelopes([None, None])
        with pytest.raises(capi.MbError, match="Envelope/sequence mismatch"):
            capi.DeviceProfileTwos(dm, [A], [B], envs=[([0], [4])])
        assert same_bits(everything(dev), plain) and capi.last_kernel_name() == "k_profile_two_rowpost"
        assert not hasattr(capi.DeviceProfileTwos, "set_envelopes")
    finally:
        dev.close(); dm.close()


def test_entry_points():
    """two_profile_loglike(backend="device", envs=...) against the numpy backend, values and both gradients;
    boss.scoreTwoProfiles(band=2) on the device against numpy."""
    em = th.split_machine()
    rng = np.random.RandomState(3)
    shapes = ((5, 6), (0, 3), (7, 7), (4, 0))
    pairs = [th.two_input(rng, em, K, L, pInf=0.0) for K, L in shapes]
    envs = [Envelope.band(5, 6, 2), None, Envelope.band(7, 7, 1), None]
    inOff, rowOff = np.cumsum([0] + [K for K, _ in shapes]), np.cumsum([0] + [L for _, L in shapes])
    res = {}
    for backend in ("device", "numpy"):
        a = torch.tensor(np.concatenate([A for A, _ in pairs]), dtype=torch.float64, requires_grad=True)
        b = torch.tensor(np.concatenate([B for _, B in pairs]), dtype=torch.float64, requires_grad=True)
        ll = two_profile_loglike(em, a, inOff, b, rowOff, envs=envs, backend=backend)
        (ll * torch.arange(1, 5, dtype=torch.float64)).sum().backward()
        res[backend] = (ll.detach().numpy(), a.grad.numpy(), b.grad.numpy())
    assert capi.last_kernel_name() == "k_profile_two_env_rowpost"
    assert logs_close(res["device"][0], res["numpy"][0]) and (res["numpy"][0] > -math.inf).all()
    assert counts_close(res["device"][1], res["numpy"][1]) and counts_close(res["device"][2], res["numpy"][2])
    m = th.machine_of(em)
    pb = th.profile_of(em.outputTokenizer.tok2sym[1:], pairs[0][1])
    pas = [th.profile_of(em.inputTokenizer.tok2sym[1:], A) for A, _ in (pairs[0], pairs[2])]
    dev, dc = boss.scoreTwoProfiles(m, pas, pb, backend="device", params={}, viterbi=True, counts=True, posteriors=True, band=2)
    ref, rc = boss.scoreTwoProfiles(m, pas, pb, backend="numpy", params={}, viterbi=True, counts=True, posteriors=True, band=2)
    assert logs_close(dev["loglike"], ref["loglike"]) and logs_close(dev["viterbi"], ref["viterbi"], 1e-12)
    for (da, db), (ra, rb) in zip(dev["posteriors"], ref["posteriors"]):
        assert counts_close(da, ra) and counts_close(db, rb)
    assert dc == rc == {}                                 # (numeric weights: no parameters)
    plain, _ = boss.scoreTwoProfiles(m, pas, pb, backend="device")
    assert all(p > d for p, d in zip(plain["loglike"], dev["loglike"]))
