"""Row posteriors of the two-profile sweeps against CTC-merged output profiles without a GPU (docs/profile_tapes.md, "Row posteriors
of pairs of profiles against a merged profile"): profile.TwoMergedProfileDP.mergedRowPosteriors held to facts it does not compute
itself -- every row of either table sums to 1, the column sums are the grouped counts() and the three masses of counts(blanks=),
postB[r][c] and postA[i][a] are the derivatives of forward() in B[r][c] and in A[i][a], K = 0 is MergedProfileDP.rowPosteriors, a
one-hot A is PairMergedProfileDP.rowPosteriors, one column per token against one-hot rows is TwoProfileDP.rowPosteriors, and the
one-state echo transducer is the CTC loss; then the layers above it: torchprofile.merged_two_profile_loglike on the numpy backend,
boss.mergedTwoPosteriors, the new error messages and the old refusals; and the input families of
test_profile_two_merge_post_gpu.py held to their conditions.

Bounds: entries as counts (pairprofilehelpers: 1e-6 relative from 1e-3 up, 1e-9 + 1e-6 x value below), row sums 1e-6, column sums
against the counts 1e-12 (the same terms in another order), central differences at h = 1e-6 within 1e-7 absolute (truncation about
h^2, rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100), likelihoods against -ctc_loss 1e-9."""
import math

import numpy as np
import pytest
import torch

import twomergehelpers as tm
import twomergeposthelpers as tq
import twoprofilehelpers as th
from pairprofilehelpers import counts_close, logs_close, pair_machine
from twomergeposthelpers import FD_H, FD_TOL, ROW_TOL
from machineboss_amd import boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile, TwoMergedProfileDP, TwoProfileDP
from machineboss_amd.torchprofile import merged_two_profile_loglike, two_profile_loglike

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"
SUM_TOL = 1e-12


@pytest.fixture(scope="module")
def swept():
    """[(em, colTok, dp, A, B, postA, postB, repeats, ll)]: the host grid, the yardstick run once."""
    out, dps = [], {}
    for em, colTok, A, B in tq.host_cases():
        dp = dps.setdefault((id(em), colTok), TwoMergedProfileDP(em, colTok))
        rep = []
        postA, postB, ll = dp.mergedRowPosteriors(A, B, repeats=rep)
        out.append((em, colTok, dp, A, B, postA, postB, rep[0], ll))
    return out


def test_rows_sum_to_one_and_columns_group_the_counts(swept):
    """Row sums of both tables; sum_i postA[i][a] against the counts() of the transitions reading a and sum_i postA[i][0] against the
    input-blank mass; postB - repeats per token against the counts() of the transitions writing it, the blank column and the
    repeats against the other two masses."""
    live, worstRow, worstGroup = [], 0.0, 0.0
    for em, colTok, dp, A, B, postA, postB, rep, ll in swept:
        blanks = []
        c, ll2 = dp.counts(A, B, blanks=blanks)
        assert postA.shape == A.shape and postB.shape == B.shape == rep.shape and ll == ll2 and ll == dp.forward(A, B)[0]
        live.append(ll > -math.inf)
        if not ll > -math.inf:
            assert not postA.any() and not postB.any() and not rep.any()
            continue
        outBlank, repeat, inBlank = blanks[0]
        byIn, byOut = tq.grouped(em, colTok, c)
        for post, T in ((postA, A), (postB, B)):
            assert (post >= 0.0).all() and not post[T == -math.inf].any()
            if len(T):
                worstRow = max(worstRow, float(np.abs(post.sum(axis=1) - 1.0).max()))
                assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
        assert (rep >= 0.0).all() and (rep <= postB).all() and not rep[:, 0].any()
        gaps = [np.abs(postA.sum(axis=0) - np.concatenate([[inBlank], byIn])).max(),
                np.abs(tq.by_token(em, colTok, (postB - rep).sum(axis=0)[1:]) - byOut).max(),
                abs(postB[:, 0].sum() - outBlank), abs(rep.sum() - repeat)]
        worstGroup = max(worstGroup, float(max(gaps)))
        assert max(gaps) <= SUM_TOL * max(1, len(A), len(B)), (len(A), len(B), gaps)
    print("%d cases, %d finite; row sums off by %.3g, grouped counts and masses by %.3g" % (len(swept), sum(live), worstRow, worstGroup))
    assert len(swept) == 147 and np.mean(live) >= 0.9, (len(swept), np.mean(live))
    assert all(len(set(ct)) < len(ct) for ct in tq.HOST_COLTOK.values() if len(ct) > 1)


def test_row_posteriors_are_the_gradients_of_forward(swept):
    """Central differences of forward() in every finite entry of A and of B, over the cases with K, L <= 3 and |LL| < 100."""
    worst, n = 0.0, 0
    for em, colTok, dp, A, B, postA, postB, rep, ll in swept:
        if len(A) > 3 or len(B) > 3 or not abs(ll) < 100:
            continue
        for t, (T, post) in enumerate(((A, postA), (B, postB))):
            for idx in np.ndindex(*T.shape):
                if T[idx] == -math.inf:
                    continue
                up, dn = T.copy(), T.copy()
                up[idx] += FD_H; dn[idx] -= FD_H
                fd = ((dp.forward(up, B)[0] - dp.forward(dn, B)[0]) if t == 0 else (dp.forward(A, up)[0] - dp.forward(A, dn)[0])) / (2 * FD_H)
                worst = max(worst, abs(fd - post[idx])); n += 1
                assert abs(fd - post[idx]) <= FD_TOL, (t, len(A), len(B), idx, fd, post[idx])
    print("%d derivatives, central differences off by at most %.3g" % (n, worst))
    assert n >= 300


def test_reductions():
    """K = 0: postB is MergedProfileDP.rowPosteriors.  A one-hot A: postB is PairMergedProfileDP.rowPosteriors on the token string and
    postA gives the one-hot rows back.  One column per token against one-hot B rows on a run-free, blank-free string: no blank, no
    repeat, so postA is that of TwoProfileDP.rowPosteriors on the same rows read plainly."""
    for S, levels in ((5, True), (8, False)):
        em = pair_machine(S, 3, levels, 2, 3)
        rng = np.random.RandomState(S)
        colTok = (3, 1, 3, 2)
        B = tm.merged_rows(rng, 4, 4, zeros=0.1)
        two = TwoMergedProfileDP(em, colTok)
        rep, wrep = [], []
        pa, pb, ll = two.mergedRowPosteriors(np.zeros((0, 3)), B, repeats=rep)
        want, wl = MergedProfileDP(em, colTok).rowPosteriors(B, repeats=wrep)
        assert pa.shape == (0, 3) and wl > -math.inf and logs_close([ll], [wl]) and np.abs(pb - want).max() <= 1e-12 and np.abs(rep[0] - wrep[0]).max() <= 1e-12
        x = rng.randint(1, 3, size=3)
        rep, wrep = [], []
        pa, pb, ll = two.mergedRowPosteriors(th.one_hot(x, 2), B, repeats=rep)
        want, wl = PairMergedProfileDP(em, colTok).rowPosteriors(x, B, repeats=wrep)
        assert wl > -math.inf and logs_close([ll], [wl]) and np.abs(pb - want).max() <= 1e-12 and np.abs(rep[0] - wrep[0]).max() <= 1e-12
        hot = np.exp(th.one_hot(x, 2))
        assert not pa[hot == 0.0].any() and np.abs(pa[hot == 1.0] - 1.0).max() <= 1e-12
        y = np.array([1, 3, 1, 2, 3])
        hotB = th.one_hot(y, 3)
        A = th.soft_profile(rng, 4, 2, 0.1)
        pa, pb, ll = TwoMergedProfileDP(em, (1, 2, 3)).mergedRowPosteriors(A, hotB)
        wa, wb, wl = TwoProfileDP(em).rowPosteriors(A, hotB)
        assert wl > -math.inf and logs_close([ll], [wl]) and np.abs(pa - wa).max() <= 1e-12 and np.abs(pb - wb).max() <= 1e-12


@pytest.mark.parametrize("normalised", (True, False))
@pytest.mark.parametrize("T", tq.CTC_T)
def test_echo_transducer_is_the_ctc_loss(T, normalised):
    """The CTC case of test_profile_pair_merge_post_host.py through the new loss with a one-hot logA: x = 1 2 2 3 needs five frames,
    so T = 3 and 4 are -inf with zeros; at 7 and 12 the likelihood is -ctc_loss and the gradient in the frames exp(lp) - d ctc_loss /
    d lp (torch differentiates through a log-softmax it assumes)."""
    lp = tq.ctc_frames(T, normalised)
    logA = torch.tensor(th.one_hot(tq.CTC_X, 3), dtype=torch.float64, requires_grad=True)
    logB = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
    ll = merged_two_profile_loglike(tq.echo_machine(), logA, [0, len(tq.CTC_X)], logB, [0, T], tq.CTC_COLTOK, backend="numpy")
    ll.sum().backward()
    loss, grad = tq.ctc_reference(lp)
    post, postA = logB.grad.numpy(), logA.grad.numpy()
    if T < 5:
        assert float(ll.detach()[0]) == -math.inf and loss == math.inf and not post.any() and not postA.any()
        return
    assert abs(float(ll.detach()[0]) + loss) <= 1e-9 * max(1.0, abs(loss)), (float(ll.detach()[0]), loss)
    assert counts_close(post, np.exp(lp) - grad), np.abs(post - (np.exp(lp) - grad)).max()
    assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
    hot = np.exp(th.one_hot(tq.CTC_X, 3))
    assert not postA[hot == 0.0].any() and np.abs(postA[hot == 1.0] - 1.0).max() <= ROW_TOL


def _torch_pairs():
    """(em, colTok, As, Bs): two small ragged pairs on one machine, every entry finite."""
    em, colTok, A, B = tq.fd_case()
    A1, B1 = tm.merged_input(np.random.RandomState(4), em, 3, 2, 2, pInf=0.0)
    return em, colTok, [A, A1], [B, B1]


def test_autograd_function_on_the_numpy_backend():
    em, colTok, As, Bs = _torch_pairs()
    A, B, inOff, rowOff = np.concatenate(As), np.concatenate(Bs), [0, 3, 5], [0, 3, 5]
    logA = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    logB = torch.tensor(B, dtype=torch.float64, requires_grad=True)
    ll = merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, backend="numpy")
    dp = TwoMergedProfileDP(em, colTok)
    refs = [dp.mergedRowPosteriors(a, b) for a, b in zip(As, Bs)]
    assert ll.shape == (2,) and np.isfinite([r[2] for r in refs]).all() and np.array_equal(ll.detach().numpy(), [r[2] for r in refs])
    (ll * torch.tensor([1.0, -2.5], dtype=torch.float64)).sum().backward()
    assert np.array_equal(logA.grad.numpy(), np.concatenate([r[0] for r in refs]) * np.repeat([1.0, -2.5], [3, 2])[:, None])
    assert np.array_equal(logB.grad.numpy(), np.concatenate([r[1] for r in refs]) * np.repeat([1.0, -2.5], [3, 2])[:, None])
    f = lambda a, b: merged_two_profile_loglike(em, a, inOff, b, rowOff, colTok, backend="numpy")
    fresh = lambda T, grad: torch.tensor(T, dtype=torch.float64, requires_grad=grad)
    assert torch.autograd.gradcheck(f, (fresh(A, True), fresh(B, True)), eps=1e-6, atol=1e-7, rtol=1e-6)
    # only the inputs that require a gradient get one
    a, b = fresh(A, False), fresh(B, True)
    f(a, b).sum().backward()
    assert a.grad is None and np.array_equal(b.grad.numpy(), np.concatenate([r[1] for r in refs]))
    a, b = fresh(A, True), fresh(B, False)
    f(a, b).sum().backward()
    assert b.grad is None and np.array_equal(a.grad.numpy(), np.concatenate([r[0] for r in refs]))


def test_error_messages_new_and_old():
    em, colTok, As, Bs = _torch_pairs()
    A, B, inOff, rowOff = np.concatenate(As), np.concatenate(Bs), [0, 3, 5], [0, 3, 5]
    logA, logB = torch.tensor(A, dtype=torch.float64), torch.tensor(B, dtype=torch.float64)
    with pytest.raises(ValueError, match="logA is a float64"):
        merged_two_profile_loglike(em, logA.float(), inOff, logB, rowOff, colTok, backend="numpy")
    with pytest.raises(ValueError, match="logB is a float64 \\[sumRows, nCols \\+ 1\\] tensor"):
        merged_two_profile_loglike(em, logA, inOff, logB.float(), rowOff, colTok, backend="numpy")
    with pytest.raises(ValueError, match="rowOff has one entry per pair"):
        merged_two_profile_loglike(em, logA, inOff, logB, [0, 5], colTok, backend="numpy")
    with pytest.raises(ValueError, match="inOff has one entry per pair"):
        merged_two_profile_loglike(em, logA, [0, 2, 4], logB, rowOff, colTok, backend="numpy")
    with pytest.raises(ValueError, match="one column per entry of colTok"):
        merged_two_profile_loglike(em, logA, inOff, logB, rowOff, (1, 2), backend="numpy")
    with pytest.raises(ValueError, match='backend is "device" or "numpy"'):
        merged_two_profile_loglike(em, logA, inOff, logB, rowOff, colTok, backend="triton")
    # the plain loss does not take merged rows, and the old names keep their refusals
    with pytest.raises(ValueError):
        two_profile_loglike(em, logA, inOff, logB[:, :2], rowOff, backend="numpy")
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        TwoMergedProfileDP(em, colTok).rowPosteriors(As[0], Bs[0])
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    pb = Profile.fromCsv(CSV)
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        boss.scoreTwoProfiles(m, [], pb, backend="numpy", params=par, merge=True, posteriors=True)
    with pytest.raises(MachineError, match='backend is "device" or "numpy"'):
        boss.mergedTwoPosteriors(m, [], pb, backend="triton", params=par)
    with pytest.raises(MachineError, match="two-profile sweeps need a machine with an input alphabet"):
        boss.mergedTwoPosteriors(_generator(), [], pb, backend="numpy")


def _generator():
    """A machine without an input alphabet: one state that writes a symbol."""
    from prefixhelpers import machine_from_edges
    return th.machine_of(machine_from_edges(1, 0, 1, [(0, 0, 0, 1, 0.0)]))


def test_merged_two_posteriors_on_the_numpy_backend(tmp_path):
    """boss.mergedTwoPosteriors: dnastore4, input profiles of 3, 1 and 3 rows against tiny_uc.csv read CTC-merged, the last of them
    dead (a row without a weight); a Profile and its (logB, colTok) give the same."""
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    a = tmp_path / "a.csv"
    a.write_text("0_3,1_3,2_3,\n.5,.25,.125,.125\n.125,.5,.25,.125\n.25,.125,.5,.125\n")
    pa, pb = Profile.fromCsv(str(a)), Profile.fromCsv(CSV)
    short = Profile(pa.header, pa.row[:1])
    dead = Profile(pa.header, [[0.0] * len(pa.header)] + [list(r) for r in pa.row[1:]])
    B, colTok = pb.mergeRows(em)
    dp = TwoMergedProfileDP(em, colTok)
    post, ll = boss.mergedTwoPosteriors(m, [pa, short, dead], pb, backend="numpy", params=par)
    again, ll2 = boss.mergedTwoPosteriors(m, [p.logRowsIn(em) for p in (pa, short, dead)], (B, colTok), backend="numpy", params=par)
    assert len(post) == 3 and ll == ll2 and [l > -math.inf for l in ll] == [True, True, False]
    for k, p in enumerate((pa, short, dead)):
        wa, wb, wl = dp.mergedRowPosteriors(p.logRowsIn(em), B)
        ga, gb = post[k]
        assert ll[k] == wl and np.array_equal(ga, wa) and np.array_equal(gb, wb) and ga.shape == (len(p), 4) and gb.shape == B.shape
        assert np.array_equal(again[k][0], ga) and np.array_equal(again[k][1], gb)
        if k < 2:
            assert np.abs(ga.sum(axis=1) - 1.0).max() <= ROW_TOL and np.abs(gb.sum(axis=1) - 1.0).max() <= ROW_TOL
        else:
            assert not ga.any() and not gb.any()


def test_gpu_inputs_are_live():
    """Every input family of test_profile_two_merge_post_gpu.py under the yardstick: at least four in five likelihoods finite per
    family (the many-blocks families hold one live pair and the dead pair planted beside it, by construction), and the block and
    chunk counts the GPU tests rely on, restated from profile_pair_rowpost_rows and lattice_chunks."""
    dps = {}

    def ll(em, colTok, A, B):
        return dps.setdefault((id(em), tuple(colTok)), TwoMergedProfileDP(em, colTok)).forward(A, B)[0]
    fam = tq.gpu_families()
    lls = {name: [ll(*c) for c in cases] for name, cases in fam.items()}
    for name, v in lls.items():
        if name.startswith("long"):
            assert [x > -math.inf for x in v] == [True, False], (name, v)
        else:
            assert np.mean(np.array(v) > -math.inf) >= 0.8, (name, v)
    print({name: "%d of %d" % (sum(x > -math.inf for x in v), len(v)) for name, v in lls.items()})
    # the lane cases: the seven shapes twice (S >= 2) or once
    for nCols, S in tm.LANE_CASES:
        shapes = [(len(A), len(B)) for _, _, A, B in fam["lanes %d x %d" % (nCols, S)]]
        assert shapes == list(tq.SHAPES) * (2 if S >= 2 else 1) and tq.SHAPES[0] == (0, 0) and tq.SHAPES[-1] == (9, 9)
    # whole wavefronts: S = 64, so that (cell, plane) boundaries are wavefront boundaries
    em, colTok, pairs = tq.wave_case()
    assert em.nStates == 64 and len(colTok) == 4 and [(len(A), len(B)) for A, B in pairs] == [(2, 5), (5, 2)] and all(x > -math.inf for x in lls["wave"])
    # many blocks: 1 100 blocks of one line on the long axis under its table, for 1 024 groups; global bins under 2; few blocks by default
    for K, L in tq.LONG_SHAPES:
        em, colTok, pairs = tq.long_case(K, L)
        axis = 1 if K > L else 0
        one, glob, full = tq.long_tables(K, L)
        assert [(len(A), len(B)) for A, B in pairs] == [(K, L)] * 2 and em.nStates == 2 and len(colTok) == 4
        assert int(one) == (em.nInTok + 1 if axis else len(colTok) + 1)
        assert tq.rowpost_rows(2, 4, K, L, axis, em.nInTok, int(one)) == 1
        assert tq.rowpost_blocks(2, 4, K, L, axis, em.nInTok, int(one)) == tq.LONG > tq.ROWPOST_GROUPS_MAX
        assert tq.rowpost_blocks(2, 4, K, L, axis, em.nInTok, int(glob)) == tq.LONG and int(glob) < min(em.nInTok + 1, len(colTok) + 1)
        assert 1 < tq.rowpost_blocks(2, 4, K, L, axis, em.nInTok) < 8 and full is None
    # wide lines: more bins than a wavefront has lanes; under 16 doubles the line goes to its global bins, the other axis takes several lines a block
    for which, axis in (("columns", 0), ("inputs", 1)):
        em, colTok, pairs = tq.wide_case(which)
        bins = em.nInTok + 1 if axis else len(colTok) + 1
        assert bins == (71 if axis else 66) > 64 and em.nStates == 2 and all(x > -math.inf for x in lls["wide " + which])
        assert tq.rowpost_rows(2, len(colTok), 7, 3, axis, em.nInTok) == (7 if axis else 3) and tq.rowpost_rows(2, len(colTok), 7, 3, axis, em.nInTok, 16) == 1
        assert tq.rowpost_rows(2, len(colTok), 4, 5, 1 - axis, em.nInTok, 16) >= 3
    # the ragged batch: the empty shapes first, the dead pair last, the ring marks between; chunks under 1.8 of the largest pair
    em, colTok, pairs = tq.ragged_case()
    shapes = [(len(A), len(B)) for A, B in pairs]
    assert shapes[:3] == [(0, 0), (0, 5), (5, 0)] and [x > -math.inf for x in lls["ragged"]] == [True] * (len(pairs) - 1) + [False]
    assert {min(s) for s in shapes[3:11]} == {9, 10, 25, 26} and em.nStates == 20 and len(colTok) == 2
    sizes = [tq.pair_bytes(20, 2, K, L, em.nInTok) for K, L in shapes]
    budget = tq.ragged_budget(em, pairs)
    chunks = th.lattice_chunks(sizes, budget)
    assert len(chunks) >= 3 and all(sum(sizes[a:b]) <= budget for a, b in chunks) and max(sizes) <= budget < 2 * max(sizes)
    # the scratch rings: the X / T ring of the two large pairs is past LDS, that of the small one inside
    em, colTok, pairs = tq.scratch_case()
    rings = [tm.ring_bytes(em.nStates, len(colTok), len(A), len(B), mat=True) for A, B in pairs]
    assert [r > tm.RING_LDS_MAX for r in rings] == [True, False, True] and all(x > -math.inf for x in lls["scratch"])
    assert all(tm.ring_bytes(20, 2, K, L, mat=True) <= tm.RING_LDS_MAX for K, L in shapes)
    # dead weights: a third of either table, the planted rows, the shift
    cases = {name: (e, ct, ps) for name, e, ct, ps in tq.dead_weight_cases()}
    # (180 and 360 weights: a third, give or take 2.5 standard deviations of the smaller table)
    assert all(0.25 <= np.mean(T == -math.inf) <= 0.42 for T in (np.concatenate([p[t].ravel() for p in cases["third"][2]]) for t in (0, 1)))
    e, ct, ps = cases["degenerate"]
    assert [ll(e, ct, A, B) > -math.inf for A, B in ps[:6]] == [True, True, True, True, False, False]
    e, ct, ps = cases["far"]
    assert ll(e, ct, *ps[0]) > -math.inf and ll(e, ct, *ps[1]) < -12000
    assert [tuple(ct) for ct, _, _ in tq.column_map_cases()[1]] == list(tm.COLMAPS) and all(x > -math.inf for x in lls["column maps"])
    em, colTok, A, B = tq.fd_case()
    assert np.isfinite(A).all() and np.isfinite(B).all() and abs(lls["finite differences"][0]) < 100 and len(tq.perturbed(A, B)) == 2 * (A.size + B.size)
    em, colTok, xs, Bs = tq.one_hot_case()
    dp = PairMergedProfileDP(em, colTok)
    assert all(dp.forward(x, B)[0] > -math.inf for x, B in zip(xs, Bs))
    em, colTok, As, Bs = _torch_pairs()
    assert all(ll(em, colTok, A, B) > -math.inf for A, B in zip(As, Bs))
