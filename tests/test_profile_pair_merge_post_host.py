"""Row posteriors of pairs against CTC-merged profiles without a GPU (docs/profile_tapes.md, "Row posteriors of pairs against a merged
profile"): the numpy yardstick profile.PairMergedProfileDP.rowPosteriors held to facts it does not compute itself -- every row sums
to 1, the fresh part groups to counts(), without an input it is MergedProfileDP.rowPosteriors, it is the derivative of forward(), and
with an echo transducer it is the gradient of torch's CTC loss -- then the layers above it on the numpy backend, the new error
messages, and the conditions the GPU suite assumes of its inputs.  Bounds: pairmergeposthelpers."""
import math

import numpy as np
import pytest
import torch

import pairmergehelpers as mh
import pairmergeposthelpers as pp
from pairprofilehelpers import counts_close
from machineboss_amd import boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairMergedProfileDP, Profile
from machineboss_amd.torchprofile import pair_profile_loglike

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"
IDENT_TOL = 1e-12

_DPS = {}


def _dp(em, colTok):
    key = (id(em), tuple(int(c) for c in colTok))
    if key not in _DPS:
        _DPS[key] = (em, PairMergedProfileDP(em, colTok))
    return _DPS[key][1]


@pytest.fixture(scope="module")
def suite():
    """[(em, colTok, x, P, post, repeats, ll)] over host_cases, computed once."""
    out = []
    for em, colTok, x, P in pp.host_cases():
        rep = []
        post, ll = _dp(em, colTok).rowPosteriors(x, P, repeats=rep)
        out.append((em, colTok, x, P, post, rep[0], ll))
    return out


def test_rows_sum_to_one_and_the_fresh_part_groups_the_counts(suite):
    live, worstRow, worstGroup = [], 0.0, 0.0
    for em, colTok, x, P, post, rep, ll in suite:
        dp = _dp(em, colTok)
        blanks = []
        c, ll2 = dp.counts(x, P, blanks=blanks)
        assert post.shape == P.shape == rep.shape and ll == ll2 and ll == dp.forward(x, P)[0]
        live.append(ll > -math.inf)
        if not ll > -math.inf:
            assert not post.any() and not rep.any()
            continue
        assert (post >= 0.0).all() and (rep >= 0.0).all() and not rep[:, 0].any() and not post[P == -math.inf].any()
        if len(P):
            worstRow = max(worstRow, float(np.abs(post.sum(axis=1) - 1.0).max()))
            assert np.abs(post.sum(axis=1) - 1.0).max() <= IDENT_TOL
        got = pp.by_token(em, colTok, (post - rep).sum(axis=0)[1:])
        want = pp.grouped(em, colTok, c)
        worstGroup = max(worstGroup, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= IDENT_TOL, (got, want)
        assert abs((post[:, 0].sum() + rep.sum()) - blanks[0]) <= IDENT_TOL * max(1.0, blanks[0])      # the blanks and repeats of counts()
    print("%d cases, %d finite; row sums off by %.3g, grouped counts by %.3g" % (len(suite), sum(live), worstRow, worstGroup))
    assert np.mean(live) >= 0.9, np.mean(live)


def test_no_input_is_the_one_tape_merged_yardstick(suite):
    n = 0
    for em, colTok, x, P, post, rep, ll in suite:
        if len(x):
            continue
        rep1 = []
        want, wl = MergedProfileDP(em, colTok).rowPosteriors(P, repeats=rep1)
        assert (ll == wl or abs(ll - wl) <= IDENT_TOL * max(1.0, abs(wl))) and post.shape == want.shape
        if post.size:
            assert np.abs(post - want).max() <= IDENT_TOL and np.abs(rep - rep1[0]).max() <= IDENT_TOL
        n += ll > -math.inf
    assert n >= 20


def test_row_posteriors_are_the_gradient_of_forward(suite):
    """Central differences of forward() in every finite entry of P, over the cases with L <= 3 and |LL| < 100."""
    worst, n = 0.0, 0
    for em, colTok, x, P, post, rep, ll in suite:
        if len(P) == 0 or len(P) > 3 or not abs(ll) < 100:
            continue
        dp = _dp(em, colTok)
        for r in range(P.shape[0]):
            for c in range(P.shape[1]):
                if P[r, c] == -math.inf:
                    continue
                up, dn = P.copy(), P.copy()
                up[r, c] += pp.FD_H; dn[r, c] -= pp.FD_H
                fd = (dp.forward(x, up)[0] - dp.forward(x, dn)[0]) / (2 * pp.FD_H)
                worst = max(worst, abs(fd - post[r, c])); n += 1
                assert abs(fd - post[r, c]) <= pp.FD_TOL, (len(x), r, c, fd, post[r, c])
    print("%d derivatives, central differences off by at most %.3g" % (n, worst))
    assert n >= 200


@pytest.mark.parametrize("normalised", (True, False))
@pytest.mark.parametrize("T", pp.CTC_T)
def test_echo_transducer_is_the_ctc_loss(T, normalised):
    """x = 1 2 2 3 needs five frames: T = 3 and 4 are -inf with zeros; at 7 and 12 the likelihood is -ctc_loss and the posteriors are
    exp(lp) - d ctc_loss / d lp (torch differentiates through a log-softmax it assumes; its gradient in lp is exp(lp) - posterior)."""
    lp = pp.ctc_frames(T, normalised)
    post, ll = PairMergedProfileDP(pp.echo_machine(), pp.CTC_COLTOK).rowPosteriors(pp.CTC_X, lp)
    loss, grad = pp.ctc_reference(lp)
    if T < 5:
        assert ll == -math.inf and loss == math.inf and not post.any()
        return
    assert abs(ll + loss) <= 1e-9 * max(1.0, abs(loss)), (ll, loss)
    assert counts_close(post, np.exp(lp) - grad), np.abs(post - (np.exp(lp) - grad)).max()
    assert np.abs(post.sum(axis=1) - 1.0).max() <= pp.ROW_TOL


def _torch_pairs():
    em, colTok, x, P = pp.fd_case()
    x1, P1 = mh.merged_input(np.random.RandomState(4), em, 3, 2, 2, zeros=0.0)
    return em, colTok, [x, x1], np.concatenate([P, P1]), np.array([0, 3, 5])


def test_autograd_function_on_the_numpy_backend():
    em, colTok, xs, P, rowOff = _torch_pairs()
    assert np.isfinite(P).all()
    logP = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    ll = pair_profile_loglike(em, xs, logP, rowOff, backend="numpy", colTok=colTok)
    dp = PairMergedProfileDP(em, colTok)
    want = [dp.forward(xs[k], P[rowOff[k]:rowOff[k + 1]])[0] for k in range(2)]
    assert ll.shape == (2,) and np.isfinite(want).all() and np.array_equal(ll.detach().numpy(), want)
    (ll * torch.tensor([1.0, -2.5], dtype=torch.float64)).sum().backward()
    post = np.concatenate([dp.rowPosteriors(xs[k], P[rowOff[k]:rowOff[k + 1]])[0] for k in range(2)])
    assert np.array_equal(logP.grad.numpy(), post * np.repeat([1.0, -2.5], [3, 2])[:, None])
    f = lambda t: pair_profile_loglike(em, xs, t, rowOff, backend="numpy", colTok=colTok)
    assert torch.autograd.gradcheck(f, (torch.tensor(P, dtype=torch.float64, requires_grad=True),), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_new_error_messages():
    em, colTok, xs, P, rowOff = _torch_pairs()
    logP = torch.tensor(P, dtype=torch.float64)
    with pytest.raises(ValueError, match="envelopes take plain profiles"):
        pair_profile_loglike(em, xs, logP, rowOff, envs=[None, None], backend="numpy", colTok=colTok)
    with pytest.raises(ValueError, match="one column per entry of colTok"):
        pair_profile_loglike(em, xs, logP, rowOff, backend="numpy", colTok=(1, 2))
    with pytest.raises(ValueError, match='backend is "device" or "numpy"'):
        pair_profile_loglike(em, xs, logP, rowOff, backend="cuda", colTok=colTok)
    m = Machine.fromFile(DNASTORE)
    with pytest.raises(MachineError, match='backend is "device" or "numpy"'):
        boss.mergedPairPosteriors(m, [[]], Profile.fromCsv(CSV), backend="cuda", params=m.getParamDefs(True))
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):      # the old entry keeps its refusal
        boss.scoreProfilePairs(m, [[]], Profile.fromCsv(CSV), backend="numpy", params=m.getParamDefs(True), merge=True, posteriors=True)


def test_merged_pair_posteriors_on_the_numpy_backend():
    m = Machine.fromFile(DNASTORE)
    par = m.getParamDefs(True)
    em = EvaluatedMachine.fromMachine(m, par)
    prof = Profile.fromCsv(CSV)
    P, colTok = boss._mergedRows(prof, em)
    dp = PairMergedProfileDP(em, colTok)
    seqs = [["0_3", "2_3", "1_3"], ["nonsense"], [], ["1_3", "1_3"]]
    post, ll = boss.mergedPairPosteriors(m, seqs, prof, backend="numpy", params=par)
    assert len(post) == len(ll) == len(seqs) and ll[1] == -math.inf and not post[1].any() and post[1].shape == P.shape
    live = 0
    for k in (0, 2, 3):
        want, wl = dp.rowPosteriors(em.inputTokenizer.tokenize(seqs[k]), P)
        assert np.array_equal(post[k], want) and ll[k] == wl
        if wl > -math.inf:
            live += 1
            assert np.abs(want.sum(axis=1) - 1.0).max() <= pp.ROW_TOL
    assert live >= 2
    post2, ll2 = boss.mergedPairPosteriors(m, seqs, (P, colTok), backend="numpy", params=par)
    assert ll2 == ll and all(np.array_equal(a, b) for a, b in zip(post, post2))


def test_gpu_suite_inputs_are_live():
    """What test_profile_pair_merge_post_gpu.py assumes of its inputs, under the yardstick and plain arithmetic."""
    lls = []
    for nCols, S in pp.LANE_CASES:
        case = []
        for em, colTok, pairs in pp.lane_case(nCols, S):
            case += [r[1] for r in pp.yardstick(em, colTok, pairs)]
        assert np.mean(np.array(case) > -math.inf) >= 0.85, (nCols, S, case)
        lls += case
    em, colTok, pairs = pp.wave_case()
    r = [q[1] for q in pp.yardstick(em, colTok, pairs)]
    assert em.nStates == 64 and all(P.shape[1] == 5 for _, P in pairs) and all(v > -math.inf for v in r)
    lls += r
    # the wrap case: more blocks than groups under a table of 5, global bins under 2, three blocks by default
    em, colTok, pairs = pp.wrap_case()
    I, L = pp.WRAP_SHAPE
    assert (len(pairs[0][0]), len(pairs[0][1]), em.nStates, len(colTok)) == (I, L, 2, 4)
    assert pp.rows_per_block(2, 4, I, L, 5) == 1 and pp.blocks(2, 4, I, L, 5) == L > pp.ROWPOST_GROUPS
    assert pp.rows_per_block(2, 4, I, L, 2) == 1 and 5 > 2
    assert pp.rows_per_block(2, 4, I, L) == 410 and pp.blocks(2, 4, I, L) == 3
    (post, ll), (dead, dl) = pp.yardstick(em, colTok, pairs)
    assert ll > -math.inf and dl == -math.inf and not dead.any() and (post[1024:] > 0).any() and np.abs(post.sum(axis=1) - 1.0).max() <= 1e-9
    # 66 bins: one row a block under a table of 16 (global bins), rows of 66 in the full table
    for em, colTok, pairs in pp.wide_case():
        assert sum(q[1] > -math.inf for q in pp.yardstick(em, colTok, pairs)) >= 6
        assert len(colTok) == 65 and pp.rows_per_block(2, 65, 9, 9, 16) == 1 and pp.rows_per_block(2, 65, 9, 9) == min(-(-8192 // 1320), 62, 9)
    # chunks: under the budget no two of the three (9, 9) pairs share a chunk
    em, colTok, pairs = pp.chunk_case()
    sizes = sorted(pp.pair_bytes(pp.CHUNK_S, 4, len(x), len(P)) for x, P in pairs)
    assert sizes[-1] <= pp.chunk_budget() < 1.8 * sizes[-1] and sizes[-3] + sizes[-2] > pp.chunk_budget() and sizes[-3] == sizes[-1]
    assert mh.ring_bytes(pp.CHUNK_S, 4, 9, 9, mat=True) <= mh.LDS_MAX
    lls += [r[1] for r in pp.yardstick(em, colTok, pairs)]
    em, colTok, pairs = pp.ragged_post_case()
    r = [q[1] for q in pp.yardstick(em, colTok, pairs)]
    assert r[-1] == -math.inf and all(v > -math.inf for v in r[:-1]) and any(len(x) == 0 for x, _ in pairs) and any(len(P) == 0 for _, P in pairs)
    lls += r[:-1]
    em, colTok, pairs = pp.third_inf_case()
    r = pp.yardstick(em, colTok, pairs)
    assert np.mean([(P == -math.inf).mean() for _, P in pairs if P.size]) >= 0.25 and sum(q[1] > -math.inf for q in r) >= 3
    em, colTok, pairs = pp.far_case()
    r = pp.yardstick(em, colTok, pairs)
    assert r[0][1] > -math.inf and r[1][1] < -6000 and counts_close(r[1][0], r[0][0])
    for name, (em, colTok, pairs) in list(mh.column_map_cases().items()) + list(mh.row_cases().items()):
        r = [q[1] for q in pp.yardstick(em, colTok, pairs)]
        assert sum(v > -math.inf for v in r) >= len(r) - 1, (name, r)
        assert name != "allblank" or all(v > -math.inf for v in r)
        assert name != "infrow" or r[1] == -math.inf
        lls += r
    em, colTok, x, P = pp.fd_case()
    ll = PairMergedProfileDP(em, colTok).forward(x, P)[0]
    assert abs(ll) < 100 and np.isfinite(P).all()
    assert np.mean(np.array(lls) > -math.inf) >= 0.9, np.mean(np.array(lls) > -math.inf)
