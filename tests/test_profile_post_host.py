"""Row posteriors of the one-tape profile sweeps without a GPU (docs/profile_tapes.md, "Row posteriors of one-tape profiles"): the
numpy yardsticks profile.ProfileDP.rowPosteriors and profile.MergedProfileDP.rowPosteriors held to facts they do not compute
themselves -- every row sums to 1, the column sums are the counts() of the transitions that write the column's token (merged: the
fresh-emission part), post[r][x] is the derivative of forward() in P[r][x], the plain posteriors are the pair sweep's at an empty
input, and with a linear-chain generator the merged ones are torch's CTC loss and its gradient -- then the layers above them: the
autograd function on the numpy backend, boss.profilePosteriors and the --profile-posteriors flag; and the inputs of
test_profile_post_gpu.py held to their liveness conditions.

Bounds: likelihoods 1e-9 relative to max(1, |value|); entries as counts (pairprofilehelpers: 1e-6 relative from 1e-3 up, 1e-9 +
1e-6 x value below); -inf entries and dead profiles exactly 0; row sums 1e-6; central differences at h = 1e-6 within 1e-7 absolute
(truncation about h^2, rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100)."""
import io
import json
import math

import numpy as np
import pytest
import torch

from conftest import golden_path
import profileposthelpers as h
from pairprofilehelpers import counts_close, logs_close
from profileposthelpers import FD_H, FD_TOL, ROW_TOL
from machineboss_amd import boss
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import MergedProfileDP, PairProfileDP, Profile, ProfileDP
from machineboss_amd.torchprofile import profile_loglike

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

CSV = golden_path("csv", "tiny_uc.csv")
DNASTORE = golden_path("machine", "dnastore4.json")
LOOP = {"state": [{"id": "S", "trans": [{"out": s, "to": "S", "weight": "p" + s} for s in "ACGT"] + [{"to": "E", "weight": "pE"}]},
                  {"id": "E", "trans": []}]}
LOOP_PARAMS = {"pA": .4, "pC": .1, "pG": .2, "pT": .1, "pE": .2}


@pytest.fixture(scope="module")
def cases():
    """[(em, colTok, P, post, ll, repeats or None)] over host_cases(), computed once."""
    out = []
    for em, colTok, profs in h.host_cases():
        dp = h.yardstick(em, colTok)
        for P in profs:
            rep = []
            post, ll = dp.rowPosteriors(P) if colTok is None else dp.rowPosteriors(P, rep)
            out.append((em, colTok, P, post, ll, rep[0] if rep else None))
    return out


def test_the_suite_is_live(cases):
    """S in {1, 2, 8, 65} with and without silent levels, plain and nCols in {1, 2, 4}, L = 0..9: nine in ten likelihoods finite."""
    assert len(cases) == len(h.HOST_SEEDS) * (1 + len(h.HOST_COLS)) * 10
    assert {(c[0].nStates, None if c[1] is None else len(c[1]), len(c[2])) for c in cases} == \
        {(S, n, L) for S in h.HOST_STATES for n in (None,) + h.HOST_COLS for L in range(10)}
    live = np.mean([c[4] > -math.inf for c in cases])
    assert live >= 0.9, live


def test_row_sums_zeros_and_grouped_counts(cases):
    worst = 0.0
    for em, colTok, P, post, ll, rep in cases:
        width = em.nOutTok + 1 if colTok is None else len(colTok) + 1
        assert post.shape == (len(P), width) and (post >= 0.0).all()
        dp = h.yardstick(em, colTok)
        c, cl = dp.counts(P)
        assert cl == ll and ll == dp.forward(P)[0]
        if not ll > -math.inf:
            assert not post.any() and (rep is None or not rep.any())
            continue
        assert not post[P == -math.inf].any()
        if len(P):
            worst = max(worst, float(np.abs(post.sum(axis=1) - 1.0).max()))
            assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
        if colTok is None:
            assert counts_close(post.sum(axis=0)[1:], h.grouped(em, c))
        else:
            assert (rep >= 0.0).all() and not rep[:, 0].any() and (rep <= post).all()
            assert counts_close(h.by_token(em, colTok, (post - rep).sum(axis=0)), h.grouped(em, c))
    print("row sums off by at most %.3g" % worst)


def test_central_differences_of_forward(cases):
    worst, n = 0.0, 0
    for em, colTok, P, post, ll, _ in cases:
        if not 1 <= len(P) <= 3 or not abs(ll) < 100:
            continue
        dp = h.yardstick(em, colTok)
        for r in range(P.shape[0]):
            for x in range(P.shape[1]):
                if P[r, x] == -math.inf:
                    assert post[r, x] == 0.0
                    continue
                up, dn = P.copy(), P.copy()
                up[r, x] += FD_H; dn[r, x] -= FD_H
                fd = (dp.forward(up)[0] - dp.forward(dn)[0]) / (2 * FD_H)
                worst = max(worst, abs(fd - post[r, x])); n += 1
                assert abs(fd - post[r, x]) <= FD_TOL, (em.nStates, colTok, r, x, fd, post[r, x])
    assert n >= 300
    print("central differences off by at most %.3g over %d entries" % (worst, n))


def test_plain_posteriors_are_the_pair_sweep_at_an_empty_input(cases):
    """A generator has no input alphabet, so both sweeps are defined on it and PairProfileDP at x = [] walks the same lattice."""
    n = 0
    for em, colTok, P, post, ll, _ in cases:
        if colTok is not None:
            continue
        want, wl = PairProfileDP(em).rowPosteriors([], P)
        assert logs_close([ll], [wl], 1e-12) and post.shape == want.shape
        assert np.allclose(post, want, rtol=1e-12, atol=0.0)
        n += 1
    assert n == 70


# ---- CTC ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalised", (True, False))
@pytest.mark.parametrize("T", h.CTC_FRAMES)
def test_a_chain_generator_gives_the_ctc_loss_and_its_gradient(T, normalised):
    """y = [1, 2, 2, 3] over three symbols: LL = -ctc_loss and post = exp(lp) - d ctc_loss / d lp, the convention of torch's native
    backward with or without normalised rows.  The twos are two symbols only with a blank between them, so y needs five frames:
    at T = 4 the one alignment of four frames has no blank and reads as [1, 2, 3], and T = 3 has not even the frames.  Both score
    -inf and get zeros, here and in torch; from T = 7 on the blank between the twos is on every path."""
    em = h.ctc_machine()
    lp = h.ctc_frames(T, normalised)
    wl, want = h.ctc_reference(lp)
    post, ll = MergedProfileDP(em, h.CTC_COLTOK).rowPosteriors(lp.numpy())
    assert logs_close([ll], [wl]), (ll, wl)
    assert post.shape == want.shape and counts_close(post, want), np.abs(post - want).max()
    if T <= 4:
        assert ll == -math.inf and wl == -math.inf and not post.any()
    else:
        assert ll > -math.inf and np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
        rep = []
        MergedProfileDP(em, h.CTC_COLTOK).rowPosteriors(lp.numpy(), rep)
        fresh = (post - rep[0]).sum(axis=0)
        assert counts_close(fresh[1:], [1.0, 2.0, 1.0])      # every symbol of y is emitted once: the twos twice in column 2


# ---- the autograd function on the numpy backend -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", (False, True))
def test_gradcheck_of_profile_loglike(merged):
    em = h.post_machine(8, 3, True, 708)
    colTok = [1, 2, 3, 1] if merged else None
    rng = np.random.RandomState(5 + merged)
    P = np.concatenate([h.long_rows(rng, 5 if merged else 4, L) for L in (2, 0, 3)])
    rowOff = [0, 2, 2, 5]
    logP = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    ll = profile_loglike(em, logP, rowOff, colTok, backend="numpy")
    assert ll.shape == (3,) and torch.isfinite(ll).all()
    dp = h.yardstick(em, colTok)
    assert ll[0].item() == dp.forward(P[:2])[0] and ll[1].item() == dp.forward(P[:0])[0]
    assert torch.autograd.gradcheck(lambda t: profile_loglike(em, t, rowOff, colTok, backend="numpy"), (logP,), eps=1e-6, atol=1e-7, rtol=1e-6)
    (ll * torch.tensor([1.0, 3.0, -2.5], dtype=torch.float64)).sum().backward()
    want = np.concatenate([dp.rowPosteriors(P[:2])[0], -2.5 * dp.rowPosteriors(P[2:])[0]])
    assert np.allclose(logP.grad.numpy(), want, rtol=1e-12, atol=0.0)


def test_profile_loglike_takes_a_dead_profile_and_refuses_bad_shapes():
    em = h.post_machine(8, 3, True, 708)
    P = h.long_rows(np.random.RandomState(6), 4, 4)
    P[1] = -np.inf
    logP = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    ll = profile_loglike(em, logP, [0, 4], backend="numpy")
    assert ll[0].item() == -math.inf
    ll.sum().backward()
    assert not logP.grad.numpy().any()
    with pytest.raises(ValueError):
        profile_loglike(em, logP.float(), [0, 4], backend="numpy")
    with pytest.raises(ValueError):
        profile_loglike(em, logP, [0, 3], backend="numpy")
    with pytest.raises(ValueError):
        profile_loglike(em, logP, [0, 4], colTok=[1, 2], backend="numpy")
    with pytest.raises(ValueError):
        profile_loglike(em, logP, [0, 4], backend="eager")


def test_ctc_through_the_autograd_function():
    """profile_loglike(backend="numpy") with the chain generator and colTok: -ctc_loss, and after backward() the gradient of
    -ctc_loss in the frames up to torch's exp(lp) convention."""
    em = h.ctc_machine()
    lp = h.ctc_frames(7, True)
    wl, want = h.ctc_reference(lp)
    logP = lp.clone().requires_grad_(True)
    ll = profile_loglike(em, logP, [0, 7], h.CTC_COLTOK, backend="numpy")
    ll.sum().backward()
    assert logs_close(ll.detach().numpy(), [wl]) and counts_close(logP.grad.numpy(), want)


# ---- the layers above -----------------------------------------------------------------------------------------------------------------------
def test_profile_posteriors_entry_point_on_the_host(tmp_path):
    (tmp_path / "loop.json").write_text(json.dumps(LOOP))
    M = Machine.fromFile(str(tmp_path / "loop.json"))
    prof = Profile.fromCsv(CSV)
    from machineboss_amd.evalmachine import EvaluatedMachine
    ev = EvaluatedMachine.fromMachine(M, LOOP_PARAMS)
    post, ll = boss.profilePosteriors(M, prof, "numpy", LOOP_PARAMS)
    want, wl = ProfileDP(ev).rowPosteriors(prof.logRows(ev))
    assert ll == wl and ll > -math.inf and np.array_equal(post, want) and post.shape == (len(prof), ev.nOutTok + 1)
    assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
    P, colTok = prof.mergeRows(ev)
    post, ll = boss.profilePosteriors(M, prof, "numpy", LOOP_PARAMS, merge=True)
    want, wl = MergedProfileDP(ev, colTok).rowPosteriors(P)
    assert ll == wl and ll > -math.inf and np.array_equal(post, want) and post.shape == (len(prof), len(colTok) + 1)
    # rows instead of a Profile, and a dead profile
    assert np.array_equal(boss.profilePosteriors(M, (P, colTok), "numpy", LOOP_PARAMS, merge=True)[0], want)
    dead = prof.logRows(ev).copy(); dead[1] = -np.inf
    post, ll = boss.profilePosteriors(M, dead, "numpy", LOOP_PARAMS)
    assert ll == -math.inf and post.shape == dead.shape and not post.any()
    # the host half of the device backend: everything it refuses before it opens the device
    with pytest.raises(MachineError, match="empty input alphabet"):
        boss.profilePosteriors(Machine.fromFile(DNASTORE), prof, "device")
    with pytest.raises(MachineError, match="backend is"):
        boss.profilePosteriors(M, prof, "eager", LOOP_PARAMS)


def test_command_line(tmp_path):
    (tmp_path / "loop.json").write_text(json.dumps(LOOP))
    (tmp_path / "par.json").write_text(json.dumps(LOOP_PARAMS))
    M = Machine.fromFile(str(tmp_path / "loop.json"))
    prof = Profile.fromCsv(CSV)
    gen = [str(tmp_path / "loop.json"), "-P", str(tmp_path / "par.json"), "--decode-backend", "numpy"]

    def run(*args):
        out = io.StringIO()
        assert boss.run(gen + list(args), out) == 0
        return out.getvalue()
    for flag, merge in (("--recognize-csv", False), ("--recognize-merge-csv", True)):
        want, ll = boss.profilePosteriors(M, prof, "numpy", LOOP_PARAMS, merge=merge)
        got = json.loads(run(flag, CSV, "--profile-posteriors"))      # it may stand alone
        assert len(got) == 1 and got[0][:2] == ["", ""] and np.array(got[0][2]).shape == want.shape
        assert np.abs(np.array(got[0][2], float) - want).max() <= 1e-5          # (%g: six significant digits)
    lines = run("--recognize-merge-csv", CSV, "-L", "-C", "-V", "--profile-posteriors").splitlines()      # after the -L / -C / -V lines
    assert len(lines) == 4 and abs(json.loads(lines[0])[0][2] - ll) <= 1e-4 and json.loads(lines[3]) == got

    def fails(args, msg):
        with pytest.raises(MachineError, match=msg):
            boss.run(args + ["--decode-backend", "numpy"], io.StringIO())
    # a machine with an input alphabet keeps today's message from these spellings
    only = "--profile-posteriors goes with --recognize-csv beside an input sequence"
    fails([DNASTORE, "--use-defaults", "--recognize-csv", CSV, "--profile-posteriors"], only)
    fails([DNASTORE, "--use-defaults", "--recognize-merge-csv", CSV, "--profile-posteriors"], only)
    fails([DNASTORE, "--use-defaults", "--profile-posteriors"], only)
    fails(gen[:3] + ["--profile-posteriors"], only)
    fails(gen[:3] + ["--recognize-csv", CSV, "--profile-posteriors", "--viterbi-decode"], only)
    fails(gen[:3] + ["--recognize-csv", CSV, "--profile-posteriors", "--profile-band", "2"], "--profile-band goes with")
    fails(gen[:3] + ["--recognize-csv", CSV, "--profile-posteriors", "--input-chars", "A"], "no input alphabet to read an input sequence")
    fails(gen[:3] + ["--recognize-csv", CSV], "needs -L, -V or -C")


# ---- the inputs of test_profile_post_gpu.py -------------------------------------------------------------------------------------------------
def test_gpu_suite_inputs_are_live():
    def live(em, colTok, profs):
        dp = h.yardstick(em, colTok)
        return [dp.forward(P)[0] > -math.inf for P in profs]
    plain = [x for S in h.GPU_STATES for silent in ((True, False) if S >= 2 else (False,)) for x in live(h.gpu_plain_case(S, silent)[0], None, h.gpu_plain_case(S, silent)[1])]
    assert np.mean(plain) >= 0.75, np.mean(plain)          # (no rows: dead without a silent path to the end)
    merged = [x for c in h.GPU_MERGED for x in live(*h.gpu_merged_case(*c))]
    assert np.mean(merged) >= 0.75, np.mean(merged)
    assert all(live(h.one_lane_rows_case()[0], None, h.one_lane_rows_case()[1]) + live(h.row_blocks_case()[0], None, h.row_blocks_case()[1]))
    assert all(live(*h.many_blocks_case(False)) + live(*h.many_blocks_case(True)))
    em, profs = h.wide_alphabet_case()
    assert em.nOutTok == 70 and all(live(em, None, profs))
    for merged in (False, True):
        em, colTok, profs = h.ragged_case(merged)
        got = live(em, colTok, profs)
        assert len(got) == 10 and len(profs[2]) == 0 and not got[5] and sum(got) == 8
    hard = h.hard_cases()
    for tag in ("", " merged"):
        assert any(live(*hard["third" + tag])) and live(*hard["infrow" + tag]) == [True, False, True]
        assert live(*hard["allblank" + tag]) == [True] and live(*hard["far" + tag]) == [True, True]
        em, colTok, (P, far) = hard["far" + tag]
        assert h.yardstick(em, colTok).forward(far)[0] < -6000
