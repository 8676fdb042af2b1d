"""Row posteriors of the two-tape profile sweeps without a GPU (docs/profile_tapes.md, "Row posteriors"): the numpy yardstick
profile.PairProfileDP.rowPosteriors held to the three facts that define it -- every row sums to 1, post[r][o] is the derivative of
the log-likelihood in P[r][o], and the column sums are the counts() of the transitions that write the column's token -- over the
suite of pairprofilehelpers, on the full lattice and under bands; then the layers above it: the autograd function on the numpy
backend, boss.scoreProfilePairs(posteriors=True), the --profile-posteriors flag and the rejection of merged profiles.

Bounds: entries as counts (pairprofilehelpers: 1e-6 relative from 1e-3 up, 1e-9 + 1e-6 x value below), row sums 1e-6 (the entries
are non-negative, each within 1e-6 relative, and sum to 1), central differences at h = 1e-6 within 1e-7 absolute (truncation about
h^2, rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100)."""
import io
import json
import math

import numpy as np
import pytest
import torch

import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, pair_input, pair_machine
from machineboss_amd import boss
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineError
from machineboss_amd.profile import PairProfileDP, Profile
from machineboss_amd.seqpair import Envelope
from machineboss_amd.torchprofile import pair_profile_loglike

CSV = "tests/golden/csv/tiny_uc.csv"
DNASTORE = "tests/golden/machine/dnastore4.json"
STATES = (1, 2, 8, 65)
ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7


def _cases(band):
    """[(em, x, P, env)]: suite_case for every S and alphabet, on the full lattice (band None) or under Envelope.band(I, L, band);
    a shape whose slope the band cannot bridge is left out."""
    out = []
    for S in STATES:
        for nIn, nOut in ph.SUITE_ALPHABETS:
            for em, x, P in ph.suite_case(S, nIn, nOut):
                if band is None:
                    out.append((em, x, P, None))
                    continue
                try:
                    out.append((em, x, P, Envelope.band(len(x), len(P), band)))
                except MachineError:
                    pass
    return out


_DPS = {}


def _dp(em):
    if id(em) not in _DPS:
        _DPS[id(em)] = (em, PairProfileDP(em))
    return _DPS[id(em)][1]


def grouped(em, counts):
    """counts[nTrans] added up by output token: [nOutTok + 1], entry 0 (the output-less transitions) left at 0."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(em.outTok, np.int64), counts)
    g[0] = 0.0
    return g


BANDS = (0, 1, 3)


@pytest.mark.parametrize("bands", ((None,), BANDS), ids=("full", "bands"))
def test_row_posteriors_sum_to_one_and_group_the_counts(bands):
    """The full lattice, and the bands of half-width 0, 1 and 3 taken together (a band of width 0 alone leaves a match as the only
    move, which kills a quarter of its cases)."""
    cases = [c for band in bands for c in _cases(band)]
    live, worstRow, worstGroup = [], 0.0, 0.0
    for em, x, P, env in cases:
        dp = _dp(em)
        post, ll = dp.rowPosteriors(x, P, env=env)
        blanks = []
        c, ll2 = dp.counts(x, P, blanks=blanks, env=env)
        assert post.shape == P.shape and ll == ll2 and ll == dp.forward(x, P, env=env)[0]
        live.append(ll > -math.inf)
        if not ll > -math.inf:
            assert not post.any()
            continue
        assert (post >= 0.0).all() and not post[P == -math.inf].any()
        if len(P):
            worstRow = max(worstRow, float(np.abs(post.sum(axis=1) - 1.0).max()))
            assert np.abs(post.sum(axis=1) - 1.0).max() <= ROW_TOL
        want = grouped(em, c)
        want[0] = blanks[0]
        got = post.sum(axis=0)
        worstGroup = max(worstGroup, float(np.abs(got - want).max()))
        assert counts_close(got, want), (got, want)
    print("bands %s: %d cases, %d finite; row sums off by %.3g, grouped counts by %.3g" % (bands, len(cases), sum(live), worstRow, worstGroup))
    assert np.mean(live) >= 0.85, np.mean(live)


@pytest.mark.parametrize("band", (None, 0, 1, 3))
def test_row_posteriors_are_the_gradient_of_forward(band):
    """Central differences of forward() in every finite entry of P, over the cases with L <= 3 and |LL| < 100."""
    worst, n = 0.0, 0
    for em, x, P, env in _cases(band):
        dp = _dp(em)
        post, ll = dp.rowPosteriors(x, P, env=env)
        if len(P) == 0 or len(P) > 3 or not abs(ll) < 100:
            continue
        for r in range(P.shape[0]):
            for o in range(P.shape[1]):
                if P[r, o] == -math.inf:
                    continue
                up, dn = P.copy(), P.copy()
                up[r, o] += FD_H; dn[r, o] -= FD_H
                fd = (dp.forward(x, up, env=env)[0] - dp.forward(x, dn, env=env)[0]) / (2 * FD_H)
                worst = max(worst, abs(fd - post[r, o])); n += 1
                assert abs(fd - post[r, o]) <= FD_TOL, (band, len(x), r, o, fd, post[r, o])
    print("band %s: %d derivatives, central differences off by at most %.3g" % (band, n, worst))
    assert n >= 50


def test_wrap_case_has_more_row_blocks_than_a_pair_has_workgroups():
    """wrap_case of test_profile_pair_mixed_gpu.py: (1, 1 100) at S = 2, C = 4.  With a table of 4 doubles a block is one row
    (profile_pair_rowpost_rows: tabMax / C), with 2 a row does not fit it and a block is one row as well: 1 100 blocks for the
    1 024 workgroups a pair gets at the most, so 76 workgroups take a second block.  The default table holds 1 024 rows: two blocks.
    The restatement's rows sum to 1 under no envelope, the full one and the staircase; the dead profile has no likelihood."""
    import pairenvhelpers as eh
    em, x, P, Pdead = eh.wrap_case()
    I, L = eh.WRAP_SHAPE
    C = em.nOutTok + 1
    assert (len(x), len(P), em.nStates, C) == (1, 1100, 2, 4) and eh.silent_levels(em) >= 1

    def rows_per_block(cells, tabMax):      # profile_pair_rowpost_rows (mb_profile_pair.h)
        if C > tabMax:
            return 1
        perRow = max(1, cells * em.nStates // (L + 1))
        return min(-(-8192 // perRow), tabMax // C, L)
    for cells in ((I + 1) * (L + 1), eh.n_cells(eh.staircase(I, L))):
        assert rows_per_block(cells, 4) == rows_per_block(cells, 2) == 1 and L > eh.WRAP_GROUPS
        assert -(-L // rows_per_block(cells, 4096)) == 2
    stairs = eh.staircase(I, L)
    assert all(b - a == 1 for a, b in zip(stairs.inStart, stairs.inEnd))
    dp = _dp(em)
    for env in (None, eh.full(I, L), stairs):
        post, ll = dp.rowPosteriors(x, P, env=env)
        assert ll > -math.inf and post.shape == (L, C) and np.abs(post.sum(axis=1) - 1.0).max() <= 1e-9 and (post[1024:] > 0).any()
    post, ll = dp.rowPosteriors(x, Pdead)
    assert ll == -math.inf and not post.any()


def _torch_pairs():
    """Two small pairs on one machine with finite entries, a ragged rowOff, the second under a band."""
    em = pair_machine(8, 108, True, 2, 3)
    (x0, P0), (x1, P1) = pair_input(np.random.RandomState(1), em, 2, 3, pZero=0.0), pair_input(np.random.RandomState(2), em, 3, 2, pZero=0.0)
    return em, [x0, x1], np.concatenate([P0, P1]), np.array([0, 3, 5]), [None, Envelope.band(3, 2, 1)]


def test_autograd_function_on_the_numpy_backend():
    em, xs, P, rowOff, envs = _torch_pairs()
    assert np.isfinite(P).all()
    logP = torch.tensor(P, dtype=torch.float64, requires_grad=True)
    ll = pair_profile_loglike(em, xs, logP, rowOff, envs=envs, backend="numpy")
    dp = PairProfileDP(em)
    want = [dp.forward(xs[k], P[rowOff[k]:rowOff[k + 1]], env=envs[k])[0] for k in range(2)]
    assert ll.shape == (2,) and np.isfinite(want).all() and np.array_equal(ll.detach().numpy(), want)
    (ll * torch.tensor([1.0, -2.5], dtype=torch.float64)).sum().backward()
    post = np.concatenate([dp.rowPosteriors(xs[k], P[rowOff[k]:rowOff[k + 1]], env=envs[k])[0] for k in range(2)])
    assert np.array_equal(logP.grad.numpy(), post * np.repeat([1.0, -2.5], [3, 2])[:, None])
    f = lambda t: pair_profile_loglike(em, xs, t, rowOff, envs=envs, backend="numpy")
    assert torch.autograd.gradcheck(f, (torch.tensor(P, dtype=torch.float64, requires_grad=True),), eps=1e-6, atol=1e-7, rtol=1e-6)
    with pytest.raises(ValueError):
        pair_profile_loglike(em, xs, logP.float(), rowOff, backend="numpy")
    with pytest.raises(ValueError):
        pair_profile_loglike(em, xs, logP, [0, 3], backend="numpy")


def _dnastore():
    m = Machine.fromFile(DNASTORE)
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    return m, em, Profile.fromCsv(CSV)


def test_score_profile_pairs_posteriors():
    m, em, prof = _dnastore()
    P = prof.logRows(em)
    dp = PairProfileDP(em)
    seqs = [["0_3", "2_3", "1_3"], ["nonsense"], [], ["1_3", "1_3"]]
    par = m.getParamDefs(True)
    plain = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par)[0]
    assert "posteriors" not in plain and set(plain) == {"loglike", "viterbi"}
    for band in (None, 2):
        sc, _ = boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par, band=band, posteriors=True)
        assert len(sc["posteriors"]) == len(seqs) and not sc["posteriors"][1].any() and sc["loglike"][1] == -math.inf
        live = 0
        for k in (0, 2, 3):
            x = em.inputTokenizer.tokenize(seqs[k])
            env = None if band is None else Envelope.band(len(x), len(P), band)
            want, ll = dp.rowPosteriors(x, P, env=env)
            assert sc["posteriors"][k].shape == P.shape and np.array_equal(sc["posteriors"][k], want) and sc["loglike"][k] == ll
            if ll > -math.inf:
                live += 1
                assert np.abs(want.sum(axis=1) - 1.0).max() <= ROW_TOL
        assert live >= 2
    with pytest.raises(MachineError, match="row posteriors take plain profiles"):
        boss.scoreProfilePairs(m, seqs, prof, backend="numpy", params=par, merge=True, posteriors=True)


def test_cli_profile_posteriors(tmp_path):
    m, em, prof = _dnastore()
    P = prof.logRows(em)
    dp = PairProfileDP(em)
    (tmp_path / "x.json").write_text(json.dumps({"name": "x1", "sequence": ["0_3", "2_3", "1_3"]}))
    base = [DNASTORE, "--use-defaults", "--recognize-csv", CSV, "--decode-backend", "numpy"]

    def run(*args):
        out = io.StringIO()
        assert boss.run(base + list(args), out) == 0
        return out.getvalue()
    got = json.loads(run("--input-json", str(tmp_path / "x.json"), "--input-chars", "", "--profile-posteriors"))
    assert [g[:2] for g in got] == [["", ""], ["x1", ""]]
    for g, x in zip(got, ([], em.inputTokenizer.tokenize(["0_3", "2_3", "1_3"]))):
        want, ll = dp.rowPosteriors(x, P)
        assert ll > -math.inf and np.array(g[2]).shape == P.shape
        assert np.abs(np.array(g[2], float) - want).max() <= 1e-5          # (%g: six significant digits)
    assert json.loads(run("--input-chars", "012", "--profile-posteriors")) == [["012", "", [[0] * P.shape[1]] * len(P)]]
    lines = run("--input-chars", "", "-L", "--profile-posteriors", "--profile-band", "3").splitlines()
    assert len(lines) == 2 and abs(json.loads(lines[0])[0][2] - dp.forward([], P, env=Envelope.band(0, len(P), 3))[0]) <= 1e-4

    def fails(args, msg):
        with pytest.raises(MachineError, match=msg):
            boss.run(args, io.StringIO())
    fails(base + ["--input-chars", ""], "needs -L, -V or -C")
    fails(base + ["--profile-posteriors"], "--profile-posteriors goes with --recognize-csv beside an input sequence")
    fails([DNASTORE, "--use-defaults", "--profile-posteriors"], "--profile-posteriors goes with --recognize-csv beside an input sequence")
    fails([DNASTORE, "--use-defaults", "--recognize-merge-csv", CSV, "--input-chars", "", "--profile-posteriors"], "takes no input sequence")
