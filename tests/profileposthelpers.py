"""Shared helpers of the row-posterior tests of the one-tape profile sweeps (test_profile_post_host.py, test_profile_post_gpu.py;
docs/profile_tapes.md, "Row posteriors of one-tape profiles"): the machines and profiles of both suites, built with the builders of
profhelpers, mergehelpers and randmachine, the grouping of counts and columns by output token, and the CTC case with torch's loss as
its reference.  Every builder is deterministic; the seeds were searched on the CPU so that the liveness conditions hold, and
test_profile_post_host.py asserts them."""
import math

import numpy as np

from mergehelpers import few_levels_machine, lane_case, merged_rows
from profhelpers import _profiles
from randmachine import random_machine
from machineboss_amd.profile import MergedProfileDP, ProfileDP

ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7


def post_machine(S, nOut, silent, seed):
    """A generator of S states (no input alphabet): cycles, emitting edges into the end state from a third of the states; with
    `silent` the default silent backbone up to 8 states and a few silent edges (a handful of levels) beyond."""
    if S <= 8:
        return random_machine(S, 0, nOut, seed, to_end=0.3) if silent else random_machine(S, 0, nOut, seed, silent_density=0.0, backbone=0.0, to_end=0.3)
    return few_levels_machine(S, 0, nOut, seed) if silent else random_machine(S, 0, nOut, seed, density=1.5, silent_density=0.0, backbone=0.0, to_end=0.3)


def yardstick(em, colTok=None):
    return ProfileDP(em) if colTok is None else MergedProfileDP(em, colTok)


def grouped(em, counts):
    """counts() added up by the output token of the transition: [nOutTok], token 1 first."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(em.outTok, np.int64), counts)
    return g[1:]


def by_token(em, colTok, cols):
    """Column sums cols[1..nCols] of a merged profile added up by the column's token: [nOutTok]."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(colTok, np.int64), np.asarray(cols)[1:])
    return g[1:]


# ---- the host suite: S in {1, 2, 8, 65} with and without silent levels, plain and nCols in {1, 2, 4}, L = 0..9 -----------------------
HOST_STATES = (1, 2, 8, 65)
HOST_COLS = (1, 2, 4)
HOST_SEEDS = {(1, False): 709, (2, True): 703, (2, False): 709, (8, True): 708, (8, False): 746, (65, True): 765, (65, False): 765}


def host_cases():
    """[(em, colTok or None, profs)]: per machine the plain profiles of 0..9 rows and, per nCols, merged ones; a tenth of the weights
    -inf.  A machine without silent levels cannot score a profile of no rows from two states on, so a twentieth of the likelihoods
    is -inf by construction."""
    out = []
    for (S, silent), seed in HOST_SEEDS.items():
        em = post_machine(S, 3, silent, seed)
        out.append((em, None, _profiles(em, range(10), seed + 1, zeros=0.1)))
        for nC in HOST_COLS:
            rng = np.random.RandomState(seed + 10 * nC)
            colTok = rng.randint(1, 4, nC)
            out.append((em, colTok, [merged_rows(rng, nC, L, zeros=0.1) for L in range(10)]))
    return out


# ---- the GPU suite --------------------------------------------------------------------------------------------------------------------
GPU_STATES = (1, 2, 63, 64, 65, 300)
GPU_LENGTHS = (0, 1, 2, 9)
GPU_SEEDS = {(1, False): 709, (2, True): 703, (2, False): 709, (63, True): 865, (63, False): 865, (64, True): 865, (64, False): 865,
             (65, True): 765, (65, False): 765, (300, True): 1100, (300, False): 1100}
GPU_MERGED = ((1, 1), (2, 1), (4, 13), (4, 65), (63, 2), (65, 2))


def gpu_plain_case(S, silent):
    em = post_machine(S, 3, silent, GPU_SEEDS[(S, silent)])
    return em, _profiles(em, GPU_LENGTHS, GPU_SEEDS[(S, silent)] + 1, zeros=0.1)


def gpu_merged_case(nCols, S):
    """(em, colTok, profs): mergehelpers.lane_case where it has the shape (lengths 0, 1, 7, 23, cut to 9 rows), else its recipe."""
    if (nCols, S) == (4, 65):
        em = few_levels_machine(65, 0, 3, 765)
        rng = np.random.RandomState(766)
        colTok = rng.randint(1, 4, nCols)
        return em, colTok, [merged_rows(rng, nCols, L, zeros=0.2) for L in (0, 1, 7, 9)]
    em, colTok, profs = lane_case(nCols, S)
    return em, colTok, [P[:9] for P in profs]


def long_rows(rng, width, L):
    """L rows without -inf and with a blank of at least log 0.3: long profiles that stay alive."""
    P = np.log(rng.uniform(0.02, 1.0, (L, width)))
    P[:, 0] = np.maximum(P[:, 0], math.log(0.3))
    return P


def one_lane_rows_case():
    """S = 1 at L = 200: 64 rows in a wavefront, every lane its own row."""
    em = post_machine(1, 3, False, 709)
    return em, [long_rows(np.random.RandomState(11), 4, 200)]


def row_blocks_case():
    """S = 40 at L = 300: 205 rows a block, two blocks."""
    em = post_machine(40, 3, True, 740)
    return em, [long_rows(np.random.RandomState(12), 4, 300)]


def many_blocks_case(merged):
    """S = 2 at L = 1 100, nOutTok = 3 or nCols = 3: with a table of 4 doubles one row a block, more blocks than the 1 024 groups."""
    em = post_machine(2, 3, True, 703)
    P = long_rows(np.random.RandomState(13), 4, 1100)
    return (em, [1, 2, 3], [P]) if merged else (em, None, [P])


def wide_alphabet_case():
    """S = 2 with 70 output tokens at L = 0, 5, 7: 71 columns, more than a wavefront has lanes."""
    em = post_machine(2, 70, True, 270)
    return em, _profiles(em, (5, 0, 7), 271, zeros=0.05)


def ragged_case(merged):
    """Ten profiles of 0..40 rows at S = 40, the third empty, the sixth dead (a row all -inf)."""
    em = post_machine(40, 3, True, 740)
    rng = np.random.RandomState(41)
    lengths = [17, 3, 0, 40, 9, 6, 1, 25, 12, 33]
    width = 5 if merged else 4
    profs = [long_rows(rng, width, L) for L in lengths]
    for P in profs[::2]:
        P[rng.rand(*P.shape) < 0.1] = -np.inf
        if len(P):
            P[:, 0] = np.maximum(P[:, 0], math.log(0.3))
    profs[5][2] = -np.inf
    return (em, [1, 2, 3, 1], profs) if merged else (em, None, profs)


def post_bytes(em, colTok, P):
    """The device bytes mb_profiles_row_posteriors charges one profile to the memory budget: two lattices and its bins (these shapes
    need no global scratch)."""
    PL = 1 if colTok is None else len(colTok) + 1
    width = em.nOutTok + 1 if colTok is None else PL
    return 2 * 8 * (len(P) + 1) * 2 * PL * em.nStates + 8 * len(P) * width


def hard_cases():
    """{name: (em, colTok or None, profs)}: a third of the weights -inf; a whole row -inf (one profile of the batch); all-blank rows;
    a profile and the same 700 lower per entry."""
    out = {}
    em = post_machine(40, 3, True, 740)
    for merged in (False, True):
        colTok, width, tag = ([1, 2, 3, 1], 5, " merged") if merged else (None, 4, "")
        rng = np.random.RandomState(50 + merged)
        profs = []
        for L in (4, 9, 9, 20):
            P = np.log(rng.uniform(0.02, 1.0, (L, width)))
            P[rng.rand(L, width) < 1.0 / 3] = -np.inf
            profs.append(P)
        out["third" + tag] = (em, colTok, profs)
        profs = [long_rows(rng, width, L) for L in (6, 9, 12)]
        profs[1][4] = -np.inf
        out["infrow" + tag] = (em, colTok, profs)
        P = np.full((12, width), -np.inf)
        P[:, 0] = np.log(rng.uniform(0.1, 1.0, 12))
        out["allblank" + tag] = (random_machine(50, 0, 3, 502), colTok, [P])      # (a silent path from 0 to S - 1: mergehelpers.all_blank_case)
        P = long_rows(rng, width, 9)
        out["far" + tag] = (em, colTok, [P, P - 700.0])
    return out


# ---- CTC: a linear-chain generator against frames, torch's ctc_loss as the reference ---------------------------------------------------
CTC_Y = [1, 2, 2, 3]
CTC_COLTOK = [1, 2, 3]
CTC_FRAMES = (3, 4, 7, 12)


def ctc_machine():
    from machineboss_amd import algebra
    from machineboss_amd.evalmachine import EvaluatedMachine
    em = EvaluatedMachine.fromMachine(algebra.generator([["a", "b", "c"][t - 1] for t in CTC_Y], "y"), {}, useDefaults=True)
    assert list(em.outputTokenizer.tok2sym[1:]) == ["a", "b", "c"]
    return em


def ctc_frames(T, normalised):
    """float64 [T, 4] frames, column 0 the blank: log-softmax rows, or the raw scores shifted (rows that do not sum to 1)."""
    import torch
    x = torch.randn(T, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(100 + T))
    return torch.log_softmax(x, 1) if normalised else x - 0.5


def ctc_reference(lp):
    """(-ctc_loss, exp(lp) - d ctc_loss / d lp) from torch's CPU loss and its native backward, which returns exp(lp) minus the
    posteriors whether or not the rows are normalised; (-inf, zeros) where the loss is infinite."""
    import torch
    lp = lp.detach().clone().requires_grad_(True)
    T = lp.shape[0]
    loss = torch.nn.functional.ctc_loss(lp.unsqueeze(1), torch.tensor([CTC_Y]), torch.tensor([T]), torch.tensor([len(CTC_Y)]), reduction="sum")
    if not math.isfinite(loss.item()):
        return -math.inf, np.zeros(tuple(lp.shape))
    loss.backward()
    return -loss.item(), (torch.exp(lp) - lp.grad).detach().numpy()
