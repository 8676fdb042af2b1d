"""Inputs, bounds and comparisons of the row-posterior tests of pairs against CTC-merged profiles (test_profile_pair_merge_post_host.py,
test_profile_pair_merge_post_gpu.py; not a test module).  The inputs are those of pairmergehelpers wherever they fit; every builder
is deterministic, and test_profile_pair_merge_post_host.py::test_gpu_suite_inputs_are_live holds the conditions the GPU tests assert
-- finite likelihoods, block counts, chunk counts -- to the yardstick and to plain arithmetic, without a GPU.

Bounds (those of the sibling suites, pairprofilehelpers): likelihoods 1e-9 relative to max(1, |value|), -inf exact; posteriors as
counts, 1e-6 relative from 1e-3 up and 1e-9 + 1e-6 x value below; -inf entries and dead pairs exactly 0; row sums 1e-6 (non-negative
entries, each within 1e-6 relative, that sum to 1); central differences at h = 1e-6 within 1e-7 absolute (truncation about h^2,
rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100)."""
import math

import numpy as np

import pairmergehelpers as mh
from pairmergehelpers import LANE_CASES, SHAPES, lane_case, merged_input
from pairprofilehelpers import counts_close, logs_close, note, note_counts, pair_machine

ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7
ROWPOST_ITEMS, ROWPOST_LDS_MAX, ROWPOST_GROUPS = 8192, 4096, 1024

HOST_STATES, HOST_COLS = (1, 2, 8, 65), (1, 2, 4)


def host_cases():
    """[(em, colTok, x, P)]: lane_case for S in 1, 2, 8, 65 (with silent levels and without) and 1, 2, 4 columns, the seven SHAPES."""
    return [(em, colTok, x, P) for S in HOST_STATES for nCols in HOST_COLS for em, colTok, pairs in lane_case(nCols, S) for x, P in pairs]


def by_token(em, colTok, cols):
    """cols[nCols] (one value per column 1..nCols) added up by the columns' tokens: [nOutTok + 1], entry 0 left at 0."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(colTok, np.int64), np.asarray(cols, np.float64))
    return g


def grouped(em, colTok, counts):
    """counts[nTrans] added up by output token, [nOutTok + 1]; entry 0 and the tokens no column stands for left at 0."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(em.outTok, np.int64), counts)
    keep = np.zeros(em.nOutTok + 1, bool)
    keep[np.asarray(colTok, np.int64)] = True
    g[~keep] = 0.0
    return g


def rows_per_block(S, nCols, I, L, tabMax=ROWPOST_LDS_MAX):
    """profile_pair_rowpost_rows (mb_profile_pair.h) over rows of (I + 1)(nCols + 1) S items and nCols + 1 bins."""
    PL = nCols + 1
    if L <= 0 or PL > tabMax:
        return 1
    perRow = max(1, (I + 1) * PL * S)
    return min(-(-ROWPOST_ITEMS // perRow), tabMax // PL, L)


def blocks(S, nCols, I, L, tabMax=ROWPOST_LDS_MAX):
    return -(-L // rows_per_block(S, nCols, I, L, tabMax)) if L else 0


def pair_bytes(S, nCols, I, L):
    """What mb_profile_pairs_row_posteriors_merged books for one pair: two lattices, the X / T ring where it does not fit LDS, the bins."""
    ring = mh.ring_bytes(S, nCols, I, L, mat=True)
    return 2 * 8 * (I + 1) * (L + 1) * 2 * (nCols + 1) * S + (ring if ring > mh.LDS_MAX else 0) + 8 * L * (nCols + 1)


# ---- the shapes of the GPU suite -------------------------------------------------------------------------------------------------------
WAVE_COLTOK = (1, 2, 3, 1)


def wave_case():
    """nCols = 4, S = 64 at (2, 5) and (5, 2), with levels: every wavefront holds exactly one (cell, plane)."""
    em = pair_machine(64, 264, True, 2, 3)
    return em, WAVE_COLTOK, [merged_input(np.random.RandomState(640 + I), em, 4, I, L) for I, L in ((2, 5), (5, 2))]


WRAP_SHAPE = (1, 1100)


def wrap_case():
    """(em, colTok, [(x, P), (x, Pdead)]): nCols = 4, S = 2 at (1, 1 100), 20 items a row; the dead pair has one row all -inf.  With a
    table of 5 doubles a block is one row: 1 100 blocks for the 1 024 groups a pair gets.  With 2 a row does not fit: global bins, one
    row a block as well.  The default takes 410 rows a block: three blocks."""
    em = pair_machine(2, 202, True, 2, 3)
    I, L = WRAP_SHAPE
    x, P = merged_input(np.random.RandomState(1100), em, 4, I, L, zeros=0.1)
    dead = P.copy()
    dead[700] = -np.inf
    return em, WAVE_COLTOK, [(x, P), (x, dead)]


def wide_case():
    """lane_case(65, 2): 66 bins a row, more than a wavefront has lanes; with a table of 16 doubles a row is summed in its global bins."""
    return lane_case(65, 2)


CHUNK_S = 65


CHUNK_SHAPES = ((9, 9), (2, 5), (9, 9), (5, 2), (9, 9), (0, 3), (3, 0))


def chunk_case():
    """nCols = 4, S = 65: (9, 9) three times with different data between small pairs (the X ring of (9, 9), 62 400 bytes, is in
    LDS).  Under 1.8 times the bytes of (9, 9) no two of the three share a chunk: three chunks or more."""
    em = pair_machine(CHUNK_S, 265, True, 2, 3)
    rng = np.random.RandomState(4065)
    return em, WAVE_COLTOK, [merged_input(rng, em, 4, I, L) for I, L in CHUNK_SHAPES]


def chunk_budget():
    return int(1.8 * max(pair_bytes(CHUNK_S, 4, I, L) for I, L in CHUNK_SHAPES)) - 1


def ragged_post_case():
    """pairmergehelpers.ragged_case (a dead pair last; (0, 40): an empty input; (40, 0): an empty profile)."""
    return mh.ragged_case()


def third_inf_case():
    """S = 20, nCols = 4: a third of the profile's weights -inf, blanks included, and a third of the machine's."""
    em = pair_machine(20, 50, True, 2, 3)
    lw = em.logWeight.copy()
    lw[np.random.RandomState(53).choice(len(lw), len(lw) // 3, replace=False)] = -np.inf
    rng = np.random.RandomState(54)
    pairs = []
    for I, L in ((3, 6), (2, 5), (4, 2), (5, 5), (0, 4), (6, 6)):
        x, P = merged_input(rng, em, 4, I, L, zeros=0.0)
        P[rng.uniform(size=P.shape) < 1.0 / 3.0] = -np.inf
        pairs.append((x, P))
    return em.withLogWeights(lw), WAVE_COLTOK, pairs


FAR_SHIFT = -700.0


def far_case():
    """(em, colTok, [(x, P), (x, P + FAR_SHIFT)]) at (9, 9), S = 65: a lattice whose cells run down to about -6 300."""
    em = pair_machine(65, 9, True, 2, 3)
    x, P = merged_input(np.random.RandomState(99), em, 4, 9, 9, zeros=0.1)
    return em, WAVE_COLTOK, [(x, P), (x, P + FAR_SHIFT)]


def fd_case():
    """(em, colTok, x, P): S = 8 with levels at (3, 3), three columns with two on one token, every weight finite."""
    em = pair_machine(8, 108, True, 2, 3)
    x, P = merged_input(np.random.RandomState(3), em, 3, 3, 3, zeros=0.0)
    return em, (1, 2, 1), x, P


# ---- CTC ------------------------------------------------------------------------------------------------------------------------------
CTC_COLTOK, CTC_X, CTC_T = (1, 2, 3), (1, 2, 2, 3), (3, 4, 7, 12)


def echo_machine():
    """One state, for each of three symbols one loop that reads it and writes it at weight 1: the pair likelihood of x against merged
    frames is the CTC likelihood of x."""
    from prefixhelpers import machine_from_edges
    return machine_from_edges(1, 3, 3, [(0, 0, a, a, 0.0) for a in (1, 2, 3)])


def ctc_frames(T, normalised):
    """[T, 4] float64 log weights, blank first; normalised: log-softmax rows."""
    lp = np.random.RandomState(7000 + T).normal(size=(T, 4)) * 1.5
    if normalised:
        lp = lp - np.logaddexp.reduce(lp, axis=1, keepdims=True)
    return lp


def ctc_reference(lp):
    """(ctc_loss, d ctc_loss / d lp) of torch.nn.functional.ctc_loss on the CPU, reduction sum, x = CTC_X; inf is kept."""
    import torch
    t = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
    loss = torch.nn.functional.ctc_loss(t.unsqueeze(1), torch.tensor([CTC_X]), torch.tensor([len(lp)]), torch.tensor([len(CTC_X)]),
                                        blank=0, reduction="sum", zero_infinity=False)
    if not math.isfinite(float(loss.detach())):
        return float(loss.detach()), None
    loss.backward()
    return float(loss.detach()), t.grad.numpy()


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
WORST = {}


def yardstick(em, colTok, pairs):
    from machineboss_amd.profile import PairMergedProfileDP
    dp = PairMergedProfileDP(em, colTok)
    return [dp.rowPosteriors(x, P) for x, P in pairs]


def compare(got, ll, refs, what="posteriors"):
    """The device's per-pair posteriors and likelihoods against the yardstick's: entries, exact zeros, row sums."""
    want = np.array([r[1] for r in refs])
    note("loglike", ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    for k, (g, (w, wl)) in enumerate(zip(got, refs)):
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if not g.size:
            continue
        note_counts(g.ravel(), w.ravel(), WORST, what)
        assert counts_close(g, w), (k, np.abs(g - w).max())
        assert not g[w == 0.0].any() and (g >= 0.0).all(), k
        if wl > -math.inf:
            WORST["row sums"] = max(WORST.get("row sums", 0.0), float(np.abs(g.sum(axis=1) - 1.0).max()))
            assert np.abs(g.sum(axis=1) - 1.0).max() <= ROW_TOL, (k, g.sum(axis=1))
        else:
            assert not g.any(), k
