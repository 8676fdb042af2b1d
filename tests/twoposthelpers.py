"""Inputs, bounds and the device-against-yardstick comparison of the row posteriors of the two-profile sweeps
(test_profile_two_post_host.py, test_profile_two_post_gpu.py; not a test module).  The machines and profiles come from
twoprofilehelpers, the bounds from pairprofilehelpers; what is new here are the input families of the GPU module, the block and
chunk rules of mb_profile_twos_row_posteriors restated, and the comparison itself."""
import math

import numpy as np

import twoprofilehelpers as th
from pairprofilehelpers import counts_close, logs_close, note, note_counts, pair_machine
from twoprofilehelpers import two_input

ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7

# ---- the rules of the host, restated -------------------------------------------------------------------------------------------------
ROWPOST_LDS_MAX = 4096
ROWPOST_ITEMS = 8192
ROWPOST_GROUPS_MAX = 1024


def rowpost_rows(S, K, L, axis, nIn, nOut, table=ROWPOST_LDS_MAX):
    """profile_pair_rowpost_rows as k_profile_two_rowpost calls it: the lines of a block on axis 0 (output rows, nOut + 1 bins each,
    (K + 1) S items each) or axis 1 (input rows, nIn + 1 bins, (L + 1) S items)."""
    lines, cols = (K, nIn + 1) if axis else (L, nOut + 1)
    if lines <= 0 or cols > table:
        return 1
    per = max(1, (K + 1) * (L + 1) * S // (lines + 1))
    return min(-(-ROWPOST_ITEMS // per), table // cols, lines)


def rowpost_blocks(S, K, L, axis, nIn, nOut, table=ROWPOST_LDS_MAX):
    lines = K if axis else L
    return -(-lines // rowpost_rows(S, K, L, axis, nIn, nOut, table))


def post_bytes(S, K, L, nIn, nOut):
    """What lattice_chunks is told a pair costs mb_profile_twos_row_posteriors: both lattices and the pair's bins of both tables."""
    return 2 * 8 * 3 * S * (K + 1) * (L + 1) + 8 * (L * (nOut + 1) + K * (nIn + 1))


def grouped(em, counts):
    """(counts by input token [1..nIn], by output token [1..nOut])"""
    a = np.zeros(em.nInTok + 1); b = np.zeros(em.nOutTok + 1)
    np.add.at(a, np.asarray(em.inTok, np.int64), counts); np.add.at(b, np.asarray(em.outTok, np.int64), counts)
    return a[1:], b[1:]


def fixed_close(got, want, items):
    """counts_close with the error of the fixed point added: ``items`` lane sums feed a bin, each rounded once to the nearest 2^-36."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.where(want >= 1e-3, 0.0, 1e-9) + 1e-6 * want + items * 2.0 ** -37))


# ---- the input families of the GPU module ----------------------------------------------------------------------------------------------
SUITE_STATES = (1, 2, 8, 64, 65)
SUITE_CASES = [(S, nIn, nOut) for S in SUITE_STATES for nIn, nOut in th.SUITE_ALPHABETS]


def suite_case(S, nIn, nOut):
    """twoprofilehelpers.suite_case: seven lattices from (0, 0) to (9, 9) on the machine with silent levels and without, a tenth of
    the weights of either profile -inf.  S = 64 is not among its states: the same builder with seeds of its own, under which nine in
    ten likelihoods are finite at every alphabet (test_profile_two_post_host.py holds them to it)."""
    if S in th.SUITE_STATES:
        return th.suite_case(S, nIn, nOut)
    out = []
    for levels in (True, False):
        em = pair_machine(S, 100 + S, levels, nIn, nOut)
        for K, L in th.SUITE_SHAPES:
            out.append((em,) + two_input(np.random.RandomState(400000 + 1000 * S + 10 * K + L), em, K, L, pInf=0.1))
    return out


WIDE_S, WIDE_K, WIDE_L = 40, 40, 40


def block_case():
    """S = 40 at K = L = 40: 1 640 items a line on either axis, five lines a block, eight blocks; one line a block under a table of 4."""
    em = pair_machine(WIDE_S, 41, True, 2, 3)
    return (em,) + two_input(np.random.RandomState(41), em, WIDE_K, WIDE_L, pInf=0.0)


COLUMN_ALPHABETS = ((70, 3), (3, 70))
COLUMN_SHAPES = ((4, 5), (0, 5), (5, 0), (7, 3))


def column_case(nIn, nOut):
    """S = 2 with 71 columns on one tape, more than a wavefront has lanes: four pairs."""
    em = pair_machine(2, 270, False, nIn, nOut)
    return em, [two_input(np.random.RandomState(270 + 10 * K + L), em, K, L, pInf=0.0) for K, L in COLUMN_SHAPES]


RAGGED_SHAPES = ((0, 0), (0, 5), (5, 0), (5, 6), (9, 2), (2, 9), (1, 1), (6, 6), (3, 7), (7, 3), (4, 4))
RAGGED_DEAD = 3


def ragged_case():
    """Eleven pairs on S = 40 with levels and (nIn, nOut) = (3, 5); the fourth has a whole -inf row in B."""
    em = pair_machine(40, 7, True, 3, 5)
    pairs = [two_input(np.random.RandomState(50 + 10 * K + L), em, K, L, pInf=0.0) for K, L in RAGGED_SHAPES]
    pairs[RAGGED_DEAD] = th.dead_pair(np.random.RandomState(59), em, *RAGGED_SHAPES[RAGGED_DEAD], 2)
    return em, pairs


def sparse_case():
    """A third of the weights of either table -inf, blanks included: twelve pairs at (5, 6) on S = 40.  About one such pair in four
    has a row without a finite weight; the seed is one under which eleven of the twelve are live."""
    em = pair_machine(40, 11, True, 2, 3)
    rng = np.random.RandomState(18)
    return em, [two_input(rng, em, 5, 6, pInf=1.0 / 3.0) for _ in range(12)]


def chunk_budget(em, pairs):
    """About two pairs: twice the largest pair and a little."""
    return 2 * max(post_bytes(em.nStates, len(A), len(B), em.nInTok, em.nOutTok) for A, B in pairs) + 4096


LONG = 1100
LONG_SHAPES = ((1, LONG), (LONG, 1))


def long_case(K, L):
    """S = 2 at (1, 1 100) or (1 100, 1), and a dead pair of the same shape: under a table of 4 doubles a line is a block, so the long
    axis has 1 100 blocks against 1 024 groups."""
    em = pair_machine(2, 1102, True, 2, 3)
    live = two_input(np.random.RandomState(1100 + K), em, K, L, pInf=0.0)
    dead = [t.copy() for t in two_input(np.random.RandomState(1200 + K), em, K, L, pInf=0.0)]
    (dead[0] if K > L else dead[1])[LONG // 2] = -np.inf
    return em, [live, tuple(dead)]


def fd_case():
    """One finite (3, 3) pair at S = 8."""
    em = pair_machine(8, 108, True, 2, 3)
    return (em,) + two_input(np.random.RandomState(3), em, 3, 3, pInf=0.0)


def perturbed(A, B, h=FD_H):
    """[(A', B')]: every entry of A, then of B, moved up and down by h."""
    out = []
    for t, T in enumerate((A, B)):
        for idx in np.ndindex(*T.shape):
            for sgn in (1.0, -1.0):
                Q = T.copy(); Q[idx] += sgn * h
                out.append((Q, B) if t == 0 else (A, Q))
    return out


# ---- the device against the yardstick (the GPU module; the device is touched only when these are called) -----------------------------
WORST = {}


def yardstick(em, pairs):
    from machineboss_amd.profile import TwoProfileDP
    dp = TwoProfileDP(em)
    return [dp.rowPosteriors(A, B) for A, B in pairs]


def split(dev, postA, postB):
    return ([postA[dev.inOff[k]:dev.inOff[k + 1]] for k in range(dev.nPairs)], [postB[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)])


def compare(em, gotA, gotB, ll, refs, what="posteriors", fixed=False):
    """The device's per-pair tables and likelihoods against the yardstick's: entries, exact zeros, row sums.  ``fixed``: the device
    ran in fixed point -- every bound then has the rounding of the lane sums that feed the bin added, and a row sum that of its
    bins."""
    want = np.array([r[2] for r in refs])
    note("loglike", ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    S = em.nStates
    for k, (wa, wb, wl) in enumerate(refs):
        for g, w, items in ((gotA[k], wa, (len(wb) + 1) * S), (gotB[k], wb, (len(wa) + 1) * S)):
            assert g.shape == w.shape, (k, g.shape, w.shape)
            if not g.size:
                continue
            note_counts(g.ravel(), w.ravel(), WORST, what)
            assert (fixed_close(g, w, items) if fixed else counts_close(g, w)), (k, np.abs(g - w).max())
            assert not g[w == 0.0].any() and (g >= 0.0).all(), k
            if wl > -math.inf:
                WORST["row sums, " + what] = max(WORST.get("row sums, " + what, 0.0), float(np.abs(g.sum(axis=1) - 1.0).max()))
                assert np.abs(g.sum(axis=1) - 1.0).max() <= ROW_TOL + (g.shape[1] * items * 2.0 ** -37 if fixed else 0.0), (k, g.sum(axis=1))
            else:
                assert not g.any(), k


def open_pairs(em, pairs):
    from machineboss_amd import capi
    dm = capi.DeviceMachine(em)
    return dm, capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs])


def check(em, pairs, launches=None, refs=None, what="posteriors", fixed=False):
    """row_posteriors() of the pairs of one machine, in one batch, against the yardstick: (gotA, gotB, ll, refs)."""
    from machineboss_amd import capi
    refs = yardstick(em, pairs) if refs is None else refs
    dm, dev = open_pairs(em, pairs)
    try:
        postA, postB, ll = dev.row_posteriors()
        assert capi.last_kernel_name() == "k_profile_two_rowpost"
        if launches is not None:
            assert capi.last_launch_count() == launches
        assert postA.shape == (dev.inOff[-1], em.nInTok + 1) and postB.shape == (dev.rowOff[-1], em.nOutTok + 1)
        gotA, gotB = split(dev, postA, postB)
        compare(em, gotA, gotB, ll, refs, what, fixed)
    finally:
        dev.close(); dm.close()
    return gotA, gotB, ll, refs
