"""Inputs, bounds and the device-against-yardstick comparison of the row posteriors of the two-profile sweeps against CTC-merged
output profiles (test_profile_two_merge_post_host.py, test_profile_two_merge_post_gpu.py; not a test module).  The machines and
profiles come from twomergehelpers and twoprofilehelpers, the CTC case from pairmergeposthelpers; what is new here are the input
families of the GPU module, the block and chunk rules of mb_profile_twos_row_posteriors_merged restated, and the comparison itself.
Every builder is deterministic, and test_profile_two_merge_post_host.py::test_gpu_inputs_are_live holds the conditions the GPU tests
assert -- finite likelihoods, block counts, chunk counts -- to the yardstick and to plain arithmetic, without a GPU.

Bounds (those of the sibling suites): likelihoods 1e-9 relative to max(1, |value|), -inf exact; posteriors as counts, 1e-6 relative
from 1e-3 up and 1e-9 + 1e-6 x value below; -inf entries and dead pairs exactly 0; row sums 1e-6; central differences at h = 1e-6
within 1e-7 absolute (truncation about h^2, rounding about 2 ulp(LL) / 2h < 1e-8 for |LL| < 100).  In fixed point a lane sum is
rounded once to the nearest 2^-36, so a bin fed by n items -- (K + 1)(nCols + 1) S for an output row, (L + 1)(nCols + 1) S for an
input row -- may be off by n 2^-37 more, and a row sum by that of its bins."""
import functools
import math

import numpy as np

import twomergehelpers as tm
import twoprofilehelpers as th
from pairmergeposthelpers import CTC_COLTOK, CTC_T, CTC_X, ctc_frames, ctc_reference, echo_machine  # noqa: F401
from pairprofilehelpers import counts_close, logs_close, note, note_counts, pair_machine
from twomergehelpers import merged_input
from twoposthelpers import fixed_close, perturbed  # noqa: F401

ROW_TOL = 1e-6
FD_H, FD_TOL = 1e-6, 1e-7
SHAPES = tm.LANE_SHAPES                              # the seven shapes from (0, 0) to (9, 9)

# ---- the rules of the host, restated -------------------------------------------------------------------------------------------------
ROWPOST_LDS_MAX = 4096
ROWPOST_ITEMS = 8192
ROWPOST_GROUPS_MAX = 1024


def rowpost_rows(S, nCols, K, L, axis, nIn, table=ROWPOST_LDS_MAX):
    """profile_pair_rowpost_rows as k_profile_two_merge_rowpost calls it: the lines of a block on axis 0 (output rows, nCols + 1 bins
    each, (K + 1)(nCols + 1) S items each) or axis 1 (input rows, nIn + 1 bins, (L + 1)(nCols + 1) S items)."""
    lines, cols = (K, nIn + 1) if axis else (L, nCols + 1)
    if lines <= 0 or cols > table:
        return 1
    per = max(1, (K + 1) * (L + 1) * (nCols + 1) * S // (lines + 1))
    return min(-(-ROWPOST_ITEMS // per), table // cols, lines)


def rowpost_blocks(S, nCols, K, L, axis, nIn, table=ROWPOST_LDS_MAX):
    lines = K if axis else L
    return -(-lines // rowpost_rows(S, nCols, K, L, axis, nIn, table))


def pair_bytes(S, nCols, K, L, nIn):
    """What lattice_chunks is told a pair costs mb_profile_twos_row_posteriors_merged: both lattices, the X / T ring where it does not
    fit LDS and the pair's bins of both tables."""
    ring = tm.ring_bytes(S, nCols, K, L, mat=True)
    return 2 * tm.cell_bytes(S, nCols, K, L) + (ring if ring > tm.RING_LDS_MAX else 0) + 8 * (L * (nCols + 1) + K * (nIn + 1))


def by_token(em, colTok, cols):
    """cols[nCols] (one value per column 1..nCols) added up by the columns' tokens: [nOutTok + 1], entry 0 left at 0."""
    g = np.zeros(em.nOutTok + 1)
    np.add.at(g, np.asarray(colTok, np.int64), np.asarray(cols, np.float64))
    return g


def grouped(em, colTok, counts):
    """(counts by input token [1..nIn], by output token [nOutTok + 1] with entry 0 and the tokens no column stands for left at 0)"""
    a = np.zeros(em.nInTok + 1); b = np.zeros(em.nOutTok + 1)
    np.add.at(a, np.asarray(em.inTok, np.int64), counts); np.add.at(b, np.asarray(em.outTok, np.int64), counts)
    keep = np.zeros(em.nOutTok + 1, bool)
    keep[np.asarray(colTok, np.int64)] = True
    b[~keep] = 0.0
    return a[1:], b


# ---- the host grid --------------------------------------------------------------------------------------------------------------------
HOST_STATES, HOST_COLS = (1, 2, 8, 65), (1, 2, 4)
HOST_COLTOK = {1: (2,), 2: (3, 3), 4: (1, 2, 3, 1)}      # (every map of more than one column repeats a token)


def host_cases():
    """[(em, colTok, A, B)]: pair_machine(S, seed, levels, 2, 3) for S in 1, 2, 8, 65, with silent levels (S >= 2) and without, one,
    two and four columns, the seven shapes; a tenth of the weights of either profile -inf."""
    out = []
    for S in HOST_STATES:
        for levels in ((True, False) if S >= 2 else (False,)):
            em = pair_machine(S, 300 + S, levels, 2, 3)
            for nCols in HOST_COLS:
                for K, L in SHAPES:
                    out.append((em, HOST_COLTOK[nCols]) + merged_input(np.random.RandomState(70000 + 1000 * S + 100 * nCols + 10 * K + L), em, nCols, K, L, pInf=0.1))
    return out


# ---- the input families of the GPU module ----------------------------------------------------------------------------------------------
WAVE_COLTOK = (1, 2, 3, 1)


def lane_case(nCols, S):
    """twomergehelpers.lane_case: (colTok, [(em, A, B)]), the machine with silent levels (S >= 2) and without, each at the seven shapes."""
    return tm.lane_case(nCols, S)


def wave_case():
    """nCols = 4, S = 64 at (2, 5) and (5, 2), with levels: every wavefront holds exactly one (cell, plane)."""
    em = pair_machine(64, 264, True, 2, 3)
    return em, WAVE_COLTOK, [merged_input(np.random.RandomState(640 + K), em, 4, K, L, pInf=0.05) for K, L in ((2, 5), (5, 2))]


LONG = 1100
LONG_SHAPES = ((1, LONG), (LONG, 1))


def long_tables(K, L):
    """MB_ROWPOST_TABLE of the many-blocks test: one line a block on the long axis (5 doubles on axis 0, nIn + 1 = 3 on axis 1), a
    table no line fits (global bins), the default."""
    return ("3" if K > L else "5", "2", None)


def long_case(K, L):
    """(em, colTok, [live, dead]): nCols = 4, S = 2 at (1, 1 100) or (1 100, 1), and a dead pair of the same shape (one row of the long
    tape all -inf).  With one line a block the long axis has 1 100 blocks against the 1 024 groups a pair gets."""
    em = pair_machine(2, 1102, True, 2, 3)
    live = merged_input(np.random.RandomState(1100 + K), em, 4, K, L, pInf=0.0)
    dead = [t.copy() for t in merged_input(np.random.RandomState(1200 + K), em, 4, K, L, pInf=0.0)]
    (dead[0] if K > L else dead[1])[LONG // 2] = -np.inf
    return em, WAVE_COLTOK, [live, tuple(dead)]


WIDE_AXES = ("columns", "inputs")
WIDE_SHAPES = ((4, 5), (0, 5), (5, 0), (7, 3))


def wide_case(which):
    """(em, colTok, pairs) at S = 2: 66 bins a line on axis 0 (nCols = 65 on three tokens) or 71 bins a line on axis 1 (nIn = 70),
    more than a wavefront has lanes; four pairs."""
    if which == "columns":
        em = pair_machine(2, 270, False, 2, 3)
        colTok = tuple(np.random.RandomState(65).randint(1, 4, 65))
    else:
        em = pair_machine(2, 271, False, 70, 3)
        colTok = WAVE_COLTOK
    return em, colTok, [merged_input(np.random.RandomState(270 + 10 * K + L), em, len(colTok), K, L, pInf=0.0) for K, L in WIDE_SHAPES]


RAGGED_EXTRA = ((0, 0), (0, 5), (5, 0))


def ragged_case():
    """(em, colTok, pairs): (0, 0), (0, 5), (5, 0), then twomergehelpers.ring_pairs() -- nCols = 2, S = 20, short sides 9 / 10 and
    25 / 26 found by i and by r, (2, 3), (0, 40), (40, 0) and a dead pair last."""
    em, pairs = tm.ring_pairs()
    extra = [merged_input(np.random.RandomState(3500 + 10 * K + L), em, tm.RING_COLS, K, L, pInf=0.0) for K, L in RAGGED_EXTRA]
    return em, tm.RING_COLTOK, extra + pairs


def ragged_budget(em, pairs):
    """About 1.8 times the bytes of the largest pair: no two of the largest share a chunk."""
    return int(1.8 * max(pair_bytes(em.nStates, tm.RING_COLS, len(A), len(B), em.nInTok) for A, B in pairs)) - 1


SCRATCH_S = 65
SCRATCH_SHAPES = ((13, 14), (2, 3), (14, 13))


def scratch_case():
    """(em, colTok, pairs): nCols = 4, S = 65.  The X / T ring of the materialised sweeps takes 48 nCols (min(K, L) + 1) S bytes:
    174 720 at a short side of 13, past the 160 KiB of LDS, so the two large pairs keep theirs in the scratch buffer and (2, 3),
    between them, in LDS."""
    em = pair_machine(SCRATCH_S, 265, True, 2, 3)
    return em, WAVE_COLTOK, [merged_input(np.random.RandomState(6500 + 10 * K + L), em, 4, K, L, pInf=0.0) for K, L in SCRATCH_SHAPES]


FAR_SHIFT = -700.0


def dead_weight_cases():
    """[(name, em, colTok, pairs)]: a third of the weights of either table -inf (blanks included), twelve pairs at (5, 6) on S = 20;
    twomergehelpers.degenerate_cases (all-blank rows on either tape, a whole -inf row on either tape, an eighth of the weights
    -inf); one (9, 9) pair on S = 8 beside itself with both profiles 700 lower."""
    em = pair_machine(20, 50, True, 2, 3)
    rng = np.random.RandomState(23)          # (about one such pair in four has a row without a finite weight; here eleven of twelve live)
    third = [merged_input(rng, em, 4, 5, 6, pInf=1.0 / 3.0) for _ in range(12)]
    emD, colTokD, deg = tm.degenerate_cases()
    emF = pair_machine(8, 9, True, 2, 3)
    A, B = merged_input(np.random.RandomState(99), emF, 4, 9, 9, pInf=0.05)
    return [("third", em, WAVE_COLTOK, third), ("degenerate", emD, colTokD, deg), ("far", emF, WAVE_COLTOK, [(A, B), (A + FAR_SHIFT, B + FAR_SHIFT)])]


def column_map_cases():
    """(em, [(colTok, A, B)]) of twomergehelpers: one column, all columns on one token, a token nothing emits, a doubled symbol."""
    return tm.column_map_cases()


def fd_case():
    """(em, colTok, A, B): S = 8 with levels at (3, 3), three columns with two on one token, every weight finite."""
    em = pair_machine(8, 108, True, 2, 3)
    return (em, (1, 2, 1)) + merged_input(np.random.RandomState(3), em, 3, 3, 3, pInf=0.0)


def one_hot_case():
    """(em, colTok, xs, Bs): four token strings and merged rows on S = 65 with levels, nIn = 3."""
    em = pair_machine(65, 165, True, 3, 2)
    rng = np.random.RandomState(165)
    xs = [rng.randint(1, 4, size=K).astype(np.int32) for K in (5, 0, 7, 1)]
    return em, (2, 1, 2), xs, [tm.merged_rows(rng, 3, L, zeros=0.0) for L in (9, 4, 2, 1)]


def gpu_families():
    """{name: [(em, colTok, A, B)]}: every input family of the GPU module."""
    fam = {}
    for nCols, S in tm.LANE_CASES:
        colTok, cases = lane_case(nCols, S)
        fam["lanes %d x %d" % (nCols, S)] = [(em, colTok, A, B) for em, A, B in cases]
    for name, (em, colTok, pairs) in (("wave", wave_case()), ("ragged", ragged_case()), ("scratch", scratch_case()),
                                      ("wide columns", wide_case("columns")), ("wide inputs", wide_case("inputs")),
                                      ("long 0", long_case(*LONG_SHAPES[0])), ("long 1", long_case(*LONG_SHAPES[1]))):
        fam[name] = [(em, colTok, A, B) for A, B in pairs]
    fam["dead weights"] = [(em, colTok, A, B) for _, em, colTok, pairs in dead_weight_cases() for A, B in pairs]
    em, cases = column_map_cases()
    fam["column maps"] = [(em, colTok, A, B) for colTok, A, B in cases]
    fam["finite differences"] = [fd_case()]
    return fam


# ---- the device against the yardstick (the GPU module; the device is touched only when these are called) -----------------------------
WORST = {}


def yardstick(em, colTok, pairs):
    from machineboss_amd.profile import TwoMergedProfileDP
    dp = TwoMergedProfileDP(em, colTok)
    return [dp.mergedRowPosteriors(A, B) for A, B in pairs]


@functools.lru_cache(maxsize=None)
def ragged_refs():
    """(em, colTok, pairs, refs) of the ragged batch, computed once for the tests that share it."""
    em, colTok, pairs = ragged_case()
    return em, colTok, pairs, yardstick(em, colTok, pairs)


@functools.lru_cache(maxsize=None)
def long_refs(K, L):
    em, colTok, pairs = long_case(K, L)
    return em, colTok, pairs, yardstick(em, colTok, pairs)


def split(dev, postA, postB):
    return ([postA[dev.inOff[k]:dev.inOff[k + 1]] for k in range(dev.nPairs)], [postB[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)])


def compare(em, colTok, gotA, gotB, ll, refs, what="posteriors", fixed=False):
    """The device's per-pair tables and likelihoods against the yardstick's: entries, exact zeros, row sums.  ``fixed``: the device
    ran in fixed point -- every bound then has the rounding of the lane sums that feed the bin added, and a row sum that of its
    bins."""
    want = np.array([r[2] for r in refs])
    note("loglike", ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    PS = (len(colTok) + 1) * em.nStates
    for k, (wa, wb, wl) in enumerate(refs):
        for g, w, items in ((gotA[k], wa, (len(wb) + 1) * PS), (gotB[k], wb, (len(wa) + 1) * PS)):
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


def open_pairs(em, colTok, pairs):
    from machineboss_amd import capi
    dm = capi.DeviceMachine(em)
    return dm, capi.DeviceProfileTwos(dm, [A for A, _ in pairs], [B for _, B in pairs], colTok=colTok)


def check(em, colTok, pairs, launches=None, refs=None, what="posteriors", fixed=False):
    """merged_row_posteriors() of the pairs of one machine, in one batch, against the yardstick: (gotA, gotB, ll, refs)."""
    from machineboss_amd import capi
    refs = yardstick(em, colTok, pairs) if refs is None else refs
    dm, dev = open_pairs(em, colTok, pairs)
    try:
        postA, postB, ll = dev.merged_row_posteriors()
        assert capi.last_kernel_name() == "k_profile_two_merge_rowpost"
        if launches is not None:
            assert capi.last_launch_count() == launches
        assert postA.shape == (dev.inOff[-1], em.nInTok + 1) and postB.shape == (dev.rowOff[-1], len(colTok) + 1)
        gotA, gotB = split(dev, postA, postB)
        compare(em, colTok, gotA, gotB, ll, refs, what, fixed)
    finally:
        dev.close(); dm.close()
    return gotA, gotB, ll, refs
