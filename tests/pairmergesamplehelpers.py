"""Cases, seeds, the exact enumeration and the bounds of the tests of the posterior path samples of pairs against CTC-merged profiles
(test_profile_pair_merge_sample_host.py, test_profile_pair_merge_sample_gpu.py; not a test module).  The reference is
profile.PairMergedProfileDP.samplePaths, called per pair with the pair's own index; the machines and inputs are those of
pairmergehelpers and pairmergeenvhelpers, the bounds those of pairsamplehelpers.

Equality of sampled paths between the device and the yardstick needs every uniform to lie clear of every partial sum of its
decision: MARGIN, held for every case below by test_profile_pair_merge_sample_host.py::test_gpu_suite_inputs_are_live.  A case whose
seed fails that takes the next seed here, before any GPU run."""
import math

import numpy as np

import pairenvhelpers as eh
import pairmergeenvhelpers as meh
import pairmergehelpers as mh
import pairsamplehelpers as sh
from pairprofilehelpers import pair_machine
from machineboss_amd.profile import PairMergedProfileDP
from machineboss_amd.seqpair import Envelope

LOG_TOL = sh.LOG_TOL        # logq and likelihoods: relative to max(1, |value|), -inf matching exactly
MARGIN = sh.MARGIN          # the least distance of a uniform from a partial sum the GPU suite's inputs may have

BASIC_STATES = (1, 2, 8, 65)
BASIC_COLS = (1, 2, 4)
BASIC_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 3), (5, 4))
BASIC_SAMPLES = sh.BASIC_SAMPLES      # 1, 3, 64, 65, 130: either side of a block of 64 lanes
ENV_SAMPLES = 5
MIXED_SAMPLES = 3
RAGGED_SAMPLES = 7
LONG_LEN, LONG_BAND, LONG_SAMPLES, LONG_CHECKED = 60, 6, 256, 8
STAT_SAMPLES, STAT_SEED = 4096, 4096
HOT_SAMPLES = 4
SEED_B = 991                # a second seed for the mixed batch: at least one path differs


# ---- the cases of the GPU module: builders of [(em, colTok, [(x, P, env)])] ----------------------------------------------------------------
def _basic(S):
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 200 + S, levels, 2, 3)
        for nCols in BASIC_COLS:
            rng = np.random.RandomState(1000 * nCols + S)
            colTok = rng.randint(1, 4, nCols)
            out.append((em, colTok, [mh.merged_input(rng, em, nCols, I, L, zeros=0.1) + (None,) for I, L in BASIC_SHAPES]))
    return out


def _maps():
    """Two columns on one token, every column on one token, a column whose token nothing emits, one column (column_map_cases); and a
    generator (no input alphabet) against merged profiles, I = 0."""
    from randmachine import random_machine
    out = [(em, colTok, [(x, P, None) for x, P in pairs]) for em, colTok, pairs in mh.column_map_cases().values()]
    gen = random_machine(8, 0, 3, 31)
    out.append((gen, (1, 2, 3, 1), [(np.zeros(0, np.int32), mh.merged_input(np.random.RandomState(31 + L), gen, 4, 0, L)[1], None) for L in (0, 1, 6)]))
    return out


def _ragged():
    """ragged_case and one more pair: ten, the dead one ninth."""
    em, colTok, pairs = mh.ragged_case()
    pairs = pairs + [mh.merged_input(np.random.RandomState(4777), em, 4, 5, 7, zeros=0.1)]
    return [(em, colTok, [(x, P, None) for x, P in pairs])]


def _envelopes():
    """cell_case(2, 8): every shape under every envelope of pairenvhelpers.envelopes, one batch per machine."""
    return [(em, colTok, [(x, P, env) for x, P, _kind, env in quads]) for em, colTok, quads in meh.cell_case(2, 8)]


def env_kinds():
    """Per machine of the "envelopes" case, the kind of each pair's envelope."""
    return [[kind for _x, _P, kind, _env in quads] for _em, _colTok, quads in meh.cell_case(2, 8)]


def _mixed():
    return [meh.mixed_case(8)]


HOT_COLTOK = (1, 2)


def _hot():
    """sh.hot_machine (one path per input) against one-hot merged frames: x over {1, 2, 3}; its symbols other than 3 in order, each
    held for one to three frames, a blank frame between two equal symbols and now and then elsewhere.  Every frame has one finite
    entry, so the pair has one lattice path and rowCol is the frames' argmax."""
    em = sh.hot_machine()
    rng = np.random.RandomState(78)
    triples = []
    for I in (12, 5, 3, 0):
        x = rng.randint(1, 4, size=I).astype(np.int32) if I != 3 else np.full(3, 3, np.int32)
        labels, prev = [], 0
        for y in x[x != 3]:
            if prev == y or rng.rand() < 0.3:
                labels.append(0)
            labels += [int(y)] * rng.randint(1, 4)
            prev = int(y)
        labels += [0] * rng.randint(0, 2)
        P = np.full((len(labels), 3), -np.inf)
        P[np.arange(len(labels)), labels] = 0.0
        triples.append((x, P, None))
    return [(em, HOT_COLTOK, triples)]


def hot_labels():
    return [np.argmax(P, axis=1).astype(np.int32) if len(P) else np.zeros(0, np.int32) for _x, P, _e in _hot()[0][2]]


def _long():
    em = mh.ring_machine()
    x, P = mh.merged_input(np.random.RandomState(6006), em, 4, LONG_LEN, LONG_LEN, zeros=0.05)
    return [(em, mh.RING_COLTOK, [(x, P, Envelope.band(LONG_LEN, LONG_LEN, LONG_BAND))])]


def _stat():
    em = pair_machine(3, 103, True, 2, 3)
    x, P = mh.merged_input(np.random.RandomState(3303), em, 2, 3, 3, zeros=0.0)
    return [(em, (1, 2), [(x, P, None)])]


# name: (samples the yardstick draws, seed, dead pairs expected, builder)
CASES = {
    "basic1": (130, 11, False, lambda: _basic(1)),
    "basic2": (130, 12, True, lambda: _basic(2)),
    "basic8": (130, 18, True, lambda: _basic(8)),
    "basic65": (130, 165, True, lambda: _basic(65)),
    "maps": (5, 41, False, _maps),
    "ragged": (RAGGED_SAMPLES, 7, True, _ragged),
    "envelopes": (ENV_SAMPLES, 5, True, _envelopes),
    "mixed": (MIXED_SAMPLES, 3, True, _mixed),
    "hot": (HOT_SAMPLES, 4, False, _hot),
    "long": (LONG_CHECKED, 120, False, _long),
}
# the share of finite likelihoods a case claims, at least: nine in ten, but for the envelope case -- under a staircase or a band of width
# 0 consecutive rows are matches, each of which needs a column other than the one before, and two columns on random tokens often
# have none
LIVE_SHARE = {"envelopes": 0.8}

BOSS_SAMPLES, BOSS_SEED, BOSS_BANDS = 6, 21, (None, 2)


def boss_case():
    """(machine, profile, inputs) of the boss.sampleMergedPairs tests: sh.boss_case's machine against five merged frames over x and
    y; the third input cannot be tokenised, the last is empty."""
    from machineboss_amd.profile import Profile
    m, _prof, inputs = sh.boss_case()
    prof = Profile(["x", "y"], [[0.5, 0.25, 0.25], [0.1, 0.6, 0.3], [0.3, 0.3, 0.4], [0.2, 0.5, 0.3], [0.6, 0.2, 0.2]])
    return m, prof, inputs


_BUILT, _REFS = {}, {}


def case(name):
    """(nSamples, seed, [(em, colTok, triples)]) of a case, built once."""
    if name not in _BUILT:
        n, seed, _dead, build = CASES[name]
        _BUILT[name] = (n, seed, build())
    return _BUILT[name]


def reference(name, margins=None):
    """[[(loglike, [(edges, rows, rowCol, logq)] * nSamples) per pair] per machine]: the yardstick's samples of a case, pair k of a
    batch under its own index k.  Computed once and shared; never changed."""
    if name not in _REFS:
        n, seed, groups = case(name)
        mg = []
        _REFS[name] = ([[PairMergedProfileDP(em, colTok).samplePaths(x, P, n, seed=seed, pair=k, env=env, margins=mg)
                         for k, (x, P, env) in enumerate(triples)] for em, colTok, triples in groups], mg)
    if margins is not None:
        margins += _REFS[name][1]
    return _REFS[name][0]


def log_close(got, want, tol=LOG_TOL):
    return sh.log_close(got, want, tol)


# ---- the exact enumeration ----------------------------------------------------------------------------------------------------------------
TooMany = sh.TooMany


def enumerate_lattice_paths(dp, x, P, env=None, budget=60000):
    """Every lattice path of (x, P) from N[0][0][0][0] forward to W[I][L][.][S-1], by a recursion written from the recurrence of
    docs/profile_tapes.md, "Pairs against a merged profile" -- over (i, r, plane, state, layer), without a lattice and without
    sampleCandidates: from N the walk stays (to W), takes row r as a blank (into plane 0, from any plane) or, on plane c >= 1, as a
    repeat; from W it takes an input-only edge of x_{i+1}, a silent edge s < d, or an edge writing colTok[c] into N of plane c != its
    own, with or without x_{i+1}.  Under ``env`` a step into a cell outside is not taken.  Returns [(edges, rows, rowCol, steps)]:
    steps lists the moves as (kind, edge or -1, plane left), the kinds of sampleCandidates, "end" last."""
    em = dp.em
    x, P = dp._checkPair(x, P)
    I, L, S = len(x), len(P), dp.S
    inside = None if env is None else eh.mask(env, I)
    ok = (lambda i, r: True) if inside is None else (lambda i, r: bool(inside[i, r]))
    fin = em.logWeight > -math.inf
    outE = [[int(e) for e in np.nonzero((em.src == s) & fin)[0]] for s in range(S)]
    cols = {}
    for c, t in enumerate(dp.colTok):
        cols.setdefault(int(t), []).append(c + 1)
    out, seen = [], [0]

    def walk(i, r, p, q, layer, edges, rows, rowCol, steps):
        seen[0] += 1
        if seen[0] > budget:
            raise TooMany()
        if layer == 0:
            walk(i, r, p, q, 1, edges, rows, rowCol, steps + [("stay", -1, p)])
            if r < L and ok(i, r + 1):
                if P[r][0] > -math.inf:
                    walk(i, r + 1, 0, q, 0, edges, rows, rowCol + [0], steps + [("blank", -1, p)])
                if p and P[r][p] > -math.inf:
                    walk(i, r + 1, p, q, 0, edges, rows, rowCol + [p], steps + [("repeat", -1, p)])
            return
        if i == I and r == L and q == S - 1:
            out.append((tuple(edges), tuple(rows), tuple(rowCol), steps + [("end", -1, p)]))
        for e in outE[q]:
            it, ot, d = int(em.inTok[e]), int(em.outTok[e]), int(em.dst[e])
            if it and (i >= I or int(x[i]) != it):
                continue
            ni = i + (1 if it else 0)
            if not ot:
                if it:
                    if ok(ni, r):
                        walk(ni, r, p, d, 1, edges + [e], rows + [r], rowCol, steps + [("ins", e, p)])
                elif q < d:
                    walk(i, r, p, d, 1, edges + [e], rows + [r], rowCol, steps + [("silent", e, p)])
            elif r < L and ok(ni, r + 1):
                for c in cols.get(ot, ()):
                    if c != p and P[r][c] > -math.inf:
                        walk(ni, r + 1, c, d, 0, edges + [e], rows + [r], rowCol + [c], steps + [("match" if it else "emit", e, p)])
    if ok(0, 0):
        walk(0, 0, 0, 0, 0, [], [], [], [])
    return out


def choice_product(dp, x, P, ll, N, W, inside, steps):
    """The product of the yardstick's choice probabilities along a lattice path given by its forward ``steps``: walked backwards,
    every decision's candidates from sampleCandidates(), the one that matches the step taken, p = exp(term - cell)."""
    i, r, p, q, layer, prob = len(x), len(P), 0, dp.S - 1, 2, 1.0
    em = dp.em
    for kind, e, k in reversed(steps):
        cur = ll if layer == 2 else float(W[i, r, p, q] if layer == 1 else N[i, r, p, q])
        cand = [c for c in dp.sampleCandidates(x, P, N, W, inside, i, r, p, q, layer) if c[0] == kind and c[1] == e and c[3] == k]
        assert len(cand) == 1, (kind, e, k, i, r, p, q, layer)
        _, _, s, _, term = cand[0]
        prob *= math.exp(term - cur)
        if kind == "end":
            p, layer = k, 1
        elif kind == "stay":
            layer = 0
        elif kind in ("ins", "silent"):
            q = s
            i -= kind == "ins"
        else:
            r -= 1
            if kind in ("match", "emit"):
                q, layer = s, 1
                i -= kind == "match"
            p = k
    assert (i, r, p, q, layer) == (0, 0, 0, 0, 0) and em is dp.em
    return prob


def blank_rows(steps):
    """The rows a lattice path took as blanks, from its forward steps."""
    rows, r = [], 0
    for kind, _e, _k in steps:
        if kind == "blank":
            rows.append(r)
        if kind in ("blank", "repeat", "match", "emit"):
            r += 1
    return rows


def key_of(edges, rows, rowCol):
    return tuple(int(e) for e in edges), tuple(int(r) for r in rows), tuple(int(c) for c in rowCol)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def row_col_within_bound(rowCols, post):
    """The mean of rowCol == c per row within 5 standard errors (from the sample variance) of post[r][c], for every entry whose
    posterior is at least 1e-3.  Returns the list of violations."""
    rc = np.asarray(rowCols)
    n, bad = len(rc), []
    for r in range(rc.shape[1]):
        for c in range(post.shape[1]):
            hit = (rc[:, r] == c).astype(np.float64)
            if post[r][c] >= 1e-3 and not abs(hit.mean() - post[r][c]) <= 5.0 * hit.std(ddof=1) / math.sqrt(n):
                bad.append((r, c, float(hit.mean()), float(post[r][c])))
    return bad


def sample_call_bytes(em, nCols, triples, nSamples):
    """What mb_profile_pairs_sample_merged tells the chunk planner a pair costs: its lattice, the ring of its fill where that lies in
    global memory, and per sample a path slot of edges and rows, a length, a log probability and a column per row."""
    nLev = eh.silent_levels(em)
    return [b + nSamples * (8 * eh.path_bound(nLev, len(x), len(P)) + 16 + 4 * len(P))
            for b, (x, P, _env) in zip(meh.call_bytes("forward", em, nCols, triples), triples)]
