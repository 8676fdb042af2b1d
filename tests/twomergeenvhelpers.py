"""Envelopes, inputs and the device-against-restatement comparison of the tests of the two-profile sweeps against CTC-merged
output profiles under an envelope (test_profile_two_merge_env_host.py, test_profile_two_merge_env_gpu.py; not a test module).  The
machines and inputs are those of twomergehelpers / twomergeposthelpers, the envelopes those of pairenvhelpers and twoenvhelpers with
K input rows for I input tokens; the reference is profile.TwoMergedProfileDP(env=...) called per pair, which
test_profile_two_merge_env_host.py first holds to an enumeration of paths, to the sibling families and to its own identities.  Every
builder is deterministic, and test_profile_two_merge_env_host.py::test_gpu_inputs_are_live holds the conditions the GPU tests assume
-- ring bytes either side of the marks, M, liveness, tie kinds, chunk counts -- to the yardstick and to plain arithmetic, without a GPU.

Bounds (the family's): log values 1e-9 relative to max(1, |value|), -inf exact; counts and posteriors >= 1e-3 at 1e-6 relative,
smaller ones at 1e-9 + 1e-6 x value; row sums 1e-6; Viterbi scores 1e-12 with equal paths, rows and input rows; fixed-point counts
under twoprofilehelpers.fixed_counts_close."""
import functools
import math

import numpy as np

import twoenvhelpers as te
import twomergehelpers as tm
import twomergeposthelpers as tq
from pairenvhelpers import diag_max, envelopes, full, mask, n_cells, staircase  # noqa: F401
from pairprofilehelpers import LOG_TOL, counts_close, logs_close, note, note_counts, pair_machine
from twoenvhelpers import band_or_full, column_stairs
from twomergehelpers import merged_input
from machineboss_amd.machine import MachineError
from machineboss_amd.seqpair import Envelope

LDS_MAX = 160 * 1024
LDS_DEFAULT = 64 * 1024
ENV_KINDS = ("full", "band0", "band1", "path", "stairs")


# ---- every path, one by one -------------------------------------------------------------------------------------------------------
def enumerate_paths(em, colTok, A, B, env=None):
    """(log of the summed weight of every path, the best path's weight, the number of paths with a finite weight): the stages of
    "Pairs of profiles against a merged profile" walked depth first over (i, r, plane, state, stage) from the arrived stage of
    (0, 0, plane 0, state 0) to the committed stage of (K, L, any plane, S - 1), one path at a time, a move taken only if the cell it
    leads to is inside the envelope.  Nothing is shared between paths and nothing is summed before a path is complete."""
    K, L, S, nC = len(A), len(B), em.nStates, len(colTok)
    inside = np.ones((K + 1, L + 1), bool) if env is None else mask(env, K)
    out = [[] for _ in range(S)]
    for e in range(em.nTransitions):
        out[int(em.src[e])].append((int(em.dst[e]), int(em.inTok[e]), int(em.outTok[e]), float(em.logWeight[e])))
    cols = {}
    for c in range(1, nC + 1):
        cols.setdefault(int(colTok[c - 1]), []).append(c)
    weights = []

    def walk(stage, i, r, p, q, w):
        if w == -math.inf:
            return
        if stage == 0:      # arrived: the output blank, the repeat, or settle
            if r < L and inside[i, r + 1]:
                walk(0, i, r + 1, 0, q, w + B[r][0])
                if p:
                    walk(0, i, r + 1, p, q, w + B[r][p])
            walk(1, i, r, p, q, w)
        elif stage == 1:    # waiting: output-only edges into a column other than the last, silent edges, or commit
            for d, a, o, lw in out[q]:
                if a:
                    continue
                if o:
                    if r < L and inside[i, r + 1]:
                        for c in cols.get(o, ()):
                            if c != p:
                                walk(0, i, r + 1, c, d, w + lw + B[r][c])
                elif d > q:
                    walk(1, i, r, p, d, w + lw)
            walk(2, i, r, p, q, w)
        else:               # committed: the end, the input blank, input-reading edges
            if i == K and r == L and q == S - 1:
                weights.append(w)
            if i < K:
                if inside[i + 1, r]:
                    walk(2, i + 1, r, p, q, w + A[i][0])
                for d, a, o, lw in out[q]:
                    if not a:
                        continue
                    if o:
                        if r < L and inside[i + 1, r + 1]:
                            for c in cols.get(o, ()):
                                if c != p:
                                    walk(0, i + 1, r + 1, c, d, w + lw + A[i][a] + B[r][c])
                    elif inside[i + 1, r]:
                        walk(1, i + 1, r, p, d, w + lw + A[i][a])

    if inside[0, 0]:
        walk(0, 0, 0, 0, 0, 0.0)
    if not weights:
        return -math.inf, -math.inf, 0
    w = np.array(weights)
    return float(w.max() + np.log(np.exp(w - w.max()).sum())), float(w.max()), len(w)


ENUM_STATES = (2, 3)
ENUM_SEED = {2: 41, 3: 51}
ENUM_COLTOK = ((1,), (2, 1), (1, 1))
ENUM_SHAPES = te.ENUM_SHAPES                       # nine lattices from (0, 0) to (3, 3)
ENUM_CAP = {True: 9, False: 10}                    # envelope cells enumerated at the most, with silent levels and without


def enum_cases():
    """(key, em, colTok, A, B, kind, env): pair_machine(S, seed, levels, 2, 3) for S in {2, 3}, the three column maps, lattices up
    to (3, 3) under twoenvhelpers.enum_envelopes (full, band(0), band(1), the staircase); every weight finite."""
    for S in ENUM_STATES:
        for levels in (True, False):
            em = pair_machine(S, ENUM_SEED[S], levels, 2, 3)
            for colTok in ENUM_COLTOK:
                for K, L in ENUM_SHAPES:
                    A, B = merged_input(np.random.RandomState(1000 * S + 100 * len(colTok) + 10 * K + L), em, len(colTok), K, L, pInf=0.0)
                    for kind, env in te.enum_envelopes(K, L):
                        yield (S, levels, colTok, K, L, kind), em, colTok, A, B, kind, env


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def env_reference(dp, A, B, env, cells=True, paths=True, counts=True, post=True):
    """Everything the yardstick says about one pair under env (None: no envelope)."""
    kw = {} if env is None else {"env": env}
    out = {}
    ll, N, W, Z = dp.forward(A, B, **kw)
    v, VN, VW, VZ = dp.forward(A, B, "max", **kw)
    out.update(ll=ll, v=v)
    if cells:
        _, NB, WB, ZB = dp.backward(A, B, **kw)
        out.update(fwd=np.stack([N, W, Z], axis=2), bwd=np.stack([NB, WB, ZB], axis=2), vit=np.stack([VN, VW, VZ], axis=2))
    if paths:
        out["path"] = dp.viterbi(A, B, **kw)[1:]
    if counts:
        out["counts"] = dp.counts(A, B, **kw)[0]
    if post:
        out["post"] = dp.mergedRowPosteriors(A, B, **kw)
    return out


def ring_bytes(S, nCols, M, mat=False):
    """The ring of a pair under an envelope (mb_profile_two_merge.h): three diagonals of M cells, each N, W, Z (nCols + 1 planes) and
    XW, XZ (nCols planes) rolling; XW, XZ alone materialised, and the Backward's TZ, TW in a ring of that shape."""
    return 8 * 3 * (2 * nCols if mat else 5 * nCols + 3) * M * S


def lattice_doubles(S, nCols, A, B, env):
    """pt_cells: three layers of nCols + 1 planes of the rectangle, or of the compact lattice of the envelope."""
    return 3 * S * (nCols + 1) * (n_cells(env) if env is not None else (len(A) + 1) * (len(B) + 1))


# ---- the lane cases ----------------------------------------------------------------------------------------------------------------
LANE_CASES = ((1, 1), (2, 1), (4, 13), (4, 65), (65, 2))          # (nCols, S)
LANE_SHAPES = tm.LANE_SHAPES                                       # seven lattices from (0, 0) to (9, 9)
LANE_SEED = {1: 301, 2: 302, 13: 313, 65: 365}


@functools.lru_cache(maxsize=None)
def lane_case(nCols, S):
    """[(em, colTok, [(A, B, kind, env)])]: the machine with silent levels (S >= 2) and without, at every shape under every envelope
    of pairenvhelpers.envelopes; a fiftieth of the weights -inf."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, LANE_SEED[S], levels, 2, 3)
        rng = np.random.RandomState(1000 * nCols + S)
        colTok = tuple(int(t) for t in rng.randint(1, 4, nCols))
        quads = []
        for K, L in LANE_SHAPES:
            A, B = merged_input(rng, em, nCols, K, L, pInf=0.02)
            quads += [(A, B, kind, env) for kind, env in envelopes(rng, K, L)]
        out.append((em, colTok, quads))
    return out


# ---- the ring marks: nCols = 4, S = 80, K = L = 40 --------------------------------------------------------------------------------------
MARK_S, MARK_LEN, MARK_COLTOK = 80, 40, (1, 2, 3, 1)
MARK_ROLLING = (1, 2, 3, 4)          # M: 24 * 23 * 80 = 44 160 M bytes = 44 160 | 88 320 either side of 64 KiB, 132 480 | 176 640 either side of 160 KiB
MARK_MAT = (4, 5, 10, 11)            # M: 24 * 8 * 80 = 15 360 M bytes = 61 440 | 76 800 and 153 600 | 168 960 (the X ring, and the Backward's T ring)
MARK_M = (1, 2, 3, 4, 5, 10, 11)


def mark_machine():
    return pair_machine(MARK_S, 880, True, 2, 3)


@functools.lru_cache(maxsize=None)
def mark_case(M):
    """(A, B, env): a band of half-width M - 1 on a square lattice has at most M cells on a diagonal.  No weight is -inf: under
    band(0) there is one alignment only."""
    A, B = merged_input(np.random.RandomState(8800 + M), mark_machine(), 4, MARK_LEN, MARK_LEN, pInf=0.0)
    return A, B, Envelope.band(MARK_LEN, MARK_LEN, M - 1)


def mark_extras():
    """A pair without an envelope, a (0, 0) pair and a dead pair (a row of B all -inf) under a band, to put beside a mark."""
    em = mark_machine()
    A0, B0 = merged_input(np.random.RandomState(8890), em, 4, 6, 5, pInf=0.0)
    Az, Bz = merged_input(np.random.RandomState(8891), em, 4, 0, 0, pInf=0.0)
    A1, B1 = merged_input(np.random.RandomState(8892), em, 4, 8, 8, pInf=0.0)
    B1 = B1.copy(); B1[4] = -np.inf
    return (A0, B0, None), (Az, Bz, None), (A1, B1, Envelope.band(8, 8, 3))


# ---- scratch rings in one launch -------------------------------------------------------------------------------------------------------
PACKED_COLTOK = tm.PACKED_COLTOK


def packed_case():
    """(em, triples): twomergehelpers.packed_case -- twenty-four pairs at S = 140, nCols = 2 -- every other pair under its full
    envelope, the rest given none (the host makes theirs).  A rolling ring takes 24 * 13 * 140 M = 43 680 M bytes: at M = 4, the
    diagonal of (3, 3), (3, 4) and (4, 3), 174 720, past 160 KiB and so in scratch; (2, 3) has M = 3 and its ring in LDS."""
    em, pairs = tm.packed_case()
    return em, [(A, B, full(len(A), len(B)) if k % 2 == 0 else None) for k, (A, B) in enumerate(pairs)]


# ---- the ragged batch: the full envelope against none ------------------------------------------------------------------------------------
def ragged_case():
    """(em, colTok, pairs): twomergeposthelpers.ragged_case without its four largest pairs -- (0, 0), (0, 5), (5, 0), short sides 9 / 10
    found by i and by r, (2, 3), (0, 40), (40, 0) and a dead pair last."""
    em, colTok, pairs = tq.ragged_case()
    keep = [k for k, (A, B) in enumerate(pairs) if min(len(A), len(B)) < 25]
    return em, colTok, [pairs[k] for k in keep]


# ---- counts past the LDS table ------------------------------------------------------------------------------------------------------------
def big_counts_env_case():
    """big_counts_case's machine (11 204 transitions), column map and pairs, the dead one last, each under band(2) (the full envelope
    where the slope defeats the band)."""
    em, pairs, dead = tm.big_counts_case()
    return em, tm.COUNT_COLTOK, [(A, B, band_or_full(len(A), len(B), 2)) for A, B in pairs + [dead]]


# ---- the axis-1 traversal -----------------------------------------------------------------------------------------------------------------
POST_STAIRS = (9, 12)
POST_STAIRS_COLTOK = (1, 2, 3, 1)


def post_stairs_case():
    """(em, colTok, A, B, env) at (9, 12) under twoenvhelpers.column_stairs (columns of many, two and one cell), S = 8."""
    em = pair_machine(8, 308, True, 2, 3)
    A, B = merged_input(np.random.RandomState(912), em, 4, *POST_STAIRS, pInf=0.0)
    return em, POST_STAIRS_COLTOK, A, B, column_stairs(*POST_STAIRS)


LONG_SHAPES = tq.LONG_SHAPES
LONG_TABLES = ("4", "2", None)


def long_case(K, L):
    """twomergeposthelpers.long_case -- S = 2, nCols = 4, a live and a dead pair -- each under the staircase of its shape."""
    em, colTok, pairs = tq.long_case(K, L)
    return em, colTok, [(A, B, staircase(K, L)) for A, B in pairs]


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------
CHUNK = (65, 60, 4, 3)            # S, K = L, w, pairs
CHUNK_COLTOK = (1, 2, 3)


def chunk_case():
    S, K, w, n = CHUNK
    em = pair_machine(S, 365, True, 2, 3)
    return em, CHUNK_COLTOK, [merged_input(np.random.RandomState(3650 + k), em, 3, K, K, pInf=0.0) for k in range(n)], Envelope.band(K, K, w)


def chunk_pair_bytes(call):
    """What lattice_chunks is told one pair of chunk_case costs: the compact lattice (twice for counts and posteriors), no ring bytes
    (the X / T ring of M = 9 cells fits LDS) and, for the posteriors, the pair's bins of both tables."""
    S, K, w, _ = CHUNK
    env = Envelope.band(K, K, w)
    assert ring_bytes(S, 3, diag_max(env), True) <= LDS_MAX
    cells = 8 * 3 * S * 4 * n_cells(env)
    return {"forward": cells, "counts": 2 * cells, "posteriors": 2 * cells + 8 * (K * 4 + K * 3)}[call]


def chunk_budget():
    """A third of one rectangle's lattice: it holds one pair's two compact lattices and not a second pair's, so three pairs make
    three chunks in counts() and merged_row_posteriors()."""
    S, K, _, _ = CHUNK
    return 8 * 3 * S * 4 * (K + 1) * (K + 1) // 3


# ---- ties, the traceback's blocks -------------------------------------------------------------------------------------------------------
TIE_OUTSIDE = ("repeat", "emit", "ins", "inblank")


def tie_env_pairs():
    """twomergehelpers.tie_pairs under band(w = 1); the shapes whose slope such a band cannot bridge are left out."""
    out = []
    for A, B in tm.tie_pairs():
        try:
            out.append((A, B, Envelope.band(len(A), len(B), 1)))
        except MachineError:
            pass
    return out


SEAM_COLTOK = tm.SEAM_COLTOK
SEAM_DEAD = tm.SEAM_DEAD


def seam_case():
    """(em, triples): twomergehelpers.seam_case -- 129 pairs, dead pairs at slots 63, 64 and 128 -- each under an envelope of its
    shape, the kinds of pairenvhelpers.envelopes in turn."""
    em, pairs = tm.seam_case()
    triples = []
    for k, (A, B) in enumerate(pairs):
        es = envelopes(np.random.RandomState(9400 + k), len(A), len(B))
        triples.append((A, B, es[k % len(es)][1]))
    return em, triples


# ---- reductions ---------------------------------------------------------------------------------------------------------------------------
def onehot_case():
    """(em, colTok, x, A, B, env): pair_machine(40) at (30, 30) under band(3), three columns with a doubled token; A is the one-hot
    profile of the token string x, its blank -inf."""
    em = pair_machine(40, 41, True, 2, 3)
    rng = np.random.RandomState(4141)
    x = rng.randint(1, em.nInTok + 1, size=30).astype(np.int32)
    B = tm.merged_rows(rng, 3, 30, zeros=0.0)
    return em, (1, 2, 1), x, tm.one_hot(x, em.nInTok), B, Envelope.band(30, 30, 3)


def no_input_case():
    """(em, colTok, [B]): K = 0 -- the one-tape merged sweep -- on S = 8 with levels."""
    em = pair_machine(8, 108, True, 2, 3)
    rng = np.random.RandomState(808)
    return em, (3, 1, 3), [tm.merged_rows(rng, 3, L, zeros=0.05) for L in (0, 1, 4, 9)]


# ---- the device against the restatement ---------------------------------------------------------------------------------------------
WORST = {}


def open_twos(em, colTok, triples, envs=None):
    from machineboss_amd import capi
    dm = capi.DeviceMachine(em)
    envs = [t[2] for t in triples] if envs is None else envs
    return dm, capi.DeviceProfileTwos(dm, [t[0] for t in triples], [t[1] for t in triples], colTok=colTok,
                                      mergedEnvs=envs if any(e is not None for e in envs) else None)


def check_paths(v, off, edges, rows, ins, refs, what="viterbi"):
    wv = np.array([r["v"] for r in refs])
    note(what, v, wv, WORST)
    assert logs_close(v, wv, 1e-12), (v, wv)
    assert len(off) == len(refs) + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows) == len(ins)
    for k, r in enumerate(refs):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(edges[sl], r["path"][0]) and np.array_equal(rows[sl], r["path"][1]) and np.array_equal(ins[sl], r["path"][2]), (k, edges[sl], r["path"][0])


def check_env_batch(em, colTok, triples, fill=False, live=None, refs=None):
    """Everything the device computes for the (A, B, env) of one machine and one column map, in one batch, against the restatement
    under env: rolling and materialised Forward (the same bits from both), Viterbi with and without paths, counts, both posterior
    tables, and with ``fill`` every pair's three lattices, -inf outside in all layers and planes."""
    from machineboss_amd import capi
    from machineboss_amd.profile import TwoMergedProfileDP
    dp = TwoMergedProfileDP(em, colTok)
    refs = [env_reference(dp, A, B, env, cells=fill) for A, B, env in triples] if refs is None else refs
    dm, dev = open_twos(em, colTok, triples)
    tag = "_env" if any(t[2] is not None for t in triples) else ""
    try:
        assert dev.cells() == sum(lattice_doubles(em.nStates, len(colTok), *t) for t in triples)      # (the full envelope has the rectangle's cells)
        want = np.array([r["ll"] for r in refs])
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        assert capi.last_kernel_name() == "k_profile_two_merge%s_fwd<sum,mat>" % tag and capi.last_launch_count() == 1
        note("forward", fr, want, WORST)
        assert logs_close(fr, want), (fr, want)
        assert np.array_equal(fr, fm), (fr, fm)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        assert capi.last_kernel_name() == "k_profile_two_merge%s_fwd<max,rolling>" % tag
        check_paths(*dev.viterbi(), refs)
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two_merge%s_counts" % tag
        wc = np.sum([r["counts"] for r in refs], axis=0)
        note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want)
        pa, pb, pl = dev.merged_row_posteriors()
        assert capi.last_kernel_name() == "k_profile_two_merge%s_rowpost" % tag and capi.last_launch_count() == 1
        tq.compare(em, colTok, *tq.split(dev, pa, pb), pl, [r["post"] for r in refs], "posteriors under an envelope")
        if fill:
            for (A, B, env), r in zip(triples, refs):
                outside = ~mask(env, len(A)) if env is not None else np.zeros((len(A) + 1, len(B) + 1), bool)
                for mode, key, tol in ((capi.MB_FORWARD, "fwd", LOG_TOL), (capi.MB_BACKWARD, "bwd", LOG_TOL), (capi.MB_VITERBI, "vit", 1e-12)):
                    got = capi.profile_two_fill_merged(dm, mode, A, B, colTok, env)
                    note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key], tol), (mode, len(A), len(B))
                    assert got.shape[2:] == (3, len(colTok) + 1, em.nStates) and np.all(got[outside] == -math.inf)
        if live is not None:
            live += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
