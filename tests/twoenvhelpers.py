"""Envelopes, inputs and the device-against-restatement comparison of the tests of the two-profile sweeps under an envelope
(test_profile_two_env_host.py, test_profile_two_env_gpu.py; not a test module).  The envelopes are those of pairenvhelpers (full,
bands, the path envelope of a random alignment, the staircase) with K input rows for I input tokens; the machines, profiles and
bounds those of twoprofilehelpers; the reference is profile.TwoProfileDP(env=...), which test_profile_two_env_host.py first holds to
an enumeration of paths, to the pair sweep and to its own identities."""
import math

import numpy as np

import twoposthelpers as tp
import twoprofilehelpers as th
from pairenvhelpers import diag_max, envelope, envelopes, full, mask, n_cells, random_alignment, staircase  # noqa: F401
from pairprofilehelpers import LOG_TOL, counts_close, logs_close, note, note_counts, pair_machine
from twoprofilehelpers import two_input
from machineboss_amd.machine import MachineError
from machineboss_amd.seqpair import Envelope

LDS_MAX = 160 * 1024


# ---- every path, one by one -------------------------------------------------------------------------------------------------------
def enumerate_paths(em, A, B, env=None):
    """(log of the summed weight of every path, the best path's weight, the number of paths with a finite weight): the stages of
    "Pairs of profiles" walked depth first from the arrived stage of (0, 0, 0) to the committed stage of (K, L, S - 1), one path at
    a time, a move taken only if the cell it leads to is inside the envelope.  Nothing is summed before a path is complete."""
    K, L, S = len(A), len(B), em.nStates
    inside = np.ones((K + 1, L + 1), bool) if env is None else mask(env, K)
    out = [[] for _ in range(S)]
    for e in range(em.nTransitions):
        out[int(em.src[e])].append((int(em.dst[e]), int(em.inTok[e]), int(em.outTok[e]), float(em.logWeight[e])))
    weights = []

    def walk(stage, i, r, q, w):
        if w == -math.inf:
            return
        if stage == 0:      # arrived: the output blank, or settle
            if r < L and inside[i, r + 1]:
                walk(0, i, r + 1, q, w + B[r][0])
            walk(1, i, r, q, w)
        elif stage == 1:    # waiting: output-only and silent edges, or commit
            for d, a, o, lw in out[q]:
                if a:
                    continue
                if o:
                    if r < L and inside[i, r + 1]:
                        walk(0, i, r + 1, d, w + lw + B[r][o])
                elif d > q:
                    walk(1, i, r, d, w + lw)
            walk(2, i, r, q, w)
        else:               # committed: the end, the input blank, input-reading edges
            if i == K and r == L and q == S - 1:
                weights.append(w)
            if i < K:
                if inside[i + 1, r]:
                    walk(2, i + 1, r, q, w + A[i][0])
                for d, a, o, lw in out[q]:
                    if not a:
                        continue
                    if o:
                        if r < L and inside[i + 1, r + 1]:
                            walk(0, i + 1, r + 1, d, w + lw + A[i][a] + B[r][o])
                    elif inside[i + 1, r]:
                        walk(1, i + 1, r, d, w + lw + A[i][a])

    if inside[0, 0]:
        walk(0, 0, 0, 0, 0.0)
    if not weights:
        return -math.inf, -math.inf, 0
    w = np.array(weights)
    return float(w.max() + np.log(np.exp(w - w.max()).sum())), float(w.max()), len(w)


ENUM_STATES = (2, 3)
ENUM_SHAPES = ((0, 0), (1, 0), (0, 2), (1, 1), (2, 1), (1, 3), (2, 2), (3, 2), (3, 3))


def enum_envelopes(K, L):
    """full, band(0), band(1) and the staircase; a band the slope defeats is left out, and so is a repeat."""
    out = [("full", full(K, L))]
    for w in (0, 1):
        try:
            out.append(("band%d" % w, Envelope.band(K, L, w)))
        except MachineError:
            pass
    out.append(("stairs", staircase(K, L)))
    seen, uniq = set(), []
    for kind, e in out:
        key = (tuple(e.inStart), tuple(e.inEnd))
        if key not in seen:
            seen.add(key); uniq.append((kind, e))
    return uniq


def enum_cases():
    """(key, em, A, B, kind, env): pair_machine(S, seed, levels, 2, 3) for S in {2, 3} on lattices up to (3, 3)."""
    for S in ENUM_STATES:
        for levels in (True, False):
            em = pair_machine(S, 30 + S, levels, 2, 3)
            for K, L in ENUM_SHAPES:
                A, B = two_input(np.random.RandomState(100 * S + 10 * K + L), em, K, L, pInf=0.1)
                for kind, env in enum_envelopes(K, L):
                    yield (S, levels, K, L, kind), em, A, B, kind, env


# ---- envelopes ---------------------------------------------------------------------------------------------------------------------
def transposed_env(env, K):
    """The envelope of the transposed pair: per input row i = 0..K the run of output rows whose interval holds i."""
    m = mask(env, K)
    st = [int(np.argmax(m[i])) for i in range(K + 1)]
    en = [int(len(m[i]) - np.argmax(m[i][::-1])) for i in range(K + 1)]
    assert all(m[i, st[i]:en[i]].all() and m[i].sum() == en[i] - st[i] for i in range(K + 1))      # (columns are runs)
    return envelope(st, en, len(env.inStart) - 1)


def column_stairs(K, L):
    """An envelope whose columns are runs of 1, 2 and many cells: rows 0 .. L - 3 hold input row 0 alone (a column of L - 2 cells and
    more), the last rows fan out so that the input rows behind take two cells, then one each."""
    assert K >= 4 and L >= 6
    st = [0] * (L + 1); en = [1] * (L + 1)
    en[L - 3] = 2                                # input row 1: rows L-3, L-2 (two cells)
    st[L - 2], en[L - 2] = 1, 3                  # input row 2: rows L-2, L-1 (two cells)
    st[L - 1], en[L - 1] = 2, 4                  # input row 3: rows L-1, L
    st[L], en[L] = 3, K + 1                      # input rows 4..K: one cell each
    return envelope(st, en, K)


def band_or_full(K, L, w):
    try:
        return Envelope.band(K, L, w)
    except MachineError:
        return full(K, L)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def env_reference(dp, A, B, env, cells=True, paths=True, counts=True, post=True):
    out = {}
    ll, N, W, Z = dp.forward(A, B, env=env)
    v, VN, VW, VZ = dp.forward(A, B, "max", env=env)
    out.update(ll=ll, v=v)
    if cells:
        _, NB, WB, ZB = dp.backward(A, B, env=env)
        out.update(fwd=np.stack([N, W, Z], axis=2), bwd=np.stack([NB, WB, ZB], axis=2), vit=np.stack([VN, VW, VZ], axis=2))
    if paths:
        out["path"] = dp.viterbi(A, B, env=env)[1:]
    if counts:
        out["counts"] = dp.counts(A, B, env=env)[0]
    if post:
        out["post"] = dp.rowPosteriors(A, B, env=env)
    return out


# ---- the input families of the GPU module --------------------------------------------------------------------------------------------
CELL_STATES = (1, 2, 8, 65)
CELL_SHAPES = th.SUITE_SHAPES                      # seven lattices from (0, 0) to (9, 9)
CELL_SEED = {1: 301, 2: 322, 8: 308, 65: 365}
ENV_KINDS = ("full", "band0", "band1", "path", "stairs")


def cell_case(S):
    """[(em, A, B, kind, env)]: the machine with silent levels (S >= 2) and without, at every shape under every envelope."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, CELL_SEED[S], levels, 2, 3)
        for K, L in CELL_SHAPES:
            rng = np.random.RandomState(3000 * S + 10 * K + L)
            A, B = two_input(rng, em, K, L, pInf=0.05)
            out += [(em, A, B, kind, env) for kind, env in envelopes(rng, K, L)]
    return out


MARK_S, MARK_LEN = 40, 72
MARK_M = (22, 23, 56, 57)          # 72 * M * 40 bytes: 63 360 / 66 240 either side of 64 KiB, 161 280 / 164 160 either side of 160 KiB


def ring_bytes(S, M):
    return 72 * M * S


def mark_machine():
    return pair_machine(MARK_S, 440, True, 2, 3)


def mark_case(M):
    """(A, B, env): a band of half-width M - 1 on a square lattice has at most M cells on a diagonal."""
    em = mark_machine()
    A, B = two_input(np.random.RandomState(7200 + M), em, MARK_LEN, MARK_LEN, pInf=0.0)
    return A, B, Envelope.band(MARK_LEN, MARK_LEN, M - 1)


def mark_extras():
    """A pair without an envelope, a (0, 0) pair and a dead pair (a row of B all -inf) under a band, to put beside the four."""
    em = mark_machine()
    A0, B0 = two_input(np.random.RandomState(7290), em, 12, 9, pInf=0.0)
    Az, Bz = two_input(np.random.RandomState(7291), em, 0, 0, pInf=0.0)
    A1, B1 = two_input(np.random.RandomState(7292), em, 10, 10, pInf=0.0)
    B1 = B1.copy(); B1[4] = -np.inf
    return (A0, B0, None), (Az, Bz, None), (A1, B1, Envelope.band(10, 10, 3))


SLOPE_CASES = ((200, 40, 6), (40, 200, 2))


def slope_machine():
    return pair_machine(8, 88, True, 2, 3)


def slope_case(K, L, w):
    em = slope_machine()
    A, B = two_input(np.random.RandomState(8800 + K), em, K, L, pInf=0.0)
    return A, B, Envelope.band(K, L, w)


PACK = (300, 24, 20, 8)           # S, pairs, K = L, w: M = 9, a ring of 72 * 9 * 300 = 194 400 bytes, past 160 KiB


def pack_case():
    S, n, K, w = PACK
    em = pair_machine(S, 301, True, 2, 3)
    return em, [two_input(np.random.RandomState(3010 + k), em, K, K, pInf=0.0) for k in range(n)], Envelope.band(K, K, w)


RAGGED_SPEC = ((9, 9, False), (2, 5, False), (0, 0, False), (7, 9, False), (0, 4, False), (6, 7, True), (9, 6, False), (4, 0, False), (5, 2, False))
RAGGED_DEAD = 5


def ragged_case():
    """(em, pairs): nine ragged pairs on the levelled machine of 8 states, the sixth dead."""
    em = th.split_machine()
    pairs = []
    for k, (K, L, dead) in enumerate(RAGGED_SPEC):
        rng = np.random.RandomState(8100 + 100 * k + 10 * K + L)
        pairs.append(th.dead_pair(rng, em, K, L, 3) if dead else two_input(rng, em, K, L, pInf=0.0))
    return em, pairs


def big_counts_env_case():
    """big_counts_case's machine (11 204 transitions) and pairs with its dead pair, each under band(2) (the full envelope where
    the slope defeats it)."""
    em, pairs, dead = th.big_counts_case()
    return em, [(A, B, band_or_full(len(A), len(B), 2)) for A, B in pairs + [dead]]


POST_STAIRS = (9, 12)


def post_stairs_case():
    """(em, A, B, env) at (9, 12) under column_stairs, S = 8."""
    em = pair_machine(8, 308, True, 2, 3)
    A, B = two_input(np.random.RandomState(912), em, *POST_STAIRS, pInf=0.0)
    return em, A, B, column_stairs(*POST_STAIRS)


LONG = 1100
LONG_SHAPES = ((1, LONG), (LONG, 1))
LONG_TABLES = ("4", "2", None)


def long_case(K, L):
    """twoposthelpers.long_case -- S = 2, a live and a dead pair -- each under the staircase of its shape."""
    em, pairs = tp.long_case(K, L)
    return em, [(A, B, staircase(K, L)) for A, B in pairs]


def env_rowpost_blocks(S, env, K, axis, nIn, nOut, table=tp.ROWPOST_LDS_MAX):
    """The line blocks of k_profile_two_rowpost under an envelope: profile_pair_rowpost_rows over the compact cell count."""
    L = len(env.inStart) - 1
    lines, cols = (K, nIn + 1) if axis else (L, nOut + 1)
    if lines <= 0:
        return 0
    if cols > table:
        return lines
    per = max(1, n_cells(env) * S // (lines + 1))
    return -(-lines // min(-(-tp.ROWPOST_ITEMS // per), table // cols, lines))


CHUNK = (65, 100, 4, 3)           # S, K = L, w, pairs


def chunk_case():
    S, K, w, n = CHUNK
    em = pair_machine(S, 365, True, 2, 3)
    return em, [two_input(np.random.RandomState(3650 + k), em, K, K, pInf=0.0) for k in range(n)], Envelope.band(K, K, w)


def lattice_bytes(S, env):
    return 8 * 3 * S * n_cells(env)


def chunk_budget():
    """A quarter of a rectangle: 4.0 MB, which holds one pair's compact Forward and Backward lattices (2.8 MB) and not a second."""
    S, K, _, _ = CHUNK
    return 8 * 3 * S * (K + 1) * (K + 1) // 4


def tie_env_pairs():
    """tie_pairs under band(1); the shapes whose slope such a band cannot bridge are left out."""
    out = []
    for A, B in th.tie_pairs():
        try:
            out.append((A, B, Envelope.band(len(A), len(B), 1)))
        except MachineError:
            pass
    return out


def onehot_case():
    """(em, x, A, B, env): pair_machine(40) at (30, 30) under band(3); A is the one-hot profile of the token string x, its blank -inf."""
    em = pair_machine(40, 41, True, 2, 3)
    rng = np.random.RandomState(4141)
    x = rng.randint(1, em.nInTok + 1, size=30).astype(np.int32)
    B = th.soft_profile(rng, 30, em.nOutTok, pInf=0.0)
    return em, x, th.one_hot(x, em.nInTok), B, Envelope.band(30, 30, 3)


def builders():
    """{name: [(em, A, B, env or None)]}: every input of the GPU module, for the liveness test."""
    out = {}
    for S in CELL_STATES:
        out["cells%d" % S] = [(em, A, B, env) for em, A, B, _, env in cell_case(S)]
    em = mark_machine()
    out["marks"] = [(em,) + mark_case(M) for M in MARK_M] + [(em,) + t for t in mark_extras()]
    out["slopes"] = [(slope_machine(),) + slope_case(*c) for c in SLOPE_CASES]
    em, pairs, env = pack_case()
    out["pack"] = [(em, A, B, env) for A, B in pairs[:4]]
    em, pairs = ragged_case()
    out["ragged"] = [(em, A, B, full(len(A), len(B))) for A, B in pairs]
    em, triples = big_counts_env_case()
    out["counts"] = [(em,) + t for t in triples]
    out["stairs"] = [post_stairs_case()]
    for K, L in LONG_SHAPES:
        em, triples = long_case(K, L)
        out["long%d" % K] = [(em,) + t for t in triples]
    em, pairs, env = chunk_case()
    out["chunks"] = [(em, A, B, env) for A, B in pairs]
    em = th.tie_machine()
    out["ties"] = [(em,) + t for t in tie_env_pairs()]
    em, _, A, B, env = onehot_case()
    out["onehot"] = [(em, A, B, env)]
    return out


# ---- the device against the restatement ---------------------------------------------------------------------------------------------
WORST = {}


def open_twos(em, triples):
    from machineboss_amd import capi
    dm = capi.DeviceMachine(em)
    return dm, capi.DeviceProfileTwos(dm, [t[0] for t in triples], [t[1] for t in triples], envs=[t[2] for t in triples])


def check_env_batch(em, triples, fill=False, live=None, refs=None, post=True):
    """Everything the device computes for the (A, B, env) of one machine, in one batch, against the restatement under env."""
    from machineboss_amd import capi
    from machineboss_amd.profile import TwoProfileDP
    dp = TwoProfileDP(em)
    refs = [env_reference(dp, A, B, env, cells=fill, post=post) for A, B, env in triples] if refs is None else refs
    dm, dev = open_twos(em, triples)
    enveloped = any(t[2] is not None for t in triples)
    tag = "_env" if enveloped else ""
    try:
        want = np.array([r["ll"] for r in refs])
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        assert capi.last_kernel_name() == "k_profile_two%s_fwd<sum,mat>" % tag and capi.last_launch_count() == 1
        note("forward", fr, want, WORST)
        assert logs_close(fr, want) and logs_close(fm, want), (fr, fm, want)
        assert np.array_equal(fr, fm)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        assert capi.last_kernel_name() == "k_profile_two%s_fwd<max,rolling>" % tag
        v, off, edges, rows, ins = dev.viterbi()
        note("viterbi", v, wv, WORST)
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, r in enumerate(refs):
            sl = slice(off[k], off[k + 1])
            assert np.array_equal(edges[sl], r["path"][0]) and np.array_equal(rows[sl], r["path"][1]) and np.array_equal(ins[sl], r["path"][2]), k
        c, s, ll = dev.counts()
        assert capi.last_kernel_name() == "k_profile_two%s_counts" % tag
        wc = np.sum([r["counts"] for r in refs], axis=0)
        note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want)
        if post:
            pa, pb, pl = dev.row_posteriors()
            assert capi.last_kernel_name() == "k_profile_two%s_rowpost" % tag and capi.last_launch_count() == 1
            tp.compare(em, *tp.split(dev, pa, pb), pl, [r["post"] for r in refs], "posteriors under an envelope")
            ga, gb = tp.grouped(em, c)
            assert counts_close(pa[:, 1:].sum(axis=0), ga) and counts_close(pb[:, 1:].sum(axis=0), gb)
        if fill:
            for (A, B, env), r in zip(triples, refs):
                outside = ~mask(env, len(A)) if env is not None else np.zeros((len(A) + 1, len(B) + 1), bool)
                for mode, key, tol in ((capi.MB_FORWARD, "fwd", LOG_TOL), (capi.MB_BACKWARD, "bwd", LOG_TOL), (capi.MB_VITERBI, "vit", 1e-12)):
                    got = capi.profile_two_fill(dm, mode, A, B, env)
                    note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key], tol), (mode, len(A), len(B))
                    assert got.shape[2] == 3 and np.all(got[outside] == -math.inf)
        if live is not None:
            live += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
