"""Inputs, bounds and the device-against-restatement comparison of the tests of pairs against CTC-merged profiles under an envelope
(test_profile_pair_merge_env_host.py, test_profile_pair_merge_env_gpu.py; not a test module).  The machines and inputs are those of
pairmergehelpers, the envelopes those of pairenvhelpers; the reference is profile.PairMergedProfileDP(env=...) called per pair.
Every builder is deterministic, and test_profile_pair_merge_env_host.py holds the conditions the GPU tests assert -- ring bytes
either side of the marks, M, liveness, tie kinds, chunk compositions -- to the yardstick and to plain arithmetic, without a GPU.

Bounds (the family's, pairprofilehelpers): log values 1e-9 relative to max(1, |value|), -inf exact; counts and posteriors >= 1e-3 at
1e-6 relative, smaller ones at 1e-9 + 1e-6 x value; row sums 1e-6; Viterbi scores 1e-12 with equal paths and rows; fixed-point
quantities the same plus (cells of the call) x 2^-36."""
import math

import numpy as np

import pairenvhelpers as eh
import pairmergehelpers as mh
import pairprofilehelpers as ph
from mergehelpers import greedy_chunks
from pairenvhelpers import diag_max, envelopes, full, mask, n_cells, staircase
from pairmergehelpers import merged_input
from pairprofilehelpers import counts_close, logs_close, pair_machine
from machineboss_amd.machine import MachineError
from machineboss_amd.seqpair import Envelope

LDS_MAX = 160 * 1024
LDS_DEFAULT = 64 * 1024
ROW_TOL = 1e-6
ENV_FWD = "k_profile_pair_merge_env_fwd<%s>"
FULL_FWD = "k_profile_pair_merge_fwd<%s>"


def ring_bytes(S, nCols, M, mat=False):
    """The ring of a pair under an envelope (mb_profile_pair_merge.h): three diagonals of M cells, each N, W (nCols + 1 planes) and
    X (nCols planes) rolling, X (or T) alone materialised."""
    return 8 * 3 * (nCols if mat else 3 * nCols + 2) * M * S


def lattice_doubles(S, nCols, x, P, env):
    """pp_cells: the rectangle's two layers of nCols + 1 planes, or those of the compact lattice of the envelope."""
    return 2 * S * (nCols + 1) * (n_cells(env) if env is not None else (len(x) + 1) * (len(P) + 1))


def scratch_bytes(S, nCols, x, P, env, mat):
    """pp_ring_bytes: 0 where the ring lies in LDS."""
    b = ring_bytes(S, nCols, diag_max(env), mat) if env is not None else mh.ring_bytes(S, nCols, len(x), len(P), mat)
    return 0 if b <= LDS_MAX else b


def call_bytes(call, em, nCols, triples, nLevels=None):
    """What each call of mb_profile_api.hip tells lattice_chunks a merged pair costs (pairenvhelpers.call_bytes with the plane
    factor and the X / T ring of the materialised sweeps)."""
    S, PL = em.nStates, nCols + 1
    nLevels = eh.silent_levels(em) if nLevels is None and call == "viterbi" else nLevels
    out = []
    for x, P, env in triples:
        cells = 8 * lattice_doubles(S, nCols, x, P, env)
        ring = scratch_bytes(S, nCols, x, P, env, True)
        out.append({"forward": cells + ring, "viterbi": cells + ring + 8 * eh.path_bound(nLevels or 0, len(x), len(P)),
                    "counts": 2 * cells + ring, "posteriors": 2 * cells + ring + 8 * len(P) * PL,
                    "rolling": scratch_bytes(S, nCols, x, P, env, False)}[call])
    return out


def env_reference(dp, x, P, env, paths=True, counts=True, cells=True, post=True):
    """Everything the yardstick says about one pair under env (None: no envelope)."""
    kw = {} if env is None else {"env": env}
    out = {}
    ll, N, W = dp.forward(x, P, **kw)
    v, VN, VW = dp.forward(x, P, "max", **kw)
    out.update(ll=ll, v=v)
    if cells:
        _, NB, WB = dp.backward(x, P, **kw)
        out.update(fwd=np.stack([N, W], axis=2), bwd=np.stack([NB, WB], axis=2), vit=np.stack([VN, VW], axis=2))
    if paths:
        out["path"] = dp.viterbi(x, P, **kw)[1:]
    if counts:
        out["counts"] = dp.counts(x, P, **kw)[0]
    if post:
        out["post"] = dp.rowPosteriors(x, P, **kw)
    return out


# ---- every cell -------------------------------------------------------------------------------------------------------------------------
CELL_CASES = ((1, 1), (2, 1), (4, 13), (4, 65), (65, 2))          # (nCols, S)
CELL_SHAPES = mh.SHAPES                                            # seven lattices from (0, 0) to (9, 9), (0, 3) and (3, 0) among them


def cell_case(nCols, S):
    """[(em, colTok, [(x, P, kind, env)])]: the machine with silent levels (S >= 2) and without, at every shape under every envelope
    of pairenvhelpers.envelopes; a twentieth of the column weights -inf (a band of width 0 leaves one alignment only)."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 200 + S, levels, 2, 3)
        rng = np.random.RandomState(1000 * nCols + S)
        colTok = rng.randint(1, 4, nCols)
        quads = []
        for I, L in CELL_SHAPES:
            x, P = merged_input(rng, em, nCols, I, L, zeros=0.05)
            quads += [(x, P, kind, env) for kind, env in envelopes(rng, I, L)]
        out.append((em, colTok, quads))
    return out


# ---- the ring marks: nCols = 4, S = 80, I = L = 40 --------------------------------------------------------------------------------------
MARK_S, MARK_LEN, MARK_COLTOK = 80, 40, (1, 2, 3, 1)
MARK_ROLLING = (2, 3, 6, 7)          # M: 336 M S bytes = 53 760 | 80 640 either side of 64 KiB, 161 280 | 188 160 either side of 160 KiB
MARK_MAT = (8, 9, 21, 22)            # M: 96 M S bytes = 61 440 | 69 120 and 161 280 | 168 960
MARK_M = MARK_ROLLING + MARK_MAT


def mark_machine():
    return pair_machine(MARK_S, 880, True, 2, 3)


def mark_case(M):
    """(x, P, env): a band of half-width M - 1 on a square lattice has at most M cells on a diagonal."""
    x, P = merged_input(np.random.RandomState(8800 + M), mark_machine(), 4, MARK_LEN, MARK_LEN, zeros=0.05)
    return x, P, Envelope.band(MARK_LEN, MARK_LEN, M - 1)


def mark_extras():
    """A pair without an envelope and a dead pair (a row all -inf) under a band, to put beside the eight."""
    em = mark_machine()
    x0, P0 = merged_input(np.random.RandomState(8890), em, 4, 12, 10, zeros=0.05)
    x1, P1 = merged_input(np.random.RandomState(8891), em, 4, 20, 20, zeros=0.05)
    P1[7] = -np.inf
    return (x0, P0, None), (x1, P1, Envelope.band(20, 20, 3))


# ---- one call over both kinds -----------------------------------------------------------------------------------------------------------
MIXED_STATES = (8, 65)
MIXED_COLTOK = (1, 2, 3, 1)
MIXED_SPEC = eh.MIXED_SPEC
MIXED_DEAD = eh.MIXED_DEAD
MIXED_BUDGET_FACTOR = 1.8
CHUNK_KINDS = {"EP", "P", "E", "PE"}


def mixed_case(S):
    """(em, colTok, [(x, P, env or None)]): pairenvhelpers.MIXED_SPEC -- twenty pairs, enveloped and plain interleaved, (0, 0), no
    rows, no input and a dead pair of each kind among them -- against merged profiles of four columns."""
    em = pair_machine(S, eh.MIXED_SEED[S], True, 2, 3)
    triples = []
    for k, (I, L, kind, dead) in enumerate(MIXED_SPEC):
        rng = np.random.RandomState(7100 * S + 100 * k + 10 * I + L)
        x, P = merged_input(rng, em, 4, I, L, zeros=0.05)
        if dead:
            P[L // 2] = -np.inf
        triples.append((x, P, eh.named_envelope(kind, rng, I, L)))
    return em, MIXED_COLTOK, triples


def mixed_budget(call, em, triples):
    return int(MIXED_BUDGET_FACTOR * max(call_bytes(call, em, 4, triples)))


def mixed_chunks(call, em, triples):
    """(budget, chunks, kinds, launches) of a call over the mixed batch under mixed_budget, by the restated chunk rule."""
    budget = mixed_budget(call, em, triples)
    chunks = greedy_chunks(call_bytes(call, em, 4, triples), budget)
    envs = [t[2] for t in triples]
    return budget, chunks, eh.chunk_kinds(chunks, envs), eh.chunk_launches(chunks, envs)


def mixed_states(triples):
    return eh.mixed_states(triples)


# ---- counts past the LDS table, ties ----------------------------------------------------------------------------------------------------
def big_counts_env_case():
    """big_counts_case's machine (11 204 transitions), column map and pairs, the dead one last, each under band(w = 2)."""
    em, colTok, pairs, dead = mh.big_counts_case()
    return em, colTok, [(x, P, Envelope.band(len(x), len(P), 2)) for x, P in pairs + [dead]]


def tie_env_pairs():
    """tie_pairs under band(w = 1); the shapes whose slope such a band cannot bridge are left out."""
    out = []
    for x, P in mh.tie_pairs():
        try:
            out.append((x, P, Envelope.band(len(x), len(P), 1)))
        except MachineError:
            pass
    return out


# ---- the traceback past one block of 64 lanes, in each of the two launches ------------------------------------------------------------
SEAM_ENV, SEAM_PLAIN = 129, 65
SEAM_DEAD_ENV, SEAM_DEAD_PLAIN = (63, 64, 128), (63, 64)      # by slot within the launch
SEAM_COLTOK = (1, 2)
SEAM_SHAPES = mh.SEAM_SHAPES


def seam_case():
    """(em, colTok, triples): 194 pairs at S = 8 with levels against merged profiles of two columns, two enveloped pairs then a
    plain one, 64 times, then one of each; the envelopes in turn from envelopes() of the shape; dead pairs (a row all -inf) at the
    seams of both launches' blocks."""
    em = pair_machine(8, 208, True, 2, 3)
    kinds = "EEP" * 64 + "PE"
    triples, nP, nE = [], 0, 0
    for k, c in enumerate(kinds):
        I, L = SEAM_SHAPES[k % len(SEAM_SHAPES)]
        dead = (nP in SEAM_DEAD_PLAIN) if c == "P" else (nE in SEAM_DEAD_ENV)
        if dead:
            I, L = 3, 3
        rng = np.random.RandomState(9300 + k)
        x, P = merged_input(rng, em, 2, I, L, zeros=0.0)
        if dead:
            P[1] = -np.inf
        env = None
        if c == "E":
            es = envelopes(rng, I, L)
            env = es[nE % len(es)][1]
        triples.append((x, P, env))
        nP += c == "P"; nE += c == "E"
    return em, SEAM_COLTOK, triples


def seam_prefix(triples, n):
    return eh.seam_prefix(triples, n)


# ---- row posteriors past the table and past 1 024 row blocks -------------------------------------------------------------------------
WRAP_SHAPE = (1, 1100)
WRAP_GROUPS = 1024
WRAP_COLTOK = (1, 2, 3, 1)


def wrap_case():
    """(em, colTok, x, P, Pdead): pairmergeposthelpers.wrap_case -- S = 2, nCols = 4 at (1, 1 100); the dead profile has row 700 all -inf."""
    import pairmergeposthelpers as mp
    em, colTok, ((x, P), (_, dead)) = mp.wrap_case()
    return em, colTok, x, P, dead


# ---- the compact pool, the scale ---------------------------------------------------------------------------------------------------------
POOL = (65, 300, 4)               # S, I = L, w
POOL_COLTOK = (1, 2, 3, 1)


def pool_case():
    S, I, w = POOL
    em = pair_machine(S, 365, True, 2, 3)
    return em, POOL_COLTOK, [merged_input(np.random.RandomState(3660 + k), em, 4, I, I, zeros=0.02) for k in range(2)], Envelope.band(I, I, w)


SCALE = (8, 1500, 3, 4)           # S, I = L, w, pairs


def scale_case():
    S, I, w, n = SCALE
    em = pair_machine(S, 208, True, 2, 3)
    return em, POOL_COLTOK, [merged_input(np.random.RandomState(1500 + k), em, 4, I, I, zeros=0.02) for k in range(n)], Envelope.band(I, I, w)


# ---- the device against the restatement ---------------------------------------------------------------------------------------------
WORST = {}


def split(dev, post):
    return [post[dev.rowOff[k]:dev.rowOff[k + 1]] for k in range(dev.nPairs)]


def open_pairs(dm, colTok, triples, envs=None):
    from machineboss_amd import capi
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples], colTok)
    envs = [t[2] for t in triples] if envs is None else envs
    if any(e is not None for e in envs):
        dev.set_merged_envelopes(envs)
    return dev


def check_paths(v, off, edges, rows, refs, what="viterbi"):
    wv = np.array([r["v"] for r in refs])
    ph.note(what, v, wv, WORST)
    assert logs_close(v, wv, 1e-12), (v, wv)
    assert len(off) == len(refs) + 1 and off[0] == 0 and off[-1] == len(edges) == len(rows)
    for k, r in enumerate(refs):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(edges[sl], r["path"][0]) and np.array_equal(rows[sl], r["path"][1]), (k, edges[sl], r["path"][0])


def check_posteriors(got, ll, posts, what="posteriors"):
    """The device's per-pair posteriors and likelihoods against rowPosteriors(env=...): entries, exact zeros, row sums."""
    want = np.array([p[1] for p in posts])
    ph.note("loglike of " + what, ll, want, WORST)
    assert logs_close(ll, want), (ll, want)
    for k, (g, (w, wl)) in enumerate(zip(got, posts)):
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if not g.size:
            continue
        ph.note_counts(g.ravel(), w.ravel(), WORST, what)
        assert counts_close(g, w), (k, np.abs(g - w).max())
        assert not g[w == 0.0].any() and (g >= 0.0).all(), k
        if wl > -math.inf:
            WORST["row sums"] = max(WORST.get("row sums", 0.0), float(np.abs(g.sum(axis=1) - 1.0).max()))
            assert np.abs(g.sum(axis=1) - 1.0).max() <= ROW_TOL, (k, g.sum(axis=1))
        else:
            assert not g.any(), k


def fixed_close(got, want, terms):
    """counts_close with the fixed point's quantum on top: at most one term per cell of the call, each rounded once to 2^-36."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.where(want >= 1e-3, 0.0, ph.COUNT_ABS) + ph.COUNT_REL * want + terms * 2.0 ** -36))


def terms(nCols, triples):
    """The (cell, plane) pairs of a call: what a transition or a bin can get a term from."""
    return (nCols + 1) * sum(n_cells(env) if env is not None else (len(x) + 1) * (len(P) + 1) for x, P, env in triples)


def check_env_batch(em, colTok, triples, fill=False, live=None):
    """Everything the device computes for the (x, P, env) of one machine, in one batch, against the restatement under env: rolling
    and materialised Forward (and the same bits from both), Viterbi with and without paths, counts, merged row posteriors, and with
    ``fill`` every pair's three lattices, -inf outside in both layers and all planes."""
    from machineboss_amd import capi
    from machineboss_amd.profile import PairMergedProfileDP
    dp = PairMergedProfileDP(em, colTok)
    refs = [env_reference(dp, x, P, env, cells=fill) for x, P, env in triples]
    dm = capi.DeviceMachine(em)
    dev = open_pairs(dm, colTok, triples)
    try:
        assert dev.cells() == sum(lattice_doubles(em.nStates, len(colTok), *t) for t in triples)
        want = np.array([r["ll"] for r in refs])
        fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
        ph.note("forward", fr, want, WORST)
        assert logs_close(fr, want), (fr, want)
        assert np.array_equal(fr, fm), (fr, fm)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        check_paths(*dev.viterbi(), refs)
        c, s, ll = dev.counts()
        wc = np.sum([r["counts"] for r in refs], axis=0)
        ph.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want)
        post, pl = dev.merged_row_posteriors()
        check_posteriors(split(dev, post), pl, [r["post"] for r in refs])
        if fill:
            for (x, P, env), r in zip(triples, refs):
                outside = ~mask(env, len(x)) if env is not None else np.zeros((len(x) + 1, len(P) + 1), bool)
                for mode, key, tol in ((capi.MB_FORWARD, "fwd", ph.LOG_TOL), (capi.MB_BACKWARD, "bwd", ph.LOG_TOL), (capi.MB_VITERBI, "vit", 1e-12)):
                    got = capi.profile_pair_fill_merged(dm, mode, x, P, colTok, env)
                    ph.note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key], tol), (mode, len(x), len(P))
                    assert np.all(got[outside] == -math.inf)
        if live is not None:
            live += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
