"""Envelopes, inputs and the device-against-restatement comparison of the tests of the two-tape profile sweeps under an envelope
(test_profile_pair_env_host.py, test_profile_pair_env_gpu.py; not a test module).  The machines, inputs and bounds are those of
pairprofilehelpers; the reference is profile.PairProfileDP(env=...)."""
import math

import numpy as np

import pairprofilehelpers as ph
from pairprofilehelpers import counts_close, logs_close, pair_input, pair_machine
from machineboss_amd.machine import MachineError
from machineboss_amd.seqpair import Envelope


def envelope(inStart, inEnd, I):
    e = Envelope()
    e.inLen, e.outLen, e.inStart, e.inEnd = I, len(inStart) - 1, [int(v) for v in inStart], [int(v) for v in inEnd]
    return e


def full(I, L):
    return envelope([0] * (L + 1), [I + 1] * (L + 1), I)


def random_alignment(rng, I, L):
    """Alignment columns of I input and L output symbols: matches, insertions and deletions in a random order."""
    cols, i, r = [], 0, 0
    while i < I or r < L:
        kinds = [k for k, ok in (("m", i < I and r < L), ("i", i < I), ("o", r < L)) if ok]
        k = kinds[rng.randint(len(kinds))]
        cols.append(("a" if k != "o" else "", "b" if k != "i" else ""))
        i += k != "o"; r += k != "i"
    return cols


def staircase(I, L):
    """Rows that share no input position, each joined to the next by a corner alone (a match is the only way across): the I + 1
    positions dealt over the L + 1 rows in order; a row left without a position of its own is a single cell below the row before.
    At I = L every row is the single cell (r, r)."""
    cut = [min(I + 1, (r * (I + 1) + L) // (L + 1)) for r in range(L + 2)]
    st, en = [], []
    for r in range(L + 1):
        a, b = cut[r], cut[r + 1]
        if b <= a:
            a, b = min(a, I), min(a, I) + 1
        st.append(a); en.append(b)
    st[0] = 0; en[L] = I + 1
    return envelope(st, en, I)


ENV_KINDS = ("full", "band0", "band1", "path", "stairs")


def envelopes(rng, I, L):
    """[(kind, Envelope)]: full, band(w = 0), band(w = 1), the path envelope of a random alignment and the staircase; a band too
    narrow for the slope of the shape is left out, and so is an envelope equal to an earlier one of the list."""
    out = [("full", full(I, L))]
    for w in (0, 1):
        try:
            out.append(("band%d" % w, Envelope.band(I, L, w)))
        except MachineError:
            pass
    out.append(("path", Envelope.pathEnvelope(random_alignment(rng, I, L))))
    out.append(("stairs", staircase(I, L)))
    seen, uniq = set(), []
    for kind, e in out:      # (a lattice of one row or one column has one envelope only: once is enough)
        assert e.connected() and e.monotone() and len(e.inStart) == L + 1
        key = (tuple(e.inStart), tuple(e.inEnd))
        if key not in seen:
            seen.add(key); uniq.append((kind, e))
    return uniq


def diag_max(env):
    """M: the largest number of envelope cells on one anti-diagonal."""
    cnt = {}
    for r, (a, b) in enumerate(zip(env.inStart, env.inEnd)):
        for i in range(a, b):
            cnt[i + r] = cnt.get(i + r, 0) + 1
    return max(cnt.values())


def n_cells(env):
    return sum(b - a for a, b in zip(env.inStart, env.inEnd))


def mask(env, I):
    """[I + 1, L + 1] booleans: the cell is inside."""
    m = np.zeros((I + 1, len(env.inStart)), bool)
    for r, (a, b) in enumerate(zip(env.inStart, env.inEnd)):
        m[a:b, r] = True
    return m


def env_reference(dp, x, P, env, paths=True, counts=True, cells=True):
    out = {}
    ll, N, W = dp.forward(x, P, env=env)
    v, VN, VW = dp.forward(x, P, "max", env=env)
    out.update(ll=ll, v=v)
    if cells:
        _, NB, WB = dp.backward(x, P, env=env)
        out.update(fwd=np.stack([N, W], axis=2), bwd=np.stack([NB, WB], axis=2), vit=np.stack([VN, VW], axis=2))
    if paths:
        out["path"] = dp.viterbi(x, P, env=env)[1:]
    if counts:
        out["counts"] = dp.counts(x, P, env=env)[0]
    return out


# ---- every cell: the shapes, machines and envelopes of test_every_cell_under_every_envelope -----------------------------------------
CELL_STATES = (1, 2, 8, 65)
CELL_SHAPES = ((0, 0), (0, 5), (5, 0), (3, 3), (9, 9), (9, 4), (4, 9))
CELL_SEED = {1: 201, 2: 222, 8: 208, 65: 265}      # machines under which nine in ten of a case's likelihoods are finite (the host test holds them to it)


def cell_case(S):
    """[(em, x, P, kind, env)]: the machine with silent levels (S >= 2) and without, at every shape under every envelope."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, CELL_SEED[S], levels, 2, 3)
        for I, L in CELL_SHAPES:
            rng = np.random.RandomState(2000 * S + 10 * I + L)
            x, P = pair_input(rng, em, I, L)
            out += [(em, x, P, kind, env) for kind, env in envelopes(rng, I, L)]
    return out


# ---- the ring marks: S = 40, I = L = 120, bands with M = 34, 35, 85, 86 ---------------------------------------------------------------
MARK_S, MARK_LEN = 40, 120
MARK_M = (34, 35, 85, 86)          # 48 * M * 40 bytes: 65 280 / 67 200 either side of 64 KiB, 163 200 / 165 120 either side of 160 KiB


def mark_machine():
    return pair_machine(MARK_S, 440, True, 2, 3)


def mark_case(M):
    """(x, P, env): a band of half-width M - 1 on a square lattice has at most M cells on a diagonal."""
    em = mark_machine()
    x, P = pair_input(np.random.RandomState(4400 + M), em, MARK_LEN, MARK_LEN)
    return x, P, Envelope.band(MARK_LEN, MARK_LEN, M - 1)


def mark_extras():
    """A pair without an envelope and a dead pair (a profile row all -inf) under a band, to put beside the four."""
    em = mark_machine()
    x0, P0 = pair_input(np.random.RandomState(4490), em, 30, 25)
    x1, P1 = pair_input(np.random.RandomState(4491), em, 20, 20)
    P1 = P1.copy(); P1[7] = -np.inf
    return (x0, P0, None), (x1, P1, Envelope.band(20, 20, 3))


# ---- i mod M: slopes where i advances several positions per row, or none ------------------------------------------------------------
SLOPE_CASES = ((200, 40, 6), (40, 200, 2))


def slope_machine():
    return pair_machine(8, 88, True, 2, 3)


def slope_case(I, L, w):
    em = slope_machine()
    x, P = pair_input(np.random.RandomState(8800 + I), em, I, L)
    return x, P, Envelope.band(I, L, w)


def area_case():
    """(x, P, env): the path-area envelope (width 3) of a random alignment of 70 input and 50 output symbols."""
    em = slope_machine()
    rng = np.random.RandomState(8899)
    x, P = pair_input(rng, em, 70, 50)
    return x, P, Envelope.pathAreaEnvelope(random_alignment(rng, 70, 50), 3)


# ---- many workgroups with rings in scratch --------------------------------------------------------------------------------------------
PACK = (300, 24, 60, 20)          # S, pairs, I = L, w: M = 21, a ring of 48 * 21 * 300 = 302 400 bytes


def pack_case():
    S, n, I, w = PACK
    em = pair_machine(S, 301, True, 2, 3)
    return em, [pair_input(np.random.RandomState(3010 + k), em, I, I) for k in range(n)], Envelope.band(I, I, w)


# ---- the compact pool -------------------------------------------------------------------------------------------------------------------
POOL = (65, 300, 4)               # S, I = L, w


def pool_case():
    S, I, w = POOL
    em = pair_machine(S, 365, True, 2, 3)
    return em, [pair_input(np.random.RandomState(3650 + k), em, I, I) for k in range(3)], Envelope.band(I, I, w)


# ---- counts past the LDS table, ties, the token cross-check ----------------------------------------------------------------------------
def big_counts_env_case():
    """big_counts_case's machine (11 204 transitions) and pairs, each under band(w = 2)."""
    em, pairs, dead = ph.big_counts_case()
    return em, [(x, P, Envelope.band(len(x), len(P), 2)) for x, P in pairs + [dead]]


def tie_env_pairs():
    """tie_pairs under band(w = 1); the shapes whose slope such a band cannot bridge are left out."""
    out = []
    for x, P in ph.tie_pairs():
        try:
            out.append((x, P, Envelope.band(len(x), len(P), 1)))
        except MachineError:
            pass
    return out


TIE_KINDS = (("blank", "match"), ("stay", "ins"), ("ins", "silent"))


def onehot_case():
    """(em, x, y, P, env): pair_machine(40) at (30, 30) under band(w = 3); P is the one-hot profile of the token string y with a
    -inf blank, so that the pair (x, P) is the token pair (x, y)."""
    em = pair_machine(40, 41, True, 2, 3)
    rng = np.random.RandomState(4141)
    x = rng.randint(1, em.nInTok + 1, size=30).astype(np.int32)
    y = rng.randint(1, em.nOutTok + 1, size=30).astype(np.int32)
    P = np.full((30, em.nOutTok + 1), -np.inf)
    P[np.arange(30), y] = 0.0
    return em, x, y, P, Envelope.band(30, 30, 3)


# ---- the device against the restatement -----------------------------------------------------------------------------------------------
WORST = {}


def check_env_batch(em, triples, fill=False, live=None):
    """Everything the device computes for the (x, P, env) of one machine, in one batch, against the restatement under env."""
    from machineboss_amd import capi
    from machineboss_amd.profile import PairProfileDP
    dp = PairProfileDP(em)
    refs = [env_reference(dp, x, P, env, cells=fill) for x, P, env in triples]
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfilePairs(dm, [t[0] for t in triples], [t[1] for t in triples])
    try:
        dev.set_envelopes([t[2] for t in triples])
        want = np.array([r["ll"] for r in refs])
        for flags in (capi.MB_ROLLING, capi.MB_MATERIALISE):
            got = dev.forward(flags)
            ph.note("forward", got, want, WORST)
            assert logs_close(got, want), (flags, got, want)
        wv = np.array([r["v"] for r in refs])
        assert logs_close(dev.viterbi(paths=False)[0], wv, 1e-12)
        v, off, edges, rows = dev.viterbi()
        assert logs_close(v, wv, 1e-12), (v, wv)
        for k, r in enumerate(refs):
            assert np.array_equal(edges[off[k]:off[k + 1]], r["path"][0]) and np.array_equal(rows[off[k]:off[k + 1]], r["path"][1]), k
        c, s, ll = dev.counts()
        wc = np.sum([r["counts"] for r in refs], axis=0)
        ph.note_counts(c, wc, WORST)
        assert counts_close(c, wc), np.abs(c - wc).max()
        assert logs_close(ll, want)
        if fill:
            for (x, P, env), r in zip(triples, refs):
                outside = ~mask(env, len(x)) if env is not None else np.zeros((len(x) + 1, len(P) + 1), bool)
                for mode, key, tol in ((capi.MB_FORWARD, "fwd", ph.LOG_TOL), (capi.MB_BACKWARD, "bwd", ph.LOG_TOL), (capi.MB_VITERBI, "vit", 1e-12)):
                    got = capi.profile_pair_fill(dm, mode, x, P, env)
                    ph.note("cells", got, r[key], WORST)
                    assert logs_close(got, r[key], tol), (mode, len(x), len(P))
                    assert np.all(got[outside] == -math.inf)
        if live is not None:
            live += list(want > -math.inf)
    finally:
        dev.close(); dm.close()
    return refs
