"""Envelopes, inputs and the device-against-restatement comparison of the tests of the two-tape profile sweeps under an envelope
(test_profile_pair_env_host.py, test_profile_pair_env_gpu.py; not a test module).  The machines, inputs and bounds are those of
pairprofilehelpers; the reference is profile.PairProfileDP(env=...)."""
import math

import numpy as np

import pairprofilehelpers as ph
from mergehelpers import greedy_chunks
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


# ---- a call that mixes plain and enveloped pairs (test_profile_pair_mixed_gpu.py; held to its conditions without a GPU by
# test_profile_pair_env_host.py) ---------------------------------------------------------------------------------------------------------
# pair_profile_descs (mb_profile_api.hip) launches a chunk's plain pairs first and its enveloped pairs second and writes the per-pair outputs
# in that order: slot = rank among the chunk's plain pairs, or nPlain + rank among its enveloped ones.
MIXED_STATES = (8, 65)
MIXED_SEED = {8: 208, 65: 265}
# (I, L, envelope or None, dead): enveloped first and plain last, so that slot order differs from pair order at both ends
MIXED_SPEC = ((9, 9, "band0", False), (20, 14, None, False), (0, 0, "full", False), (0, 0, None, False), (18, 14, None, False),
              (5, 6, None, True), (0, 6, None, False), (20, 14, "full", False), (12, 12, "band1", False), (6, 6, "stairs", False),
              (8, 7, "band2", True), (6, 0, "full", False), (19, 13, None, False), (20, 14, "area", False), (0, 5, "full", False),
              (4, 0, None, False), (11, 8, "full", False), (10, 13, "band2", False), (9, 4, None, False), (3, 8, None, False))
MIXED_DEAD = tuple(k for k, s in enumerate(MIXED_SPEC) if s[3])


def named_envelope(kind, rng, I, L):
    if kind is None:
        return None
    if kind == "full":
        return full(I, L)
    if kind == "stairs":
        return staircase(I, L)
    if kind == "area":
        return Envelope.pathAreaEnvelope(random_alignment(rng, I, L), 2)
    return Envelope.band(I, L, int(kind[4:]))


def mixed_case(S):
    """(em, [(x, P, env or None)]): MIXED_SPEC on the machine of S states with silent levels; a dead pair has its middle row all -inf."""
    em = pair_machine(S, MIXED_SEED[S], True, 2, 3)
    triples = []
    for k, (I, L, kind, dead) in enumerate(MIXED_SPEC):
        rng = np.random.RandomState(7000 * S + 100 * k + 10 * I + L)
        x, P = pair_input(rng, em, I, L)
        if dead:
            P = P.copy(); P[L // 2] = -np.inf
        triples.append((x, P, named_envelope(kind, rng, I, L)))
    return em, triples


def mixed_states(triples):
    """The envelope states of section 4, in order: all plain, the mix, every pair enveloped (full for the plain ones), the mix with
    plain and enveloped swapped (a formerly plain pair under band(3), or the full envelope where its slope needs more), none."""
    envs = [t[2] for t in triples]
    swapped = []
    for x, P, env in triples:
        if env is not None:
            swapped.append(None)
            continue
        try:
            swapped.append(Envelope.band(len(x), len(P), 3))
        except MachineError:
            swapped.append(full(len(x), len(P)))
    return [("plain", [None] * len(envs)), ("mixed", envs), ("all", [e if e is not None else full(len(x), len(P)) for (x, P, _), e in zip(triples, envs)]),
            ("swapped", swapped), ("cleared", None)]


def slots(envs):
    """slot[k] of PairProfPlan for one chunk whose pairs have these envelopes."""
    nPlain = sum(e is None for e in envs)
    out, p, e = [], 0, 0
    for env in envs:
        if env is None:
            out.append(p); p += 1
        else:
            out.append(nPlain + e); e += 1
    return out


LDS_MAX = 160 * 1024
CALLS = ("forward", "viterbi", "counts", "posteriors", "rolling")


def silent_levels(em):
    """nLevF - 1 of the device's machine: the silent levels of the restatement."""
    from machineboss_amd.profile import PairProfileDP
    return len(PairProfileDP(em).fLevels)


def lattice_doubles(S, x, P, env):
    """pp_cells: the rectangle's two layers, or those of the compact lattice of the envelope."""
    return 2 * S * (n_cells(env) if env is not None else (len(x) + 1) * (len(P) + 1))


def path_bound(nLevels, I, L):
    """profile_pair_path_bound with nLevels = nLevF - 1."""
    return I + L + (I + L + 1) * nLevels


def scratch_ring_bytes(S, x, P, env):
    """pp_ring_bytes of the rolling sweeps: 0 where the ring lies in LDS."""
    b = 48 * S * (diag_max(env) if env is not None else min(len(x), len(P)) + 1)
    return 0 if b <= LDS_MAX else b


def call_bytes(call, em, triples, nLevels=None):
    """What each call of mb_profile_api.hip tells lattice_chunks a pair costs: the lattice for materialised Forward, the traceback slot on
    top of it for Viterbi with paths, two lattices for counts, the pair's bins beside them for row posteriors, the scratch ring
    alone for the rolling sweeps."""
    S, C = em.nStates, em.nOutTok + 1
    nLevels = silent_levels(em) if nLevels is None and call == "viterbi" else nLevels
    out = []
    for x, P, env in triples:
        cells = 8 * lattice_doubles(S, x, P, env)
        out.append({"forward": cells, "viterbi": cells + 8 * path_bound(nLevels or 0, len(x), len(P)), "counts": 2 * cells,
                    "posteriors": 2 * cells + 8 * len(P) * C, "rolling": scratch_ring_bytes(S, x, P, env)}[call])
    return out


def chunk_kinds(chunks, envs):
    """Per chunk "P" (plain pairs only), "E" (enveloped only), "PE" (mixed, its first pair plain) or "EP"."""
    out = []
    for p0, p1 in chunks:
        kinds = ["E" if e is not None else "P" for e in envs[p0:p1]]
        out.append(kinds[0] if len(set(kinds)) == 1 else kinds[0] + ("E" if kinds[0] == "P" else "P"))
    return out


def chunk_launches(chunks, envs):
    """PairProfPlan::launches summed: two for a chunk that holds both kinds."""
    return sum(2 if len(k) == 2 else 1 for k in chunk_kinds(chunks, envs))


# The budget of the chunked calls of the mixed batch, in units of the largest pair's bytes under that call (at or above 1.2, below
# which a pair alone may be refused): five chunks for each of the four calls at S = 8 and at S = 65 -- pairs 0-3 (mixed, the first
# enveloped), 4-6 (plain), 7-11 (enveloped), 12-13 (mixed, the first plain), 14-19 (mixed, the first enveloped)
MIXED_BUDGET_FACTOR = 1.8
MIXED_CHUNKS = [(0, 4), (4, 7), (7, 12), (12, 14), (14, 20)]
MIXED_CHUNK_KINDS = ["EP", "P", "E", "PE", "EP"]


def mixed_budget(call, em, triples):
    return int(MIXED_BUDGET_FACTOR * max(call_bytes(call, em, triples)))


# ---- rolling sweeps in chunks: scratch rings at S = 300 ----------------------------------------------------------------------------
ROLL_SHAPE = (12, 14)                    # a ring of 48 * 13 * 300 = 187 200 bytes, plain or under band(12) (M = 13): past 160 KiB
ROLL_ORDER = "EpPPeEEEePPp"              # E, P: (12, 14) with a scratch ring; e, p: (3, 3), ring in LDS, no bytes: they ride along
ROLL_CHUNKS = ("EP", "PE", "EE", "PP")   # of the ring-bearing pairs, under a budget of 2.5 rings


def roll_case():
    """(em, triples): pack_case's machine; eight pairs at (12, 14) in the order E P P E E E P P and two small pairs of each kind."""
    em = pair_machine(PACK[0], 301, True, 2, 3)
    triples = []
    for k, c in enumerate(ROLL_ORDER):
        I, L = ROLL_SHAPE if c in "EP" else (3, 3)
        x, P = pair_input(np.random.RandomState(3300 + k), em, I, L)
        triples.append((x, P, Envelope.band(I, L, 12 if c == "E" else 1) if c in "Ee" else None))
    return em, triples


ROLL_BUDGET = 5 * 187200 // 2


# ---- the traceback past one block of 64 lanes, in each of the two launches of a call ----------------------------------------------------
SEAM_PLAIN, SEAM_ENV = 129, 65
SEAM_DEAD_PLAIN, SEAM_DEAD_ENV = (63, 64, 128), (63, 64)      # by slot within the launch
SEAM_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 4), (4, 2), (4, 4), (3, 3))


def seam_case():
    """(em, triples): 194 pairs at S = 8 with levels, two plain pairs then an enveloped one, 64 times, then one of each; the
    envelopes in turn from envelopes() of the shape; dead pairs at the seams of both launches' blocks."""
    em = pair_machine(8, 208, True, 2, 3)
    kinds = "PPE" * 64 + "EP"
    triples, nP, nE = [], 0, 0
    for k, c in enumerate(kinds):
        I, L = SEAM_SHAPES[k % len(SEAM_SHAPES)]
        dead = (nP in SEAM_DEAD_PLAIN) if c == "P" else (nE in SEAM_DEAD_ENV)
        if dead:
            I, L = 3, 4
        rng = np.random.RandomState(9100 + k)
        x, P = pair_input(rng, em, I, L)
        if dead:
            P = P.copy(); P[1] = -np.inf
        env = None
        if c == "E":
            es = envelopes(rng, I, L)
            env = es[nE % len(es)][1]
        triples.append((x, P, env))
        nP += c == "P"; nE += c == "E"
    return em, triples


def seam_prefix(triples, n):
    """The indices of the pairs whose slot within their launch is below n."""
    out, nP, nE = [], 0, 0
    for k, t in enumerate(triples):
        if (nE if t[2] is not None else nP) < n:
            out.append(k)
        nP += t[2] is None; nE += t[2] is not None
    return out


# ---- row posteriors past 1 024 row blocks ---------------------------------------------------------------------------------------------------
WRAP_SHAPE = (1, 1100)
WRAP_GROUPS = 1024                       # the cap of mb_profile_pairs_row_posteriors on a pair's workgroups


def wrap_case():
    """(em, x, P, Pdead): S = 2 with levels, nOut = 3 (C = 4), one input symbol against 1 100 rows; the dead profile has row 1 050,
    past the first pass of the row-block loop, all -inf."""
    em = pair_machine(2, 222, True, 2, 3)
    x, P = pair_input(np.random.RandomState(1100), em, *WRAP_SHAPE)
    Pd = P.copy(); Pd[1050] = -np.inf
    return em, x, P, Pd
