"""Machines, inputs and bounds of the two-tape profile tests (test_profile_pair_host.py, test_profile_pair_gpu.py; not a test module)."""
import math

import numpy as np

from prefixhelpers import machine_edges, machine_from_edges, populated_machine
from profileprefixhelpers import random_profile

LOG_TOL = 1e-9          # log values: relative to max(1, |value|), -inf matching exactly
COUNT_REL = 1e-6        # counts >= 1e-3: relative
COUNT_ABS = 1e-9        # counts below 1e-3: COUNT_ABS + COUNT_REL * count, absolute


def pair_machine(S, seed, levels, nIn, nOut):
    """populated_machine(S, seed, levels, nIn, nOut) plus, on each of start -> start, start -> end and end -> end, one input-only
    edge per input symbol, one output-only edge per output symbol and one matching edge per input symbol.  populated_machine alone
    sends its edges to random states, so a lattice of a handful of cells -- (I, L) = (3, 0), (1, 1), (7, 2) -- cannot reach the end
    state of a machine without silent levels and scores -inf whatever the seed; with these edges every shape but (0, 0) without
    levels (where nothing can move at all) has a finite likelihood, and the liveness conditions of the suites can hold.  No silent
    edge is added: a machine without levels stays without."""
    em = populated_machine(S, seed, levels, nIn, nOut)
    lw = float(np.log(0.15))
    extra = []
    for s, d in sorted({(0, 0), (0, S - 1), (S - 1, S - 1)}):
        extra += [(s, d, a, 0, lw) for a in range(1, nIn + 1)]
        extra += [(s, d, 0, o, lw) for o in range(1, nOut + 1)]
        extra += [(s, d, a, a % nOut + 1, lw) for a in range(1, nIn + 1)]
    return machine_from_edges(S, nIn, nOut, machine_edges(em) + extra)


def pair_input(rng, em, I, L, pZero=0.2):
    """(x, P): I input tokens and a random profile of L rows with a positive blank."""
    x = rng.randint(1, em.nInTok + 1, size=I).astype(np.int32) if I else np.zeros(0, np.int32)
    return x, random_profile(rng, L, em.nOutTok, pZero)


def logs_close(got, want, tol=LOG_TOL):
    """Every entry within tol * max(1, |want|), -inf (and only -inf) matching -inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or np.isnan(got).any():
        return False
    dead = want == -math.inf
    if not np.array_equal(got == -math.inf, dead):
        return False
    return bool(np.all(np.abs(got[~dead] - want[~dead]) <= tol * np.maximum(1.0, np.abs(want[~dead]))))


def log_dev(got, want):
    """The worst deviation relative to max(1, |want|) over the finite entries."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    fin = want > -math.inf
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])), initial=0.0))


def counts_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    big = want >= 1e-3
    return bool(np.all(np.abs(got[big] - want[big]) <= COUNT_REL * want[big]) and
                np.all(np.abs(got[~big] - want[~big]) <= COUNT_ABS + COUNT_REL * want[~big]))


# ---- the GPU suite (test_profile_pair_gpu.py; held to its liveness conditions without a GPU by
# test_profile_pair_host.py::test_pair_suite_inputs_are_live) ---------------------------------------------------------------------
SUITE_STATES = (1, 2, 8, 65, 300)
SUITE_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (2, 7), (7, 2), (9, 9))
SUITE_ALPHABETS = ((1, 1), (2, 3), (3, 2))
SUITE_CASES = [(S, nIn, nOut) for S in SUITE_STATES for nIn, nOut in SUITE_ALPHABETS]


def suite_case(S, nIn, nOut):
    """[(em, x, P)] of one case: the machine with silent levels (S >= 2) and without, each at every shape of SUITE_SHAPES."""
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = pair_machine(S, 100 + S, levels, nIn, nOut)
        for I, L in SUITE_SHAPES:
            out.append((em,) + pair_input(np.random.RandomState(1000 * S + 10 * I + L), em, I, L))
    return out


def wide_case():
    """A diagonal with more items than lanes and a ring that wraps many times: S = 40, I = L = 40."""
    em = pair_machine(40, 41, True, 2, 3)
    return (em,) + pair_input(np.random.RandomState(41), em, 40, 40)


RING_BYTES_PER_STATE = 48 * 4      # 3 diagonals x 2 layers x (min(I, L) + 1 = 4) cells x 8 bytes, at I = L = 3
# the largest S whose ring fits the LDS limit and the first beyond it (LDS, then global scratch), around 160 KiB and around the
# 64 KiB from which the kernel has to be told; and the same marks for a ring of 24 * 4 * S bytes, a single layer
LDS_STATES = sorted({lim // per + k for lim in (160 * 1024, 64 * 1024) for per in (RING_BYTES_PER_STATE, 24 * 4) for k in (0, 1)})


def lds_case(S):
    em = pair_machine(S, S, False, 2, 2)
    return (em,) + pair_input(np.random.RandomState(S), em, 3, 3, pZero=0.0)


def ragged_case():
    """Ten pairs with I = 0..9 and L = 9..0 on one machine: S = 40 with levels."""
    em = pair_machine(40, 7, True, 3, 5)
    return em, [pair_input(np.random.RandomState(50 + I), em, I, 9 - I) for I in range(10)]


CHUNK_SHAPE = (300, 24, 12, 12)      # S, pairs, I, L


def chunk_case():
    S, n, I, L = CHUNK_SHAPE
    em = pair_machine(S, 300, True, 2, 3)
    return em, [pair_input(np.random.RandomState(70 + k), em, I, L) for k in range(n)]


def chained_case():
    """S = 65, (nIn, nOut) = (3, 2), I = 5, L = 9, four pairs: against the chained prefix fills."""
    em = pair_machine(65, 165, True, 3, 2)
    return em, [pair_input(np.random.RandomState(90 + k), em, 5, 9) for k in range(4)]


def sparse_case():
    """A third of the profile's weights -inf, blanks included."""
    em = pair_machine(40, 11, True, 2, 3)
    rng = np.random.RandomState(11)
    pairs = []
    for k in range(6):
        x = rng.randint(1, 3, size=6).astype(np.int32)
        w = rng.uniform(0.05, 1.0, (8, 4))
        with np.errstate(divide="ignore"):
            pairs.append((x, np.log(np.where(rng.rand(8, 4) < 1.0 / 3.0, 0.0, w))))
    return em, pairs
