"""Cases, seeds, the exact enumeration and the replay of the tests of the posterior path samples of the pair profile sweeps
(test_profile_pair_sample_host.py, test_profile_pair_sample_gpu.py; not a test module).  The reference is
profile.PairProfileDP.samplePaths, called per pair with the pair's own index; the machines and inputs are those of pairprofilehelpers
and pairenvhelpers.

Equality of sampled paths between the device and the yardstick needs every uniform to lie clear of every partial sum of its
decision: MARGIN, held for every case below by test_profile_pair_sample_host.py::test_gpu_suite_inputs_are_live.  A case whose seed
fails that takes the next seed here, before any GPU run."""
import math

import numpy as np

import pairenvhelpers as eh
import pairprofilehelpers as ph
from prefixhelpers import machine_from_edges
from machineboss_amd import dp as mbdp
from machineboss_amd.machine import Machine, MachineState, MachineTransition
from machineboss_amd.profile import PairProfileDP
from machineboss_amd.seqpair import Envelope

LOG_TOL = 1e-9          # logq and likelihoods: relative to max(1, |value|), -inf matching exactly
MARGIN = 1e-9           # the least distance of a uniform from a partial sum the GPU suite's inputs may have


# ---- the cases of the GPU module: name -> (nSamples of the yardstick, seed, dead pairs expected, builder of [(em, [(x, P, env)])]) ------
BASIC_STATES = (1, 2, 8, 65)
BASIC_SHAPES = ((0, 0), (0, 3), (3, 0), (1, 1), (4, 5), (9, 9))
BASIC_SAMPLES = (1, 3, 64, 65, 130)      # one lane, a partial block, a block exactly, a pair's samples across two blocks, several blocks
ENV_SAMPLES = 5
MIXED_SAMPLES = 3
RAGGED_SAMPLES = 7
LONG_SAMPLES, LONG_CHECKED = 256, 8
STAT_SAMPLES = 4096
HOT_SAMPLES = 4


def _basic(S):
    out = []
    for levels in ((True, False) if S >= 2 else (False,)):
        em = ph.pair_machine(S, 100 + S, levels, 2, 3)
        out.append((em, [ph.pair_input(np.random.RandomState(1000 * S + 10 * I + L), em, I, L) + (None,) for I, L in BASIC_SHAPES]))
    return out


def _ragged():
    em, pairs = ph.ragged_case()
    return [(em, [(x, P, None) for x, P in pairs])]


def _envelopes():
    """cell_case(8), one batch per machine; the kinds ride along in ENV_KINDS_OF."""
    groups = {}
    for em, x, P, kind, env in eh.cell_case(8):
        groups.setdefault(id(em), (em, []))[1].append((x, P, env, kind))
    return [(em, [t[:3] for t in ts]) for em, ts in groups.values()], [[t[3] for t in ts] for _, ts in groups.values()]


def env_kinds():
    """Per machine of the "envelopes" case, the kind of each pair's envelope."""
    return _envelopes()[1]


def _mixed():
    return [eh.mixed_case(8)]


def _chain():
    em, pairs = ph.chain_case()
    return [(em, [(x, P, None) for x, P in pairs])]


def hot_machine():
    """One path per pair: on the start state a match per input symbol 1, 2 (writing the same output symbol) and an input-only edge
    on symbol 3, then one silent edge to the end state."""
    edges = [(0, 0, 1, 1, math.log(0.3)), (0, 0, 2, 2, math.log(0.2)), (0, 0, 3, 0, math.log(0.4)), (0, 1, 0, 0, math.log(0.1))]
    return machine_from_edges(2, 3, 2, edges)


def _hot():
    """x over {1, 2, 3} against the one-hot profile (a -inf blank) of x without its 3s; a pair without rows and one without input."""
    em = hot_machine()
    rng = np.random.RandomState(77)
    triples = []
    for I in (12, 5, 3, 0):
        x = rng.randint(1, 4, size=I).astype(np.int32) if I != 3 else np.full(3, 3, np.int32)
        y = x[x != 3]
        P = np.full((len(y), 3), -np.inf)
        P[np.arange(len(y)), y] = 0.0
        triples.append((x, P, None))
    return [(em, triples)]


def _long():
    em = eh.mark_machine()
    x, P = ph.pair_input(np.random.RandomState(4406), em, eh.MARK_LEN, eh.MARK_LEN)
    return [(em, [(x, P, Envelope.band(eh.MARK_LEN, eh.MARK_LEN, 6))])]


def _stat():
    em = ph.pair_machine(3, 103, True, 2, 3)
    x, P = ph.pair_input(np.random.RandomState(3303), em, 3, 3)
    return [(em, [(x, P, None)])]


# name: (samples the yardstick draws, seed, dead pairs expected, builder)
CASES = {
    "basic1": (130, 11, False, lambda: _basic(1)),
    "basic2": (130, 12, True, lambda: _basic(2)),
    "basic8": (130, 18, True, lambda: _basic(8)),
    "basic65": (130, 165, True, lambda: _basic(65)),
    "ragged": (RAGGED_SAMPLES, 7, False, _ragged),
    "envelopes": (ENV_SAMPLES, 5, True, lambda: _envelopes()[0]),
    "mixed": (MIXED_SAMPLES, 3, True, _mixed),
    "chain": (3, 9, False, _chain),
    "hot": (HOT_SAMPLES, 4, False, _hot),
    "long": (LONG_CHECKED, 120, False, _long),
}
STAT_SEED = 4096
SEED_B = 991          # a second seed for the mixed batch: at least one path differs

BOSS_SAMPLES, BOSS_SEED, BOSS_BANDS = 6, 21, (None, 2)


def boss_case():
    """(machine, profile, inputs) of the boss.sampleProfilePairs tests: a loop that matches, deletes and inserts, then ends; the third
    input cannot be tokenised, the last is empty."""
    from machineboss_amd.profile import Profile
    j = {"state": [{"id": "S", "trans": [{"to": "S", "in": "a", "out": "x", "weight": 0.4}, {"to": "S", "in": "a", "weight": 0.1},
                                         {"to": "S", "out": "y", "weight": 0.2}, {"to": "E", "weight": 0.3}]}, {"id": "E", "trans": []}]}
    prof = Profile(["x", "y"], [[0.5, 0.25, 0.25], [0.1, 0.6, 0.3], [0.3, 0.3, 0.4]])
    return Machine.fromJson(j), prof, [["a"], ["a", "a", "a"], ["z"], []]


_BUILT, _REFS = {}, {}


def case(name):
    """(nSamples, seed, [(em, triples)]) of a case, built once."""
    if name not in _BUILT:
        n, seed, _dead, build = CASES[name]
        _BUILT[name] = (n, seed, build())
    return _BUILT[name]


def reference(name, margins=None):
    """[[(loglike, [(edges, rows, logq)] * nSamples) per pair] per machine]: the yardstick's samples of a case, pair k of a batch under
    its own index k.  Computed once and shared; never changed."""
    if name not in _REFS:
        n, seed, groups = case(name)
        mg = []
        _REFS[name] = ([[PairProfileDP(em).samplePaths(x, P, n, seed=seed, pair=k, env=env, margins=mg) for k, (x, P, env) in enumerate(triples)]
                        for em, triples in groups], mg)
    if margins is not None:
        margins += _REFS[name][1]
    return _REFS[name][0]


def log_close(got, want, tol=LOG_TOL):
    return ph.logs_close(got, want, tol)


# ---- replay -------------------------------------------------------------------------------------------------------------------------------
def machine_of(em):
    """A Machine with em's transitions, in em's order within each state: what dp.edgesToPath resolves (state, transition index) in."""
    m = Machine()
    for s in range(em.nStates):
        es = sorted(np.nonzero(em.src == s)[0], key=lambda e: int(em.transIndex[e]))
        m.state.append(MachineState(name=s, trans=[MachineTransition(int(em.dst[e]), em.inputTokenizer.tok2sym[int(em.inTok[e])],
                                                                     em.outputTokenizer.tok2sym[int(em.outTok[e])], float(np.exp(em.logWeight[e])))
                                                   for e in es]))
    return m


def replay(em, m, x, P, edges, rows):
    """The path through dp.edgesToPath: from the start state to the end state, edge by edge, consuming exactly x and, with the blanks
    between its emissions, the L rows in order.  Returns the path's log weight: its edges, the profile entries of its emissions and
    the blank of every other row."""
    path = mbdp.edgesToPath(em, m, edges)
    assert len(path.steps) == len(path.trans) == len(edges) == len(rows)
    state, pos, xs, w, emitted = 0, 0, [], 0.0, set()
    for (s, ti), t, e, r in zip(path.steps, path.trans, edges, rows):
        assert s == state == int(em.src[e]) and t.dest == int(em.dst[e])
        assert int(r) >= pos, (r, pos)
        if t.inp != "":
            xs.append(em.inputTokenizer.sym2tok[t.inp])
        w += float(em.logWeight[e])
        if t.out != "":
            assert int(r) < len(P)
            w += float(P[int(r)][em.outputTokenizer.sym2tok[t.out]])
            emitted.add(int(r)); pos = int(r) + 1
        else:
            pos = int(r)
        state = t.dest
    assert state == em.nStates - 1 and pos <= len(P) and xs == [int(v) for v in x], (state, pos, xs)
    return w + sum(float(P[r][0]) for r in range(len(P)) if r not in emitted)


# ---- the exact enumeration ----------------------------------------------------------------------------------------------------------------
class TooMany(Exception):
    pass


def enumerate_paths(dp, x, P, env=None, budget=200000):
    """Every path from W[I][L][S-1] back to N[0][0][0] one by one, walking sampleCandidates() backwards over forward(x, P, env=env):
    {(edges, rows): (product of the choice probabilities, log weight of the path's own terms)}.  Nothing is shared between paths.
    The log weight is summed from the edges, the profile entries and the blanks alone (not from the lattice)."""
    x, P = dp._checkPair(x, P)
    ll, N, W = dp.forward(x, P, env=env) if env is not None else dp.forward(x, P)
    inside = dp.envelopeRows(env, len(x), len(P))
    if inside is not None:
        inside = [set(rs) for rs in inside]
    out, seen = {}, [0]
    ew = dp.em.logWeight

    def walk(i, r, q, layer, prob, weight, edges, rows):
        seen[0] += 1
        if seen[0] > budget:
            raise TooMany()
        if layer == 0 and r == 0:
            if i == 0 and q == 0:
                key = (tuple(edges[::-1]), tuple(rows[::-1]))
                assert key not in out
                out[key] = (prob, weight)
            return
        cur = float(W[i, r, q] if layer == 1 else N[i, r, q])
        for kind, e, s, term in dp.sampleCandidates(x, P, N, W, inside, i, r, q, layer):
            if not term > -math.inf:
                continue
            p = prob * math.exp(term - cur)
            if kind == "stay":
                walk(i, r, q, 0, p, weight, edges, rows)
            elif kind == "blank":
                walk(i, r - 1, q, 0, p, weight + float(P[r - 1][0]), edges, rows)
            elif kind in ("ins", "silent"):
                walk(i - (kind == "ins"), r, s, 1, p, weight + float(ew[e]), edges + [e], rows + [r])
            else:
                o = int(dp.em.outTok[e])
                walk(i - (kind == "match"), r - 1, s, 1, p, (weight + float(ew[e])) + float(P[r - 1][o]), edges + [e], rows + [r - 1])
    if ll > -math.inf:
        walk(len(x), len(P), dp.S - 1, 1, 1.0, 0.0, [], [])
    return ll, out


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def usage(nTrans, paths):
    """[nSamples, nTrans]: how often each sample used each transition."""
    u = np.zeros((len(paths), nTrans))
    for j, e in enumerate(paths):
        np.add.at(u[j], np.asarray(e, np.int64), 1.0)
    return u


def usage_within_bound(u, counts, emitting, blankMass, L):
    """The bound of the statistics case: the mean usage of every transition whose expected count is at least 1e-3 within 5 standard
    errors (from the sample variance) of it, and the mean number of emitting edges plus the blank mass within 5 standard errors of L.
    Returns the list of violations."""
    n = len(u)
    bad = []
    mean, se = u.mean(axis=0), u.std(axis=0, ddof=1) / math.sqrt(n)
    for t in np.nonzero(counts >= 1e-3)[0]:
        if not abs(mean[t] - counts[t]) <= 5.0 * se[t]:
            bad.append((int(t), float(mean[t]), float(counts[t]), float(se[t])))
    em_ = u[:, emitting].sum(axis=1)
    if not abs(em_.mean() + blankMass - L) <= 5.0 * em_.std(ddof=1) / math.sqrt(n):
        bad.append(("rows", float(em_.mean()), float(blankMass), L))
    return bad


def sample_call_bytes(em, triples, nSamples):
    """What mb_profile_pairs_sample tells the chunk planner a pair costs: its lattice, and per sample a path slot of edges and rows, a
    length and a log probability."""
    nLev = eh.silent_levels(em)
    return [8 * eh.lattice_doubles(em.nStates, x, P, env) + nSamples * (8 * eh.path_bound(nLev, len(x), len(P)) + 16) for x, P, env in triples]
