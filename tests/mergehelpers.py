"""Shared helpers of the merged (CTC) profile tests (test_profile_merge_host.py, test_profile_merge_gpu.py,
test_profile_merge_edges_gpu.py): random CSV profiles with duplicated and foreign header symbols, the weight of a merged Viterbi path,
the device-against-restatement comparison, and the input builders of the edge suite."""
import numpy as np

from machineboss_amd import capi
from machineboss_amd.profile import MergedProfileDP, Profile
from profhelpers import _close


def random_merge_profile(rng, em, L, quantised=False, zeros=0.1):
    """A CSV profile whose header holds every output symbol of em, the first of them twice, and a foreign symbol, shuffled; rows
    of uniform weights (weights 1, 1/2, 1/4 if quantised), a tenth of them zero, a third of the rows without the blank and the last
    symbol column.  (Up to 40 rows must each leave the machine a blank, a repeat or an emission: with more zeros most cases are -inf.)"""
    syms = list(em.outputTokenizer.tok2sym[1:])
    header = syms + ["zz"] + syms[:1]
    rng.shuffle(header)
    rows = []
    for _ in range(L):
        v = np.array([1.0, .5, .25])[rng.randint(0, 3, len(header) + 1)] if quantised else rng.uniform(0.05, 1.0, len(header) + 1)
        v[rng.rand(len(v)) < zeros] = 0.0
        rows.append([float(np.float32(x)) for x in v[:rng.randint(len(header) - 1, len(header) + 2)]])
    return Profile(header, rows)


def merged_rows(rng, nCols, L, zeros=0.2):
    P = np.log(rng.uniform(0.02, 1.0, (L, nCols + 1)))
    P[rng.rand(L, nCols + 1) < zeros] = -np.inf
    return P


def quantised_rows(rng, nCols, L, p_inf=0.15):
    """[L, nCols + 1] log weights 0, log 1/2, log 1/4 and -inf: the blank, the repeat and the symbol columns often tie."""
    P = np.log(np.array([1.0, .5, .25]))[rng.randint(0, 3, (L, nCols + 1))]
    P[rng.rand(L, nCols + 1) < p_inf] = -np.inf
    return P


def merged_path_weight(em, P, colTok, edges, rows):
    """The weight of a merged Viterbi path: its edges' weights plus the best reading of the rows -- an emitting edge of token o at
    row r takes a column of o other than the last column taken; a row with no edge is a blank or a repeat of the last column."""
    colTok = np.asarray(colTok)
    PL = len(colTok) + 1
    emit = {int(r): int(em.outTok[e]) for e, r in zip(edges, rows) if em.outTok[e]}
    best = np.full(PL, -np.inf)
    best[0] = 0.0
    for r in range(len(P)):
        nxt = np.full(PL, -np.inf)
        if r in emit:
            for c in range(1, PL):
                if colTok[c - 1] == emit[r]:
                    nxt[c] = max(best[k] for k in range(PL) if k != c) + P[r, c]
        else:
            nxt[0] = best.max() + P[r, 0]
            nxt[1:] = best[1:] + P[r, 1:]
        best = nxt
    return float(best.max()) + float(sum(em.logWeight[e] for e in edges))


def check_all_merged(em, colTok, profs, fill=True):
    """Every device sweep of the merged `profs` against MergedProfileDP, in the manner of profhelpers._check_all: rolling and
    materialised Forward (and the same bits from both), Viterbi scores and paths exactly with and without paths, counts (exactly 0
    on transitions that read input, the same bits from two calls), and the three lattices of the longest profile."""
    dm = capi.DeviceMachine(em)
    dp = MergedProfileDP(em, colTok)
    dev = capi.DeviceProfiles(dm, profs, colTok)
    ref = [dp.forward(P) for P in profs]
    want = np.array([r[0] for r in ref])
    fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
    assert _close(fr, want, 1e-9), (fr, want)
    assert _close(fm, want, 1e-9), (fm, want)
    assert np.array_equal(fr, fm)
    v, off, edges, rows = dev.viterbi()
    v0, _, _, _ = dev.viterbi(paths=False)
    for k, P in enumerate(profs):
        rv, re_, rr = dp.viterbi(P)
        assert v[k] == rv and v0[k] == rv, (k, v[k], v0[k], rv)
        assert np.array_equal(edges[off[k]:off[k + 1]], re_) and np.array_equal(rows[off[k]:off[k + 1]], rr), k
    c, s, ll = dev.counts()
    rc = np.zeros(em.nTransitions)
    for P in profs:
        rc += dp.counts(P)[0]
    assert _close(ll, want, 1e-9)
    assert np.allclose(c, rc, rtol=1e-6, atol=1e-9), np.abs(c - rc).max()
    assert np.all(c[np.asarray(em.inTok) != 0] == 0.0)
    assert np.array_equal(dev.counts()[0], c)
    if np.all(want > -np.inf):
        assert abs(s - float(np.sum(want))) <= 1e-9 * max(1.0, abs(float(np.sum(want))))
    if fill and profs:
        k = int(np.argmax([len(q) for q in profs]))
        P, (_, N, W) = profs[k], ref[k]
        F = capi.profile_fill_merged(dm, capi.MB_FORWARD, P, colTok)
        assert _close(F[:, 0], N, 1e-9) and _close(F[:, 1], W, 1e-9)
        _, Nv, Wv = dp.forward(P, "max")
        V = capi.profile_fill_merged(dm, capi.MB_VITERBI, P, colTok)
        assert np.array_equal(V[:, 0], Nv) and np.array_equal(V[:, 1], Wv)
        _, NB, WB = dp.backward(P)
        B = capi.profile_fill_merged(dm, capi.MB_BACKWARD, P, colTok)
        assert _close(B[:, 0], NB, 1e-9) and _close(B[:, 1], WB, 1e-9)
    return dm, dev, want


# ---- shared builders of the edge suite (test_profile_merge_edges_gpu.py) and of its CPU liveness test ---------------------------------
# Every builder is deterministic; the seeds were searched on the CPU so that the condition its case states (finite profiles, tie
# counts, chunk counts) holds under the restatement -- test_profile_merge_host.py::test_edge_suite_inputs_are_live asserts them.
PM_LDS_MAX = 160 * 1024                      # mb_profile_merge.hip
PM_THREADS = 1024


def few_levels_machine(S, nIn, nOut, seed):
    """As machine_for(S, nOut, silent=True, seed) of test_profile_merge_gpu.py beyond 8 states: cycles, a few silent edges (a handful
    of levels), emitting edges into the end state from a third of the states."""
    from randmachine import random_machine
    return random_machine(S, nIn, nOut, seed, density=1.5, silent_density=0.05, backbone=0.0, to_end=0.3)


def lanes_of(nCols, S):
    """(lanes of the workgroup, groups G, lanes per plane LPP) as pm_threads / pm_lanes choose them."""
    PL = nCols + 1
    lanes = min(PM_THREADS, max(64, (PL * S + 63) // 64 * 64))
    G = min(PL, lanes)
    return lanes, G, lanes // G


LANE_CASES = [(1, 1), (2, 1), (4, 13), (4, 204), (4, 205), (63, 2), (64, 2), (65, 2), (1023, 2), (1024, 2), (1030, 3)]
LANE_SEEDS = {(1, 1): 101, (2, 1): 102, (4, 13): 115, (4, 204): 318, (4, 205): 318, (63, 2): 102, (64, 2): 102, (65, 2): 102,
              (1023, 2): 102, (1024, 2): 102, (1030, 3): 103}


def lane_case(nCols, S):
    """(em, colTok, profs): colTok at random from 1..3; lengths 0, 1, 7, 23 up to 66 planes, 0..3 from 1 024 planes on."""
    from randmachine import random_machine
    seed = LANE_SEEDS[(nCols, S)]
    em = random_machine(S, 0, 3, seed, to_end=0.3) if S <= 8 else few_levels_machine(S, 0, 3, seed)
    rng = np.random.RandomState(seed + 1)
    colTok = rng.randint(1, 4, nCols)
    lengths = [0, 1, 7, 23] if nCols + 1 <= 66 else [0, 1, 2, 3]
    profs = [merged_rows(rng, nCols, L, zeros=0.2) for L in lengths]
    return em, colTok, profs


LDS_CASES = [431, 432, 1077, 1078, 1365, 1366, 5120, 5121]
LDS_SEEDS = {431: 631, 432: 632, 1077: 1279, 1078: 1278, 1365: 1565, 1366: 1566, 5120: 5320, 5121: 5321}


def lds_case(S):
    """(em, colTok, profs) at nCols = 4: lengths 0, 9, 24 with 20% -inf, the blank of the last kept >= log 0.02."""
    em = few_levels_machine(S, 0, 4, LDS_SEEDS[S])
    rng = np.random.RandomState(S + 4)
    profs = [merged_rows(rng, 4, L, zeros=0.2) for L in (0, 9, 24)]
    profs[-1][:, 0] = np.maximum(profs[-1][:, 0], np.log(0.02))
    return em, [1, 2, 3, 4], profs


ALPHABET_CASES = [(1, 1), (2, 3), (3, 4)]
ALPHABET_SEQ_SEEDS = {(1, 1): 0, (2, 3): 2, (3, 4): 0}


def alphabet_case(nIn, nOut):
    """(em, colTok, profs): 40 states with an input alphabet, every token a column and token 1 twice; lengths 0, 3, 17, 40, 10% -inf."""
    from randmachine import random_machine
    em = random_machine(40, nIn, nOut, 300 + 10 * nIn + nOut, to_end=0.3)
    colTok = list(range(1, nOut + 1)) + [1]
    rng = np.random.RandomState(300 + nIn)
    return em, colTok, [merged_rows(rng, len(colTok), L, zeros=0.1) for L in (0, 3, 17, 40)]


def one_hot_runs(rng, colTok, y, doubled_by_blank=True):
    """A one-hot merged profile that reads as the token sequence y and nothing else: per symbol a run of 1-3 rows at 0 in one column
    of its token (every other entry -inf), some blank-only rows between the runs.  Two equal adjacent symbols are kept apart by a
    blank row, or -- where the token heads two columns and doubled_by_blank is False -- by changing the column."""
    colTok = np.asarray(colTok)
    rows, last = [], 0
    for t in y:
        cols = [c + 1 for c in np.nonzero(colTok == t)[0]]
        c = cols[rng.randint(len(cols))]
        if c == last:
            other = [k for k in cols if k != last]
            if other and not doubled_by_blank:
                c = other[0]
            else:
                rows.append(0)
        elif rng.rand() < 0.3:
            rows.append(0)
        rows += [c] * rng.randint(1, 4)
        last = c if rows[-1] else 0
    if rng.rand() < 0.5:
        rows.append(0)
    P = np.full((len(rows), len(colTok) + 1), -np.inf)
    P[np.arange(len(rows)), rows] = 0.0
    return P


def run_heads(P, colTok):
    """The token sequence a one-hot merged profile reads as: the heads of its runs of equal consecutive columns, blanks dropped."""
    cols = [int(np.argmax(r)) for r in P]
    return [int(colTok[c - 1]) for k, c in enumerate(cols) if c and (k == 0 or cols[k - 1] != c)]


def alphabet_one_hot_case(nIn, nOut):
    """(em, colTok, profs, seqs): one-hot profiles and the token sequences they must score as.  The last three are the doubled
    symbol: (a, a) with a blank row between, (a, a) on the two columns of token 1 without a blank, and the same column twice
    without a blank, which is the single symbol (a)."""
    em, colTok, _ = alphabet_case(nIn, nOut)
    rng = np.random.RandomState(ALPHABET_SEQ_SEEDS[(nIn, nOut)])
    seqs = [list(rng.randint(1, nOut + 1, n)) for n in (0, 1, 2, 3, 5, 8)]
    profs = [one_hot_runs(rng, colTok, y, doubled_by_blank=bool(k % 2)) for k, y in enumerate(seqs)]
    a, b = 1, len(colTok)                                 # the two columns of token 1
    for rows, y in (([a, 0, a], [1, 1]), ([a, b, b], [1, 1]), ([a, a], [1])):
        P = np.full((len(rows), len(colTok) + 1), -np.inf)
        P[np.arange(len(rows)), rows] = 0.0
        profs.append(P); seqs.append(y)
    assert all(run_heads(P, colTok) == [int(t) for t in y] for P, y in zip(profs, seqs))
    return em, colTok, profs, seqs


COLMAP_SEEDS = {"one": 40, "same": 40, "unused": 40}


def column_map_cases():
    """S = 12: one column; three columns on one token; a column whose token (3) no transition emits."""
    import dataclasses
    from randmachine import random_machine
    from machineboss_amd.evalmachine import Tokenizer
    out = {}
    for name, nOut, colTok, seed in (("one", 2, [2], COLMAP_SEEDS["one"]), ("same", 2, [1, 1, 1], COLMAP_SEEDS["same"]), ("unused", 2, [1, 3, 2], COLMAP_SEEDS["unused"])):
        em = random_machine(12, 0, nOut, seed, to_end=0.3)
        if name == "unused":
            em = dataclasses.replace(em, outputTokenizer=Tokenizer(["a", "b", "c"]))
            assert em.nOutTok == 3 and not np.any(em.outTok == 3)
        rng = np.random.RandomState(seed + 1)
        out[name] = (em, colTok, [merged_rows(rng, len(colTok), L, zeros=0.15) for L in (0, 1, 7, 23)])
    return out


DEGENERATE_SEEDS = {"noblank": 400, "infrow": 400, "infweights1": 401, "infweights2": 402}


def degenerate_cases():
    """(em, colTok, profs) by name: the blank -inf in every row; a whole row -inf in one profile of a batch; machines with an eighth
    of their weights -inf."""
    from randmachine import random_machine
    out = {}
    colTok = [1, 2, 3, 1]
    em = random_machine(40, 0, 3, DEGENERATE_SEEDS["noblank"], to_end=0.3)
    rng = np.random.RandomState(11)
    profs = [merged_rows(rng, 4, L, zeros=0.1) for L in (0, 4, 12, 25)]
    for P in profs:
        P[:, 0] = -np.inf
    out["noblank"] = (em, colTok, profs)
    em = random_machine(40, 0, 3, DEGENERATE_SEEDS["infrow"], to_end=0.3)
    rng = np.random.RandomState(12)
    profs = [merged_rows(rng, 4, L, zeros=0.1) for L in (10, 25, 0, 33, 18)]
    profs[1][7] = -np.inf
    profs[4][0] = -np.inf
    out["infrow"] = (em, colTok, profs)
    for k in (1, 2):
        seed = DEGENERATE_SEEDS["infweights%d" % k]
        em = random_machine(40, 0, 3, seed, allow_inf=True, to_end=0.3)
        lw = em.logWeight.copy()
        lw[np.random.RandomState(seed).choice(len(lw), len(lw) // 8, replace=False)] = -np.inf
        rng = np.random.RandomState(seed + 1)
        out["infweights%d" % k] = (em.withLogWeights(lw), colTok, [merged_rows(rng, 4, L, zeros=0.1) for L in (10, 25, 0, 33, 18, 40)])
    return out


def all_blank_case():
    """(em, colTok, P): 30 rows whose symbol columns are -inf; the machine has a silent path from 0 to S - 1."""
    from randmachine import random_machine
    em = random_machine(50, 0, 3, 502)
    P = np.full((30, 5), -np.inf)
    P[:, 0] = np.log(np.random.RandomState(501).uniform(0.1, 1.0, 30))
    return em, [1, 2, 3, 1], P


TIE_COLTOK = [1, 1, 2, 2, 3]
TIE_CASES = [(6, 607, 607), (12, 637, 637), (30, 638, 638)]                         # (states, machine seed, profile seed)
TIE_KINDS = ("plane", "end", "stay", "silent", "repeat", "blank", "emit")


def tie_cases():
    """[(em, colTok, profs)]: quantised machines of 6, 12 and 30 states with silent edges against 70 quantised profiles of up to 24
    rows each, tokens 1 and 2 on two columns each."""
    from randmachine import quantised_machine
    out = []
    for S, mseed, pseed in TIE_CASES:
        em = quantised_machine(S, 0, 3, mseed)
        rng = np.random.RandomState(pseed)
        out.append((em, TIE_COLTOK, [quantised_rows(rng, len(TIE_COLTOK), int(L)) for L in rng.randint(0, 25, 70)]))
    return out


BATCH_CASES = [(300, 120, 40), (1400, 12, 24)]
BATCH_SEEDS = {300: 1000, 1400: 2100}


def batch_case(S, n, maxL):
    """(em, colTok, profs) at nCols = 4: n profiles of 0..maxL rows (the first two of 0 and maxL), 10% -inf, every fifth with one row
    all -inf."""
    em = few_levels_machine(S, 0, 4, BATCH_SEEDS[S])
    rng = np.random.RandomState(700 + S)
    lengths = [0, maxL] + list(rng.randint(0, maxL + 1, n - 2))
    profs = [merged_rows(rng, 4, int(L), zeros=0.1) for L in lengths]
    for k in range(3, n, 5):
        if len(profs[k]):
            profs[k][rng.randint(len(profs[k]))] = -np.inf
    return em, [1, 2, 3, 4], profs


def batch_bytes(em, nCols, profs, levels):
    """Per profile, the device bytes mb_profile_api.hip charges to the memory budget: (counts(), viterbi() with paths).  The lattice is
    (L+1) x 2 x (nCols+1) x S doubles; counts() adds nTrans x (nCols+1) accumulators, viterbi() the path slot of L + (L+1)(levels-1)
    entries at 8 bytes; both add the workgroup's global scratch (the ring of (3 (nCols+1) + nCols) S doubles) when their rolling
    state is beyond LDS -- X (nCols S doubles) for the materialised sweeps, 3 (nCols+1) S for the rolling Backward."""
    S, PL, nT = em.nStates, nCols + 1, em.nTransitions
    ring = (3 * PL + nCols) * S
    vScratch = ring if nCols * S * 8 > PM_LDS_MAX else 0
    cScratch = ring if 3 * PL * S * 8 > PM_LDS_MAX else vScratch
    c = [8 * (len(P) + 1) * 2 * PL * S + 8 * nT * PL + 8 * cScratch for P in profs]
    v = [8 * (len(P) + 1) * 2 * PL * S + 8 * (len(P) + (len(P) + 1) * (levels - 1)) + 8 * vScratch for P in profs]
    return c, v


def greedy_chunks(bytes_, budget):
    """The chunks lattice_chunks (mb_profile_api.hip) cuts: even shares of ceil(total / budget) chunks, 5% slack, never over the budget."""
    total = float(sum(bytes_))
    share = min(budget, total / max(1.0, np.ceil(total / budget)) * 1.05)
    out, p0, acc = [], 0, 0.0
    for k, b in enumerate(bytes_):
        if k > p0 and (acc + b > budget or (acc >= share and acc + b > share)):
            out.append((p0, k)); p0 = k; acc = 0.0
        acc += b
    if len(bytes_) > p0:
        out.append((p0, len(bytes_)))
    return out


LONG_SEEDS = {False: 801, True: 801, "restatement": 850}


def long_case(with_input):
    """(em, colTok, profs): 200 states, nCols = 4, three profiles of 1 500 to 3 000 rows without -inf."""
    em = few_levels_machine(200, 2 if with_input else 0, 4, LONG_SEEDS[with_input])
    rng = np.random.RandomState(801)
    return em, [1, 2, 3, 4], [merged_rows(rng, 4, L, zeros=0.0) for L in (1500, 2200, 3000)]


def long_restatement_case():
    """(em, colTok, P): one profile of 1 200 rows (5% -inf) at 100 states, token 1 on two columns."""
    em = few_levels_machine(100, 0, 3, LONG_SEEDS["restatement"])
    return em, [1, 2, 3, 1], merged_rows(np.random.RandomState(802), 4, 1200, zeros=0.05)


def composed_case(which, zeros):
    """(M, em, prof): a 50-symbol generator over ACGT or a random 6-state machine, and a CSV profile whose header holds one symbol
    twice -- 30 rows for the random machine, 90 for the generator, which must emit its 50 symbols and a blank between equal ones; with `zeros` a tenth of its weights are 0."""
    from profhelpers import _machine_of
    from randmachine import random_machine
    from machineboss_amd import algebra
    from machineboss_amd.evalmachine import EvaluatedMachine
    rng = np.random.RandomState(11)
    if which == "generator":
        M = algebra.generator(list(rng.choice(list("ACGT"), 50)), "g")
        hdr = ["A", "C", "G", "T", "A"]
    else:
        M = _machine_of(random_machine(6, 0, 3, 901 + 2 * zeros))
        hdr = ["a", "b", "c", "b"]
    em = EvaluatedMachine.fromMachine(M, {}, useDefaults=True)
    rows = rng.dirichlet([0.5] * (len(hdr) + 1), 30 if which == "random" else 90).astype(np.float32).astype(np.float64)
    if zeros:
        rows[rng.rand(*rows.shape) < 0.1] = 0.0
    return M, em, Profile(hdr, rows.tolist())


