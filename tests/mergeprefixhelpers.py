"""Shared helpers of the tests of decoding against a CTC-merged profile (test_prefix_merge_host.py, test_prefix_merge_gpu.py,
test_prefix_merge_edges_gpu.py; not a test module): the composite compose(M, merging recogniser) with a map from its states to the cells of the native lattice, the node
families of both fills, and the deterministic inputs of the device cases.  The seeds were searched on the CPU so that the
conditions the cases state (finite results, populated layers) hold under the numpy restatement alone."""
import dataclasses

import numpy as np

from machineboss_amd import algebra, prefixtree
from machineboss_amd.evalmachine import EvaluatedMachine
from machineboss_amd.machine import Machine, MachineState, MachineTransition
from mergehelpers import merged_rows
from prefixhelpers import family_paths, populated_machine


def named_machine(em0):
    """An EvaluatedMachine as (Machine, EvaluatedMachine): numeric weights, state s named s, so that algebra.compose names the
    states of a composite by the pair they came from."""
    m = Machine()
    isym, osym = em0.inputTokenizer.tok2sym, em0.outputTokenizer.tok2sym
    for s in range(em0.nStates):
        ms = MachineState(); ms.name = s
        m.state.append(ms)
    for e in range(em0.nTransitions):
        m.state[int(em0.src[e])].trans.append(MachineTransition(dest=int(em0.dst[e]), inp=isym[em0.inTok[e]] if em0.inTok[e] else "",
                                                                out=osym[em0.outTok[e]] if em0.outTok[e] else "",
                                                                weight=float(np.exp(em0.logWeight[e]))))
    return m, EvaluatedMachine.fromMachine(m, {}, useDefaults=True)


def merged_composite(M, em, prof, params=None):
    """(C, cellOf): the EvaluatedMachine of algebra.compose(M, prof.mergingRecogniserMachine()) and, per state of C, the cell of
    the native lattice its seq value is -- (r, plane, q), plane None for the end state of the recogniser (every plane of row L) --
    or None for a state of the arrived stage (N, which a node does not store).  The recogniser's states are renamed to their
    indices first: the names CSVProfile gives them do not tell two columns of one symbol apart.  M's states must be named 0..S-1
    in order."""
    rec = prof.mergingRecogniserMachine()
    for k, ms in enumerate(rec.state):
        ms.name = k
    split = {next(iter(ms.name.values())) for ms in algebra.waitingMachine(rec).state if isinstance(ms.name, dict)}
    nHdr, L = len(prof.header), len(prof.row)
    known = {s: t for t, s in enumerate(em.outputTokenizer.tok2sym) if t}
    planeOf = {nHdr: 0}
    for c, h in enumerate(prof.header):
        if h in known:
            planeOf[c] = len(planeOf)
    cm = algebra.compose(M, rec, True, False)
    C = EvaluatedMachine.fromMachine(cm, M.getParamDefs(True) if params is None else params)
    cellOf = []
    for ms in cm.state:
        if not isinstance(ms.name, list):
            cellOf.append(None)
            continue
        q, j = ms.name
        waiting = isinstance(j, dict)
        if waiting:
            j = next(iter(j.values()))
        elif j in split:
            cellOf.append(None)          # the arrived stage of a recogniser state that was split
            continue
        if j == 0:
            cellOf.append((0, 0, q))
        elif j == len(rec.state) - 1:
            cellOf.append((L, None, q))
        else:
            pos, tok = divmod(j - 1, nHdr + 1)
            cellOf.append((pos + 1, planeOf[tok], q) if tok in planeOf else None)
    return C, cellOf


def composite_fills(C, em, paths):
    """{path: (cells, logSeqProb, logPrefixProb)} of the token search (PrefixDP, unchanged) on C with an empty output; a path is
    in em's input tokens.  A symbol that C's alphabet lost makes the node impossible."""
    dp = prefixtree.PrefixDP(C)
    tok = {t: C.inputTokenizer.tok2sym.index(s) if s in C.inputTokenizer.tok2sym else 0 for t, s in enumerate(em.inputTokenizer.tok2sym) if t}
    dead = (np.full((1, 2, C.nStates), -np.inf), -np.inf, -np.inf)
    out = {}
    for p in sorted(paths, key=len):
        if not p:
            out[p] = dp.fill([])
        elif tok[p[-1]] == 0 or out[p[:-1]] is dead:
            out[p] = dead
        else:
            out[p] = dp.fill([], out[p[:-1]][0], tok[p[-1]])
    return out


def composite_w_cells(cells, cellOf, L, PL, S):
    """(want[L+1][PL][S], have[L+1][PL][S] bool, last[S], haveLast[S]): the composite's seq cells laid out as W; ``last`` is
    (+)_p W[L][p][q] where the composite kept the state."""
    want, have = np.full((L + 1, PL, S), -np.inf), np.zeros((L + 1, PL, S), bool)
    last, haveLast = np.full(S, -np.inf), np.zeros(S, bool)
    for k, c in enumerate(cellOf):
        if c is None:
            continue
        r, p, q = c
        if p is None:
            last[q], haveLast[q] = cells[0, 0, k], True
        else:
            want[r, p, q], have[r, p, q] = cells[0, 0, k], True
    return want, have, last, haveLast


def merged_fills(em, P, colTok, paths, logR=None):
    """{path: (cells, logSeqProb, logPrefixProb)} of MergedProfilePrefixDP."""
    dp = prefixtree.MergedProfilePrefixDP(em, colTok, logR)
    out = {}
    for p in sorted(paths, key=len):
        out[p] = dp.fill(P) if not p else dp.fill(P, out[p[:-1]][0], p[-1])
    return out


def worst(got, ref):
    """Worst |got - ref| / max(1, |ref|) over the finite entries; -inf (and nothing else) must sit where the reference has it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (got, ref)
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(ref)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin])))) if fin.any() else 0.0


def sharp_merged_profile(rng, toks, colTok, sharp=0.9):
    """A merged profile that reads as the output tokens ``toks``: per token a run of 1 to 3 rows with weight ``sharp`` on a column of
    the token, a blank row between equal neighbours; the rest of a row's weight is spread evenly."""
    colTok = np.asarray(colTok)
    PL = len(colTok) + 1
    cols, last = [], 0
    for t in toks:
        c = int(np.nonzero(colTok == t)[0][0]) + 1
        if c == last:
            cols.append(0)
        cols += [c] * int(rng.randint(1, 4))
        last = c
    P = np.full((len(cols), PL), (1.0 - sharp) / (PL - 1))
    P[np.arange(len(cols)), cols] = sharp
    return np.log(P)


# ---- device cases (test_prefix_merge_gpu.py) --------------------------------------------------------------------------------------
def device_machine(S, nOut, seed, levels=True):
    """Machines with an input alphabet of 2 whose prefix-search lattices are populated: populated_machine (output-less mass at
    most 0.8 per state, so a child's prefix probability stays below its parent's)."""
    return populated_machine(S, seed, levels, nIn=2, nOut=nOut)


def live_rows(rng, nCols, L, zeros=0.1):
    """merged_rows with a positive blank in every row."""
    P = merged_rows(rng, nCols, L, zeros)
    if L:
        P[:, 0] = np.maximum(P[:, 0], np.log(0.02))
    return P


LANE_CASES = [(1, 1), (2, 1), (4, 13), (4, 204), (4, 205), (63, 2), (64, 2), (65, 2)]
LANE_ROWS = [0, 1, 2, 33]


def lane_case(nCols, S, L, seed=0):
    """(em, colTok, P): three output tokens, the columns on them in turn; a tenth of the weights -inf up to 2 rows, none at 33 rows
    (there nine tenths of the cells of a layer must be finite, and row 0 and the states out of reach are -inf already)."""
    em = device_machine(S, 3, 700 + seed)
    colTok = [1 + c % 3 for c in range(nCols)]
    return em, colTok, live_rows(np.random.RandomState(10 * S + nCols + L), nCols, L, zeros=0.1 if L < 33 else 0.0)


def column_map_cases():
    """{name: (em, colTok, P)} at S = 40, L = 20: two columns on one token, every column on one token, a column whose token nothing
    emits, one column."""
    from machineboss_amd.evalmachine import Tokenizer
    out = {}
    for name, nOut, colTok in (("two", 3, [1, 2, 1, 3]), ("same", 2, [2, 2, 2]), ("unused", 2, [1, 3, 2]), ("one", 2, [1])):
        em = device_machine(40, nOut, 40)
        if name == "unused":
            em = dataclasses.replace(em, outputTokenizer=Tokenizer(["a", "b", "c"]))
            assert em.nOutTok == 3 and not np.any(em.outTok == 3)
        out[name] = (em, colTok, live_rows(np.random.RandomState(41), len(colTok), 20))
    return out


def family_fills(nodes, nIn, seq=0):
    """{path: (slot, logSeqProb, logPrefixProb)} of the root, its children (ONE extend) and one grandchild of each (ONE extend) of
    search ``seq`` in a lattice store."""
    paths = family_paths(nIn)
    out = {(): nodes.root(seq)}
    for depth in (1, 2):
        ps = [p for p in paths if len(p) == depth]
        slots, lsp, lpp = nodes.extend([seq] * len(ps), [out[p[:-1]][0] for p in ps], [p[-1] for p in ps])
        for p, s, a, b in zip(ps, slots, lsp, lpp):
            out[p] = (int(s), float(a), float(b))
    return out


def dnastore_merged_profiles(lengths=(2, 3, 4, 5, 6, 7, 8, 9)):
    """(machine, em, colTok, inputs, profiles): sharp merged profiles of the Viterbi encodings of random inputs of dnastore4, one per
    input length (rows repeated 1 to 3 times, a blank row between equal neighbours), one column per output token."""
    from conftest import golden_path
    from machineboss_amd import boss
    m = Machine.fromFile(golden_path("machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, None, useDefaults=True)
    rng = np.random.RandomState(5)
    syms = m.inputAlphabet()
    ins = [[syms[k] for k in rng.randint(0, len(syms), n)] for n in lengths]
    colTok = list(range(1, em.nOutTok + 1))
    profs = [sharp_merged_profile(rng, em.outputTokenizer.tokenize(o), colTok) for o in boss.viterbiEncode(m, ins, "numpy")]
    return m, em, colTok, ins, profs


def fed_machine(S, nOut, seed, levels):
    """device_machine with one more input-free emitting edge INTO every state per output token, from a random state: without
    silent levels a populated_machine leaves e^-2 of the (state, token) pairs without such an edge, and those cells of W are -inf
    in every plane of the token -- more than the tenth a populated case may have."""
    em = device_machine(S, nOut, seed, levels)
    rng = np.random.RandomState(seed + 1)
    n = S * nOut
    src = np.concatenate([em.src, rng.randint(0, S, n).astype(np.uint32)])
    dst = np.concatenate([em.dst, np.repeat(np.arange(S, dtype=np.uint32), nOut)])
    it = np.concatenate([em.inTok, np.zeros(n, np.uint16)])
    ot = np.concatenate([em.outTok, np.tile(np.arange(1, nOut + 1, dtype=np.uint16), S)])
    lw = np.concatenate([em.logWeight, np.log(rng.uniform(0.1, 0.5, n))])
    order = np.argsort(src, kind="stable")
    src, dst, it, ot, lw = src[order], dst[order], it[order], ot[order], lw[order]
    off = np.zeros(S + 1, np.int64)
    np.add.at(off, src.astype(np.int64) + 1, 1)
    off = np.cumsum(off)
    tidx = (np.arange(len(src)) - off[src]).astype(np.uint32)
    return EvaluatedMachine(S, em.inputTokenizer, em.outputTokenizer, src, dst, it, ot, tidx, lw, off, [None] * S)


def levels_case(levels):
    """(em, colTok, P): 300 states with or without silent levels, nCols = 4 with token 1 on two columns, 65 rows without -inf."""
    em = fed_machine(300, 3, 300, levels)
    return em, [1, 2, 3, 1], live_rows(np.random.RandomState(65 + levels), 4, 65, zeros=0.0)


def two_column_profile(rng, em, L):
    """A CSV profile of L full rows over the two output symbols of em, a foreign symbol between them; a tenth of the weights 0."""
    from machineboss_amd.profile import Profile
    a, b = em.outputTokenizer.tok2sym[1:3]
    v = rng.uniform(0.05, 1.0, (L, 4))
    v[rng.rand(L, 4) < 0.1] = 0.0
    v[:, 3] = np.maximum(v[:, 3], 0.05)
    return Profile([b, "zz", a], [[float(np.float32(x)) for x in row] for row in v])


def lds_case(S):
    """(em, colTok, P) at nCols = 4, 3 rows, for the machines at the LDS limit."""
    em = device_machine(S, 3, S)
    return em, [1, 2, 3, 1], live_rows(np.random.RandomState(S), 4, 3, zeros=0.1)


# ---- the edge suite of the merged fill (test_prefix_merge_edges_gpu.py; held to its liveness conditions without a GPU by
# test_prefix_merge_host.py::test_edge_suite_inputs_are_live) -------------------------------------------------------------------------
# (nCols, S, L).  PL = nCols + 1 planes: from 513 on a lane serves one plane alone (LPP = 1) and the lanes past PL idle; 1 024 planes
# fill the workgroup exactly; from 1 025 on a lane owns several planes in every phase.  The last two need 104.7 and 152.4 KiB of LDS.
PLANE_CASES = [(600, 1, 3), (1023, 1, 3), (1024, 1, 3), (1030, 2, 3), (1500, 2, 2)]
SHORT_FAMILY = [(), (1,), (1, 2)]          # the root, one child, one grandchild: where the yardstick takes a second per node


def plane_paths(nCols):
    """The family compared at ``nCols`` columns: the whole one up to 1 024 planes, SHORT_FAMILY beyond."""
    return family_paths(2) if nCols < 1024 else SHORT_FAMILY


# (S, nIn, nOut, levels): the strides C = nOut + 1 and K = (nIn + 1)(nOut + 1) from alphabets of different sizes
ALPHABET_CASES = [(1, 1, 1, False), (2, 1, 4, True), (63, 3, 5, True), (64, 5, 3, False), (65, 3, 5, True), (65, 5, 3, False)]
EDGE_ROWS = 33
DEAD_ROW = 16


def alphabet_case(S, nIn, nOut, levels):
    """(em, colTok, P): 2 nOut - 1 columns on the tokens in turn, so all but the last token have two columns; 33 rows without
    -inf."""
    em = populated_machine(S, 100 + S, levels, nIn, nOut)
    nCols = 2 * nOut - 1
    return em, [1 + c % nOut for c in range(nCols)], live_rows(np.random.RandomState(S + EDGE_ROWS), nCols, EDGE_ROWS, zeros=0.0)


def batch_machine():
    """S = 40, silent levels, nIn = 3, nOut = 5: the machine of the dead-weight and the batch cases."""
    return populated_machine(40, 7, True, 3, 5)


DEAD_COLTOK = [1, 2, 3, 4, 5, 1, 3]


def sparse_rows():
    """33 rows over DEAD_COLTOK, each weight -inf with probability one third, the blank included: rows with a dead blank skip the
    blank sums, and bN / bXn, eP / eW / eY stay from an earlier row where a column is dead."""
    rng = np.random.RandomState(0)
    w = rng.uniform(0.05, 1.0, (EDGE_ROWS, len(DEAD_COLTOK) + 1))
    with np.errstate(divide="ignore"):
        return np.log(np.where(rng.rand(*w.shape) < 1.0 / 3.0, 0.0, w))


def dead_row_rows():
    """33 rows over DEAD_COLTOK without -inf, but row DEAD_ROW -inf throughout: nothing passes it."""
    P = live_rows(np.random.RandomState(1), len(DEAD_COLTOK), EDGE_ROWS, zeros=0.0)
    P[DEAD_ROW] = -np.inf
    return P


def dead_blank_case():
    """lane_case(65, 2, 6) with the blank of every row -inf: the group of plane 0 never forms a blank sum."""
    em, colTok, P = lane_case(65, 2, 6)
    P[:, 0] = -np.inf
    return em, colTok, P


def far_column_rows():
    """Two rows over colTok = [1, 2] that read mostly a, then mostly b (prefixhelpers.far_column_case)."""
    return np.log(np.array([[0.05, 0.9, 0.05], [0.05, 0.05, 0.9]]))


TWIN_COLTOK = [1, 2, 1]
# A quantised sharp row: 2^0 on its column, 2^-6 elsewhere; two output tokens per profile.  Searched on the CPU: the numpy searches
# take 121 to 145 fills each (three tokens, or 2^-1 against 2^-4, take 500 to 4 000 on this machine, whose weights are flat).
QUANT_BITS, QUANT_TOKENS = (0, 6), 2


def twin_merged_profiles(em, quantised):
    """Four sharp merged profiles over TWIN_COLTOK that read as output strings of prefixhelpers.twin_outputs.  ``quantised``:
    every weight is a multiple of log 0.5, as the weights of the quantised twin machine are, so that different paths tie exactly."""
    import prefixhelpers as ph
    rng = np.random.RandomState(ph.TWIN_SEED)
    profs = []
    for o in ph.twin_outputs(em, ph.TWIN_SEARCHES, QUANT_TOKENS if quantised else ph.TWIN_L, ph.TWIN_SEED):
        P = sharp_merged_profile(rng, em.outputTokenizer.tokenize(list(o)), TWIN_COLTOK, sharp=0.8)
        if quantised:
            P = np.where(P == P.max(), QUANT_BITS[0], QUANT_BITS[1]) * np.log(0.5)
        profs.append(P)
    return profs


SELF_LOOP_COLTOK = [1, 2, 3, 4, 5, 2]


def self_loop_rows():
    return live_rows(np.random.RandomState(8), len(SELF_LOOP_COLTOK), 12, zeros=0.1)


BATCH_COLTOK = [1, 2, 3, 4, 5, 2, 4]
BATCH_LENGTHS = tuple(range(10))


def batch_rows():
    """One table per search, of 0, 1, ..., 9 rows."""
    return [live_rows(np.random.RandomState(20 + L), len(BATCH_COLTOK), L, zeros=0.05) for L in BATCH_LENGTHS]


MANY_FILLS = (300, 600)          # (S, children in one extend): 69 640 B of LDS, two workgroups per CU, more fills than are resident
LDS_MARK_STATES = (282, 283, 706)          # nCols = 4: 65 464 B (within 64 KiB), 65 696 B (the opt-in), 163 832 B (the limit)
