"""Prefix search: imputing the most likely input of a transducer for a given output (docs/decoding.md).

The reference's ``PrefixTree`` (src/ctc.h, src/ctc.cpp) is a best-first search over input prefixes.  A node is an input prefix
x[1..n]; its only arithmetic is a dense sweep over (L+1) x 2 x S cells against the output y[1..L] (``Node::fill``,
src/ctc.cpp:25-88), restated here with a = x[n] the node's own symbol and P its parent:

    A[j][d]      = [root, j = 0, d = 0] (+) sum_{t: s->d, in = a, out = y[j]} P.seq[j-1][s] + w_t
                                        (+) sum_{t: s->d, in = a, out = eps } P.seq[j][s]   + w_t
    seq[j][d]    = A[j][d] (+) sum_{t: s->d, in = eps, out = y[j]} seq[j-1][s] + w_t
                           (+) sum_{silent t: s->d, s < d} seq[j][s] + w_t                       (same row: silent levels)
    V[j-1][s]    = logsum_p prefix[j-1][p] + R[p][s]
    prefix[j][d] = A[j][d] (+) sum_{t: s->d, any in, out = y[j]} V[j-1][s] + w_t
    logSeqProb   = seq[L][S-1],     logPrefixProb = logsum_d prefix[L][d] + R[d][S-1]

R = log((I - N)^-1), N[s][d] the summed weight of the transitions s->d with empty output (``logSumInTrans``).  ``seq`` is the
Forward likelihood of the pair (x, y), ``prefix`` the likelihood of y given any input that starts with x.

This module holds the numpy restatement of the fill (``PrefixDP``, the yardstick of mb_prefix.hip), the search itself
(``PrefixTree``) over either backend -- "numpy" or "device" -- and the lock-step driver that decodes many outputs at once with
one device launch per round (``decodeBatch``).  The device owns the lattices, the host the tree.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .evalmachine import EvaluatedMachine
from .machine import MachineError
from .profile import _lse_fold, _red_planes

_NEG = -math.inf
NO_BACKTRACK_LIMIT = (1 << 63) - 1      # numeric_limits<long>::max(), target/boss.cpp:851
DEFAULT_MAX_NODES = 4096


def logSumInTrans(em: EvaluatedMachine) -> np.ndarray:
    """EvaluatedMachine::logSumInTrans(false) (src/eval.cpp:146-184): log of (I - N)^-1, N[s][d] = sum of exp(w) over the
    transitions s->d with empty output, whatever their input; non-positive entries of the inverse become -inf."""
    S = em.nStates
    M = np.eye(S)
    sel = em.outTok == 0
    with np.errstate(under="ignore"):
        np.subtract.at(M, (em.src[sel].astype(np.int64), em.dst[sel].astype(np.int64)), np.exp(em.logWeight[sel]))
    inv = np.linalg.inv(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inv > 0, np.log(np.where(inv > 0, inv, 1.0)), _NEG)


class PrefixDP:
    """The node fill in numpy with exact (max-shifted) sums: ``fill(y, parentCells, a)`` -> (cells[L+1][2][S], logSeqProb,
    logPrefixProb); layer 0 = seq, layer 1 = prefix."""

    def __init__(self, em: EvaluatedMachine, logR: Optional[np.ndarray] = None):
        self.em = em
        self.S = em.nStates
        self.logR = logSumInTrans(em) if logR is None else np.asarray(logR, np.float64)
        src, dst = em.src.astype(np.int64), em.dst.astype(np.int64)
        it, ot, w = em.inTok.astype(np.int64), em.outTok.astype(np.int64), em.logWeight
        self._by: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray, np.ndarray]] = {}
        for i in range(em.nInTok + 1):
            for o in range(em.nOutTok + 1):
                k = np.nonzero((it == i) & (ot == o))[0]
                if i == 0 and o == 0:
                    k = k[src[k] < dst[k]]              # a silent self-loop never fires
                if len(k):
                    self._by[(i, o)] = (src[k], dst[k], w[k])
        self._anyIn = {}
        for o in range(1, em.nOutTok + 1):
            k = np.nonzero(ot == o)[0]
            self._anyIn[o] = (src[k], dst[k], w[k])
        lv = em.silentLevels()
        sil = self._by.get((0, 0))
        self._levels = [] if sil is None else [np.nonzero(lv[sil[1]] == l)[0] for l in range(1, int(lv.max(initial=0)) + 1)]
        # R by column, finite entries only (what the device reads)
        cols, rows = np.nonzero((self.logR > _NEG).T)
        self._rCol, self._rRow, self._rVal = cols, rows, self.logR[rows, cols]

    def _edges(self, i: int, o: int):
        e = self._by.get((i, o))
        return e if e is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))

    def columnSums(self, row: np.ndarray) -> np.ndarray:
        """V[s] = logsum_p row[p] + R[p][s]."""
        if 4 * len(self._rCol) <= self.S * self.S:       # a sparse R: its finite entries only
            return _lse_fold(np.full(self.S, _NEG), self._rCol, row[self._rRow] + self._rVal)
        M = row[:, None] + self.logR
        mx = M.max(axis=0)
        ms = np.where(mx > _NEG, mx, 0.0)
        with np.errstate(divide="ignore"):
            return np.where(mx > _NEG, ms + np.log(np.exp(M - ms).sum(axis=0)), _NEG)

    def fill(self, y: Sequence[int], parent: Optional[np.ndarray] = None, a: int = 0) -> Tuple[np.ndarray, float, float]:
        y = np.asarray(y, np.int64)
        L, S = len(y), self.S
        cells = np.full((L + 1, 2, S), _NEG)
        for j in range(L + 1):
            o = int(y[j - 1]) if j else 0
            A = np.full(S, _NEG)
            if parent is None:
                if j == 0:
                    A[0] = 0.0
            else:
                if j:
                    s, d, w = self._edges(a, o)
                    A = _lse_fold(A, d, parent[j - 1, 0][s] + w)
                s, d, w = self._edges(a, 0)
                A = _lse_fold(A, d, parent[j, 0][s] + w)
            sq, px = A, A
            if j:
                s, d, w = self._anyIn[o]
                px = _lse_fold(A, d, self.columnSums(cells[j - 1, 1])[s] + w)
                s, d, w = self._edges(0, o)
                sq = _lse_fold(A, d, cells[j - 1, 0][s] + w)
            if self._levels:
                s, d, w = self._by[(0, 0)]
                sq = sq.copy()
                for lvl in self._levels:
                    sq = _lse_fold(sq, d[lvl], sq[s[lvl]] + w[lvl])
            cells[j, 0], cells[j, 1] = sq, px
        with np.errstate(invalid="ignore"):
            lpp = float(_lse_fold(np.full(1, _NEG), np.zeros(S, np.int64), cells[L, 1] + self.logR[:, S - 1])[0])
        return cells, float(cells[L, 0, S - 1]), lpp


class ProfilePrefixDP(PrefixDP):
    """The node fill against a PROFILE (rows of output-symbol log weights plus a blank, profile.Profile.logRows) in place of the
    output string: the prefix search on compose(M, profile recogniser) with an empty output, swept natively over rows r = 0..L
    and M's own S states (docs/decoding.md, "Decoding against a profile").  As in profile.ProfileDP a row has two stages: N, the
    mass that has ARRIVED at the row (only there may the blank fire), and W, the mass after M's output-less moves -- the order the
    composition fixes, so that a blank and an output-less move of M are not counted in both orders:

        An[r][d] = [root, r = 0, d = 0] (+) sum_{t: s->d, in = a, out = o} Pa.W[r-1][s] + w_t + P[r-1][o]
        Aw[r][d] = sum_{t: s->d, in = a, out = eps} Pa.W[r][s] + w_t
        N[r][d]  = An[r][d] (+) (N[r-1][d] + P[r-1][0]) (+) sum_{t: s->d, in = eps, out = o} W[r-1][s] + w_t + P[r-1][o]
        W[r][d]  = Aw[r][d] (+) N[r][d] (+) sum_{silent t: s->d, s < d} W[r][s] + w_t
        Xn[r][d] = An[r][d] (+) (Xn[r-1][d] + P[r-1][0]) (+) sum_{t: s->d, any in, out = o} Y[r-1][s] + w_t + P[r-1][o]
        X[r][d]  = Aw[r][d] (+) Xn[r][d]
        Y[r][s]  = logsum_p X[r][p] + R[p][s]
        logSeqProb = W[L][S-1],     logPrefixProb = Y[L][S-1]

    ``fill(P, parentCells, a)`` -> (cells[L+1][2][S], logSeqProb, logPrefixProb); layer 0 = W, layer 1 = X."""

    def __init__(self, em: EvaluatedMachine, logR: Optional[np.ndarray] = None):
        super().__init__(em, logR)
        none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64))

        def emitting(sel):
            parts = [self._by[k] + (np.full(len(self._by[k][0]), k[1], np.int64),) for k in sorted(self._by) if k[1] > 0 and sel(k[0])]
            return tuple(np.concatenate(c) for c in zip(*parts)) if parts else none
        self._emitIn = [emitting(lambda i, a=a: i == a) for a in range(em.nInTok + 1)]      # [a]: in = a, out = o > 0 (src, dst, w, o)
        self._emitAny = emitting(lambda i: True)
        self._all = np.arange(self.S, dtype=np.int64)

    def fill(self, P, parent: Optional[np.ndarray] = None, a: int = 0) -> Tuple[np.ndarray, float, float]:
        P = np.asarray(P, np.float64).reshape(-1, self.em.nOutTok + 1)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        L, S = len(P), self.S
        cells = np.full((L + 1, 2, S), _NEG)
        Y = N = Xn = np.full(S, _NEG)
        for r in range(L + 1):
            Pr = P[r - 1] if r else None
            An, Aw = np.full(S, _NEG), np.full(S, _NEG)
            if parent is None:
                if r == 0:
                    An[0] = 0.0
            else:
                s, d, w = self._edges(a, 0)
                Aw = _lse_fold(Aw, d, parent[r, 0][s] + w)
                if r:
                    s, d, w, o = self._emitIn[a]
                    An = _lse_fold(An, d, (parent[r - 1, 0][s] + w) + Pr[o])
            if r:
                s, d, w, o = self._emitIn[0]
                N = _lse_fold(An, np.concatenate([self._all, d]), np.concatenate([N + Pr[0], (cells[r - 1, 0][s] + w) + Pr[o]]))
                s, d, w, o = self._emitAny
                Xn = _lse_fold(An, np.concatenate([self._all, d]), np.concatenate([Xn + Pr[0], (Y[s] + w) + Pr[o]]))
            else:
                N = Xn = An
            sq, px = _lse_fold(Aw, self._all, N), _lse_fold(Aw, self._all, Xn)
            if self._levels:
                s, d, w = self._by[(0, 0)]
                for lvl in self._levels:
                    sq = _lse_fold(sq, d[lvl], sq[s[lvl]] + w[lvl])
            cells[r, 0], cells[r, 1] = sq, px
            Y = self.columnSums(px)
        return cells, float(cells[L, 0, S - 1]), float(Y[S - 1])


class MergedProfilePrefixDP(PrefixDP):
    """The node fill against a CTC-MERGED profile (profile.Profile.mergeRows: rows of nCols + 1 log weights, column 0 the blank,
    column c the CSV column whose output token is colTok[c - 1]): the prefix search on compose(M, merging recogniser) with an
    empty output (docs/decoding.md, "Decoding against a merged profile").  A node gains the "last column seen" axis of
    profile.MergedProfileDP -- plane 0 = blank or no row yet, plane c = the last row took column c -- and keeps the two stages
    of ProfilePrefixDP: the blank and the repeat read the ARRIVED stage (N, Xn), never W or X.  With excl_c(V)[s] the sum of
    V[k][s] over the planes k != c:

        An[r][0][d] = [root, r = 0, d = 0]
        An[r][c][d] = sum_{t: s->d, in = a, out = colTok[c]} excl_c(Pa.W[r-1])[s] + w_t + P[r-1][c]
        Aw[r][p][d] = sum_{t: s->d, in = a, out = eps} Pa.W[r][p][s] + w_t
        N[r][0][d]  = An[r][0][d] (+) (+)_p (N[r-1][p][d] + P[r-1][0])
        N[r][c][d]  = An[r][c][d] (+) (N[r-1][c][d] + P[r-1][c]) (+) sum_{t: in = eps, out = colTok[c]} excl_c(W[r-1])[s] + w_t + P[r-1][c]
        W[r][p][d]  = Aw[r][p][d] (+) N[r][p][d] (+) sum_{silent t: s->d, s < d} W[r][p][s] + w_t
        Xn[r][0][d] = An[r][0][d] (+) (+)_p (Xn[r-1][p][d] + P[r-1][0])
        Xn[r][c][d] = An[r][c][d] (+) (Xn[r-1][c][d] + P[r-1][c]) (+) sum_{t: any in, out = colTok[c]} excl_c(Y[r-1])[s] + w_t + P[r-1][c]
        X[r][p][d]  = Aw[r][p][d] (+) Xn[r][p][d]
        Y[r][p][s]  = logsum_q X[r][p][q] + R[q][s]
        logSeqProb  = (+)_p W[L][p][S-1],     logPrefixProb = (+)_p Y[L][p][S-1]

    ``fill(P, parentCells, a)`` -> (cells[L+1][2][nCols+1][S], logSeqProb, logPrefixProb); layer 0 = W, layer 1 = X."""

    def __init__(self, em: EvaluatedMachine, colTok: Sequence[int], logR: Optional[np.ndarray] = None):
        super().__init__(em, logR)
        self.colTok = np.asarray(colTok, np.int64).reshape(-1)
        if len(self.colTok) and (self.colTok.min() < 1 or self.colTok.max() > em.nOutTok):
            raise MachineError("column token outside 1..nOutTok")
        self.nCols = len(self.colTok)
        self.PL = self.nCols + 1
        self._all = np.arange(self.S, dtype=np.int64)

    def _excl(self, V: np.ndarray) -> np.ndarray:
        """[nCols, S]: row c - 1 is the sum of the planes of V other than c."""
        out = np.full((self.nCols, self.S), _NEG)
        for c in range(1, self.PL):
            out[c - 1] = _red_planes(V[[k for k in range(self.PL) if k != c]], False)
        return out

    def fill(self, P, parent: Optional[np.ndarray] = None, a: int = 0) -> Tuple[np.ndarray, float, float]:
        P = np.asarray(P, np.float64).reshape(-1, self.PL)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        L, S, PL = len(P), self.S, self.PL
        cells = np.full((L + 1, 2, PL, S), _NEG)
        N = Xn = Y = np.full((PL, S), _NEG)
        for r in range(L + 1):
            An, Aw = np.full((PL, S), _NEG), np.full((PL, S), _NEG)
            if parent is None:
                if r == 0:
                    An[0, 0] = 0.0
            else:
                s, d, w = self._edges(a, 0)
                for p in range(PL):
                    Aw[p] = _lse_fold(Aw[p], d, parent[r, 0, p][s] + w)
                if r:
                    ex = self._excl(parent[r - 1, 0])
                    for c in range(1, PL):
                        s, d, w = self._edges(a, int(self.colTok[c - 1]))
                        An[c] = _lse_fold(An[c], d, (ex[c - 1][s] + w) + P[r - 1][c])
            if r:
                Pr = P[r - 1]
                exW, exY = self._excl(cells[r - 1, 0]), self._excl(Y)
                Nn, Xnn = np.empty((PL, S)), np.empty((PL, S))
                Nn[0] = _red_planes(np.concatenate([An[:1], N + Pr[0]]), False)
                Xnn[0] = _red_planes(np.concatenate([An[:1], Xn + Pr[0]]), False)
                for c in range(1, PL):
                    tok = int(self.colTok[c - 1])
                    s, d, w = self._edges(0, tok)
                    Nn[c] = _lse_fold(An[c], np.concatenate([self._all, d]), np.concatenate([N[c] + Pr[c], (exW[c - 1][s] + w) + Pr[c]]))
                    s, d, w = self._anyIn[tok]
                    Xnn[c] = _lse_fold(An[c], np.concatenate([self._all, d]), np.concatenate([Xn[c] + Pr[c], (exY[c - 1][s] + w) + Pr[c]]))
                N, Xn = Nn, Xnn
            else:
                N = Xn = An
            Y = np.empty((PL, S))
            for p in range(PL):
                sq, px = _lse_fold(Aw[p], self._all, N[p]), _lse_fold(Aw[p], self._all, Xn[p])
                if self._levels:
                    s, d, w = self._by[(0, 0)]
                    for lvl in self._levels:
                        sq = _lse_fold(sq, d[lvl], sq[s[lvl]] + w[lvl])
                cells[r, 0, p], cells[r, 1, p] = sq, px
                Y[p] = self.columnSums(px)
        return cells, float(_red_planes(cells[L, 0, :, S - 1:S], False)[0]), float(_red_planes(Y[:, S - 1:S], False)[0])


# ---- backends: who keeps the lattices ----------------------------------------------------------------------------------------
class NumpyNodes:
    """Node lattices on the host, filled by PrefixDP (token outputs) or ProfilePrefixDP (``profiles``: one [rows, nOutTok + 1]
    array of log weights per search) or, with ``colTok``, MergedProfilePrefixDP ([rows, nCols + 1] arrays); the same interface and
    the same fixed pool size as the device backend."""

    def __init__(self, em: EvaluatedMachine, outputs: Optional[Sequence[Sequence[int]]], logR: np.ndarray, maxNodes: int, profiles=None,
                 colTok=None):
        if colTok is not None:
            self.dp = MergedProfilePrefixDP(em, colTok, logR)
            self.outputs = [np.asarray(p, np.float64).reshape(-1, self.dp.PL) for p in profiles]
        elif profiles is not None:
            self.dp = ProfilePrefixDP(em, logR)
            self.outputs = [np.asarray(p, np.float64).reshape(-1, em.nOutTok + 1) for p in profiles]
        else:
            self.dp = PrefixDP(em, logR)
            self.outputs = [np.asarray(o, np.int64) for o in outputs]
        self.maxNodes = int(maxNodes)
        self.cells: Dict[int, np.ndarray] = {}
        self._free = list(range(self.maxNodes - 1, -1, -1))

    def _take(self, n: int) -> List[int]:
        if n > len(self._free):
            raise MachineError("prefix node pool is full (%d nodes, %d free, %d wanted)" % (self.maxNodes, len(self._free), n))
        return [self._free.pop() for _ in range(n)]

    def root(self, seq: int = 0) -> Tuple[int, float, float]:
        (slot,) = self._take(1)
        self.cells[slot], a, b = self.dp.fill(self.outputs[seq])
        return slot, a, b

    def extend(self, seq, parent, inTok):
        slots = self._take(len(seq))
        lsp, lpp = np.empty(len(seq)), np.empty(len(seq))
        for k, (q, p, t) in enumerate(zip(seq, parent, inTok)):
            self.cells[slots[k]], lsp[k], lpp[k] = self.dp.fill(self.outputs[q], self.cells[int(p)], int(t))
        return np.array(slots, np.int64), lsp, lpp

    def release(self, nodes) -> None:
        for n in nodes:
            del self.cells[int(n)]
            self._free.append(int(n))

    def free_nodes(self) -> int:
        return len(self._free)

    def node_cells(self, node: int, seq: int) -> np.ndarray:
        return self.cells[int(node)]

    def close(self) -> None:
        self.cells.clear()


def makeNodes(em: EvaluatedMachine, outputs=None, backend: str = "device", maxNodes: Optional[int] = None, logR: Optional[np.ndarray] = None,
              profiles=None, colTok=None):
    """The lattice store of ``len(outputs)`` searches: "numpy" (host, PrefixDP) or "device" (capi.DevicePrefix, mb_prefix.hip).
    With ``profiles`` (one [rows, nOutTok + 1] array of log weights per search, column 0 the blank) the searches decode soft
    outputs and ``outputs`` is not read; with ``colTok`` as well the profiles are CTC-merged: [rows, nCols + 1] tables and the
    column map of profile.Profile.mergeRows (a slot then has nCols + 1 planes).
    ``maxNodes`` None: DEFAULT_MAX_NODES per search, on the device no more than half the memory budget holds (a slot is
    2 (maxL + 1) S doubles, so long outputs on large machines get fewer); a number is taken as it is and fails if it does not fit."""
    R = logSumInTrans(em) if logR is None else logR
    if colTok is not None and profiles is None:
        raise MachineError("a column map needs profiles")
    planes = 1 if colTok is None else len(np.asarray(colTok).reshape(-1)) + 1
    if profiles is not None:
        outputs = [np.asarray(p, np.float64).reshape(-1, em.nOutTok + 1 if colTok is None else planes) for p in profiles]     # (only their lengths are read below)
    want = DEFAULT_MAX_NODES * max(1, len(outputs)) if maxNodes is None else int(maxNodes)
    if backend == "numpy":
        return NumpyNodes(em, outputs, R, want, profiles, colTok)
    if backend != "device":
        raise MachineError("unknown prefix search backend %s" % backend)
    from . import capi, dp
    dm = dp._device_machine(em)
    if maxNodes is None:
        slot = 16 * (max([len(o) for o in outputs] + [0]) + 1) * em.nStates * planes
        want = max(len(outputs) * (em.nInTok + 1), min(want, capi.memory_budget() // 2 // slot))
    return capi.DevicePrefix(dm, outputs, R, want, profiles, colTok)


# ---- std::push_heap / pop_heap / make_heap as libstdc++ orders them: which of two equal prefixes comes out first is theirs -------
def _push_heap(v: list, hole: int, top: int, value, less) -> None:
    parent = (hole - 1) // 2
    while hole > top and less(v[parent], value):
        v[hole] = v[parent]
        hole = parent
        parent = (hole - 1) // 2
    v[hole] = value


def _adjust_heap(v: list, hole: int, n: int, value, less) -> None:
    top, child = hole, hole
    while child < (n - 1) // 2:
        child = 2 * (child + 1)
        if less(v[child], v[child - 1]):
            child -= 1
        v[hole] = v[child]
        hole = child
    if n % 2 == 0 and child == (n - 2) // 2:
        child = 2 * (child + 1)
        v[hole] = v[child - 1]
        hole = child - 1
    _push_heap(v, hole, top, value, less)


def _make_heap(v: list, less) -> None:
    n = len(v)
    if n < 2:
        return
    parent = (n - 2) // 2
    while True:
        _adjust_heap(v, parent, n, v[parent], less)
        if parent == 0:
            return
        parent -= 1


class _Node:
    __slots__ = ("inTok", "parent", "length", "slot", "logSeqProb", "logPrefixProb", "extended", "child", "alive")

    def __init__(self, inTok: int, parent: Optional["_Node"], slot: int, lsp: float, lpp: float):
        self.inTok, self.parent, self.slot = inTok, parent, slot
        self.length = parent.length + 1 if parent else 0
        self.logSeqProb, self.logPrefixProb = lsp, lpp
        self.extended = False
        self.child: List["_Node"] = []
        self.alive = True

    def traceback(self) -> List[int]:
        out, n = [], self
        while n.inTok:
            out.append(n.inTok)
            n = n.parent
        return out[::-1]


_less = lambda x, y: x.logPrefixProb < y.logPrefixProb


def _logRows(em: EvaluatedMachine, profile, colTok=None) -> np.ndarray:
    """The table of a profile: logRows, or with a column map the table of mergeRows (whose map must be that one)."""
    if colTok is None:
        return profile.logRows(em) if hasattr(profile, "logRows") else np.asarray(profile, np.float64).reshape(-1, em.nOutTok + 1)
    colTok = np.asarray(colTok).reshape(-1)
    if not hasattr(profile, "mergeRows"):
        return np.asarray(profile, np.float64).reshape(-1, len(colTok) + 1)
    P, ct = profile.mergeRows(em)
    if not np.array_equal(ct, colTok):
        raise MachineError("the profile's columns are not the column map of the batch")
    return P


class PrefixTree:
    """One search (src/ctc.cpp:112-395) over a lattice store.  The order of operations is the reference's and decides ties:
    children are made for input tokens 1..nIn in order, a child enters the heap only if its prefix probability exceeds the best
    sequence so far, and the best sequence is replaced only on strict improvement.

    ``nodes`` is a lattice store (makeNodes) that may be shared with other searches; ``seq`` is this search's index in it."""

    def __init__(self, em: EvaluatedMachine, nodes, seq: int = 0, maxBacktrack: int = NO_BACKTRACK_LIMIT, owner: bool = False):
        self.em, self.nodes, self.seq, self.maxBacktrack, self._owner = em, nodes, seq, maxBacktrack, owner
        self.nIn = em.nInTok
        self.queue: List[_Node] = []
        self.bestSeqNode: Optional[_Node] = None
        self.bestLogSeqProb = _NEG
        self.maxPrefixLen = 0
        self.nFills = 0
        self.root: Optional[_Node] = None
        self.monotone = True                # no child's prefix probability rose above its parent's (+1e-12)

    @classmethod
    def forOutput(cls, em: EvaluatedMachine, outSym: Sequence[str], maxBacktrack: int = NO_BACKTRACK_LIMIT, backend: str = "device",
                  maxNodes: Optional[int] = None) -> "PrefixTree":
        """PrefixTree(machine, outSym, maxBacktrack): a search with a lattice store of its own."""
        t = cls(em, makeNodes(em, [em.outputTokenizer.tokenize(list(outSym))], backend, maxNodes), 0, maxBacktrack, owner=True)
        t.start()
        return t

    @classmethod
    def forProfile(cls, em: EvaluatedMachine, profile, maxBacktrack: int = NO_BACKTRACK_LIMIT, backend: str = "device",
                   maxNodes: Optional[int] = None, colTok=None) -> "PrefixTree":
        """A search for the most likely input given a PROFILE: a profile.Profile, or its [rows, nOutTok + 1] log-weight table.
        With ``colTok`` the profile is CTC-merged: a Profile read through mergeRows, or its [rows, nCols + 1] table."""
        t = cls(em, makeNodes(em, None, backend, maxNodes, profiles=[_logRows(em, profile, colTok)], colTok=colTok), 0, maxBacktrack, owner=True)
        t.start()
        return t

    def close(self) -> None:
        if self._owner and self.nodes is not None:
            self.nodes.close()
        self.nodes = None

    # -- the three steps a lock-step driver interleaves: start, request, absorb --
    def start(self) -> None:
        slot, lsp, lpp = self.nodes.root(self.seq)
        self.root = self._admit(None, 0, slot, lsp, lpp)

    def nextParent(self) -> Optional[_Node]:
        """The loop head of doPrefixSearch: the best open prefix if it can still beat the best sequence, else None (finished)."""
        if not self.queue:
            return None
        parent = self.queue[0]
        last = self.queue.pop()                      # pop_heap + pop_back
        if self.queue:
            _adjust_heap(self.queue, 0, len(self.queue), last, _less)
        if parent.logPrefixProb > self.bestLogSeqProb:
            return parent
        return None

    def missingTokens(self, parent: _Node) -> List[int]:
        have = {c.inTok for c in parent.child}
        return [t for t in range(1, self.nIn + 1) if t not in have]

    def absorb(self, parent: _Node, toks: Sequence[int], slots, lsp, lpp) -> None:
        """extendNode (src/ctc.cpp:305-329) once the fills of the missing children are back."""
        for t, s, a, b in zip(toks, slots, lsp, lpp):
            self._admit(parent, int(t), int(s), float(a), float(b))
        parent.extended = True
        if self.maxPrefixLen > parent.length:
            minLen = 0 if self.maxPrefixLen < self.maxBacktrack else self.maxPrefixLen - self.maxBacktrack
            if minLen:
                keep = []
                for n in self.queue:
                    if n.length >= minLen:
                        keep.append(n)
                    else:
                        self._remove(n)
                _make_heap(keep, _less)
                self.queue = keep

    def _admit(self, parent: Optional[_Node], tok: int, slot: int, lsp: float, lpp: float) -> _Node:
        """addNode (src/ctc.cpp:342-379) after the fill."""
        n = _Node(tok, parent, slot, lsp, lpp)
        self.nFills += 1
        if parent is not None:
            parent.child.append(n)
            if lpp > parent.logPrefixProb + 1e-12:
                self.monotone = False
        self.maxPrefixLen = max(self.maxPrefixLen, n.length)
        if lpp > self.bestLogSeqProb:
            self.queue.append(n)
            _push_heap(self.queue, len(self.queue) - 1, 0, n, _less)
        if lsp > self.bestLogSeqProb:
            old = self.bestSeqNode
            self.bestSeqNode, self.bestLogSeqProb = n, lsp
            if old is not None and old.extended:
                self._remove(old)
        return n

    def _remove(self, n: _Node) -> None:
        """removeNode (src/ctc.cpp:381-391): a childless node that is not the best sequence goes, and so up the tree."""
        while n is not self.bestSeqNode and not n.child and n.alive:
            n.alive = False
            self.nodes.release([n.slot])
            if n.parent is None:
                break
            n.parent.child.remove(n)
            n = n.parent

    def _extend(self, parent: _Node) -> None:
        toks = self.missingTokens(parent)
        slots, lsp, lpp = self.nodes.extend([self.seq] * len(toks), [parent.slot] * len(toks), toks) if toks else ([], [], [])
        self.absorb(parent, toks, slots, lsp, lpp)

    # -- the reference's public interface --
    def doPrefixSearch(self) -> List[str]:
        while True:
            parent = self.nextParent()
            if parent is None:
                break
            self._extend(parent)
        if self.bestSeqNode is None:
            raise MachineError("No valid sequence found")
        return self.bestSeq()

    def bestSeq(self) -> List[str]:
        return self.em.inputTokenizer.detokenize(self.bestSeqNode.traceback())

    def _child(self, parent: _Node, tok: int) -> _Node:
        for c in parent.child:
            if c.inTok == tok:
                return c
        slots, lsp, lpp = self.nodes.extend([self.seq], [parent.slot], [tok])
        return self._admit(parent, tok, int(slots[0]), float(lsp[0]), float(lpp[0]))

    def logSeqProb(self, inTok: Sequence[int]) -> float:
        """log P(x, y) of the input token sequence x, through (and extending) the tree (src/ctc.cpp:298-303)."""
        cur = self.root
        for t in inTok:
            cur = self._child(cur, int(t))
        return cur.logSeqProb

    def sampleTokSeq(self, rng) -> List[int]:
        """src/ctc.cpp:157-167 with randomChild (:101-110): walks down, at every node choosing a child in proportion to its
        prefix probability or stopping there with the rest.  ``rng()`` gives uniform variates in [0, 1)."""
        cur = self.root
        while cur.logPrefixProb > cur.logSeqProb:
            self._extend(cur)
            r = rng()
            nxt = None
            for c in cur.child:
                r -= math.exp(c.logPrefixProb - cur.logPrefixProb)
                if not r > 0:
                    nxt = c
                    break
            if nxt is None:
                break
            cur = nxt
        return cur.traceback()

    def sampleSeq(self, rng) -> List[str]:
        return self.em.inputTokenizer.detokenize(self.sampleTokSeq(rng))


def decodeBatch(em: EvaluatedMachine, outputs: Optional[Sequence[Sequence[str]]], maxBacktrack: int = NO_BACKTRACK_LIMIT, backend: str = "device",
                maxNodes: Optional[int] = None, profiles=None, colTok=None) -> Tuple[List[List[str]], List[PrefixTree]]:
    """doPrefixSearch for every output at once, in lock step: per round every unfinished search names the prefix it extends, and
    ONE ``extend`` (one device launch) fills the children of all of them.  A search sees exactly the fills, in the order, that it
    would see alone, so its answer and its node count are those of a single search.  Returns (decoded inputs, the searches).
    ``profiles`` (profile.Profile objects or log-weight tables) in place of ``outputs`` decodes soft outputs; with ``colTok`` they are
    CTC-merged profiles (mergeRows tables, or Profile objects read through mergeRows) under that one column map."""
    if profiles is not None:
        toks = [_logRows(em, p, colTok) for p in profiles]
        nodes = makeNodes(em, None, backend, maxNodes, profiles=toks, colTok=colTok)
    else:
        toks = [em.outputTokenizer.tokenize(list(o)) for o in outputs]
        nodes = makeNodes(em, toks, backend, maxNodes)
    trees = [PrefixTree(em, nodes, k, maxBacktrack) for k in range(len(toks))]
    try:
        for t in trees:
            t.start()
        live = list(trees)
        while live:
            work = []
            for t in live:
                p = t.nextParent()
                if p is not None:
                    work.append((t, p, t.missingTokens(p)))
            if not work:
                break
            seq = [t.seq for t, p, ks in work for _ in ks]
            par = [p.slot for t, p, ks in work for _ in ks]
            tok = [k for t, p, ks in work for k in ks]
            slots, lsp, lpp = nodes.extend(seq, par, tok) if seq else ([], [], [])
            at = 0
            for t, p, ks in work:
                n = len(ks)
                t.absorb(p, ks, slots[at:at + n], lsp[at:at + n], lpp[at:at + n])
                at += n
            live = [t for t, _, _ in work]
        for t in trees:
            if t.bestSeqNode is None:
                raise MachineError("No valid sequence found")
        return [t.bestSeq() for t in trees], trees
    finally:
        nodes.close()
