"""Profile tapes: a machine with an empty input tape scored against a soft output sequence (docs/profile_tapes.md).

A profile is a table of per-row symbol weights -- a basecaller's output, say -- instead of a string of tokens.  The reference
reads it with ``--recognize-csv`` (target/boss.cpp:606-611, src/csv.cpp:8-72) into an (L+1)-state recogniser and composes that
onto the model.  Here the DP runs natively over the (L+1) x 2 x S lattice of the model itself (mb_profile.hip); this module holds
the CSV reader, the row table the device reads, the recogniser (for the composition cross-check) and a numpy restatement of the
recurrence -- the yardstick of the device sweeps:

    N[0][q]   = 0 if q == 0 else -inf
    W[r][q]   = N[r][q] (+) sum_{silent t: s->q, s < q} W[r][s] + w_t
    N[r+1][q] = (N[r][q] + P[r][0]) (+) sum_{t: s->q, in = eps, out = o != eps} (W[r][s] + w_t) + P[r][o]
    loglike   = W[L][S-1]

(+) is log-sum-exp (Forward) or max (Viterbi).  P[r][0] is the blank: the row is consumed and the machine does not move.

CTC-merged profiles (``--recognize-merge-csv``, src/csv.cpp:20-46; mb_profile_merge.hip) have the recogniser
(Profile.mergingMachine), the row table (Profile.mergeRows) and the yardstick (MergedProfileDP) here too.
"""
from __future__ import annotations

import math
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .evalmachine import EvaluatedMachine
from .machine import Machine, MachineError, MachineState, MachineTransition
from .seqpair import Envelope

_STOF = re.compile(r"[ \t\n\v\f\r]*([+-]?(?:inf(?:inity)?|nan|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?))", re.I)


def _split(s: str, splitChars: str) -> List[str]:
    """MachineBoss::split (src/util.cpp:71-85): runs of separators collapse, so there are no empty fields."""
    return [f for f in re.split("[" + re.escape(splitChars) + "]+", s) if f]


def _stof(s: str) -> float:
    """std::stof: the longest leading number (leading white space skipped, trailing text ignored), rounded to float32."""
    m = _STOF.match(s)
    if not m:
        raise MachineError("stof: no conversion of %r" % s)
    return float(np.float32(float(m.group(1))))


class Profile:
    """CSVProfile (src/csv.h): a header of symbols and rows of probabilities; column len(header) of a row is the blank."""

    def __init__(self, header: Sequence[str], rows: Sequence[Sequence[float]]):
        self.header = list(header)
        self.row = [list(r) for r in rows]

    @classmethod
    def fromCsv(cls, path: str, splitChars: str = ",") -> "Profile":
        """CSVProfile::read (src/csv.cpp:48-72): the header is split like the rows, trailing empty header fields dropped
        (a no-op after split, kept for the record); rows that split to nothing are skipped."""
        with open(path, "rb") as f:
            lines = f.read().decode("latin-1").split("\n")
        if lines and lines[-1] == "":
            lines.pop()            # getline yields no line after the final newline
        header = _split(lines[0], splitChars) if lines else []
        while header and not header[-1]:
            header.pop()
        rows = []
        for line in lines[1:]:
            cols = _split(line, splitChars)
            if cols:
                rows.append([_stof(c) for c in cols])
        return cls(header, rows)

    def __len__(self) -> int:
        return len(self.row)

    def logRows(self, em: EvaluatedMachine) -> np.ndarray:
        """[rows, nOutTok + 1] log weights in the machine's output alphabet: column 0 the blank (header column len(header);
        0 if the row is shorter), column t the output token t (the sum over header columns of that symbol; 0 if none or the row
        is shorter).  Header symbols outside the alphabet are dropped; columns beyond the blank are ignored."""
        return self._logRows(em.outputTokenizer.tok2sym)

    def _logRows(self, syms: Sequence[str]) -> np.ndarray:
        cols: List[List[int]] = [[len(self.header)]] + [[c for c, h in enumerate(self.header) if h == syms[t]] for t in range(1, len(syms))]
        P = np.empty((len(self.row), len(cols)), np.float64)
        for r, row in enumerate(self.row):
            for t, cs in enumerate(cols):
                v = sum(row[c] for c in cs if c < len(row))
                if v < 0 or math.isnan(v):
                    raise MachineError("Profile row %d: weight %g is not a probability" % (r, v))
                P[r, t] = math.log(v) if v > 0 else -math.inf
        return P

    def logRowsIn(self, em: EvaluatedMachine) -> np.ndarray:
        """[rows, nInTok + 1] log weights in the machine's INPUT alphabet, by the rules of logRows: the profile as the generator
        of ``--generate-csv`` (docs/profile_tapes.md, "Pairs of profiles").  Column 0 is the blank."""
        return self._logRows(em.inputTokenizer.tok2sym)

    def machine(self) -> Machine:
        """CSVProfile::machine (src/csv.cpp:8-18): the profile as a generator of L+1 states."""
        m = Machine()
        for pos in range(len(self.row) + 1):
            ms = MachineState(); ms.name = str(pos)
            m.state.append(ms)
        for pos, row in enumerate(self.row):
            for col in range(min(len(row), len(self.header) + 1)):
                m.state[pos].trans.append(MachineTransition(dest=pos + 1, inp="", out=self.header[col] if col < len(self.header) else "",
                                                            weight=row[col]))
        return m

    def recogniserMachine(self) -> Machine:
        """CSVProfile::machine().transpose() -- what ``--recognize-csv`` composes onto the model."""
        m = self.machine()
        for ms in m.state:
            ms.trans = [MachineTransition(dest=t.dest, inp=t.out, out=t.inp, weight=t.weight) for t in ms.trans]
        return m

    def mergingMachine(self) -> Machine:
        """CSVProfile::mergingMachine (src/csv.cpp:20-46): the profile as a CTC generator.  State (pos, tok) = "row pos - 1 took
        column tok" (tok = len(header): the blank); a row that repeats the last column, or takes the blank, emits nothing.  All
        columns of the last row lead to the one end state: (L - 1)(nCols + 1) + 2 states for L >= 1 rows."""
        if not self.header:
            raise MachineError("Need header to build mergingMachine from CSVProfile")
        nCols, nRows = len(self.header), len(self.row)

        def index(pos: int, tok: int) -> int:
            return 0 if pos == 0 else (pos - 1) * (nCols + 1) + (0 if pos == nRows else tok) + 1
        m = Machine()
        for _ in range(index(nRows, 0) + 1):
            m.state.append(MachineState())
        for pos in range(1, nRows):
            for tok in range(nCols + 1):
                m.state[index(pos, tok)].name = [pos, "" if tok == nCols else self.header[tok]]
        m.state[0].name = "START"
        m.state[-1].name = "END"
        for pos, row in enumerate(self.row):
            for col in range(min(len(row), nCols + 1)):
                dest = index(pos + 1, col)
                for tok in range((nCols if pos else 0) + 1):
                    emit = "" if (col == tok and pos > 0) or col == nCols else self.header[col]
                    m.state[index(pos, tok)].trans.append(MachineTransition(dest=dest, inp="", out=emit, weight=row[col]))
        return m

    def mergingRecogniserMachine(self) -> Machine:
        """CSVProfile::mergingMachine().transpose() -- what ``--recognize-merge-csv`` composes onto the model."""
        m = self.mergingMachine()
        for ms in m.state:
            ms.trans = [MachineTransition(dest=t.dest, inp=t.out, out=t.inp, weight=t.weight) for t in ms.trans]
        return m

    def mergeRows(self, em: EvaluatedMachine) -> Tuple[np.ndarray, np.ndarray]:
        """(logP[rows, nCols + 1], colTok[nCols]) for the merged (CTC) sweeps: the header columns whose symbol is in the machine's
        output alphabet, in header order, as columns 1..nCols with colTok[c - 1] their output token; column 0 the blank (header
        column len(header)).  A symbol that heads two columns gives two columns (they do not merge with each other); short rows
        weigh 0; columns beyond the blank are ignored."""
        if not self.header:
            raise MachineError("Need header to build mergingMachine from CSVProfile")
        tok = {s: t for t, s in enumerate(em.outputTokenizer.tok2sym) if t}
        cols = [len(self.header)] + [c for c, h in enumerate(self.header) if h in tok]
        P = np.empty((len(self.row), len(cols)), np.float64)
        for r, row in enumerate(self.row):
            for k, c in enumerate(cols):
                v = row[c] if c < len(row) else 0.0
                if v < 0 or math.isnan(v):
                    raise MachineError("Profile row %d: weight %g is not a probability" % (r, v))
                P[r, k] = math.log(v) if v > 0 else -math.inf
        return P, np.array([tok[self.header[c]] for c in cols[1:]], np.int32)


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
_NEG = -math.inf
_TABLE: Optional[np.ndarray] = None


def table_log_sum_exp(a: float, b: float) -> float:
    """The reference's log_sum_exp (src/logsumexp.h:72-90, mb_log_sum_exp): max + log(1 + exp(-d)) from a 100 001-entry table at
    step 1e-4 with linear interpolation, 0 for d >= 10 -- which drops terms more than 10 nats below the running maximum."""
    global _TABLE
    if _TABLE is None:
        _TABLE = np.append(np.log1p(np.exp(-(np.arange(100001) * 1e-4))), 0.0)
    if a == b:
        mx, d = a, 0.0
    elif a < b:
        mx, d = b, b - a
    else:
        mx, d = a, a - b
    if d >= 10.0 or math.isnan(d) or math.isinf(d):
        return mx
    n = int(d / 1e-4)
    f0, f1 = _TABLE[n], _TABLE[n + 1]
    return mx + (f0 + (f1 - f0) * ((d - n * 1e-4) / 1e-4))


_M32 = 0xffffffff


def philox4x32(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """Philox4x32-10 (Salmon et al., SC'11): four 32-bit counter words and two key words to four output words.  The restatement of
    philox_uniform's rounds in mb_profile_common.h (docs/profile_tapes.md, "Posterior path samples")."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def sample_uniform(seed: int, k: int, j: int, t: int) -> float:
    """The uniform in [0, 1) of decision ``t`` of sample ``j`` of pair ``k``: key (seed & 0xffffffff, seed >> 32), counter
    (t, j, k & 0xffffffff, k >> 32), and the 53-bit recipe of the Mt19937 variates on the first two output words."""
    seed, k = int(seed) & 0xffffffffffffffff, int(k) & 0xffffffffffffffff
    x0, x1, _, _ = philox4x32((t, j, k & _M32, k >> 32), (seed & _M32, seed >> 32))
    return ((x0 >> 5) * 67108864 + (x1 >> 6)) * (1.0 / 9007199254740992.0)


def _lse_fold(base: np.ndarray, idx: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """out[q] = log(exp(base[q]) + sum_{k: idx[k] = q} exp(vals[k])), exactly (max-shifted); out[q] = base[q] where no term."""
    if len(idx) == 0:
        return base.copy()
    m = base.copy()
    np.maximum.at(m, idx, vals)
    fin = m > _NEG
    ms = np.where(fin, m, 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        acc = np.where(base > _NEG, np.exp(base - ms), 0.0)
        np.add.at(acc, idx, np.exp(vals - ms[idx]))
        return np.where(fin, ms + np.log(acc), _NEG)


def _max_fold(base: np.ndarray, idx: np.ndarray, vals: np.ndarray) -> np.ndarray:
    out = base.copy()
    if len(idx):
        np.maximum.at(out, idx, vals)
    return out


class ProfileDP:
    """Forward / Backward / Viterbi (first-maximum traceback) / posterior counts of one machine against profiles, in numpy.

    ``mode``: "exact" (exact log-sum-exp), "table" (the reference's table log_sum_exp, accumulated in the device's candidate
    order: the blank, then emitting edges in `incoming` order; then "no move", then silent edges) or "max" (Viterbi)."""

    def __init__(self, em: EvaluatedMachine):
        self.em = em
        self.S = em.nStates
        order = em.incomingOrder()
        it, ot, src, dst = em.inTok[order], em.outTok[order], em.src[order].astype(np.int64), em.dst[order].astype(np.int64)
        em_ = (it == 0) & (ot > 0)
        si = (it == 0) & (ot == 0) & (src < dst)
        self.eId, self.eS, self.eD = order[em_], src[em_], dst[em_]
        self.eW, self.eO = em.logWeight[self.eId], ot[em_].astype(np.int64)
        self.sId, self.sS, self.sD = order[si], src[si], dst[si]
        self.sW = em.logWeight[self.sId]
        lvF = em.silentLevels()
        self.fLevels = [np.nonzero(lvF[self.sD] == l)[0] for l in range(1, int(lvF.max(initial=0)) + 1)]
        lvB = np.zeros(self.S, np.int64)
        for k in sorted(range(len(self.sS)), key=lambda k: -int(self.sS[k])):
            s, d = int(self.sS[k]), int(self.sD[k])
            lvB[s] = max(lvB[s], lvB[d] + 1)
        self.bLevels = [np.nonzero(lvB[self.sS] == l)[0] for l in range(1, int(lvB.max(initial=0)) + 1)]
        # per destination, candidates in `incoming` order (table mode and the traceback)
        self.inEmit: List[List[int]] = [[] for _ in range(self.S)]
        self.inSil: List[List[int]] = [[] for _ in range(self.S)]
        for k, d in enumerate(self.eD):
            self.inEmit[int(d)].append(k)
        for k, d in enumerate(self.sD):
            self.inSil[int(d)].append(k)

    def _check(self, P) -> np.ndarray:
        P = np.asarray(P, np.float64).reshape(-1, self.em.nOutTok + 1)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        return P

    def forward(self, P, mode: str = "exact") -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, N[L+1][S], W[L+1][S])."""
        P = self._check(P)
        if mode == "table":
            return self._forward_table(P)
        fold = _max_fold if mode == "max" else _lse_fold
        L, S = len(P), self.S
        N = np.full((L + 1, S), _NEG); W = np.full((L + 1, S), _NEG)
        N[0, 0] = 0.0
        for r in range(L + 1):
            if r:
                Pr = P[r - 1]
                N[r] = fold(N[r - 1] + Pr[0], self.eD, (W[r - 1][self.eS] + self.eW) + Pr[self.eO])
            w = N[r].copy()
            for lv in self.fLevels:
                w = fold(w, self.sD[lv], w[self.sS[lv]] + self.sW[lv])
            W[r] = w
        return float(W[L, S - 1]), N, W

    def _forward_table(self, P: np.ndarray) -> Tuple[float, np.ndarray, np.ndarray]:
        L, S = len(P), self.S
        N = np.full((L + 1, S), _NEG); W = np.full((L + 1, S), _NEG)
        N[0, 0] = 0.0
        lvF = self.em.silentLevels()
        stateOrder = sorted(range(S), key=lambda q: (int(lvF[q]), q))
        eS, eW, eO, sS, sW = self.eS.tolist(), self.eW.tolist(), self.eO.tolist(), self.sS.tolist(), self.sW.tolist()
        for r in range(L + 1):
            if r:
                Pr = P[r - 1].tolist(); Wp = W[r - 1].tolist(); Np = N[r - 1].tolist()
                row = N[r]
                for q in range(S):
                    acc = Np[q] + Pr[0]
                    for k in self.inEmit[q]:
                        acc = table_log_sum_exp(acc, (Wp[eS[k]] + eW[k]) + Pr[eO[k]])
                    row[q] = acc
            Wr = W[r]; Nr = N[r]
            for q in stateOrder:
                acc = Nr[q]
                for k in self.inSil[q]:
                    acc = table_log_sum_exp(acc, Wr[sS[k]] + sW[k])
                Wr[q] = acc
        return float(W[L, S - 1]), N, W

    def backward(self, P) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, NB[L+1][S], WB[L+1][S]), exact log-sum-exp."""
        P = self._check(P)
        L, S = len(P), self.S
        NB = np.full((L + 1, S), _NEG); WB = np.full((L + 1, S), _NEG)
        for r in range(L, -1, -1):
            base = np.full(S, _NEG)
            if r == L:
                base[S - 1] = 0.0
            else:
                base = _lse_fold(base, self.eS, (self.eW + P[r][self.eO]) + NB[r + 1][self.eD])
            for lv in self.bLevels:
                base = _lse_fold(base, self.sS[lv], base[self.sD[lv]] + self.sW[lv])
            WB[r] = base
            NB[r] = np.logaddexp(base, P[r][0] + NB[r + 1]) if r < L else base
        return float(NB[0, 0]), NB, WB

    def counts(self, P) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf profile."""
        P = self._check(P)
        ll, _, WF = self.forward(P)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB = self.backward(P)
        with np.errstate(invalid="ignore"):
            for r in range(len(P) + 1):
                f = WF[r] - ll
                if r < len(P):
                    np.add.at(out, self.eId, np.exp(f[self.eS] + ((self.eW + P[r][self.eO]) + NB[r + 1][self.eD])))
                np.add.at(out, self.sId, np.exp(f[self.sS] + (WB[r][self.sD] + self.sW)))
        return out, ll

    def rowPosteriors(self, P) -> Tuple[np.ndarray, float]:
        """(post[L, nOutTok + 1], Forward loglike): post[r][o] is the posterior probability that row r was consumed as output token
        o (column 0: as the blank) -- the emitting terms of counts() and the blank term of backward(), binned by (row, column),
        which is the gradient of loglike in P[r][o] (docs/profile_tapes.md, "Row posteriors of one-tape profiles").  Every row
        sums to 1; zeros for a -inf profile; exactly 0 where P[r][o] is -inf."""
        P = self._check(P)
        ll, NF, WF = self.forward(P)
        post = np.zeros((len(P), self.em.nOutTok + 1))
        if not ll > _NEG:
            return post, ll
        _, NB, _ = self.backward(P)
        with np.errstate(invalid="ignore"):
            for r in range(len(P)):
                b = (NF[r] - ll) + (P[r][0] + NB[r + 1])
                post[r, 0] = float(np.exp(b[b > _NEG]).sum())
                t = (WF[r] - ll)[self.eS] + ((self.eW + P[r][self.eO]) + NB[r + 1][self.eD])
                np.add.at(post[r], self.eO[t > _NEG], np.exp(t[t > _NEG]))
        return post, ll

    def viterbi(self, P) -> Tuple[float, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, row at which each fired); the first maximum in the fill's candidate order."""
        P = self._check(P)
        v, N, W = self.forward(P, "max")
        edges: List[int] = []; rows: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32)
        r, q, layer = len(P), self.S - 1, 1
        while True:
            if layer == 1:
                cur = W[r, q]
                if N[r, q] == cur:
                    layer = 0
                    continue
                k = next(k for k in self.inSil[q] if W[r, self.sS[k]] + self.sW[k] == cur)
                edges.append(int(self.sId[k])); rows.append(r); q = int(self.sS[k])
            else:
                if r == 0:
                    assert q == 0
                    break
                Pr, cur = P[r - 1], N[r, q]
                if N[r - 1, q] + Pr[0] == cur:
                    r -= 1
                    continue
                k = next(k for k in self.inEmit[q] if (W[r - 1, self.eS[k]] + self.eW[k]) + Pr[self.eO[k]] == cur)
                r -= 1
                edges.append(int(self.eId[k])); rows.append(r); q = int(self.eS[k]); layer = 1
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32)


def _red_planes(A: np.ndarray, mx: bool) -> np.ndarray:
    """(+) over axis 0 of A[planes, S]: max, or the exact (max-shifted) log-sum-exp."""
    m = A.max(axis=0)
    if mx:
        return m
    fin = m > _NEG
    ms = np.where(fin, m, 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.where(fin, ms + np.log(np.exp(A - ms).sum(axis=0)), _NEG)


class MergedProfileDP(ProfileDP):
    """The merged (CTC) profile recurrence in numpy -- the yardstick of mb_profile_merge.hip (docs/profile_tapes.md, "Merged (CTC)
    profiles"): the semantics of compose(M, transpose(CSVProfile::mergingMachine())) with empty tapes.  Beside the S states of M
    the lattice has a "last column seen" axis of nCols + 1 planes: plane 0 = the last row took the blank (or no row yet), plane c
    = the last row took column c, whose output token is colTok[c - 1]:

        N[0][0][q]   = [q == 0], every other plane -inf
        W[r][p][q]   = N[r][p][q] (+) sum_{silent t: s->q, s < q} W[r][p][s] + w_t
        N[r+1][0][q] = (+)_p (N[r][p][q] + P[r][0])
        N[r+1][c][q] = (N[r][c][q] + P[r][c]) (+) sum_{t: s->q, in = eps, out = colTok[c]} (X[r][c][s] + w_t) + P[r][c]
        X[r][c][s]   = (+)_{k != c} W[r][k][s]
        loglike      = (+)_p W[L][p][S-1]

    Viterbi keeps the first maximum: W takes "no move" first, then silent edges in `incoming` order; N[.][0] the planes ascending;
    N[.][c] the repeat first, then emitting edges in `incoming` order, each from the lowest plane k != c that attains X; the end
    the planes ascending.  Lattices are [L + 1, nCols + 1, S]."""

    def __init__(self, em: EvaluatedMachine, colTok: Sequence[int]):
        super().__init__(em)
        self.colTok = np.asarray(colTok, np.int64).reshape(-1)
        if len(self.colTok) and (self.colTok.min() < 1 or self.colTok.max() > em.nOutTok):
            raise MachineError("column token outside 1..nOutTok")
        self.nCols = len(self.colTok)
        self.PL = self.nCols + 1
        # per column, the emitting edges of its token (positions in the `incoming`-ordered emitting list)
        self.colSel = [np.nonzero(self.eO == t)[0] for t in self.colTok]

    def _check(self, P) -> np.ndarray:
        P = np.asarray(P, np.float64).reshape(-1, self.PL)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        return P

    def _others(self, c: int) -> List[int]:
        return [k for k in range(self.PL) if k != c]

    def forward(self, P, mode: str = "exact") -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, N[L+1][nCols+1][S], W[L+1][nCols+1][S]); mode "exact" or "max"."""
        P = self._check(P)
        mx = mode == "max"
        fold = _max_fold if mx else _lse_fold
        L, S, PL = len(P), self.S, self.PL
        N = np.full((L + 1, PL, S), _NEG); W = np.full((L + 1, PL, S), _NEG)
        N[0, 0, 0] = 0.0
        for r in range(L + 1):
            if r:
                Pr, Np, Wp = P[r - 1], N[r - 1], W[r - 1]
                N[r, 0] = _red_planes(Np + Pr[0], mx)
                for c in range(1, PL):
                    X = _red_planes(Wp[self._others(c)], mx)
                    sel = self.colSel[c - 1]
                    N[r, c] = fold(Np[c] + Pr[c], self.eD[sel], (X[self.eS[sel]] + self.eW[sel]) + Pr[c])
            for p in range(PL):
                w = N[r, p].copy()
                for lv in self.fLevels:
                    w = fold(w, self.sD[lv], w[self.sS[lv]] + self.sW[lv])
                W[r, p] = w
        return float(_red_planes(W[L, :, S - 1:S], mx)[0]), N, W

    def backward(self, P) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, NB[L+1][nCols+1][S], WB[L+1][nCols+1][S]), exact log-sum-exp; loglike = NB[0][0][0]."""
        P = self._check(P)
        L, S, PL = len(P), self.S, self.PL
        NB = np.full((L + 1, PL, S), _NEG); WB = np.full((L + 1, PL, S), _NEG)
        for r in range(L, -1, -1):
            for k in range(PL):
                base = np.full(S, _NEG)
                if r == L:
                    base[S - 1] = 0.0
                else:
                    for c in range(1, PL):
                        if c != k:
                            sel = self.colSel[c - 1]
                            base = _lse_fold(base, self.eS[sel], (self.eW[sel] + P[r][c]) + NB[r + 1][c][self.eD[sel]])
                for lv in self.bLevels:
                    base = _lse_fold(base, self.sS[lv], base[self.sD[lv]] + self.sW[lv])
                WB[r, k] = base
                if r < L:
                    terms = [base, P[r][0] + NB[r + 1][0]] + ([P[r][k] + NB[r + 1][k]] if k else [])
                    NB[r, k] = _red_planes(np.stack(terms), False)
                else:
                    NB[r, k] = base
        return float(NB[0, 0, 0]), NB, WB

    def counts(self, P) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf profile."""
        P = self._check(P)
        ll, _, WF = self.forward(P)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB = self.backward(P)
        with np.errstate(invalid="ignore"):
            for r in range(len(P) + 1):
                for k in range(self.PL):
                    f = WF[r, k] - ll
                    if r < len(P):
                        for c in range(1, self.PL):
                            if c != k:
                                sel = self.colSel[c - 1]
                                np.add.at(out, self.eId[sel], np.exp(f[self.eS[sel]] + ((self.eW[sel] + P[r][c]) + NB[r + 1][c][self.eD[sel]])))
                    np.add.at(out, self.sId, np.exp(f[self.sS] + (WB[r, k][self.sD] + self.sW)))
        return out, ll

    def rowPosteriors(self, P, repeats: Optional[list] = None) -> Tuple[np.ndarray, float]:
        """(post[L, nCols + 1], Forward loglike): post[r][c] is the posterior probability that row r was consumed as column c
        (column 0: as the blank), the gradient of loglike in P[r][c] (docs/profile_tapes.md, "Row posteriors of one-tape
        profiles"): the blank out of every plane, and for a column its repeat (plane c stays) plus the fresh emissions of
        colTok[c - 1] out of every plane k != c -- the emitting terms of counts().  ``repeats``, if a list, receives the
        [L, nCols + 1] repeat part, so that post - repeats sums per token to the counts.  Every row sums to 1; zeros for a -inf
        profile; exactly 0 where P[r][c] is -inf."""
        P = self._check(P)
        ll, NF, WF = self.forward(P)
        L, PL = len(P), self.PL
        post = np.zeros((L, PL)); rep = np.zeros((L, PL))
        if repeats is not None:
            repeats.append(rep)
        if not ll > _NEG:
            return post, ll
        _, NB, _ = self.backward(P)
        with np.errstate(invalid="ignore"):
            for r in range(L):
                for k in range(PL):
                    n, f = NF[r, k] - ll, WF[r, k] - ll
                    b = n + (P[r][0] + NB[r + 1][0])
                    post[r, 0] += float(np.exp(b[b > _NEG]).sum())
                    if k:
                        b = n + (P[r][k] + NB[r + 1][k])
                        rep[r, k] = float(np.exp(b[b > _NEG]).sum())
                    for c in range(1, PL):
                        if c != k:
                            sel = self.colSel[c - 1]
                            t = f[self.eS[sel]] + ((self.eW[sel] + P[r][c]) + NB[r + 1][c][self.eD[sel]])
                            post[r, c] += float(np.exp(t[t > _NEG]).sum())
        post += rep
        return post, ll

    def viterbi(self, P, census: Optional[dict] = None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, row at which each fired); the first maximum in the fill's candidate order.  Blank
        and repeat rows are not edges.  ``census``: counts, by the candidate taken ("blank" / "repeat" / "emit" at an N cell,
        "stay" / "silent" at a W cell, "plane" for an emitting edge whose X has two attaining planes, "end"), the steps at which
        two or more candidates equal the cell."""
        P = self._check(P)
        v, N, W = self.forward(P, "max")
        edges: List[int] = []; rows: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32)

        def tie(kind: str, n: int):
            if census is not None and n > 1:
                census[kind] = census.get(kind, 0) + 1
        r, q, layer = len(P), self.S - 1, 1
        ends = [p for p in range(self.PL) if W[r, p, q] == v]
        tie("end", len(ends))
        p = ends[0]
        while True:
            if layer == 1:
                cur = W[r, p, q]
                cand = [N[r, p, q] == cur] + [W[r, p, self.sS[k]] + self.sW[k] == cur for k in self.inSil[q]]
                tie("stay" if cand[0] else "silent", sum(cand))
                if cand[0]:
                    layer = 0
                    continue
                k = self.inSil[q][cand.index(True, 1) - 1]
                edges.append(int(self.sId[k])); rows.append(r); q = int(self.sS[k])
            else:
                if r == 0:
                    assert q == 0 and p == 0
                    break
                Pr, cur = P[r - 1], N[r, p, q]
                if p == 0:
                    cand = [N[r - 1, k, q] + Pr[0] == cur for k in range(self.PL)]
                    tie("blank", sum(cand))
                    p = cand.index(True)
                    r -= 1
                    continue
                oth = self._others(p)
                ks = [k for k in self.inEmit[q] if self.eO[k] == self.colTok[p - 1]]
                X = [max(W[r - 1, o, self.eS[k]] for o in oth) for k in ks]
                cand = [N[r - 1, p, q] + Pr[p] == cur] + [(x + self.eW[k]) + Pr[p] == cur for k, x in zip(ks, X)]
                tie("repeat" if cand[0] else "emit", sum(cand))
                r -= 1
                if cand[0]:
                    continue
                j = cand.index(True, 1) - 1
                k = ks[j]
                src = [o for o in oth if W[r, o, self.eS[k]] == X[j]]
                tie("plane", len(src))
                edges.append(int(self.eId[k])); rows.append(r); q = int(self.eS[k]); p = src[0]; layer = 1
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32)


class PairProfileDP(ProfileDP):
    """A machine WITH an input alphabet on a known input sequence x[1..I] against a profile of L rows, in numpy -- the yardstick of
    mb_profile_pair.hip (docs/profile_tapes.md, "Pairs: an input sequence against a profile"): the semantics of
    compose(M, transpose(CSVProfile::machine())) run on input x with an empty output.  N = "arrived at (i, r)", W = "after M's
    output-less moves there":

        N[i][r][d] = [i = 0, r = 0, d = 0]
                     (+) N[i][r-1][d] + P[r-1][0]                                              (blank; r > 0)
                     (+) sum_{t: s->d, in = x_i, out = o}  W[i-1][r-1][s] + w_t + P[r-1][o]      (match;  i > 0, r > 0)
                     (+) sum_{t: s->d, in = eps, out = o}  W[i][r-1][s]   + w_t + P[r-1][o]      (output-only; r > 0)
        W[i][r][d] = N[i][r][d]
                     (+) sum_{t: s->d, in = x_i, out = eps} W[i-1][r][s] + w_t                   (input-only; i > 0)
                     (+) sum_{silent t: s->d, s < d}        W[i][r][s]   + w_t                   (silent levels)
        loglike    = W[I][L][S-1]

    The blank reads N, never W (the waiting-machine order of docs/decoding.md).  Viterbi keeps the FIRST maximum -- N: the blank,
    then match edges in `incoming` order, then output-only edges in `incoming` order; W: "no move" (N), then input-only edges in
    `incoming` order, then silent edges in `incoming` order.  Every method takes (x, P): x the input tokens (1..nInTok), P the
    [L, nOutTok + 1] log weights of Profile.logRows.  Lattices are [I + 1, L + 1, S].

    ``env`` (forward, backward, counts, viterbi): a seqpair.Envelope or an (inStart, inEnd) pair -- row r holds the input positions
    inStart[r] <= i < inEnd[r]; both layers of every other cell are -inf (docs/profile_tapes.md, "Pairs under an envelope").  The
    sweeps visit the envelope cells alone.  Without it not one operation differs."""

    def __init__(self, em: EvaluatedMachine):
        super().__init__(em)
        order = em.incomingOrder()
        it, ot, src, dst = em.inTok[order], em.outTok[order], em.src[order].astype(np.int64), em.dst[order].astype(np.int64)

        def table(sel):
            return order[sel], src[sel], dst[sel], em.logWeight[order[sel]], ot[sel].astype(np.int64)
        # [a]: (edge id, src, dst, w, out token) of the edges reading input token a, in `incoming` order; [0] unused
        self.match = [table((it == a) & (ot > 0)) for a in range(em.nInTok + 1)]
        self.ins = [table((it == a) & (ot == 0)) for a in range(em.nInTok + 1)]
        self._all = np.arange(self.S, dtype=np.int64)

    def _checkPair(self, x, P) -> Tuple[np.ndarray, np.ndarray]:
        x = np.asarray(x, np.int64).reshape(-1)
        if len(x) and (x.min() < 1 or x.max() > self.em.nInTok):
            raise MachineError("input token outside 1..nInTok")
        return x, self._check(P)

    @staticmethod
    def envelopeRows(env, I: int, L: int):
        """Per input position i the rows r of the envelope cells (i, r), ascending; None without an envelope.  Raises what
        mb_profile_pairs_set_envelopes rejects: a mismatch, an envelope that is not connected or not monotone."""
        if env is None:
            return None
        st, en = (env.inStart, env.inEnd) if hasattr(env, "inStart") else env
        st = [int(v) for v in st]; en = [int(v) for v in en]
        if len(st) != L + 1 or len(en) != L + 1 or any(a < 0 or b > I + 1 or a > b for a, b in zip(st, en)):
            raise MachineError("Envelope/sequence mismatch")
        e = Envelope(); e.inLen, e.outLen, e.inStart, e.inEnd = I, L, st, en
        if not e.connected():
            raise MachineError("Envelope is not connected")
        if not e.monotone():
            raise MachineError("Envelope is not monotone")
        rows: List[List[int]] = [[] for _ in range(I + 1)]
        for r in range(L + 1):
            for i in range(st[r], en[r]):
                rows[i].append(r)
        return rows

    def forward(self, x, P, mode: str = "exact", env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, N[I+1][L+1][S], W[I+1][L+1][S]); mode "exact" or "max"."""
        x, P = self._checkPair(x, P)
        fold = _max_fold if mode == "max" else _lse_fold
        I, L, S = len(x), len(P), self.S
        N = np.full((I + 1, L + 1, S), _NEG); W = np.full((I + 1, L + 1, S), _NEG)
        inside = self.envelopeRows(env, I, L)
        for i in range(I + 1):
            for r in (range(L + 1) if inside is None else inside[i]):      # (a cell outside stays -inf and is read as such)
                base = np.full(S, _NEG)
                if i == 0 and r == 0:
                    base[0] = 0.0
                if r:
                    Pr = P[r - 1]
                    idx, vals = [self._all], [N[i, r - 1] + Pr[0]]
                    if i:
                        _, s, d, w, o = self.match[x[i - 1]]
                        idx.append(d); vals.append((W[i - 1, r - 1][s] + w) + Pr[o])
                    idx.append(self.eD); vals.append((W[i, r - 1][self.eS] + self.eW) + Pr[self.eO])
                    base = fold(base, np.concatenate(idx), np.concatenate(vals))
                N[i, r] = base
                w_ = base
                if i:
                    _, s, d, w, _o = self.ins[x[i - 1]]
                    w_ = fold(w_, d, W[i - 1, r][s] + w)
                else:
                    w_ = w_.copy()
                for lv in self.fLevels:
                    w_ = fold(w_, self.sD[lv], w_[self.sS[lv]] + self.sW[lv])
                W[i, r] = w_
        return float(W[I, L, S - 1]), N, W

    def backward(self, x, P, env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, NB[I+1][L+1][S], WB[I+1][L+1][S]), exact log-sum-exp; loglike = NB[0][0][0].  WB[i][r][s] is the mass from
        the waiting stage of (i, r, s) to the end, NB from the arrived stage: NB = WB (+) (P[r][0] + NB[i][r+1])."""
        x, P = self._checkPair(x, P)
        I, L, S = len(x), len(P), self.S
        NB = np.full((I + 1, L + 1, S), _NEG); WB = np.full((I + 1, L + 1, S), _NEG)
        inside = self.envelopeRows(env, I, L)
        for i in range(I, -1, -1):
            for r in (range(L, -1, -1) if inside is None else reversed(inside[i])):
                base = np.full(S, _NEG)
                if i == I and r == L:
                    base[S - 1] = 0.0
                if r < L:
                    if i < I:
                        _, s, d, w, o = self.match[x[i]]
                        base = _lse_fold(base, s, (w + P[r][o]) + NB[i + 1, r + 1][d])
                    base = _lse_fold(base, self.eS, (self.eW + P[r][self.eO]) + NB[i, r + 1][self.eD])
                if i < I:
                    _, s, d, w, _o = self.ins[x[i]]
                    base = _lse_fold(base, s, WB[i + 1, r][d] + w)
                for lv in self.bLevels:
                    base = _lse_fold(base, self.sS[lv], base[self.sD[lv]] + self.sW[lv])
                WB[i, r] = base
                NB[i, r] = np.logaddexp(base, P[r][0] + NB[i, r + 1]) if r < L else base
        return float(NB[0, 0, 0]), NB, WB

    def counts(self, x, P, blanks: Optional[list] = None, env=None) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf pair.  Blank rows are not edges;
        ``blanks`` (a list) receives their posterior mass, summed over the lattice."""
        x, P = self._checkPair(x, P)
        ll, NF, WF = self.forward(x, P) if env is None else self.forward(x, P, env=env)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB = self.backward(x, P) if env is None else self.backward(x, P, env=env)
        I, L = len(x), len(P)
        inside = self.envelopeRows(env, I, L)
        blank = 0.0
        with np.errstate(invalid="ignore"):
            for i in range(I + 1):
                for r in (range(L + 1) if inside is None else inside[i]):
                    f = WF[i, r] - ll
                    if r < L:
                        if i < I:
                            e, s, d, w, o = self.match[x[i]]
                            np.add.at(out, e, np.exp(f[s] + ((w + P[r][o]) + NB[i + 1, r + 1][d])))
                        np.add.at(out, self.eId, np.exp(f[self.eS] + ((self.eW + P[r][self.eO]) + NB[i, r + 1][self.eD])))
                        b = (NF[i, r] - ll) + (P[r][0] + NB[i, r + 1])
                        blank += float(np.exp(b[b > _NEG]).sum())
                    if i < I:
                        e, s, d, w, _o = self.ins[x[i]]
                        np.add.at(out, e, np.exp(f[s] + (WB[i + 1, r][d] + w)))
                    np.add.at(out, self.sId, np.exp(f[self.sS] + (WB[i, r][self.sD] + self.sW)))
        if blanks is not None:
            blanks.append(blank)
        return out, ll

    def rowPosteriors(self, x, P, env=None) -> Tuple[np.ndarray, float]:
        """(post[L, nOutTok + 1], Forward loglike): post[r][o] is the posterior probability that row r was consumed as output token
        o (column 0: as the blank) -- the emitting terms of counts() and its blank term, binned by (row, column) instead of by
        transition, which is the gradient of loglike in P[r][o] (docs/profile_tapes.md, "Row posteriors").  Every row sums to 1;
        zeros for a -inf pair; exactly 0 where P[r][o] is -inf."""
        x, P = self._checkPair(x, P)
        ll, NF, WF = self.forward(x, P) if env is None else self.forward(x, P, env=env)
        I, L = len(x), len(P)
        post = np.zeros((L, self.em.nOutTok + 1))
        if not ll > _NEG:
            return post, ll
        _, NB, WB = self.backward(x, P) if env is None else self.backward(x, P, env=env)
        inside = self.envelopeRows(env, I, L)
        with np.errstate(invalid="ignore"):
            for i in range(I + 1):
                for r in (range(L) if inside is None else inside[i]):
                    if r == L:
                        continue
                    f = WF[i, r] - ll
                    b = (NF[i, r] - ll) + (P[r][0] + NB[i, r + 1])
                    post[r, 0] += float(np.exp(b[b > _NEG]).sum())
                    if i < I:
                        _, s, d, w, o = self.match[x[i]]
                        t = f[s] + ((w + P[r][o]) + NB[i + 1, r + 1][d])
                        np.add.at(post[r], o[t > _NEG], np.exp(t[t > _NEG]))
                    t = f[self.eS] + ((self.eW + P[r][self.eO]) + NB[i, r + 1][self.eD])
                    np.add.at(post[r], np.asarray(self.eO)[t > _NEG], np.exp(t[t > _NEG]))
        return post, ll

    def viterbi(self, x, P, census: Optional[dict] = None, env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, row at which each fired); the first maximum in the fill's candidate order.  The
        row of an emitting edge is the row it consumed, of an output-less edge the number of rows consumed before it; the input
        position follows by counting the input-consuming edges.  ``census``: per step at which two or more candidates equal the
        cell, a count under the tuple of the kinds that tie, in candidate order ("blank", "match", "emit" at an N cell; "stay",
        "ins", "silent" at a W cell).  Under ``env`` a candidate whose source cell lies outside the envelope is -inf and loses; the
        census counts, under ("outside", kind), the steps that had such a candidate of that kind."""
        x, P = self._checkPair(x, P)
        v, N, W = self.forward(x, P, "max") if env is None else self.forward(x, P, "max", env=env)
        inside = self.envelopeRows(env, len(x), len(P))
        edges: List[int] = []; rows: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32)
        i, r, q, layer = len(x), len(P), self.S - 1, 1
        while True:
            cand = []          # (kind, edge id or -1, source state, attains the cell)
            if layer == 1:
                cur = W[i, r, q]
                cand.append(("stay", -1, q, N[i, r, q] == cur))
                if i:
                    e, s, d, w, _o = self.ins[x[i - 1]]
                    cand += [("ins", int(e[k]), int(s[k]), W[i - 1, r, s[k]] + w[k] == cur) for k in np.nonzero(d == q)[0]]
                cand += [("silent", int(self.sId[k]), int(self.sS[k]), W[i, r, self.sS[k]] + self.sW[k] == cur) for k in self.inSil[q]]
            else:
                if r == 0:
                    assert i == 0 and q == 0
                    break
                Pr, cur = P[r - 1], N[i, r, q]
                cand.append(("blank", -1, q, N[i, r - 1, q] + Pr[0] == cur))
                if i:
                    e, s, d, w, o = self.match[x[i - 1]]
                    cand += [("match", int(e[k]), int(s[k]), (W[i - 1, r - 1, s[k]] + w[k]) + Pr[o[k]] == cur) for k in np.nonzero(d == q)[0]]
                cand += [("emit", int(self.eId[k]), int(self.eS[k]), (W[i, r - 1, self.eS[k]] + self.eW[k]) + Pr[self.eO[k]] == cur)
                         for k in self.inEmit[q]]
            hits = [c for c in cand if c[3]]
            if census is not None and inside is not None:
                back = {"ins": (1, 0), "blank": (0, 1), "emit": (0, 1), "match": (1, 1)}
                for kind in dict.fromkeys(c[0] for c in cand if c[0] in back):
                    si, sr = i - back[kind][0], r - back[kind][1]
                    if sr not in inside[si]:
                        census[("outside", kind)] = census.get(("outside", kind), 0) + 1
            if census is not None and len(hits) > 1:
                kinds = tuple(dict.fromkeys(c[0] for c in hits))
                census[kinds] = census.get(kinds, 0) + 1
            kind, e, s, _ = hits[0]
            if kind == "stay":
                layer = 0
            elif kind == "blank":
                r -= 1
            elif kind in ("ins", "silent"):
                edges.append(e); rows.append(r); q = s
                i -= kind == "ins"
            else:
                r -= 1
                edges.append(e); rows.append(r); q = s; layer = 1
                i -= kind == "match"
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32)

    def sampleCandidates(self, x, P, N, W, inside, i: int, r: int, q: int, layer: int):
        """The candidates of the sampling decision at cell (i, r, q) of ``layer`` (1: W, 0: N with r > 0) over the sum lattice
        (N, W): (kind, edge id or -1, source state, term) in the fill's order, the list viterbi() enumerates.  ``inside``:
        envelopeRows(); a candidate whose source cell lies outside is left out."""
        ok = (lambda si, sr: True) if inside is None else (lambda si, sr: sr in inside[si])
        cand = []
        if layer == 1:
            cand.append(("stay", -1, q, float(N[i, r, q])))
            if i and ok(i - 1, r):
                e, s, d, w, _o = self.ins[x[i - 1]]
                cand += [("ins", int(e[k]), int(s[k]), float(W[i - 1, r, s[k]] + w[k])) for k in np.nonzero(d == q)[0]]
            cand += [("silent", int(self.sId[k]), int(self.sS[k]), float(W[i, r, self.sS[k]] + self.sW[k])) for k in self.inSil[q]]
        else:
            Pr = P[r - 1]
            up = ok(i, r - 1)
            if up:
                cand.append(("blank", -1, q, float(N[i, r - 1, q] + Pr[0])))
            if i and ok(i - 1, r - 1):
                e, s, d, w, o = self.match[x[i - 1]]
                cand += [("match", int(e[k]), int(s[k]), float((W[i - 1, r - 1, s[k]] + w[k]) + Pr[o[k]])) for k in np.nonzero(d == q)[0]]
            if up:
                cand += [("emit", int(self.eId[k]), int(self.eS[k]), float((W[i, r - 1, self.eS[k]] + self.eW[k]) + Pr[self.eO[k]]))
                         for k in self.inEmit[q]]
        return cand

    def samplePaths(self, x, P, nSamples: int, seed: int = 0, pair: int = 0, env=None, margins: Optional[list] = None):
        """(loglike, [(edges, rows, logq), ...]): ``nSamples`` paths drawn from the posterior by a stochastic traceback over
        forward(x, P, env=env) -- the yardstick of k_profile_pair_sample (docs/profile_tapes.md, "Posterior path samples").  From
        W[I][L][S-1] back to N[0][0][0]; every visit of a W cell, or of an N cell with r > 0, is one decision among
        sampleCandidates(): p_c = exp(term_c - cell), acc adds them in order from 0.0, the first c with u < acc is taken, else the
        last c with p_c > 0.  u = sample_uniform(seed, pair, j, t) for decision t of sample j.  logq sums term - cell over the
        decisions: the path's log posterior probability.  Paths are as viterbi()'s; a -inf pair gives empty paths and logq = -inf.
        ``margins`` (a list) receives per decision the least |u - acc_c| over all partial sums acc_c of the decision."""
        x, P = self._checkPair(x, P)
        ll, N, W = self.forward(x, P) if env is None else self.forward(x, P, env=env)
        inside = self.envelopeRows(env, len(x), len(P))
        if inside is not None:
            inside = [set(rs) for rs in inside]
        out = []
        for j in range(int(nSamples)):
            edges: List[int] = []; rows: List[int] = []
            if not ll > _NEG:
                out.append((np.zeros(0, np.uint32), np.zeros(0, np.int32), _NEG))
                continue
            i, r, q, layer, t, logq = len(x), len(P), self.S - 1, 1, 0, 0.0
            while layer == 1 or r > 0:
                cur = float(W[i, r, q] if layer == 1 else N[i, r, q])
                cand = self.sampleCandidates(x, P, N, W, inside, i, r, q, layer)
                u = sample_uniform(seed, pair, j, t)
                t += 1
                acc, pick, last, margin = 0.0, None, None, math.inf
                for c in cand:
                    p = math.exp(c[3] - cur) if c[3] > _NEG else 0.0
                    acc += p
                    margin = min(margin, abs(u - acc))
                    if p > 0.0:
                        last = c
                    if pick is None and u < acc:
                        pick = c
                if pick is None:
                    pick = last
                if pick is None:
                    raise MachineError("samplePaths: no candidate with a positive probability")
                if margins is not None:
                    margins.append(margin)
                kind, e, s, term = pick
                logq += term - cur
                if kind == "stay":
                    layer = 0
                elif kind == "blank":
                    r -= 1
                elif kind in ("ins", "silent"):
                    edges.append(e); rows.append(r); q = s
                    i -= kind == "ins"
                else:
                    r -= 1
                    edges.append(e); rows.append(r); q = s; layer = 1
                    i -= kind == "match"
            assert i == 0 and q == 0
            out.append((np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32), logq))
        return ll, out


def _excl_planes(A: np.ndarray, mx: bool) -> np.ndarray:
    """out[k] = (+)_{j != k} A[j] over axis 0 of A[planes, ...], every k at once: a prefix and a suffix reduction joined, planes + 1
    vector operations instead of planes^2 (one plane: all -inf).  Pairwise max or exact pairwise log-sum-exp."""
    op = np.maximum if mx else np.logaddexp
    out = np.full(A.shape, _NEG)
    if len(A) > 1:
        pre, suf = op.accumulate(A, axis=0), op.accumulate(A[::-1], axis=0)[::-1]
        out[1:] = pre[:-1]
        out[:-1] = op(out[:-1], suf[1:])
    return out


class PairMergedProfileDP(PairProfileDP):
    """A machine WITH an input alphabet on a known input sequence x[1..I] against a CTC-MERGED profile of L rows, in numpy -- the
    yardstick of mb_profile_pair_merge.hip (docs/profile_tapes.md, "Pairs against a merged profile"): the semantics of
    compose(M, transpose(CSVProfile::mergingMachine())) run on input x with an empty output.  The lattice of PairProfileDP with the
    plane axis of MergedProfileDP: plane 0 = the last row took the blank (or no row yet), plane c = the last row took column c, whose
    output token is colTok[c - 1].  N = "arrived", W = "after M's output-less moves", X the exclusion vector:

        X[i][r][c][s] = (+)_{k != c} W[i][r][k][s]
        N[i][r][0][d] = [i = 0, r = 0, d = 0]  (+)  (+)_p (N[i][r-1][p][d] + P[r-1][0])                    (blank; r > 0)
        N[i][r][c][d] = (N[i][r-1][c][d] + P[r-1][c])                                                      (repeat; r > 0)
                        (+) sum_{t: s->d, in = x_i, out = colTok[c]} X[i-1][r-1][c][s] + w_t + P[r-1][c]    (match; i > 0, r > 0)
                        (+) sum_{t: s->d, in = eps, out = colTok[c]} X[i][r-1][c][s]   + w_t + P[r-1][c]    (output-only; r > 0)
        W[i][r][p][d] = N[i][r][p][d]
                        (+) sum_{t: s->d, in = x_i, out = eps} W[i-1][r][p][s] + w_t                        (input-only; same plane)
                        (+) sum_{silent t: s->d, s < d}        W[i][r][p][s]   + w_t                        (silent levels, per plane)
        loglike       = (+)_p W[I][L][p][S-1]

    The blank and the repeat read N, never W.  Viterbi keeps the FIRST maximum -- N[.][.][0]: planes ascending; N[.][.][c]: the
    repeat, then match edges in `incoming` order, then output-only edges in `incoming` order, each from the lowest plane k != c
    that attains its X; W: "no move", then input-only edges, then silent edges, each in `incoming` order; the end: planes
    ascending.  Every method takes (x, P): P the [L, nCols + 1] log weights of Profile.mergeRows.  Lattices are
    [I + 1, L + 1, nCols + 1, S].

    ``env`` (forward, backward, counts, rowPosteriors, viterbi): as PairProfileDP's, checked by envelopeRows -- cell (i, r) exists
    iff inStart[r] <= i < inEnd[r], in every plane; N, W and X (NB, WB and T) of every other cell are -inf (docs/profile_tapes.md,
    "Pairs against a merged profile under an envelope").  The sweeps visit the envelope cells alone.  Without it not one operation
    differs."""

    def __init__(self, em: EvaluatedMachine, colTok: Sequence[int]):
        super().__init__(em)
        self.colTok = np.asarray(colTok, np.int64).reshape(-1)
        self.nCols = len(self.colTok)
        if self.nCols < 1:
            raise MachineError("merged profiles need at least one column")
        if self.colTok.min() < 1 or self.colTok.max() > em.nOutTok:
            raise MachineError("column token outside 1..nOutTok")
        self.PL = self.nCols + 1

        def by_column(tab):
            """(edge id, src, dst, w, column) of the edges of ``tab`` whose token heads a column: column-major, `incoming` order within"""
            e, s, d, w, o = tab
            sel = [np.nonzero(o == t)[0] for t in self.colTok]
            col = np.concatenate([np.full(len(k), c + 1, np.int64) for c, k in enumerate(sel)])
            k = np.concatenate(sel).astype(np.int64)
            return e[k], s[k], d[k], w[k], col
        self.matchCol = [by_column(t) for t in self.match]
        self.emitCol = by_column((self.eId, self.eS, self.eD, self.eW, self.eO))

    def _check(self, P) -> np.ndarray:
        P = np.asarray(P, np.float64).reshape(-1, self.PL)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        return P

    def _planes(self, fold, base: np.ndarray, d: np.ndarray, vals: np.ndarray) -> np.ndarray:
        """fold over (plane, state) at once: vals[PL, n] into base[PL, S] at column d[n] of every plane"""
        S = self.S
        idx = (np.arange(self.PL)[:, None] * S + d[None, :]).ravel()
        return fold(base.ravel(), idx, vals.ravel()).reshape(self.PL, S)

    def forward(self, x, P, mode: str = "exact", env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, N[I+1][L+1][nCols+1][S], W[I+1][L+1][nCols+1][S]); mode "exact" or "max"."""
        return self._sweep(x, P, mode, env)[:3]

    def _sweep(self, x, P, mode: str, env=None):
        """forward() and the exclusion vectors X[I+1][L+1][nCols+1][S] (plane 0 of X is not read)"""
        x, P = self._checkPair(x, P)
        mx = mode == "max"
        fold = _max_fold if mx else _lse_fold
        I, L, S, PL = len(x), len(P), self.S, self.PL
        N = np.full((I + 1, L + 1, PL, S), _NEG); W = np.full((I + 1, L + 1, PL, S), _NEG)
        X = np.full((I + 1, L + 1, PL, S), _NEG)
        inside = self.envelopeRows(env, I, L)
        for i in range(I + 1):
            for r in (range(L + 1) if inside is None else inside[i]):      # (a cell outside stays -inf and is read as such)
                base = np.full((PL, S), _NEG)
                if i == 0 and r == 0:
                    base[0, 0] = 0.0
                if r:
                    Pr = P[r - 1]
                    base[0] = _red_planes(N[i, r - 1] + Pr[0], mx)
                    flat = (N[i, r - 1] + Pr[:, None]).ravel()
                    flat[:S] = base[0]
                    idx, vals = [], []
                    if i:
                        _, s, d, w, c = self.matchCol[x[i - 1]]
                        idx.append(c * S + d); vals.append((X[i - 1, r - 1][c, s] + w) + Pr[c])
                    _, s, d, w, c = self.emitCol
                    idx.append(c * S + d); vals.append((X[i, r - 1][c, s] + w) + Pr[c])
                    base = fold(flat, np.concatenate(idx), np.concatenate(vals)).reshape(PL, S)
                N[i, r] = base
                w_ = base.copy()
                if i:
                    _, s, d, w, _o = self.ins[x[i - 1]]
                    w_ = self._planes(fold, w_, d, W[i - 1, r][:, s] + w)
                for lv in self.fLevels:
                    w_ = self._planes(fold, w_, self.sD[lv], w_[:, self.sS[lv]] + self.sW[lv])
                W[i, r] = w_
                X[i, r] = _excl_planes(w_, mx)
        return float(_red_planes(W[I, L, :, S - 1:S], mx)[0]), N, W, X

    def backward(self, x, P, env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(loglike, NB[I+1][L+1][nCols+1][S], WB[I+1][L+1][nCols+1][S]), exact log-sum-exp; loglike = NB[0][0][0][0]."""
        x, P = self._checkPair(x, P)
        I, L, S, PL = len(x), len(P), self.S, self.PL
        NB = np.full((I + 1, L + 1, PL, S), _NEG); WB = np.full((I + 1, L + 1, PL, S), _NEG)
        inside = self.envelopeRows(env, I, L)
        for i in range(I, -1, -1):
            for r in (range(L, -1, -1) if inside is None else reversed(inside[i])):
                base = np.full((PL, S), _NEG)
                if r < L:
                    # T[c][s]: everything that leaves s through column c; WB[k] takes the columns other than k
                    idx, vals = [], []
                    if i < I:
                        _, s, d, w, c = self.matchCol[x[i]]
                        idx.append(c * S + s); vals.append((w + P[r][c]) + NB[i + 1, r + 1][c, d])
                    _, s, d, w, c = self.emitCol
                    idx.append(c * S + s); vals.append((w + P[r][c]) + NB[i, r + 1][c, d])
                    T = _lse_fold(np.full(PL * S, _NEG), np.concatenate(idx), np.concatenate(vals)).reshape(PL, S)
                    base = _excl_planes(T, False)
                if i == I and r == L:
                    base[:, S - 1] = 0.0
                if i < I:
                    _, s, d, w, _o = self.ins[x[i]]
                    base = self._planes(_lse_fold, base, s, WB[i + 1, r][:, d] + w)
                for lv in self.bLevels:
                    base = self._planes(_lse_fold, base, self.sS[lv], base[:, self.sD[lv]] + self.sW[lv])
                WB[i, r] = base
                if r < L:
                    nb = np.logaddexp(base, P[r][0] + NB[i, r + 1][0])
                    nb[1:] = np.logaddexp(nb[1:], P[r][1:, None] + NB[i, r + 1][1:])
                    NB[i, r] = nb
                else:
                    NB[i, r] = base
        return float(NB[0, 0, 0, 0]), NB, WB

    def counts(self, x, P, blanks: Optional[list] = None, env=None) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf pair.  Blank and repeat rows are not
        edges; ``blanks`` (a list) receives their posterior mass, summed over the lattice."""
        x, P = self._checkPair(x, P)
        ll, NF, WF, XF = self._sweep(x, P, "exact", env)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB = self.backward(x, P) if env is None else self.backward(x, P, env=env)
        I, L = len(x), len(P)
        inside = self.envelopeRows(env, I, L)
        blank = 0.0
        with np.errstate(invalid="ignore"):
            for i in range(I + 1):
                for r in (range(L + 1) if inside is None else inside[i]):
                    f, fx = WF[i, r] - ll, XF[i, r] - ll
                    if r < L:
                        if i < I:
                            e, s, d, w, c = self.matchCol[x[i]]
                            np.add.at(out, e, np.exp(fx[c, s] + ((w + P[r][c]) + NB[i + 1, r + 1][c, d])))
                        e, s, d, w, c = self.emitCol
                        np.add.at(out, e, np.exp(fx[c, s] + ((w + P[r][c]) + NB[i, r + 1][c, d])))
                        n = NF[i, r] - ll
                        b = np.concatenate([(n + (P[r][0] + NB[i, r + 1][0])).ravel(), (n[1:] + (P[r][1:, None] + NB[i, r + 1][1:])).ravel()])
                        blank += float(np.exp(b[b > _NEG]).sum())
                    if i < I:
                        e, s, d, w, _o = self.ins[x[i]]
                        np.add.at(out, e, np.exp(f[:, s] + (WB[i + 1, r][:, d] + w)).sum(axis=0))
                    np.add.at(out, self.sId, np.exp(f[:, self.sS] + (WB[i, r][:, self.sD] + self.sW)).sum(axis=0))
        if blanks is not None:
            blanks.append(blank)
        return out, ll

    def rowPosteriors(self, x, P, repeats: Optional[list] = None, env=None) -> Tuple[np.ndarray, float]:
        """(post[L, nCols + 1], Forward loglike): post[r][c] is the posterior probability that row r was consumed as column c
        (column 0: as the blank), the gradient of loglike in P[r][c] (docs/profile_tapes.md, "Row posteriors of pairs against a
        merged profile"): the blank out of every plane of every cell of the row, and for a column its repeat (plane c stays) plus
        the match and output-only edges of colTok[c - 1] out of every plane k != c -- the emitting terms of counts(), taken plane
        by plane off W instead of through X, binned by (row, column).  ``repeats``, if a list, receives the [L, nCols + 1] repeat
        part, so that post - repeats sums per token to the counts.  Every row sums to 1; zeros for a -inf pair; exactly 0 where
        P[r][c] is -inf."""
        x, P = self._checkPair(x, P)
        ll, NF, WF = self.forward(x, P) if env is None else self.forward(x, P, env=env)
        I, L, PL = len(x), len(P), self.PL
        post = np.zeros((L, PL)); rep = np.zeros((L, PL))
        if repeats is not None:
            repeats.append(rep)
        if not ll > _NEG:
            return post, ll
        _, NB, _ = self.backward(x, P) if env is None else self.backward(x, P, env=env)
        inside = self.envelopeRows(env, I, L)
        planes = np.arange(PL)

        def emit(row, f, tab, NBn):
            """the edges of ``tab`` (column-major) out of plane k into column c != k of the cell whose arrived Backward is NBn"""
            _, s, d, w, c = tab
            t = f[:, s] + ((w + P[r][c]) + NBn[c, d])[None, :]
            keep = (c[None, :] != planes[:, None]) & (t > _NEG)
            np.add.at(row, np.broadcast_to(c, t.shape)[keep], np.exp(t[keep]))
        with np.errstate(invalid="ignore"):
            for i in range(I + 1):
                for r in (range(L) if inside is None else inside[i]):
                    if r == L:
                        continue
                    n, f = NF[i, r] - ll, WF[i, r] - ll
                    b = n + (P[r][0] + NB[i, r + 1][0])
                    post[r, 0] += float(np.exp(b[b > _NEG]).sum())
                    b = n[1:] + (P[r][1:, None] + NB[i, r + 1][1:])
                    rep[r, 1:] += np.where(b > _NEG, np.exp(b), 0.0).sum(axis=1)
                    if i < I:
                        emit(post[r], f, self.matchCol[x[i]], NB[i + 1, r + 1])
                    emit(post[r], f, self.emitCol, NB[i, r + 1])
        post += rep
        return post, ll

    def viterbi(self, x, P, census: Optional[dict] = None, env=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, row at which each fired); the first maximum in the fill's candidate order.  Rows as
        PairProfileDP.viterbi; blank and repeat rows are not edges.  ``census`` counts, by the candidate taken, the steps at which
        two or more candidates equal the cell: "end"; "stay" / "input" / "silent" at a W cell; "blank" at N[.][.][0]; "repeat" /
        "match" / "emit" at N[.][.][c]; "plane" for an emitting edge whose X two planes attain.  Under ``env`` a candidate whose
        source cell lies outside the envelope is -inf and loses; the census counts, under ("outside", kind), the steps that had
        such a candidate of that kind."""
        x, P = self._checkPair(x, P)
        v, N, W = self.forward(x, P, "max") if env is None else self.forward(x, P, "max", env=env)
        inside = self.envelopeRows(env, len(x), len(P))
        edges: List[int] = []; rows: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32)

        def tie(kind: str, n: int):
            if census is not None and n > 1:
                census[kind] = census.get(kind, 0) + 1

        def outside(cand):
            """the census of the candidates (kind, ..., input position of the source at [3]) of a cell whose sources lie outside"""
            if census is None or inside is None:
                return
            for kind in dict.fromkeys(c[0] for c in cand if c[0] != "stay" and c[0] != "silent"):
                si = i - (kind in ("input", "match"))
                sr = r - (kind != "input")
                if sr not in inside[si]:
                    census[("outside", kind)] = census.get(("outside", kind), 0) + 1
        i, r, q, layer = len(x), len(P), self.S - 1, 1
        ends = [p for p in range(self.PL) if W[i, r, p, q] == v]
        tie("end", len(ends))
        p = ends[0]
        while True:
            cand = []          # (kind, edge id or -1, source state, input position of the source, attains the cell)
            if layer == 1:
                cur = W[i, r, p, q]
                cand.append(("stay", -1, q, i, N[i, r, p, q] == cur))
                if i:
                    e, s, d, w, _o = self.ins[x[i - 1]]
                    cand += [("input", int(e[k]), int(s[k]), i - 1, W[i - 1, r, p, s[k]] + w[k] == cur) for k in np.nonzero(d == q)[0]]
                cand += [("silent", int(self.sId[k]), int(self.sS[k]), i, W[i, r, p, self.sS[k]] + self.sW[k] == cur) for k in self.inSil[q]]
                outside(cand)
                hits = [c for c in cand if c[4]]
                kind, e, s, ni, _ = hits[0]
                tie(kind, len(hits))
                if kind == "stay":
                    layer = 0
                else:
                    edges.append(e); rows.append(r); q = s; i = ni
                continue
            if r == 0:
                assert i == 0 and q == 0 and p == 0
                break
            Pr, cur = P[r - 1], N[i, r, p, q]
            if p == 0:
                outside([("blank",)])
                hit = [N[i, r - 1, k, q] + Pr[0] == cur for k in range(self.PL)]
                tie("blank", sum(hit))
                p = hit.index(True)
                r -= 1
                continue
            oth = [k for k in range(self.PL) if k != p]
            tok = self.colTok[p - 1]
            cand.append(("repeat", -1, q, i, None, N[i, r - 1, p, q] + Pr[p] == cur))
            if i:
                e, s, d, w, o = self.match[x[i - 1]]
                for k in np.nonzero((d == q) & (o == tok))[0]:
                    xv = max(W[i - 1, r - 1, o_, s[k]] for o_ in oth)
                    cand.append(("match", int(e[k]), int(s[k]), i - 1, xv, (xv + w[k]) + Pr[p] == cur))
            for k in self.inEmit[q]:
                if self.eO[k] == tok:
                    xv = max(W[i, r - 1, o_, self.eS[k]] for o_ in oth)
                    cand.append(("emit", int(self.eId[k]), int(self.eS[k]), i, xv, (xv + self.eW[k]) + Pr[p] == cur))
            outside(cand)
            hits = [c for c in cand if c[5]]
            kind, e, s, ni, xv, _ = hits[0]
            tie(kind, len(hits))
            r -= 1
            if kind == "repeat":
                continue
            src = [k for k in oth if W[ni, r, k, s] == xv]
            tie("plane", len(src))
            edges.append(e); rows.append(r); q = s; i = ni; p = src[0]; layer = 1
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32)

    def sampleCandidates(self, x, P, N, W, inside, i: int, r: int, p: int, q: int, layer: int):
        """The candidates of the sampling decision at (i, r, plane p, state q) of ``layer`` over the sum lattice (N, W), as
        (kind, edge id or -1, source state, source plane, term), in the order of docs/profile_tapes.md, "Posterior path samples of
        pairs against a merged profile".  layer 2, the end: W[I][L][k][S-1], planes ascending.  layer 1, a W cell: "stay" (N), the
        input-only edges, the silent edges, each in `incoming` order, all on plane p.  layer 0, an N cell with r > 0: on plane 0 the
        blank out of every plane k ascending; on plane c the repeat, then the match edges in `incoming` order, then the output-only
        edges in `incoming` order, every edge once per source plane k != c ascending -- the fill's X taken apart.  ``inside``:
        envelopeRows() as sets; a candidate whose source cell lies outside is left out."""
        ok = (lambda si, sr: True) if inside is None else (lambda si, sr: sr in inside[si])
        cand = []
        if layer == 2:
            return [("end", -1, q, k, float(W[i, r, k, q])) for k in range(self.PL)]
        if layer == 1:
            cand.append(("stay", -1, q, p, float(N[i, r, p, q])))
            if i and ok(i - 1, r):
                e, s, d, w, _o = self.ins[x[i - 1]]
                cand += [("ins", int(e[k]), int(s[k]), p, float(W[i - 1, r, p, s[k]] + w[k])) for k in np.nonzero(d == q)[0]]
            cand += [("silent", int(self.sId[k]), int(self.sS[k]), p, float(W[i, r, p, self.sS[k]] + self.sW[k])) for k in self.inSil[q]]
            return cand
        Pr = P[r - 1]
        up = ok(i, r - 1)
        if p == 0:
            if up:
                cand += [("blank", -1, q, k, float(N[i, r - 1, k, q] + Pr[0])) for k in range(self.PL)]
            return cand
        oth = [k for k in range(self.PL) if k != p]
        tok = self.colTok[p - 1]
        if up:
            cand.append(("repeat", -1, q, p, float(N[i, r - 1, p, q] + Pr[p])))
        if i and ok(i - 1, r - 1):
            e, s, d, w, o = self.match[x[i - 1]]
            for a in np.nonzero((d == q) & (o == tok))[0]:
                cand += [("match", int(e[a]), int(s[a]), k, float((W[i - 1, r - 1, k, s[a]] + w[a]) + Pr[p])) for k in oth]
        if up:
            for a in self.inEmit[q]:
                if self.eO[a] == tok:
                    cand += [("emit", int(self.eId[a]), int(self.eS[a]), k, float((W[i, r - 1, k, self.eS[a]] + self.eW[a]) + Pr[p])) for k in oth]
        return cand

    def samplePaths(self, x, P, nSamples: int, seed: int = 0, pair: int = 0, env=None, margins: Optional[list] = None):
        """(loglike, [(edges, rows, rowCol, logq), ...]): ``nSamples`` lattice paths drawn from the posterior by a stochastic
        traceback over forward(x, P, env=env) -- the yardstick of k_profile_pair_merge_sample (docs/profile_tapes.md, "Posterior
        path samples of pairs against a merged profile").  Decision 0 picks the end plane among W[I][L][.][S-1] against loglike;
        then every visit of a W cell, or of an N cell with r > 0, is one decision among sampleCandidates(): p_c = exp(term_c -
        cell), acc adds them in order from 0.0, the first c with u < acc is taken, else the last c with p_c > 0.  u =
        sample_uniform(seed, pair, j, t) for decision t of sample j.  logq sums term - cell over the decisions: the lattice path's
        log weight minus loglike.  edges and rows are as viterbi()'s; rowCol[r] is the column row r took (0: the blank; c: column
        c, fresh or repeated), which with the edges determines the lattice path.  A -inf pair gives empty paths, rowCol = -1 and
        logq = -inf.  ``margins`` (a list) receives per decision the least |u - acc_c| over all partial sums acc_c of the decision."""
        x, P = self._checkPair(x, P)
        ll, N, W = self.forward(x, P) if env is None else self.forward(x, P, env=env)
        inside = self.envelopeRows(env, len(x), len(P))
        if inside is not None:
            inside = [set(rs) for rs in inside]
        out = []
        for j in range(int(nSamples)):
            edges: List[int] = []; rows: List[int] = []
            rowCol = np.full(len(P), -1, np.int32)
            if not ll > _NEG:
                out.append((np.zeros(0, np.uint32), np.zeros(0, np.int32), rowCol, _NEG))
                continue
            i, r, p, q, layer, t, logq = len(x), len(P), 0, self.S - 1, 2, 0, 0.0
            while layer or r > 0:
                cur = ll if layer == 2 else float(W[i, r, p, q] if layer == 1 else N[i, r, p, q])
                cand = self.sampleCandidates(x, P, N, W, inside, i, r, p, q, layer)
                u = sample_uniform(seed, pair, j, t)
                t += 1
                acc, pick, last, margin = 0.0, None, None, math.inf
                for c in cand:
                    pc = math.exp(c[4] - cur) if c[4] > _NEG else 0.0
                    acc += pc
                    margin = min(margin, abs(u - acc))
                    if pc > 0.0:
                        last = c
                    if pick is None and u < acc:
                        pick = c
                if pick is None:
                    pick = last
                if pick is None:
                    raise MachineError("samplePaths: no candidate with a positive probability")
                if margins is not None:
                    margins.append(margin)
                kind, e, s, k, term = pick
                logq += term - cur
                if kind == "end":
                    p = k; layer = 1
                elif kind == "stay":
                    layer = 0
                elif kind in ("ins", "silent"):
                    edges.append(e); rows.append(r); q = s
                    i -= kind == "ins"
                else:
                    r -= 1
                    rowCol[r] = p
                    if kind in ("match", "emit"):
                        edges.append(e); rows.append(r); q = s; layer = 1
                        i -= kind == "match"
                    p = k
            assert i == 0 and q == 0 and p == 0
            out.append((np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32), rowCol, logq))
        return ll, out

    def pathWeight(self, x, P, edges, rows, rowCol) -> float:
        """The log weight of the lattice path (edges, rows, rowCol) replayed from the definition, without a lattice: the weights of
        its edges plus P[r][rowCol[r]] of every row; -inf where it is no lattice path of (x, P).  The edges chain from state 0 to
        S - 1 and read x in order; silent edges climb (s < d); rows[k] is the row an emitting edge consumed, else the rows consumed
        when the edge fired, so the stamps never fall.  A row no edge consumed was taken on arrival (the blank and the repeat read
        N, never W): once an output-less edge has fired at a stamp, the next edge carries the same stamp, and the walk ends there
        only at L.
        The labels: a row with label c >= 1 that an edge consumed needs the edge to write colTok[c - 1] and the row before it
        ("no row yet" counts as 0) a label other than c; one that no edge consumed needs the row before it to carry c; label 0 goes
        with no edge."""
        x, P = self._checkPair(x, P)
        em = self.em
        I, L = len(x), len(P)
        edges = [int(e) for e in np.asarray(edges).reshape(-1)]
        rows = [int(v) for v in np.asarray(rows).reshape(-1)]
        rowCol = [int(v) for v in np.asarray(rowCol).reshape(-1)]
        if len(rows) != len(edges) or len(rowCol) != L or any(c < 0 or c > self.nCols for c in rowCol):
            return _NEG
        # at: the rows consumed so far; waiting: the walk has left N for W there, so the next row needs an edge
        w, q, i, at, waiting = 0.0, 0, 0, 0, False
        by: List[Optional[int]] = [None] * L    # the edge that consumed each row
        for e, r in zip(edges, rows):
            if e < 0 or e >= em.nTransitions or int(em.src[e]) != q:
                return _NEG
            it, ot, d = int(em.inTok[e]), int(em.outTok[e]), int(em.dst[e])
            if r < at or (waiting and r != at) or r > L - (1 if ot else 0):      # (the rows at..r-1 were taken on arrival)
                return _NEG
            if it:
                if i >= I or x[i] != it:
                    return _NEG
                i += 1
            elif not ot and not q < d:
                return _NEG
            if ot:
                by[r] = e
            at, waiting = (r + 1, False) if ot else (r, True)
            w += float(em.logWeight[e])
            q = d
        if q != self.S - 1 or i != I or (waiting and at != L):
            return _NEG
        prev = 0
        for r in range(L):
            c = rowCol[r]
            if by[r] is None:
                if c and prev != c:
                    return _NEG
            elif c == 0 or int(em.outTok[by[r]]) != int(self.colTok[c - 1]) or prev == c:
                return _NEG
            w += float(P[r][c])
            prev = c
        return w if w > _NEG else _NEG


class TwoProfileDP(PairProfileDP):
    """A machine WITH an input alphabet between two profiles, in numpy -- the yardstick of mb_profile_two.hip
    (docs/profile_tapes.md, "Pairs of profiles"): the semantics of compose(A.machine(), compose(M, B.recogniserMachine())) with both
    tapes empty.  A[i][0..nInTok] are the log rows of the input profile (K rows, Profile.logRowsIn), B[r][0..nOutTok] those of the
    output profile (L rows, Profile.logRows); column 0 of either is its blank.  N = "arrived at (i, r)", W = "after M's output-less
    moves there", Z = "committed to wait for the next input row":

        N[i][r][d] = [i = 0, r = 0, d = 0]
                     (+) N[i][r-1][d] + B[r-1][0]                                                          (output blank; r > 0)
                     (+) sum_{t: s->d, in = a, out = o}   ((Z[i-1][r-1][s] + w_t) + A[i-1][a]) + B[r-1][o]   (match; i, r > 0)
                     (+) sum_{t: s->d, in = eps, out = o} (W[i][r-1][s] + w_t) + B[r-1][o]                   (output-only; r > 0)
        W[i][r][d] = N[i][r][d]
                     (+) sum_{t: s->d, in = a, out = eps} (Z[i-1][r][s] + w_t) + A[i-1][a]                   (input-only; i > 0)
                     (+) sum_{silent t: s->d, s < d}      W[i][r][s] + w_t                                   (silent levels)
        Z[i][r][d] = W[i][r][d] (+) Z[i-1][r][d] + A[i-1][0]                                                 (input blank; i > 0)
        loglike    = Z[K][L][S-1]

    The generator moves only while M waits, so M's output-only and silent moves at an input position come before the input blank
    there: after a blank only input-reading edges follow (Z feeds the match and the input-only edges alone).  The output blank reads
    N, never W.  Viterbi keeps the FIRST maximum -- N: the output blank, then the match edges, then the output-only edges; W: "no
    move", then the input-only edges, then the silent edges; Z: W, then the input blank; edges of a kind in `incoming` order, which
    is ascending input token first, then ascending output token.  Lattices are [K + 1, L + 1, S].

    ``env`` (forward, backward, counts, rowPosteriors, viterbi): a seqpair.Envelope or an (inStart, inEnd) pair -- output row r
    holds the input-row positions inStart[r] <= i < inEnd[r]; all three layers of every other cell are -inf, so the input blank
    Z[i-1][r] -> Z[i][r] is left out when (i-1, r) is outside like any other move along i (docs/profile_tapes.md, "Pairs of
    profiles under an envelope").  The sweeps visit the envelope cells alone and read a cell outside as the -inf it is.  Without it
    not one operation differs."""

    def __init__(self, em: EvaluatedMachine):
        super().__init__(em)
        order = em.incomingOrder()
        it, ot, src, dst = em.inTok[order], em.outTok[order], em.src[order].astype(np.int64), em.dst[order].astype(np.int64)

        def table(sel):
            return order[sel], src[sel], dst[sel], em.logWeight[order[sel]], it[sel].astype(np.int64), ot[sel].astype(np.int64)
        # (edge id, src, dst, w, in token, out token) of the edges that read input, in `incoming` order
        self.mAll = table((it > 0) & (ot > 0))
        self.iAll = table((it > 0) & (ot == 0))

    def _checkTwo(self, A, B) -> Tuple[np.ndarray, np.ndarray]:
        if not self.em.nInTok:
            raise MachineError("two-profile sweeps need a machine with an input alphabet")
        A = np.asarray(A, np.float64).reshape(-1, self.em.nInTok + 1)
        if np.isnan(A).any() or (A == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        return A, self._check(B)

    def forward(self, A, B, mode: str = "exact", env=None) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
        """(loglike, N, W, Z), each [K+1][L+1][S]; mode "exact" or "max"."""
        A, B = self._checkTwo(A, B)
        fold = _max_fold if mode == "max" else _lse_fold
        K, L, S = len(A), len(B), self.S
        N = np.full((K + 1, L + 1, S), _NEG); W = np.full((K + 1, L + 1, S), _NEG); Z = np.full((K + 1, L + 1, S), _NEG)
        _, mS, mD, mW, mA, mO = self.mAll
        _, iS, iD, iW, iA, _ = self.iAll
        inside = self.envelopeRows(env, K, L)
        for i in range(K + 1):
            for r in (range(L + 1) if inside is None else inside[i]):      # (a cell outside stays -inf and is read as such)
                base = np.full(S, _NEG)
                if i == 0 and r == 0:
                    base[0] = 0.0
                if r:
                    Br = B[r - 1]
                    idx, vals = [self._all], [N[i, r - 1] + Br[0]]
                    if i:
                        idx.append(mD); vals.append(((Z[i - 1, r - 1][mS] + mW) + A[i - 1][mA]) + Br[mO])
                    idx.append(self.eD); vals.append((W[i, r - 1][self.eS] + self.eW) + Br[self.eO])
                    base = fold(base, np.concatenate(idx), np.concatenate(vals))
                N[i, r] = base
                w_ = fold(base, iD, (Z[i - 1, r][iS] + iW) + A[i - 1][iA]) if i else base.copy()
                for lv in self.fLevels:
                    w_ = fold(w_, self.sD[lv], w_[self.sS[lv]] + self.sW[lv])
                W[i, r] = w_
                Z[i, r] = fold(w_, self._all, Z[i - 1, r] + A[i - 1][0]) if i else w_
        return float(Z[K, L, S - 1]), N, W, Z

    def backward(self, A, B, env=None) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
        """(loglike, NB, WB, ZB), exact log-sum-exp; loglike = NB[0][0][0].  ZB[i][r][s] is the mass from the committed stage of
        (i, r, s) to the end, WB from the waiting stage, NB from the arrived stage."""
        A, B = self._checkTwo(A, B)
        K, L, S = len(A), len(B), self.S
        NB = np.full((K + 1, L + 1, S), _NEG); WB = np.full((K + 1, L + 1, S), _NEG); ZB = np.full((K + 1, L + 1, S), _NEG)
        _, mS, mD, mW, mA, mO = self.mAll
        _, iS, iD, iW, iA, _ = self.iAll
        inside = self.envelopeRows(env, K, L)
        for i in range(K, -1, -1):
            for r in (range(L, -1, -1) if inside is None else reversed(inside[i])):
                base = np.full(S, _NEG)
                if i == K and r == L:
                    base[S - 1] = 0.0
                if i < K:
                    base = _lse_fold(base, self._all, A[i][0] + ZB[i + 1, r])
                    if r < L:
                        base = _lse_fold(base, mS, ((mW + A[i][mA]) + B[r][mO]) + NB[i + 1, r + 1][mD])
                    base = _lse_fold(base, iS, (iW + A[i][iA]) + WB[i + 1, r][iD])
                ZB[i, r] = base
                if r < L:
                    base = _lse_fold(base, self.eS, (self.eW + B[r][self.eO]) + NB[i, r + 1][self.eD])
                for lv in self.bLevels:
                    base = _lse_fold(base, self.sS[lv], base[self.sD[lv]] + self.sW[lv])
                WB[i, r] = base
                NB[i, r] = np.logaddexp(base, B[r][0] + NB[i, r + 1]) if r < L else base
        return float(NB[0, 0, 0]), NB, WB, ZB

    def counts(self, A, B, blanks: Optional[list] = None, env=None) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf pair.  Blanks are not edges;
        ``blanks`` (a list) receives (mass of the output blanks, mass of the input blanks), summed over the lattice."""
        A, B = self._checkTwo(A, B)
        ll, NF, WF, ZF = self.forward(A, B) if env is None else self.forward(A, B, env=env)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB, ZB = self.backward(A, B) if env is None else self.backward(A, B, env=env)
        K, L = len(A), len(B)
        inside = self.envelopeRows(env, K, L)
        mE, mS, mD, mW, mA, mO = self.mAll
        iE, iS, iD, iW, iA, _ = self.iAll
        outBlank = inBlank = 0.0

        def mass(b):
            return float(np.exp(b[b > _NEG]).sum())
        with np.errstate(invalid="ignore"):
            for i in range(K + 1):
                for r in (range(L + 1) if inside is None else inside[i]):
                    f, z = WF[i, r] - ll, ZF[i, r] - ll
                    if r < L:
                        if i < K:
                            np.add.at(out, mE, np.exp(z[mS] + (((mW + A[i][mA]) + B[r][mO]) + NB[i + 1, r + 1][mD])))
                        np.add.at(out, self.eId, np.exp(f[self.eS] + ((self.eW + B[r][self.eO]) + NB[i, r + 1][self.eD])))
                        outBlank += mass((NF[i, r] - ll) + (B[r][0] + NB[i, r + 1]))
                    if i < K:
                        np.add.at(out, iE, np.exp(z[iS] + ((iW + A[i][iA]) + WB[i + 1, r][iD])))
                        inBlank += mass(z + (A[i][0] + ZB[i + 1, r]))
                    np.add.at(out, self.sId, np.exp(f[self.sS] + (WB[i, r][self.sD] + self.sW)))
        if blanks is not None:
            blanks.append((outBlank, inBlank))
        return out, ll

    def rowPosteriors(self, A, B, env=None) -> Tuple[np.ndarray, np.ndarray, float]:
        """(postA[K, nInTok + 1], postB[L, nOutTok + 1], Forward loglike): postB[r][o] is the posterior probability that output
        row r was consumed as output token o, postA[i][a] that input row i was consumed as input token a (column 0 of either: as
        its blank) -- the terms of counts() and its two blank masses, binned by (row, column) of either tape instead of by
        transition, which are the gradients of loglike in B[r][o] and in A[i][a] (docs/profile_tapes.md, "Row posteriors of pairs
        of profiles").  Every row of either table sums to 1; zeros for a -inf pair; exactly 0 where the weight is -inf."""
        A, B = self._checkTwo(A, B)
        ll, NF, WF, ZF = self.forward(A, B) if env is None else self.forward(A, B, env=env)
        K, L = len(A), len(B)
        postA = np.zeros((K, self.em.nInTok + 1)); postB = np.zeros((L, self.em.nOutTok + 1))
        if not ll > _NEG:
            return postA, postB, ll
        _, NB, WB, ZB = self.backward(A, B) if env is None else self.backward(A, B, env=env)
        inside = self.envelopeRows(env, K, L)
        _, mS, mD, mW, mA, mO = self.mAll
        _, iS, iD, iW, iA, _ = self.iAll
        eO = np.asarray(self.eO)

        def mass(b):
            return float(np.exp(b[b > _NEG]).sum())
        with np.errstate(invalid="ignore"):
            for i in range(K + 1):
                for r in (range(L + 1) if inside is None else inside[i]):
                    f, z = WF[i, r] - ll, ZF[i, r] - ll
                    if r < L:
                        if i < K:
                            t = z[mS] + (((mW + A[i][mA]) + B[r][mO]) + NB[i + 1, r + 1][mD])
                            live = t > _NEG
                            np.add.at(postB[r], mO[live], np.exp(t[live]))
                            np.add.at(postA[i], mA[live], np.exp(t[live]))
                        t = f[self.eS] + ((self.eW + B[r][eO]) + NB[i, r + 1][self.eD])
                        np.add.at(postB[r], eO[t > _NEG], np.exp(t[t > _NEG]))
                        postB[r, 0] += mass((NF[i, r] - ll) + (B[r][0] + NB[i, r + 1]))
                    if i < K:
                        t = z[iS] + ((iW + A[i][iA]) + WB[i + 1, r][iD])
                        np.add.at(postA[i], iA[t > _NEG], np.exp(t[t > _NEG]))
                        postA[i, 0] += mass(z + (A[i][0] + ZB[i + 1, r]))
        return postA, postB, ll

    def viterbi(self, A, B, census: Optional[dict] = None, env=None) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, output row, input row at which each fired); the first maximum in the fill's
        candidate order.  The output row of an emitting edge is the row it consumed, of an output-less edge the number of rows
        consumed before it; the input row likewise on the input tape -- input blanks advance it without an edge, so it does not
        follow from counting edges.  ``census``: per step at which two or more candidates equal the cell, a count under the tuple
        of the kinds that tie, in candidate order ("blank", "match", "emit" at an N cell; "stay", "ins", "silent" at a W cell;
        "wait", "inblank" at a Z cell).  Under ``env`` a candidate whose source cell lies outside the envelope is -inf and loses
        to the finite cell it is compared with."""
        A, B = self._checkTwo(A, B)
        v, N, W, Z = self.forward(A, B, "max") if env is None else self.forward(A, B, "max", env=env)
        edges: List[int] = []; rows: List[int] = []; ins: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32)
        mE, mS, mD, mW, mA, mO = self.mAll
        iE, iS, iD, iW, iA, _ = self.iAll
        i, r, q, layer = len(A), len(B), self.S - 1, 2
        while True:
            cand = []          # (kind, edge id or -1, source state, attains the cell)
            if layer == 2:
                cur = Z[i, r, q]
                cand.append(("wait", -1, q, W[i, r, q] == cur))
                if i:
                    cand.append(("inblank", -1, q, Z[i - 1, r, q] + A[i - 1][0] == cur))
            elif layer == 1:
                cur = W[i, r, q]
                cand.append(("stay", -1, q, N[i, r, q] == cur))
                if i:
                    cand += [("ins", int(iE[k]), int(iS[k]), (Z[i - 1, r, iS[k]] + iW[k]) + A[i - 1][iA[k]] == cur) for k in np.nonzero(iD == q)[0]]
                cand += [("silent", int(self.sId[k]), int(self.sS[k]), W[i, r, self.sS[k]] + self.sW[k] == cur) for k in self.inSil[q]]
            else:
                if r == 0:
                    assert i == 0 and q == 0
                    break
                Br, cur = B[r - 1], N[i, r, q]
                cand.append(("blank", -1, q, N[i, r - 1, q] + Br[0] == cur))
                if i:
                    cand += [("match", int(mE[k]), int(mS[k]), ((Z[i - 1, r - 1, mS[k]] + mW[k]) + A[i - 1][mA[k]]) + Br[mO[k]] == cur)
                             for k in np.nonzero(mD == q)[0]]
                cand += [("emit", int(self.eId[k]), int(self.eS[k]), (W[i, r - 1, self.eS[k]] + self.eW[k]) + Br[self.eO[k]] == cur)
                         for k in self.inEmit[q]]
            hits = [c for c in cand if c[3]]
            if census is not None and len(hits) > 1:
                kinds = tuple(dict.fromkeys(c[0] for c in hits))
                census[kinds] = census.get(kinds, 0) + 1
            kind, e, s, _ = hits[0]
            if kind == "wait":
                layer = 1
            elif kind == "inblank":
                i -= 1
            elif kind == "stay":
                layer = 0
            elif kind == "blank":
                r -= 1
            elif kind == "silent":
                edges.append(e); rows.append(r); ins.append(i); q = s
            elif kind == "ins":
                i -= 1
                edges.append(e); rows.append(r); ins.append(i); q = s; layer = 2
            elif kind == "emit":
                r -= 1
                edges.append(e); rows.append(r); ins.append(i); q = s; layer = 1
            else:
                r -= 1; i -= 1
                edges.append(e); rows.append(r); ins.append(i); q = s; layer = 2
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32), np.array(ins[::-1], np.int32)

    def sampleCandidates(self, A, B, N, W, Z, inside, i: int, r: int, q: int, layer: int):
        """The candidates of the sampling decision at cell (i, r, q) of ``layer`` (2: Z with i > 0, 1: W, 0: N with r > 0) over the
        sum lattice (N, W, Z): (kind, edge id or -1, source state, term) in the fill's order, the list viterbi() enumerates.
        ``inside``: per input row the set of its output rows, or None; a candidate whose source cell lies outside is left out."""
        ok = (lambda si, sr: True) if inside is None else (lambda si, sr: sr in inside[si])
        mE, mS, mD, mW, mA, mO = self.mAll
        iE, iS, iD, iW, iA, _ = self.iAll
        cand = []
        if layer == 2:
            cand.append(("wait", -1, q, float(W[i, r, q])))
            if ok(i - 1, r):
                cand.append(("inblank", -1, q, float(Z[i - 1, r, q] + A[i - 1][0])))
        elif layer == 1:
            cand.append(("stay", -1, q, float(N[i, r, q])))
            if i and ok(i - 1, r):
                cand += [("ins", int(iE[k]), int(iS[k]), float((Z[i - 1, r, iS[k]] + iW[k]) + A[i - 1][iA[k]])) for k in np.nonzero(iD == q)[0]]
            cand += [("silent", int(self.sId[k]), int(self.sS[k]), float(W[i, r, self.sS[k]] + self.sW[k])) for k in self.inSil[q]]
        else:
            Br = B[r - 1]
            up = ok(i, r - 1)
            if up:
                cand.append(("blank", -1, q, float(N[i, r - 1, q] + Br[0])))
            if i and ok(i - 1, r - 1):
                cand += [("match", int(mE[k]), int(mS[k]), float(((Z[i - 1, r - 1, mS[k]] + mW[k]) + A[i - 1][mA[k]]) + Br[mO[k]]))
                         for k in np.nonzero(mD == q)[0]]
            if up:
                cand += [("emit", int(self.eId[k]), int(self.eS[k]), float((W[i, r - 1, self.eS[k]] + self.eW[k]) + Br[self.eO[k]]))
                         for k in self.inEmit[q]]
        return cand

    @staticmethod
    def _sampleMove(kind: str, e: int, s: int, i: int, r: int, q: int, layer: int, edges: list, rows: list, ins: list):
        """One taken candidate: the cell it leads back to, its edge (if it is one) appended with both coordinates."""
        if kind == "wait":
            return i, r, q, 1
        if kind == "inblank":
            return i - 1, r, q, 2
        if kind == "stay":
            return i, r, q, 0
        if kind == "blank":
            return i, r - 1, q, 0
        if kind in ("match", "emit"):
            r -= 1
        if kind in ("match", "ins"):
            i -= 1
        edges.append(e); rows.append(r); ins.append(i)
        return i, r, s, 2 if kind in ("match", "ins") else 1

    def _sampleLattice(self, A, B, env):
        A, B = self._checkTwo(A, B)
        ll, N, W, Z = self.forward(A, B) if env is None else self.forward(A, B, env=env)
        inside = self.envelopeRows(env, len(A), len(B))
        if inside is not None:
            inside = [set(rs) for rs in inside]
        return A, B, ll, N, W, Z, inside

    def samplePaths(self, A, B, nSamples: int, seed: int = 0, pair: int = 0, env=None, margins: Optional[list] = None):
        """(loglike, [(edges, rows, inRows, logq), ...]): ``nSamples`` paths drawn from the posterior by a stochastic traceback over
        forward(A, B, env=env) -- the yardstick of k_profile_two_sample (docs/profile_tapes.md, "Posterior path samples of pairs of
        profiles").  From Z[K][L][S-1] back to N[0][0][0]; every visit of a Z cell with i > 0, of a W cell, or of an N cell with
        r > 0 is one decision among sampleCandidates() and takes one counter value t, however many candidates it has; a Z cell with
        i = 0 moves to its W without one.  The draw is PairProfileDP.samplePaths': p_c = exp(term_c - cell), acc adds them in order
        from 0.0, the first c with u < acc is taken, else the last c with p_c > 0; u = sample_uniform(seed, pair, j, t).  logq sums
        term - cell over the decisions: the path's log posterior probability.  Paths are as viterbi()'s; a -inf pair gives empty
        paths and logq = -inf.  ``margins`` (a list) receives per decision the least |u - acc_c| over all partial sums acc_c of
        the decision."""
        A, B, ll, N, W, Z, inside = self._sampleLattice(A, B, env)
        layers = (N, W, Z)
        out = []
        for j in range(int(nSamples)):
            edges: List[int] = []; rows: List[int] = []; ins: List[int] = []
            if not ll > _NEG:
                out.append((np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), _NEG))
                continue
            i, r, q, layer, t, logq = len(A), len(B), self.S - 1, 2, 0, 0.0
            while layer or r > 0:
                if layer == 2 and i == 0:
                    layer = 1
                    continue
                cur = float(layers[layer][i, r, q])
                cand = self.sampleCandidates(A, B, N, W, Z, inside, i, r, q, layer)
                u = sample_uniform(seed, pair, j, t)
                t += 1
                acc, pick, last, margin = 0.0, None, None, math.inf
                for c in cand:
                    p = math.exp(c[3] - cur) if c[3] > _NEG else 0.0
                    acc += p
                    margin = min(margin, abs(u - acc))
                    if p > 0.0:
                        last = c
                    if pick is None and u < acc:
                        pick = c
                if pick is None:
                    pick = last
                if pick is None:
                    raise MachineError("samplePaths: no candidate with a positive probability")
                if margins is not None:
                    margins.append(margin)
                kind, e, s, term = pick
                logq += term - cur
                i, r, q, layer = self._sampleMove(kind, e, s, i, r, q, layer, edges, rows, ins)
            assert i == 0 and q == 0
            out.append((np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32), np.array(ins[::-1], np.int32), logq))
        return ll, out

    def pathProbability(self, A, B, edges, rows, inRows, env=None) -> float:
        """The log posterior probability of one path (in the format of viterbi()): the path replayed backwards through the
        decisions of samplePaths() over forward(A, B, env=env), the sum of term - cell over them.  The edges with both coordinates
        fix every decision: an edge arrives at the input row it read plus one (at inRows, if it read none) and likewise on the
        output tape, so at a Z cell the input blank is taken while the cell lies past the arrival of the edge before it, then at the
        W cell that edge if it wrote nothing, else "stay", and at the N cell the output blank while the cell lies past the arrival.
        Raises MachineError where the path leaves the lattice (or the envelope); -inf for a pair whose likelihood is -inf."""
        A, B, ll, N, W, Z, inside = self._sampleLattice(A, B, env)
        if not ll > _NEG:
            return _NEG
        layers = (N, W, Z)
        em = self.em
        edges = [int(e) for e in edges]; rows = [int(v) for v in rows]; inRows = [int(v) for v in inRows]
        if not len(edges) == len(rows) == len(inRows):
            raise MachineError("pathProbability: edges, rows and inRows differ in length")
        p = len(edges) - 1
        i, r, q, layer, logq = len(A), len(B), self.S - 1, 2, 0.0
        sink: List[int] = []
        while layer or r > 0:
            if layer == 2 and i == 0:
                layer = 1
                continue
            e = edges[p] if p >= 0 else -1
            reads, writes = (bool(em.inTok[e]), bool(em.outTok[e])) if p >= 0 else (False, False)
            ai, ar = (inRows[p] + reads, rows[p] + writes) if p >= 0 else (0, 0)      # where the edge before arrives
            if layer == 2:
                want = ("wait", -1) if ai == i else ("inblank", -1)
            elif layer == 1:
                want = (("ins" if reads else "silent"), e) if p >= 0 and not writes and (ai, ar) == (i, r) else ("stay", -1)
            else:
                want = (("match" if reads else "emit"), e) if p >= 0 and writes and (ai, ar) == (i, r) else ("blank", -1)
            cur = float(layers[layer][i, r, q])
            hit = [c for c in self.sampleCandidates(A, B, N, W, Z, inside, i, r, q, layer) if (c[0], c[1]) == want]
            if len(hit) != 1 or not hit[0][3] > _NEG:
                raise MachineError("pathProbability: the path leaves the lattice at (%d, %d, %d)" % (i, r, q))
            kind, e, s, term = hit[0]
            logq += term - cur
            if e >= 0:
                p -= 1
            i, r, q, layer = self._sampleMove(kind, e, s, i, r, q, layer, sink, sink, sink)
        if i != 0 or q != 0 or p >= 0:
            raise MachineError("pathProbability: the path does not reach the start")
        return logq


class TwoMergedProfileDP(TwoProfileDP):
    """A machine WITH an input alphabet between an input profile and a CTC-MERGED output profile, in numpy -- the yardstick of
    mb_profile_two_merge.hip (docs/profile_tapes.md, "Pairs of profiles against a merged profile"): the semantics of
    compose(A.machine(), compose(M, mergingRecogniserMachine())) with both tapes empty.  The lattice of TwoProfileDP with the plane
    axis of MergedProfileDP: plane 0 = the last row took the blank (or no row yet), plane c = the last row took column c, whose
    output token is colTok[c - 1].  XW and XZ are the exclusion vectors over W and over Z:

        XW[i][r][c][s] = (+)_{k != c} W[i][r][k][s]          XZ[i][r][c][s] = (+)_{k != c} Z[i][r][k][s]
        N[i][r][0][d]  = [i = 0, r = 0, d = 0]  (+)  (+)_p (N[i][r-1][p][d] + B[r-1][0])                      (output blank; r > 0)
        N[i][r][c][d]  = (N[i][r-1][c][d] + B[r-1][c])                                                        (repeat; r > 0)
                         (+) sum_{t: s->d, in = a,   out = colTok[c]} ((XZ[i-1][r-1][c][s] + w_t) + A[i-1][a]) + B[r-1][c]   (match)
                         (+) sum_{t: s->d, in = eps, out = colTok[c]} (XW[i][r-1][c][s] + w_t) + B[r-1][c]                   (output-only)
        W[i][r][p][d]  = N[i][r][p][d]
                         (+) sum_{t: in = a, out = eps} (Z[i-1][r][p][s] + w_t) + A[i-1][a]                   (input-only; same plane)
                         (+) sum_{silent t, s < d}      W[i][r][p][s] + w_t                                   (silent levels, per plane)
        Z[i][r][p][d]  = W[i][r][p][d]  (+)  Z[i-1][r][p][d] + A[i-1][0]                                      (input blank; same plane)
        loglike        = (+)_p Z[K][L][p][S-1]

    The output blank and the repeat read N, never W.  Viterbi keeps the FIRST maximum -- N[.][.][0]: planes ascending; N[.][.][c]:
    the repeat, then the match edges in `incoming` order (input token ascending), then the output-only edges, each from the lowest
    plane k != c that attains its XZ / XW; W: "no move", then the input-only edges, then the silent edges; Z: W, then the input
    blank; the end: planes ascending.  Every method takes (A, B): A the [K, nInTok + 1] log rows of Profile.logRowsIn, B the
    [L, nCols + 1] log rows of Profile.mergeRows.  Lattices are [K + 1, L + 1, nCols + 1, S]; every sweep is vectorised over planes
    and states.

    ``env`` (forward, backward, counts, mergedRowPosteriors, viterbi): as TwoProfileDP's, checked by envelopeRows with K for I --
    cell (i, r) exists iff inStart[r] <= i < inEnd[r], in every plane; N, W, Z, XW, XZ and NB, WB, ZB of every other cell are -inf
    (docs/profile_tapes.md, "Pairs of profiles against a merged profile under an envelope").  The sweeps visit the envelope cells
    alone and read a cell outside as the -inf it is.  Without it not one operation differs."""

    def __init__(self, em: EvaluatedMachine, colTok: Sequence[int]):
        super().__init__(em)
        self.colTok = np.asarray(colTok, np.int64).reshape(-1)
        self.nCols = len(self.colTok)
        if self.nCols < 1:
            raise MachineError("merged profiles need at least one column")
        if self.colTok.min() < 1 or self.colTok.max() > em.nOutTok:
            raise MachineError("column token outside 1..nOutTok")
        self.PL = self.nCols + 1

        def by_column(o):
            """(indices into a table whose out tokens are ``o``, column) of its edges whose token heads a column: column-major,
            `incoming` order within"""
            sel = [np.nonzero(o == t)[0] for t in self.colTok]
            col = np.concatenate([np.full(len(k), c + 1, np.int64) for c, k in enumerate(sel)])
            return np.concatenate(sel).astype(np.int64), col
        mE, mS, mD, mW, mA, mO = self.mAll
        k, col = by_column(mO)
        self.mCol = (mE[k], mS[k], mD[k], mW[k], mA[k], col)       # (edge id, src, dst, w, in token, column)
        k, col = by_column(np.asarray(self.eO))
        self.emitCol = (self.eId[k], self.eS[k], self.eD[k], self.eW[k], col)

    def _check(self, P) -> np.ndarray:
        P = np.asarray(P, np.float64).reshape(-1, self.PL)
        if np.isnan(P).any() or (P == math.inf).any():
            raise MachineError("profile weight is NaN or +infinity")
        return P

    def _planes(self, fold, base: np.ndarray, d: np.ndarray, vals: np.ndarray) -> np.ndarray:
        """fold over (plane, state) at once: vals[PL, n] into base[PL, S] at column d[n] of every plane"""
        S = self.S
        idx = (np.arange(self.PL)[:, None] * S + d[None, :]).ravel()
        return fold(base.ravel(), idx, vals.ravel()).reshape(self.PL, S)

    def sampleCandidates(self, *args, **kwargs):
        """Merged pairs of profiles are not sampled (mb_profile_twos_sample refuses them): the plain rule knows no planes."""
        raise MachineError("sampling takes plain profiles")

    samplePaths = pathProbability = sampleCandidates

    def forward(self, A, B, mode: str = "exact", env=None):
        """(loglike, N, W, Z), each [K+1][L+1][nCols+1][S]; mode "exact" or "max"."""
        return self._sweep(A, B, mode, env)[:4]

    def _sweep(self, A, B, mode: str, env=None):
        """forward() and the exclusion vectors XW, XZ [K+1][L+1][nCols+1][S] (plane 0 of either is not read)"""
        A, B = self._checkTwo(A, B)
        mx = mode == "max"
        fold = _max_fold if mx else _lse_fold
        K, L, S, PL = len(A), len(B), self.S, self.PL
        shape = (K + 1, L + 1, PL, S)
        N = np.full(shape, _NEG); W = np.full(shape, _NEG); Z = np.full(shape, _NEG)
        XW = np.full(shape, _NEG); XZ = np.full(shape, _NEG)
        _, mS, mD, mW, mA, mC = self.mCol
        _, eS, eD, eW, eC = self.emitCol
        _, iS, iD, iW, iA, _ = self.iAll
        inside = self.envelopeRows(env, K, L)
        for i in range(K + 1):
            for r in (range(L + 1) if inside is None else inside[i]):      # (a cell outside stays -inf and is read as such)
                base = np.full((PL, S), _NEG)
                if i == 0 and r == 0:
                    base[0, 0] = 0.0
                if r:
                    Br = B[r - 1]
                    base[0] = _red_planes(N[i, r - 1] + Br[0], mx)
                    flat = (N[i, r - 1] + Br[:, None]).ravel()
                    flat[:S] = base[0]
                    idx, vals = [], []
                    if i:
                        idx.append(mC * S + mD); vals.append(((XZ[i - 1, r - 1][mC, mS] + mW) + A[i - 1][mA]) + Br[mC])
                    idx.append(eC * S + eD); vals.append((XW[i, r - 1][eC, eS] + eW) + Br[eC])
                    base = fold(flat, np.concatenate(idx), np.concatenate(vals)).reshape(PL, S)
                N[i, r] = base
                w_ = base.copy()
                if i:
                    w_ = self._planes(fold, w_, iD, (Z[i - 1, r][:, iS] + iW) + A[i - 1][iA])
                for lv in self.fLevels:
                    w_ = self._planes(fold, w_, self.sD[lv], w_[:, self.sS[lv]] + self.sW[lv])
                W[i, r] = w_
                z_ = self._planes(fold, w_, self._all, Z[i - 1, r] + A[i - 1][0]) if i else w_
                Z[i, r] = z_
                XW[i, r] = _excl_planes(w_, mx)
                XZ[i, r] = _excl_planes(z_, mx)
        return float(_red_planes(Z[K, L, :, S - 1:S], mx)[0]), N, W, Z, XW, XZ

    def backward(self, A, B, env=None):
        """(loglike, NB, WB, ZB), each [K+1][L+1][nCols+1][S], exact log-sum-exp; loglike = NB[0][0][0][0]."""
        A, B = self._checkTwo(A, B)
        K, L, S, PL = len(A), len(B), self.S, self.PL
        shape = (K + 1, L + 1, PL, S)
        NB = np.full(shape, _NEG); WB = np.full(shape, _NEG); ZB = np.full(shape, _NEG)
        _, mS, mD, mW, mA, mC = self.mCol
        _, eS, eD, eW, eC = self.emitCol
        _, iS, iD, iW, iA, _ = self.iAll
        neg = np.full(PL * S, _NEG)
        inside = self.envelopeRows(env, K, L)
        for i in range(K, -1, -1):
            for r in (range(L, -1, -1) if inside is None else reversed(inside[i])):
                base = np.full((PL, S), _NEG)
                if i == K and r == L:
                    base[:, S - 1] = 0.0
                if i < K:
                    base = np.logaddexp(base, A[i][0] + ZB[i + 1, r])
                    if r < L:
                        # TZ[c][s]: everything that leaves the committed s through column c; ZB[k] takes the columns other than k
                        TZ = _lse_fold(neg, mC * S + mS, ((mW + A[i][mA]) + B[r][mC]) + NB[i + 1, r + 1][mC, mD]).reshape(PL, S)
                        base = np.logaddexp(base, _excl_planes(TZ, False))
                    base = self._planes(_lse_fold, base, iS, (iW + A[i][iA]) + WB[i + 1, r][:, iD])
                ZB[i, r] = base
                if r < L:
                    TW = _lse_fold(neg, eC * S + eS, (eW + B[r][eC]) + NB[i, r + 1][eC, eD]).reshape(PL, S)
                    base = np.logaddexp(base, _excl_planes(TW, False))
                for lv in self.bLevels:
                    base = self._planes(_lse_fold, base, self.sS[lv], base[:, self.sD[lv]] + self.sW[lv])
                WB[i, r] = base
                if r < L:
                    nb = np.logaddexp(base, B[r][0] + NB[i, r + 1][0])
                    nb[1:] = np.logaddexp(nb[1:], B[r][1:, None] + NB[i, r + 1][1:])
                    NB[i, r] = nb
                else:
                    NB[i, r] = base
        return float(NB[0, 0, 0, 0]), NB, WB, ZB

    def counts(self, A, B, blanks: Optional[list] = None, env=None) -> Tuple[np.ndarray, float]:
        """(posterior expected use of every transition, Forward loglike); nothing for a -inf pair.  Blanks of either tape and
        repeat rows are not edges; ``blanks`` (a list) receives (mass of the output blanks, mass of the repeats, mass of the input
        blanks), summed over the lattice."""
        A, B = self._checkTwo(A, B)
        ll, NF, WF, ZF, XW, XZ = self._sweep(A, B, "exact", env)
        out = np.zeros(self.em.nTransitions)
        if not ll > _NEG:
            return out, ll
        _, NB, WB, ZB = self.backward(A, B) if env is None else self.backward(A, B, env=env)
        K, L = len(A), len(B)
        inside = self.envelopeRows(env, K, L)
        mE, mS, mD, mW, mA, mC = self.mCol
        eE, eS, eD, eW, eC = self.emitCol
        iE, iS, iD, iW, iA, _ = self.iAll
        outBlank = repeat = inBlank = 0.0

        def mass(b):
            return float(np.exp(b[b > _NEG]).sum())
        with np.errstate(invalid="ignore"):
            for i in range(K + 1):
                for r in (range(L + 1) if inside is None else inside[i]):      # (a term into a cell outside is exp(-inf))
                    f, z = WF[i, r] - ll, ZF[i, r] - ll
                    fx, zx = XW[i, r] - ll, XZ[i, r] - ll
                    if r < L:
                        if i < K:
                            np.add.at(out, mE, np.exp(zx[mC, mS] + (((mW + A[i][mA]) + B[r][mC]) + NB[i + 1, r + 1][mC, mD])))
                        np.add.at(out, eE, np.exp(fx[eC, eS] + ((eW + B[r][eC]) + NB[i, r + 1][eC, eD])))
                        n = NF[i, r] - ll
                        outBlank += mass(n + (B[r][0] + NB[i, r + 1][0]))
                        repeat += mass(n[1:] + (B[r][1:, None] + NB[i, r + 1][1:]))
                    if i < K:
                        np.add.at(out, iE, np.exp(z[:, iS] + ((iW + A[i][iA]) + WB[i + 1, r][:, iD])).sum(axis=0))
                        inBlank += mass(z + (A[i][0] + ZB[i + 1, r]))
                    np.add.at(out, self.sId, np.exp(f[:, self.sS] + (WB[i, r][:, self.sD] + self.sW)).sum(axis=0))
        if blanks is not None:
            blanks.append((outBlank, repeat, inBlank))
        return out, ll

    def rowPosteriors(self, A, B, env=None):
        raise MachineError("row posteriors take plain profiles")

    def mergedRowPosteriors(self, A, B, repeats: Optional[list] = None, env=None) -> Tuple[np.ndarray, np.ndarray, float]:
        """(postA[K, nInTok + 1], postB[L, nCols + 1], Forward loglike): postB[r][c] is the posterior probability that output row r
        was consumed as column c (column 0: as the blank), postA[i][a] that input row i was consumed as input token a (column 0:
        as the input blank) -- the gradients of loglike in B[r][c] and in A[i][a] (docs/profile_tapes.md, "Row posteriors of pairs
        of profiles against a merged profile").  The terms of counts() and of its three masses, the emitting ones taken plane by
        plane off Z and W instead of through XZ and XW, binned by (row, column) of either tape; a match term goes to both tables.
        ``repeats``, if a list, receives the [L, nCols + 1] repeat part of postB, so that postB - repeats sums per token to the
        counts.  Every row of either table sums to 1; zeros for a -inf pair; exactly 0 where the weight is -inf."""
        A, B = self._checkTwo(A, B)
        ll, NF, WF, ZF = self.forward(A, B) if env is None else self.forward(A, B, env=env)
        K, L, PL = len(A), len(B), self.PL
        postA = np.zeros((K, self.em.nInTok + 1)); postB = np.zeros((L, PL)); rep = np.zeros((L, PL))
        if repeats is not None:
            repeats.append(rep)
        if not ll > _NEG:
            return postA, postB, ll
        _, NB, WB, ZB = self.backward(A, B) if env is None else self.backward(A, B, env=env)
        inside = self.envelopeRows(env, K, L)
        _, mS, mD, mW, mA, mC = self.mCol
        _, eS, eD, eW, eC = self.emitCol
        _, iS, iD, iW, iA, _ = self.iAll
        planes = np.arange(PL)[:, None]
        mKeep, eKeep = mC[None, :] != planes, eC[None, :] != planes      # [plane k, edge]: the edge's column is another than k

        def mass(b):
            return float(np.exp(b[b > _NEG]).sum())
        with np.errstate(invalid="ignore"):
            for i in range(K + 1):
                for r in (range(L + 1) if inside is None else inside[i]):      # (a term into a cell outside is dead)
                    f, z = WF[i, r] - ll, ZF[i, r] - ll
                    if r < L:
                        if i < K:
                            t = z[:, mS] + (((mW + A[i][mA]) + B[r][mC]) + NB[i + 1, r + 1][mC, mD])[None, :]
                            live = mKeep & (t > _NEG)
                            np.add.at(postB[r], np.broadcast_to(mC, t.shape)[live], np.exp(t[live]))
                            np.add.at(postA[i], np.broadcast_to(mA, t.shape)[live], np.exp(t[live]))
                        t = f[:, eS] + ((eW + B[r][eC]) + NB[i, r + 1][eC, eD])[None, :]
                        live = eKeep & (t > _NEG)
                        np.add.at(postB[r], np.broadcast_to(eC, t.shape)[live], np.exp(t[live]))
                        n = NF[i, r] - ll
                        postB[r, 0] += mass(n + (B[r][0] + NB[i, r + 1][0]))
                        b = n[1:] + (B[r][1:, None] + NB[i, r + 1][1:])
                        rep[r, 1:] += np.where(b > _NEG, np.exp(b), 0.0).sum(axis=1)
                    if i < K:
                        t = z[:, iS] + ((iW + A[i][iA]) + WB[i + 1, r][:, iD])
                        live = t > _NEG
                        np.add.at(postA[i], np.broadcast_to(iA, t.shape)[live], np.exp(t[live]))
                        postA[i, 0] += mass(z + (A[i][0] + ZB[i + 1, r]))
        postB += rep
        return postA, postB, ll

    def viterbi(self, A, B, census: Optional[dict] = None, env=None) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
        """(score, global edge ids start -> end, output row, input row at which each fired); the first maximum in the fill's
        candidate order, rows as TwoProfileDP.viterbi; blanks of either tape and repeat rows are not edges.  ``census``: per step
        at which two or more candidates equal the cell, a count under the tuple of the kinds that tie, in candidate order ("repeat",
        "match", "emit" at N[.][.][c]; "stay", "ins", "silent" at a W cell; "wait", "inblank" at a Z cell); under ("blank",) the
        steps at N[.][.][0] that two planes attain, under ("plane",) the emitting edges whose XZ / XW two planes attain, under
        ("end",) an end that two planes attain.  Under ``env`` a candidate whose source cell lies outside the envelope is -inf and
        loses; the census counts, under ("outside", kind), the steps that had such a candidate of that kind ("blank" for the
        step at N[.][.][0])."""
        A, B = self._checkTwo(A, B)
        v, N, W, Z = self.forward(A, B, "max") if env is None else self.forward(A, B, "max", env=env)
        inside = self.envelopeRows(env, len(A), len(B))
        edges: List[int] = []; rows: List[int] = []; ins: List[int] = []
        if not v > _NEG:
            return v, np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32)

        def tie(kinds, n: int = 2):
            if census is not None and n > 1:
                census[kinds] = census.get(kinds, 0) + 1

        def outside(kinds):
            """the census of the candidate kinds of cell (i, r) whose sources lie outside"""
            if census is None or inside is None:
                return
            for kind in dict.fromkeys(k for k in kinds if k not in ("wait", "stay", "silent")):
                si = i - (kind in ("inblank", "ins", "match"))
                sr = r - (kind in ("blank", "repeat", "match", "emit"))
                if sr not in inside[si]:
                    census[("outside", kind)] = census.get(("outside", kind), 0) + 1
        mE, mS, mD, mW, mA, mO = self.mAll
        iE, iS, iD, iW, iA, _ = self.iAll
        i, r, q, layer = len(A), len(B), self.S - 1, 2
        ends = [p for p in range(self.PL) if Z[i, r, p, q] == v]
        tie(("end",), len(ends))
        p = ends[0]
        while True:
            cand = []          # (kind, edge id or -1, source state, exclusion value or None, attains the cell)
            if layer == 2:
                cur = Z[i, r, p, q]
                cand.append(("wait", -1, q, None, W[i, r, p, q] == cur))
                if i:
                    cand.append(("inblank", -1, q, None, Z[i - 1, r, p, q] + A[i - 1][0] == cur))
            elif layer == 1:
                cur = W[i, r, p, q]
                cand.append(("stay", -1, q, None, N[i, r, p, q] == cur))
                if i:
                    cand += [("ins", int(iE[k]), int(iS[k]), None, (Z[i - 1, r, p, iS[k]] + iW[k]) + A[i - 1][iA[k]] == cur)
                             for k in np.nonzero(iD == q)[0]]
                cand += [("silent", int(self.sId[k]), int(self.sS[k]), None, W[i, r, p, self.sS[k]] + self.sW[k] == cur) for k in self.inSil[q]]
            else:
                if r == 0:
                    assert i == 0 and q == 0 and p == 0
                    break
                Br, cur = B[r - 1], N[i, r, p, q]
                if p == 0:
                    outside(["blank"])
                    hit = [N[i, r - 1, k, q] + Br[0] == cur for k in range(self.PL)]
                    tie(("blank",), sum(hit))
                    p = hit.index(True)
                    r -= 1
                    continue
                oth = [k for k in range(self.PL) if k != p]
                tok = self.colTok[p - 1]
                cand.append(("repeat", -1, q, None, N[i, r - 1, p, q] + Br[p] == cur))
                if i:
                    for k in np.nonzero((mD == q) & (mO == tok))[0]:
                        xv = max(Z[i - 1, r - 1, o_, mS[k]] for o_ in oth)
                        cand.append(("match", int(mE[k]), int(mS[k]), xv, ((xv + mW[k]) + A[i - 1][mA[k]]) + Br[p] == cur))
                for k in self.inEmit[q]:
                    if self.eO[k] == tok:
                        xv = max(W[i, r - 1, o_, self.eS[k]] for o_ in oth)
                        cand.append(("emit", int(self.eId[k]), int(self.eS[k]), xv, (xv + self.eW[k]) + Br[p] == cur))
            outside(c[0] for c in cand)
            hits = [c for c in cand if c[4]]
            if len(hits) > 1:
                tie(tuple(dict.fromkeys(c[0] for c in hits)))
            kind, e, s, xv, _ = hits[0]
            if kind == "wait":
                layer = 1
            elif kind == "inblank":
                i -= 1
            elif kind == "stay":
                layer = 0
            elif kind == "repeat":
                r -= 1
            elif kind == "silent":
                edges.append(e); rows.append(r); ins.append(i); q = s
            elif kind == "ins":
                i -= 1
                edges.append(e); rows.append(r); ins.append(i); q = s; layer = 2
            else:
                r -= 1
                if kind == "match":
                    i -= 1
                V = Z if kind == "match" else W
                src = [k for k in oth if V[i, r, k, s] == xv]
                tie(("plane",), len(src))
                edges.append(e); rows.append(r); ins.append(i); q = s; p = src[0]
                layer = 2 if kind == "match" else 1
        return v, np.array(edges[::-1], np.uint32), np.array(rows[::-1], np.int32), np.array(ins[::-1], np.int32)
