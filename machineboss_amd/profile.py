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
"""
from __future__ import annotations

import math
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .evalmachine import EvaluatedMachine
from .machine import Machine, MachineError, MachineState, MachineTransition

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
        syms = em.outputTokenizer.tok2sym
        cols: List[List[int]] = [[len(self.header)]] + [[c for c, h in enumerate(self.header) if h == syms[t]] for t in range(1, len(syms))]
        P = np.empty((len(self.row), len(cols)), np.float64)
        for r, row in enumerate(self.row):
            for t, cs in enumerate(cols):
                v = sum(row[c] for c in cs if c < len(row))
                if v < 0 or math.isnan(v):
                    raise MachineError("Profile row %d: weight %g is not a probability" % (r, v))
                P[r, t] = math.log(v) if v > 0 else -math.inf
        return P

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
