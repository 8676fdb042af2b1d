"""Shared helpers of the merged (CTC) profile tests (test_profile_merge_host.py, test_profile_merge_gpu.py): random CSV profiles with
duplicated and foreign header symbols, the weight of a merged Viterbi path, and the device-against-restatement comparison."""
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
