"""Shared helpers of the profile-tape tests (test_profile_gpu.py, test_profile_edges_gpu.py, test_profile_host.py): random
profiles, the device-against-restatement comparison, the restatement's Viterbi tie census, machines as Machine objects."""
import numpy as np

from machineboss_amd import capi
from machineboss_amd.machine import Machine, MachineState, MachineTransition
from machineboss_amd.profile import ProfileDP


def _profiles(em, lengths, seed, zeros=0.2):
    rng = np.random.RandomState(seed)
    out = []
    for L in lengths:
        P = np.log(rng.uniform(0.02, 1.0, (L, em.nOutTok + 1)))
        P[rng.rand(L, em.nOutTok + 1) < zeros] = -np.inf
        out.append(P)
    return out


def _close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    both_inf = (a == -np.inf) & (b == -np.inf)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_inf | (np.abs(a - b) <= rel * np.maximum(1.0, np.abs(b)))))


def _check_all(em, profs, fill=True):
    """Every device sweep of `profs` against the restatement: rolling and materialised Forward (and the same bits from both),
    Viterbi scores and paths exactly, counts (exactly 0 on transitions that read input), and the three lattices of the longest
    profile through profile_fill."""
    import pytest
    dm = capi.DeviceMachine(em)
    dp = ProfileDP(em)
    dev = capi.DeviceProfiles(dm, profs)
    ref = [dp.forward(P) for P in profs]
    want = np.array([r[0] for r in ref])
    fr, fm = dev.forward(capi.MB_ROLLING), dev.forward(capi.MB_MATERIALISE)
    assert _close(fr, want, 1e-9)
    assert _close(fm, want, 1e-9)
    assert np.array_equal(fr, fm)                     # the same arithmetic in LDS / scratch and in the pool
    v, off, edges, rows = dev.viterbi()
    v0, _, _, _ = dev.viterbi(paths=False)
    for k, P in enumerate(profs):
        rv, re_, rr = dp.viterbi(P)
        assert v[k] == rv and v0[k] == rv, (k, v[k], rv)
        assert np.array_equal(edges[off[k]:off[k + 1]], re_) and np.array_equal(rows[off[k]:off[k + 1]], rr), k
    c, s, ll = dev.counts()
    rc = np.zeros(em.nTransitions)
    for P in profs:
        rc += dp.counts(P)[0]
    assert _close(ll, want, 1e-9)
    assert np.allclose(c, rc, rtol=1e-6, atol=1e-9), np.abs(c - rc).max()
    assert np.all(c[np.asarray(em.inTok) != 0] == 0.0)   # the input tape is empty: nothing that reads it fires
    assert s == pytest.approx(float(np.sum(want)), rel=1e-9) if np.all(want > -np.inf) else True
    if fill and profs:
        k = int(np.argmax([len(q) for q in profs]))
        P, (_, N, W) = profs[k], ref[k]
        F = capi.profile_fill(dm, capi.MB_FORWARD, P)
        assert _close(F[:, 0], N, 1e-9) and _close(F[:, 1], W, 1e-9)
        _, Nv, Wv = dp.forward(P, "max")
        V = capi.profile_fill(dm, capi.MB_VITERBI, P)
        assert np.array_equal(V[:, 0], Nv) and np.array_equal(V[:, 1], Wv)
        _, NB, WB = dp.backward(P)
        B = capi.profile_fill(dm, capi.MB_BACKWARD, P)
        assert _close(B[:, 0], NB, 1e-9) and _close(B[:, 1], WB, 1e-9)
    return dm, dev, c


def tie_census(dp, P):
    """Steps of the restatement's first-maximum traceback of P at which two or more candidates equal the cell, by the candidate
    taken: "blank" / "emit" at an N cell, "stay" (no move) / "silent" at a W cell."""
    out = {"blank": 0, "emit": 0, "stay": 0, "silent": 0}
    v, N, W = dp.forward(P, "max")
    if not v > -np.inf:
        return out
    r, q, layer = len(P), dp.S - 1, 1
    while True:
        if layer == 1:
            cur = W[r, q]
            c = [N[r, q] == cur] + [W[r, dp.sS[k]] + dp.sW[k] == cur for k in dp.inSil[q]]
            if sum(c) > 1:
                out["stay" if c[0] else "silent"] += 1
            if c[0]:
                layer = 0
                continue
            k = next(k for k in dp.inSil[q] if W[r, dp.sS[k]] + dp.sW[k] == cur)
            q = int(dp.sS[k])
        else:
            if r == 0:
                break
            Pr, cur = P[r - 1], N[r, q]
            c = [N[r - 1, q] + Pr[0] == cur] + [(W[r - 1, dp.eS[k]] + dp.eW[k]) + Pr[dp.eO[k]] == cur for k in dp.inEmit[q]]
            if sum(c) > 1:
                out["blank" if c[0] else "emit"] += 1
            if c[0]:
                r -= 1
                continue
            k = next(k for k in dp.inEmit[q] if (W[r - 1, dp.eS[k]] + dp.eW[k]) + Pr[dp.eO[k]] == cur)
            r -= 1
            q, layer = int(dp.eS[k]), 1
    return out


def _machine_of(em):
    """An EvaluatedMachine (randmachine) as a Machine with numeric weights, transitions in global-id order."""
    m = Machine()
    for _ in range(em.nStates):
        m.state.append(MachineState())
    isym, osym = em.inputTokenizer.tok2sym, em.outputTokenizer.tok2sym
    for e in range(em.nTransitions):
        m.state[int(em.src[e])].trans.append(MachineTransition(dest=int(em.dst[e]), inp=isym[em.inTok[e]] if em.inTok[e] else "",
                                                                out=osym[em.outTok[e]] if em.outTok[e] else "", weight=float(np.exp(em.logWeight[e]))))
    return m
