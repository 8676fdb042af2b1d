"""Profile tapes on the GPU (docs/profile_tapes.md): rolling Forward, Viterbi with paths and posterior counts of a machine against
profile tapes, in G lattice cells (row x state) per second, next to the same machine's token sweep at the same length and the
composed-machine route (compose(M, recogniser) swept by the generic family with empty tapes) at a size it finishes.

    python scripts/bench_profile.py [--quick] [--out FILE.json]

(a) a 2 kb DNA generator against 64 profiles x 8 000 rows x 5 columns; (b) the 5 063-state config-5 machine (bench.py) against
64 x 10 000-row DNA profiles.  --quick: 1/8 of the rows (a rehearsal).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from machineboss_amd import algebra as A, capi  # noqa: E402
from machineboss_amd.evalmachine import EvaluatedMachine  # noqa: E402
from machineboss_amd.machine import Machine  # noqa: E402
from machineboss_amd.profile import Profile  # noqa: E402


def timed(fn, reps=1):
    fn()                                   # warm-up: code objects, pools
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.synchronize()
    return r, (time.perf_counter() - t) / reps


def dna_profiles(em, n, rows, seed):
    """Basecaller-like rows over A, C, G, T + blank (probabilities, one dominant symbol), as log weights in em's alphabet."""
    rng = np.random.RandomState(seed)
    hdr = ["A", "C", "G", "T"]
    out = []
    for _ in range(n):
        v = rng.dirichlet([0.3] * 5, rows).astype(np.float32).astype(np.float64)
        out.append(Profile(hdr, v.tolist()).logRows(em))
    return out


def run_case(name, em, profs, tokenLen, out):
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, profs)
    cells = float(sum(len(p) + 1 for p in profs)) * em.nStates
    ll, tf = timed(lambda: dev.forward(capi.MB_ROLLING), 2)
    _, tv = timed(lambda: dev.viterbi(), 1)
    _, tc = timed(lambda: dev.counts(), 1)
    rng = np.random.RandomState(1)
    b = capi.DeviceBatch.from_pairs(dm, [([], rng.randint(1, em.nOutTok + 1, tokenLen)) for _ in profs])
    _, tt = timed(lambda: b.forward(capi.MB_ROLLING), 2)
    ktok = capi.last_kernel_name()
    r = {"states": em.nStates, "transitions": em.nTransitions, "silent_levels": dm.n_levels(), "profiles": len(profs),
         "rows": int(len(profs[0])), "cells": cells,
         "forward_rolling_gcells_s": round(cells / tf / 1e9, 3), "viterbi_paths_gcells_s": round(cells / tv / 1e9, 3),
         "counts_gcells_s": round(cells / tc / 1e9, 3), "forward_s": round(tf, 4), "viterbi_s": round(tv, 4), "counts_s": round(tc, 4),
         "token_sweep_forward_rolling_gcells_s": round(cells / tt / 1e9, 3), "token_sweep_kernel": ktok,
         "loglike_0": float(ll[0])}
    out[name] = r
    print(name, json.dumps(r), flush=True)


def composed_route(out):
    """compose(generator, recogniser) with empty tapes on the generic token path, at a size the host composition finishes."""
    rng = np.random.RandomState(3)
    seq = list(rng.choice(list("ACGT"), 60))
    G = A.generator(seq, "g")
    em = EvaluatedMachine.fromMachine(G, {}, useDefaults=True)
    rows = np.random.RandomState(4).dirichlet([0.3] * 5, 200).astype(np.float32).astype(np.float64).tolist()
    prof = Profile(["A", "C", "G", "T"], rows)
    t0 = time.perf_counter()
    C = A.compose(G, prof.recogniserMachine())
    ec = EvaluatedMachine.fromMachine(C, {}, useDefaults=True)
    tcomp = time.perf_counter() - t0
    dmc = capi.DeviceMachine(ec)
    b = capi.DeviceBatch.from_pairs(dmc, [([], [])] * 64)
    llc, tcd = timed(lambda: b.forward(capi.MB_ROLLING), 1)
    dm = capi.DeviceMachine(em)
    dev = capi.DeviceProfiles(dm, [prof.logRows(em)] * 64)
    ll, tp = timed(lambda: dev.forward(capi.MB_ROLLING), 2)
    cells = 64.0 * (len(rows) + 1) * em.nStates
    r = {"generator_states": em.nStates, "rows": len(rows), "composed_states": ec.nStates, "host_compose_s": round(tcomp, 3),
         "composed_forward_s": round(tcd, 4), "profile_forward_s": round(tp, 5), "speedup": round(tcd / tp, 1),
         "composed_gcells_s": round(cells / tcd / 1e9, 4), "profile_gcells_s": round(cells / tp / 1e9, 3),
         "agree": bool(abs(llc[0] - ll[0]) <= 1e-6 * abs(ll[0]))}
    out["composed_route"] = r
    print("composed_route", json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if capi.device_count() == 0:
        raise SystemExit("bench_profile.py needs a GPU")
    capi.set_device(0)
    div = 8 if a.quick else 1
    out = {}
    rng = np.random.RandomState(2)
    G = A.generator(list(rng.choice(list("ACGT"), 2000)), "g")
    emA = EvaluatedMachine.fromMachine(G, {}, useDefaults=True)
    run_case("a_dna_generator_2kb", emA, dna_profiles(emA, 64, 8000 // div, 5), 8000 // div, out)
    from machineboss_amd.hmmer import HmmerModel
    P = lambda n: Machine.fromFile(os.path.join(ROOT, "tests", "golden", "preset", n + ".json"))
    h = HmmerModel.fromFile(os.path.join(ROOT, "tests", "golden", "hmmer", "fn3.hmm")).truncated(20)
    em5 = EvaluatedMachine.fromMachine(A.composeLeftToRight([h.machine(True), P("simple_introns"), P("translate"), P("dnapsw")]), None, useDefaults=True)
    run_case("b_config5", em5, dna_profiles(em5, 64, 10000 // div, 6), 10000 // div, out)
    composed_route(out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
