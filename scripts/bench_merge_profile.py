"""Merged (CTC) profile sweeps next to the plain ones (docs/profile_tapes.md, "Merged (CTC) profiles"): workload (a) of
scripts/bench_profile.py -- a 2 kb DNA generator (2 001 states) against 64 profiles x 8 000 rows over A, C, G, T + blank -- through
the plain sweeps (mb_profile.hip) and the merged sweeps (mb_profile_merge.hip, nCols = 4) in one session: rolling Forward, Viterbi
with paths, counts, and the merged / plain time ratio of each.

    python scripts/bench_merge_profile.py [--quick] [--out profiles/merge_profile_bench.json]

Times are wall clock around synchronised calls, after one warm-up call.  --quick: 1/8 of the rows (a rehearsal).
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
from machineboss_amd.profile import Profile  # noqa: E402


def timed(fn, reps):
    fn()                                   # warm-up: code objects, pools
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.synchronize()
    return r, (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_profile_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    rows, n = (1000 if args.quick else 8000), 64
    rng = np.random.RandomState(2)
    em = EvaluatedMachine.fromMachine(A.generator(list(rng.choice(list("ACGT"), 2000)), "g"), {}, useDefaults=True)
    rng = np.random.RandomState(5)
    profs = [Profile(["A", "C", "G", "T"], rng.dirichlet([0.3] * 5, rows).astype(np.float32).astype(np.float64).tolist()) for _ in range(n)]
    dm = capi.DeviceMachine(em)
    plain = capi.DeviceProfiles(dm, [p.logRows(em) for p in profs])
    merged_rows = [p.mergeRows(em) for p in profs]
    merged = capi.DeviceProfiles(dm, [P for P, _ in merged_rows], merged_rows[0][1])
    out = {"states": em.nStates, "silent_levels": dm.n_levels(), "profiles": n, "rows": rows, "nCols": int(len(merged_rows[0][1])),
           "cells_plain": float(n * (rows + 1)) * em.nStates}
    for name, dev in (("plain", plain), ("merged", merged)):
        ll, tf = timed(lambda: dev.forward(capi.MB_ROLLING), 3)
        kf = capi.last_kernel_name()
        _, tv = timed(lambda: dev.viterbi(), 2)
        _, tc = timed(lambda: dev.counts(), 2)
        out[name] = {"forward_rolling_s": round(tf, 5), "viterbi_paths_s": round(tv, 5), "counts_s": round(tc, 5), "forward_kernel": kf,
                     "loglike_0": float(ll[0]), "finite": int(np.isfinite(ll).sum())}
        print(name, json.dumps(out[name]), flush=True)
    out["merged_over_plain"] = {k: round(out["merged"][k] / out["plain"][k], 3) for k in ("forward_rolling_s", "viterbi_paths_s", "counts_s")}
    print("merged / plain", json.dumps(out["merged_over_plain"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
