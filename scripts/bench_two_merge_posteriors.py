"""Row posteriors of pairs of profiles against CTC-merged output profiles next to the posterior counts of the same pairs
(docs/profile_tapes.md, "Row posteriors of pairs of profiles against a merged profile"): dnastore4 (110 states, 3 input tokens) on
pairs of a random input profile of K = 200 rows and a random merged output profile of L = 200 rows with nCols = 4 (column c = a CSV
column of token c) + blank, 1 and 64 pairs -- the shapes of scripts/bench_two_merge_profile.py.

  merged_row_posteriors  DeviceProfileTwos.merged_row_posteriors(): materialised merged Forward, materialised merged Backward,
                         k_profile_two_merge_rowpost once per table
  counts                 DeviceProfileTwos.counts() of the same object in the same process: the same two fills, a memset and
                         k_profile_two_merge_counts

The two calls share the fills, which are serial in the anti-diagonals, and differ in the flat kernels over the same items, so
counts() is the yardstick.  Times are wall clock around synchronised calls after one warm-up call, every repetition kept; the
median, the spread (max - min) and last_device_ms() of each call (its kernels together, between events on the stream).

    python scripts/bench_two_merge_posteriors.py [--reps N] [--out profiles/two_merge_posteriors_bench.json]

The output file is rewritten after every shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from machineboss_amd import capi  # noqa: E402
from machineboss_amd.evalmachine import EvaluatedMachine  # noqa: E402
from machineboss_amd.machine import Machine  # noqa: E402


def timed(fn, reps):
    """(last result, wall seconds of every repetition, device milliseconds of every repetition), after one warm-up call."""
    fn()
    capi.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        capi.synchronize()
        wall.append(time.perf_counter() - t)
        dev.append(capi.last_device_ms())
    return r, wall, dev


def soft(rng, rows, nTok):
    return np.log(rng.dirichlet([0.3] * (nTok + 1), rows).astype(np.float32).astype(np.float64) + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_merge_posteriors_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    colTok = np.arange(1, em.nOutTok + 1, dtype=np.int32)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "output_tokens": em.nOutTok, "silent_levels": dm.n_levels(),
           "nCols": len(colTok), "runs": []}
    med = lambda v: float(np.median(v))
    spread = lambda v: float(np.max(v) - np.min(v))
    for size, n in ((200, 1), (200, 64)):
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, len(colTok)) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        dev = capi.DeviceProfileTwos(dm, As, Bs, colTok=colTok)
        (postA, postB, ll), wp, dp = timed(dev.merged_row_posteriors, args.reps)
        kernel, launches = capi.last_kernel_name(), capi.last_launch_count()
        (_, _, llb), wb, db = timed(lambda: dev.merged_row_posteriors(inputs=False), args.reps)
        (c, _, llc), wc, dc = timed(dev.counts, args.reps)
        live = np.repeat(np.isfinite(ll), size)
        run = {"K": size, "L": size, "pairs": n, "reps": args.reps, "kernel": kernel, "launches": launches, "lattice_doubles": dev.cells(),
               "merged_row_posteriors_s": [round(t, 6) for t in wp], "counts_s": [round(t, 6) for t in wc],
               "merged_row_posteriors_outputs_only_s": [round(t, 6) for t in wb],
               "merged_row_posteriors_device_ms": [round(t, 3) for t in dp], "counts_device_ms": [round(t, 3) for t in dc],
               "merged_row_posteriors_outputs_only_device_ms": [round(t, 3) for t in db],
               "merged_row_posteriors_median_s": round(med(wp), 6), "merged_row_posteriors_spread_s": round(spread(wp), 6),
               "counts_median_s": round(med(wc), 6), "counts_spread_s": round(spread(wc), 6),
               "merged_row_posteriors_over_counts": round(med(wp) / med(wc), 3), "device_merged_row_posteriors_over_counts": round(med(dp) / med(dc), 3),
               "merged_row_posteriors_minus_counts_device_ms": round(med(dp) - med(dc), 3),
               "input_table_device_ms": round(med(dp) - med(db), 3),
               "finite": int(np.isfinite(ll).sum()), "loglike_equal": bool(np.array_equal(ll, llc) and np.array_equal(ll, llb)),
               "worst_row_sum_error": float(max(np.abs(postA[live].sum(axis=1) - 1.0).max(initial=0.0), np.abs(postB[live].sum(axis=1) - 1.0).max(initial=0.0)))}
        dev.close()
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
