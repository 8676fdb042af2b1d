"""Row posteriors of pairs against CTC-merged profiles next to the posterior counts of the same pairs (docs/profile_tapes.md, "Row
posteriors of pairs against a merged profile"): dnastore4 (110 states, 3 input tokens) on pairs of a random input sequence of
I = 200 symbols and a random merged profile of L = 200 rows with nCols = 4 (column c = a CSV column of token c) + blank, 1 and 64
pairs -- the shapes of scripts/bench_pair_merge_profile.py.

  merged_row_posteriors  DeviceProfilePairs.merged_row_posteriors(): materialised merged Forward, materialised merged Backward,
                         k_profile_pair_merge_rowpost
  counts                 DeviceProfilePairs.counts() of the same object in the same process: the same two fills, a memset and
                         k_profile_pair_merge_counts

The two calls share the fills, which are serial in the anti-diagonals, and differ in one flat kernel over the same items, so
counts() is the yardstick.  Times are wall clock around synchronised calls after one warm-up call, every repetition kept; the
median, the spread (max - min) and last_device_ms() of each call (its kernels together, between events on the stream).

    python scripts/bench_pair_merge_posteriors.py [--reps N] [--out profiles/pair_merge_posteriors_bench.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_merge_posteriors_bench.json"))
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
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        profs = [np.log(rng.dirichlet([0.3] * (len(colTok) + 1), size).astype(np.float32).astype(np.float64) + 1e-6) for _ in range(n)]
        dev = capi.DeviceProfilePairs(dm, xs, profs, colTok)
        (post, ll), wp, dp = timed(dev.merged_row_posteriors, args.reps)
        kernel, launches = capi.last_kernel_name(), capi.last_launch_count()
        (c, _, llc), wc, dc = timed(dev.counts, args.reps)
        run = {"I": size, "L": size, "pairs": n, "reps": args.reps, "kernel": kernel, "launches": launches, "lattice_doubles": dev.cells(),
               "merged_row_posteriors_s": [round(t, 6) for t in wp], "counts_s": [round(t, 6) for t in wc],
               "merged_row_posteriors_device_ms": [round(t, 3) for t in dp], "counts_device_ms": [round(t, 3) for t in dc],
               "merged_row_posteriors_median_s": round(med(wp), 6), "merged_row_posteriors_spread_s": round(spread(wp), 6),
               "counts_median_s": round(med(wc), 6), "counts_spread_s": round(spread(wc), 6),
               "merged_row_posteriors_over_counts": round(med(wp) / med(wc), 3), "device_merged_row_posteriors_over_counts": round(med(dp) / med(dc), 3),
               "merged_row_posteriors_minus_counts_device_ms": round(med(dp) - med(dc), 3),
               "finite": int(np.isfinite(ll).sum()), "loglike_equal": bool(np.array_equal(ll, llc)),
               "worst_row_sum_error": float(np.abs(post[np.repeat(np.isfinite(ll), size)].sum(axis=1) - 1.0).max(initial=0.0))}
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
