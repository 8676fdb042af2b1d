"""Row posteriors of pairs of profiles next to the posterior counts of the same pairs (docs/profile_tapes.md, "Row posteriors of
pairs of profiles"): dnastore4 (110 states, 3 input tokens) at K = L = 200 with 1 and 64 pairs, random profiles on both tapes --
the shapes of scripts/bench_two_profile.py.

  row_posteriors  DeviceProfileTwos.row_posteriors(): materialised Forward, materialised Backward, k_profile_two_rowpost per axis
  counts          DeviceProfileTwos.counts() of the same object in the same process: the same two fills, k_profile_two_counts

The two calls share the fills, so the difference is what the two binning kernels cost beside the counts kernel.  Times are wall
clock around synchronised calls after one warm-up call, every repetition kept (the table in the doc has their median and spread),
and last_device_ms() of each call (its kernels together, between events on the stream).  No ratio is asked.

    python scripts/bench_two_posteriors.py [--reps N] [--out profiles/two_posteriors_bench.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_posteriors_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "output_tokens": em.nOutTok, "silent_levels": dm.n_levels(), "runs": []}
    for size, n in ((200, 1), (200, 64)):
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        dev = capi.DeviceProfileTwos(dm, As, Bs)
        (postA, postB, ll), wp, dp = timed(dev.row_posteriors, args.reps)
        kernel, launches = capi.last_kernel_name(), capi.last_launch_count()
        (c, _, llc), wc, dc = timed(dev.counts, args.reps)
        byIn = np.zeros(em.nInTok + 1); byOut = np.zeros(em.nOutTok + 1)
        np.add.at(byIn, np.asarray(em.inTok, np.int64), c); np.add.at(byOut, np.asarray(em.outTok, np.int64), c)
        med = lambda v: float(np.median(v))
        live = np.repeat(np.isfinite(ll), size)
        rel = lambda got, want: float(np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
        run = {"K": size, "L": size, "pairs": n, "reps": args.reps, "kernel": kernel, "launches": launches,
               "lattice_doubles": 3 * em.nStates * (size + 1) * (size + 1) * n,
               "row_posteriors_s": [round(t, 6) for t in wp], "counts_s": [round(t, 6) for t in wc],
               "row_posteriors_device_ms": [round(t, 3) for t in dp], "counts_device_ms": [round(t, 3) for t in dc],
               "row_posteriors_median_s": round(med(wp), 6), "row_posteriors_spread_s": round(max(wp) - min(wp), 6),
               "counts_median_s": round(med(wc), 6), "counts_spread_s": round(max(wc) - min(wc), 6),
               "row_posteriors_minus_counts_device_ms": round(med(dp) - med(dc), 3),
               "finite": int(np.isfinite(ll).sum()), "loglike_equal": bool(np.array_equal(ll, llc)),
               "worst_row_sum_error": float(max(np.abs(postA[live].sum(axis=1) - 1.0).max(initial=0.0), np.abs(postB[live].sum(axis=1) - 1.0).max(initial=0.0))),
               "worst_grouped_counts_relative": max(rel(postA.sum(axis=0)[1:], byIn[1:]), rel(postB.sum(axis=0)[1:], byOut[1:]))}
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
