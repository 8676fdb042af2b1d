"""Row posteriors next to the posterior counts of the same pairs (docs/profile_tapes.md, "Row posteriors"): dnastore4 (110 states,
3 input tokens) on pairs of a random input sequence of I symbols and a random profile of L rows over A, C, G, T + blank -- the
shapes of scripts/bench_pair_profile.py: I = L = 200 with 1 and 64 pairs on the full lattice, I = L = 2 000 with 1 and 64 pairs
under seqpair.Envelope.band(15).

  row_posteriors  DeviceProfilePairs.row_posteriors(): materialised Forward, materialised Backward, k_profile_pair_rowpost
  counts          DeviceProfilePairs.counts() of the same object in the same process: the same two fills, k_profile_pair_counts

The two calls share the fills and differ in one kernel over the same items, so counts() is the yardstick.  Times are wall clock
around synchronised calls after one warm-up call, every repetition kept, and last_device_ms() of each call (the three kernels of
a call together, between events on the stream).

    python scripts/bench_pair_posteriors.py [--quick] [--reps N] [--out profiles/pair_posteriors_bench.json]

--quick: the small shapes only (a rehearsal).  The output file is rewritten after every shape.
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
from machineboss_amd.seqpair import Envelope  # noqa: E402


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
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_posteriors_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "output_tokens": em.nOutTok, "silent_levels": dm.n_levels(), "runs": []}
    shapes = [(200, 1, None), (200, 64, None)] + ([] if args.quick else [(2000, 1, 15), (2000, 64, 15)])
    for size, n, band in shapes:
        rng = np.random.RandomState(size + n)
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        profs = [np.log(rng.dirichlet([0.3] * (em.nOutTok + 1), size).astype(np.float32).astype(np.float64) + 1e-6) for _ in range(n)]
        dev = capi.DeviceProfilePairs(dm, xs, profs)
        if band is not None:
            dev.set_envelopes([Envelope.band(size, size, band)] * n)
        (post, ll), wp, dp = timed(dev.row_posteriors, args.reps)
        kernel, launches = capi.last_kernel_name(), capi.last_launch_count()
        (c, _, llc), wc, dc = timed(dev.counts, args.reps)
        grouped = np.zeros(em.nOutTok + 1)
        np.add.at(grouped, np.asarray(em.outTok, np.int64), c)
        med = lambda v: float(np.median(v))
        run = {"I": size, "L": size, "pairs": n, "band": band, "reps": args.reps, "kernel": kernel, "launches": launches, "lattice_doubles": dev.cells(),
               "row_posteriors_s": [round(t, 6) for t in wp], "counts_s": [round(t, 6) for t in wc],
               "row_posteriors_device_ms": [round(t, 3) for t in dp], "counts_device_ms": [round(t, 3) for t in dc],
               "row_posteriors_over_counts": round(med(wp) / med(wc), 3), "device_row_posteriors_over_counts": round(med(dp) / med(dc), 3),
               "row_posteriors_minus_counts_device_ms": round(med(dp) - med(dc), 3),
               "finite": int(np.isfinite(ll).sum()), "loglike_equal": bool(np.array_equal(ll, llc)),
               "worst_row_sum_error": float(np.abs(post[np.repeat(np.isfinite(ll), size)].sum(axis=1) - 1.0).max(initial=0.0)),
               "worst_grouped_counts_relative": float(np.max(np.abs(post.sum(axis=0)[1:] - grouped[1:]) / np.maximum(grouped[1:], 1e-300)))}
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
