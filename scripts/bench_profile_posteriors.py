"""Row posteriors of one-tape profiles next to the posterior counts of the same profiles (docs/profile_tapes.md, "Row posteriors of
one-tape profiles"): workload (a) of scripts/bench_profile.py and scripts/bench_merge_profile.py -- a 2 kb DNA generator (2 001
states) against 64 profiles x 8 000 rows over A, C, G, T + blank -- plain and CTC-merged.

  row_posteriors  DeviceProfiles.row_posteriors(): materialised Forward, materialised Backward, k_profile_rowpost over all rows
  counts          DeviceProfiles.counts() of the same object in the same process: materialised Forward, rolling Backward with counts

counts() is code the row posteriors do not touch, so it is the yardstick; the posteriors run one more materialised sweep (the
Backward writes its lattice) and the flat kernel.  Times are wall clock around synchronised calls after one warm-up call, every
repetition kept, and last_device_ms() of each call (its kernels together, between events on the stream).  The split recorded is the
materialised Forward, which both calls begin with and forward(MB_MATERIALISE) times alone, and the rest of either call: the
materialised Backward plus the flat kernel, against the rolling Backward that counts.

    python scripts/bench_profile_posteriors.py [--quick] [--reps N] [--out profiles/profile_posteriors_bench.json]

--quick: 1 000 rows a profile (a rehearsal).  The output file is rewritten after every kind.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from machineboss_amd import algebra as A  # noqa: E402
from machineboss_amd import capi  # noqa: E402
from machineboss_amd.evalmachine import EvaluatedMachine  # noqa: E402
from machineboss_amd.profile import Profile  # noqa: E402


def timed(fn, reps):
    """(last result, wall seconds of every repetition, device milliseconds of every repetition, launches), after one warm-up call."""
    fn()
    capi.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        capi.synchronize()
        wall.append(time.perf_counter() - t)
        dev.append(capi.last_device_ms())
    return r, wall, dev, capi.last_launch_count()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_posteriors_bench.json"))
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
    merged_rows = [p.mergeRows(em) for p in profs]
    colTok = merged_rows[0][1]
    out = {"states": em.nStates, "silent_levels": dm.n_levels(), "profiles": n, "rows": rows, "nCols": int(len(colTok)), "reps": args.reps,
           "memory_budget_bytes": int(capi.memory_budget()), "runs": {}}
    med = lambda v: float(np.median(v))
    for name, dev in (("plain", lambda: capi.DeviceProfiles(dm, [p.logRows(em) for p in profs])),
                      ("merged", lambda: capi.DeviceProfiles(dm, [P for P, _ in merged_rows], colTok))):
        dev = dev()
        (post, ll), wp, dp, lp = timed(dev.row_posteriors, args.reps)
        kernel = capi.last_kernel_name()
        (c, _, llc), wc, dc, lc = timed(dev.counts, args.reps)
        _, wf, df, _ = timed(lambda: dev.forward(capi.MB_MATERIALISE), args.reps)
        grouped = np.zeros(em.nOutTok + 1)
        np.add.at(grouped, np.asarray(em.outTok, np.int64), c)
        planes = len(colTok) + 1 if name == "merged" else 1
        run = {"kernel": kernel, "lattice_bytes_each": 8 * n * (rows + 1) * 2 * planes * em.nStates,
               "row_posteriors_launches": lp, "counts_launches": lc, "chunked": bool(lp > 1),
               "row_posteriors_s": [round(t, 6) for t in wp], "counts_s": [round(t, 6) for t in wc], "forward_materialised_s": [round(t, 6) for t in wf],
               "row_posteriors_device_ms": [round(t, 3) for t in dp], "counts_device_ms": [round(t, 3) for t in dc],
               "forward_materialised_device_ms": [round(t, 3) for t in df],
               "row_posteriors_over_counts": round(med(wp) / med(wc), 3), "device_row_posteriors_over_counts": round(med(dp) / med(dc), 3),
               "backward_and_rowpost_device_ms": round(med(dp) - med(df), 3), "counts_backward_device_ms": round(med(dc) - med(df), 3),
               "spread_row_posteriors_s": round(max(wp) - min(wp), 6), "spread_counts_s": round(max(wc) - min(wc), 6),
               "finite": int(np.isfinite(ll).sum()), "loglike_equal": bool(np.array_equal(ll, llc)),
               "worst_row_sum_error": float(np.abs(post[np.repeat(np.isfinite(ll), rows)].sum(axis=1) - 1.0).max(initial=0.0))}
        if name == "plain":
            run["worst_grouped_counts_relative"] = float(np.max(np.abs(post.sum(axis=0)[1:] - grouped[1:]) / np.maximum(grouped[1:], 1e-300)))
        dev.close()
        out["runs"][name] = run
        print(name, json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
