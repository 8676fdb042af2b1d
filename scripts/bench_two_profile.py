"""Two-profile sweeps next to the token sweep they generalise (docs/profile_tapes.md, "Pairs of profiles"): dnastore4 (110 states, 3
input tokens) at K = L = 200, 1 and 64 pairs, random profiles on both tapes.  Two timings per shape, in one process:

  two      DeviceProfileTwos.forward(MB_ROLLING): the anti-diagonal sweep of mb_profile_two.hip, edge loops over all input tokens
  token    DeviceProfilePairs.forward(MB_ROLLING) on a random token input of the same length against the same output profiles

    python scripts/bench_two_profile.py [--out profiles/two_profile_bench.json]
    python scripts/bench_two_profile.py --band [W ...] [--out profiles/two_profile_band_bench.json]

With --band (docs/profile_tapes.md, "Pairs of profiles under an envelope"): K = L = 200 and 2 000, 1 and 64 pairs, under
Envelope.band(K, L, W) for every W (default 15 and 63) -- forward(MB_ROLLING), counts() and row_posteriors() under the band beside
the full sweep of the same pairs where the full one fits.

Times are wall clock around synchronised calls, after one warm-up call; the repetitions of each are in the output.  The output file
is rewritten after every shape.  No rate is asked of the sweep; what to expect is nIn times the edge work of the token sweep and a
ring 1.5 times as large.
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
    fn()                                   # warm-up: code objects, pools
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.synchronize()
    return r, (time.perf_counter() - t) / reps


def soft(rng, rows, nTok):
    return np.log(rng.dirichlet([0.3] * (nTok + 1), rows).astype(np.float32).astype(np.float64) + 1e-6)


FULL_LATTICES_MAX = 16e9      # the full counts() / row_posteriors() are run where both lattices of every pair fit this many bytes


def band_runs(dm, em, widths, out_path):
    """--band: forward(MB_ROLLING), counts() and row_posteriors() under Envelope.band(K, L, W), beside the full sweep of the same
    pairs in the same process where the full one fits: K = L = 200 and 2 000, 1 and 64 pairs."""
    from machineboss_amd.seqpair import Envelope
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "runs": []}
    for size, n, reps in ((200, 1, 3), (200, 64, 3), (2000, 1, 1), (2000, 64, 1)):
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        two = capi.DeviceProfileTwos(dm, As, Bs)
        fullBytes = 2.0 * 8 * two.cells()
        run = {"K": size, "L": size, "pairs": n, "reps": reps, "full_cells": (size + 1) ** 2, "full_lattice_bytes_per_pair": 8 * two.cells() // n}
        lf, run["full_forward_rolling_s"] = timed(lambda: two.forward(capi.MB_ROLLING), reps)
        run["full_forward_rolling_s"] = round(run["full_forward_rolling_s"], 6)
        if fullBytes <= FULL_LATTICES_MAX:
            run["full_counts_s"] = round(timed(lambda: two.counts(), reps)[1], 6)
            run["full_row_posteriors_s"] = round(timed(lambda: two.row_posteriors(), reps)[1], 6)
        run["full_loglike_0"] = float(lf[0])
        run["bands"] = []
        for w in widths:
            env = Envelope.band(size, size, w)
            two.envelopes([env] * n)
            cells = sum(b - a for a, b in zip(env.inStart, env.inEnd))
            b = {"W": w, "cells": cells, "cell_ratio": round(cells / (size + 1) ** 2, 5), "lattice_bytes_per_pair": 8 * two.cells() // n}
            lb, t = timed(lambda: two.forward(capi.MB_ROLLING), reps)
            b["kernel"] = capi.last_kernel_name()
            b["forward_rolling_s"] = round(t, 6)
            b["counts_s"] = round(timed(lambda: two.counts(), reps)[1], 6)
            b["row_posteriors_s"] = round(timed(lambda: two.row_posteriors(), reps)[1], 6)
            b["forward_over_full"] = round(t / run["full_forward_rolling_s"], 5)
            for what in ("counts", "row_posteriors"):
                if "full_%s_s" % what in run:
                    b[what + "_over_full"] = round(b[what + "_s"] / run["full_%s_s" % what], 5)
            b["finite"] = int(np.isfinite(lb).sum()); b["loglike_0"] = float(lb[0])
            run["bands"].append(b)
        two.close()
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--band", type=int, nargs="*", default=None, metavar="W",
                    help="the sweeps under Envelope.band(K, L, W) beside the full ones (default widths: 15 63), into profiles/two_profile_band_bench.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "two_profile_bench.json" if args.band is None else "two_profile_band_bench.json")
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    if args.band is not None:
        band_runs(dm, em, args.band or [15, 63], args.out)
        dm.close()
        return
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "runs": []}
    for size, n, reps in ((200, 1, 5), (200, 64, 5)):
        rng = np.random.RandomState(size + n)
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        two = capi.DeviceProfileTwos(dm, As, Bs)
        tok = capi.DeviceProfilePairs(dm, xs, Bs)
        l2, t2 = timed(lambda: two.forward(capi.MB_ROLLING), reps)
        kernel = capi.last_kernel_name()
        l1, t1 = timed(lambda: tok.forward(capi.MB_ROLLING), reps)
        two.close(); tok.close()
        run = {"K": size, "L": size, "pairs": n, "reps": reps, "two_forward_rolling_s": round(t2, 6), "token_forward_rolling_s": round(t1, 6),
               "two_over_token": round(t2 / t1, 2), "kernel": kernel, "ring_bytes_two": 72 * (size + 1) * em.nStates,
               "ring_bytes_token": 48 * (size + 1) * em.nStates, "finite": int(np.isfinite(l2).sum()), "loglike_0": float(l2[0]),
               "token_loglike_0": float(l1[0])}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
