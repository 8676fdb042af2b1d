"""Two-profile sweeps against CTC-merged output profiles under a band next to the full merged sweeps (docs/profile_tapes.md, "Pairs
of profiles against a merged profile under an envelope"): dnastore4 (110 states, 3 input tokens) on pairs of a random input
profile of K rows and a random merged output profile of L rows, nCols = 4 (column c = a CSV column of token c), 1 and 64 pairs.
At K = L = 200 the full merged rolling Forward (mb_profile_two_merge.hip over the rectangle) runs beside the one under
seqpair.Envelope.band of half-width W (default 15 and 63) on the same pairs in the same process, and counts() and
merged_row_posteriors() run under the band; at K = L = 2 000 the banded calls run alone (a full merged lattice there is 53 GB a
pair).  The compact lattice bytes are reported.

    python scripts/bench_two_merge_band.py [W ...] [--quick] [--out profiles/two_merge_band_bench.json]

Times are wall clock around synchronised calls, after one warm-up call; the repetitions of each are in the output.  --quick: the
small shape only (a rehearsal).  The output file is rewritten after every run.  No rate is asked of the sweeps."""
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
    fn()                                   # warm-up: code objects, pools
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.synchronize()
    return r, (time.perf_counter() - t) / reps


def soft(rng, rows, nTok):
    return np.log(rng.dirichlet([0.3] * (nTok + 1), rows).astype(np.float32).astype(np.float64) + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("band", type=int, nargs="*", metavar="W", help="half-widths of the bands (default 15 63)")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_merge_band_bench.json"))
    args = ap.parse_args()
    bands = args.band or [15, 63]
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    colTok = np.arange(1, em.nOutTok + 1, dtype=np.int32)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "nCols": len(colTok), "runs": []}
    shapes = [(200, 1, 5, True), (200, 64, 5, True)] + ([] if args.quick else [(2000, 1, 2, False), (2000, 64, 2, False)])
    for size, n, reps, withFull in shapes:
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        dev = capi.DeviceProfileTwos(dm, As, Bs, colTok=colTok)
        full, tf, fullKernel, fullBytes = None, None, None, 8 * dev.cells() // n
        if withFull:
            full, tf = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
            fullKernel = capi.last_kernel_name()
        for w in bands:
            dev.merged_envelopes([Envelope.band(size, size, w)] * n)
            ll, tb = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
            kernel = capi.last_kernel_name()
            (_, _, llc), tc = timed(lambda: dev.counts(), 1)
            countChunks = capi.last_launch_count()
            (pa, pb, llp), tp = timed(lambda: dev.merged_row_posteriors(), 1)
            run = {"K": size, "L": size, "pairs": n, "band": w, "band_forward_rolling_s": round(tb, 6), "band_counts_s": round(tc, 6),
                   "band_row_posteriors_s": round(tp, 6), "reps": reps, "counts_reps": 1, "row_posteriors_reps": 1, "kernel": kernel,
                   "counts_chunks": countChunks, "posteriors_chunks": capi.last_launch_count(), "lattice_doubles": dev.cells(),
                   "lattice_bytes_per_pair": 8 * dev.cells() // n, "full_lattice_bytes_per_pair": fullBytes,
                   "finite": int(np.isfinite(ll).sum()), "loglike_0": float(ll[0]),
                   "counts_loglike_equal": bool(np.array_equal(ll, llc)), "posteriors_loglike_equal": bool(np.array_equal(ll, llp)),
                   "worst_row_sum_error": float(max(np.abs(pa.sum(axis=1) - 1.0).max(), np.abs(pb.sum(axis=1) - 1.0).max()))}
            if withFull:
                run.update(full_forward_rolling_s=round(tf, 6), full_over_band=round(tf / tb, 2), full_kernel=fullKernel, full_loglike_0=float(full[0]))
            dev.merged_envelopes(None)
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1, sort_keys=True)
                f.write("\n")
        dev.close()
    dm.close()


if __name__ == "__main__":
    main()
