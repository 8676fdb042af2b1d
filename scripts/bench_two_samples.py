"""Posterior path samples of pairs of profiles next to the Viterbi call with paths (docs/profile_tapes.md, "Posterior path samples of
pairs of profiles"): dnastore4 (110 states, 3 input tokens) on pairs of a random input profile of K rows and a random output profile
of L rows -- the profiles of scripts/bench_two_posteriors.py -- under seqpair.Envelope.band(15), 1 and 64 pairs at K = L = 200 and at
K = L = 2 000, with 1, 64 and 1 024 samples per pair.  Per shape, on one object in one process:

  viterbi   DeviceProfileTwos.viterbi(paths=True): the materialised max sweep, one traceback lane per pair, the paths copied out
  sample    DeviceProfileTwos.sample_paths(nSamples): the materialised sum sweep, one lane per (pair, sample), the paths copied out
  forward   DeviceProfileTwos.forward(MB_MATERIALISE): the fill the sample call starts with, alone

    python scripts/bench_two_samples.py [--quick] [--out profiles/two_samples_bench.json]

Wall times are around synchronised calls after one warm-up call each; the repetitions are in the output.  Device times are the
library's own (events around the launches of a call, mb_last_device_ms): sample_launch_device_ms is the sample call's minus the
materialised Forward call's, both on the same object -- the sample launch alone, by difference.  --quick: the small shape only.  The
output file is rewritten after every run.
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

BAND = 15
SAMPLES = (1, 64, 1024)


def soft(rng, rows, nTok):
    return np.log(rng.dirichlet([0.3] * (nTok + 1), rows).astype(np.float32).astype(np.float64) + 1e-6)


def timed(fn, reps):
    """(result, wall seconds per call, device ms of the last call) after one warm-up call."""
    fn()
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    capi.synchronize()
    return r, (time.perf_counter() - t) / reps, capi.last_device_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_samples_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "output_tokens": em.nOutTok, "silent_levels": dm.n_levels(), "band": BAND,
           "runs": []}
    shapes = [(200, 1, 5), (200, 64, 5)] + ([] if args.quick else [(2000, 1, 2), (2000, 64, 1)])
    for size, n, reps in shapes:
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        dev = capi.DeviceProfileTwos(dm, As, Bs, envs=[Envelope.band(size, size, BAND)] * n)
        (v, voff, _, _, _), tv, dv = timed(lambda: dev.viterbi(), reps)
        ll, tf, df = timed(lambda: dev.forward(capi.MB_MATERIALISE), reps)
        for ns in SAMPLES:
            run = {"K": size, "L": size, "pairs": n, "nSamples": ns, "reps": reps, "viterbi_paths_s": round(tv, 6), "viterbi_device_ms": round(dv, 3),
                   "forward_materialised_s": round(tf, 6), "forward_device_ms": round(df, 3), "path_cap": dev.path_cap(),
                   "lattice_doubles": dev.cells(), "viterbi_path_length_0": int(voff[1] - voff[0])}
            try:
                (sl, off, edges, _, _, logq), ts, ds = timed(lambda: dev.sample_paths(ns, seed=size + n), reps)
                run.update(sample_paths_s=round(ts, 6), sample_device_ms=round(ds, 3), sample_launch_device_ms=round(ds - df, 3),
                           sample_launch_over_forward=round((ds - df) / df, 4), sample_over_viterbi=round(ts / tv, 2), kernel=capi.last_kernel_name(),
                           launches=capi.last_launch_count(), finite=int(np.isfinite(sl).sum()), loglike_equals_forward=bool(np.array_equal(sl, ll)),
                           mean_path_length=float(np.diff(off).mean()), mean_logq=float(logq[np.isfinite(logq)].mean()),
                           best_logq=float(logq.max()), distinct_paths_of_pair_0=len({edges[off[j]:off[j + 1]].tobytes() for j in range(ns)}))
            except (capi.MbError, MemoryError) as e:
                run["sample_error"] = str(e) or type(e).__name__
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
