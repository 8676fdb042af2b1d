"""Two-tape profile sweeps next to the route that existed before them (docs/profile_tapes.md, "Pairs: an input sequence against a
profile"): dnastore4 (110 states, 3 input tokens) on pairs of a random input sequence of I symbols and a random profile of L rows
over A, C, G, T + blank, 1 and 64 pairs, at I = L = 200 and at I = L = 2 000.  Two timings per shape:

  pairs    DeviceProfilePairs.forward(MB_ROLLING): one launch, the anti-diagonal sweep of mb_profile_pair.hip
  chained  logSeqProb through I chained mb_prefix_extend fills (k_prefix_fill_profile) against mb_prefix_create_profiles on the same
           inputs: I launches of a row-serial fill, every pair of the batch in each

    python scripts/bench_pair_profile.py [--quick] [--chained-large] [--out profiles/pair_profile_bench.json]
    python scripts/bench_pair_profile.py --band [W ...] [--quick] [--out profiles/pair_profile_band_bench.json]

--band (docs/profile_tapes.md, "Pairs under an envelope"): the same shapes under seqpair.Envelope.band of half-width W (default 15
and 63) -- forward(MB_ROLLING) under the band beside the full sweep of the same pairs in the same process, and counts() under the
band; nothing is chained.

Times are wall clock around synchronised calls, after one warm-up call; the repetitions of each are in the output.  --quick: the
small shape only (a rehearsal).  The chained route at I = L = 2 000 is 2 000 launches of 2 001 serial rows each -- minutes per call --
and runs only with --chained-large; without it the run says so.  The output file is rewritten after every shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from machineboss_amd import capi, prefixtree  # noqa: E402
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


def chained(dm, logR, xs, profs):
    """logSeqProb of every pair: the root of each search, then one extend call per input position for the whole batch."""
    n = len(xs)
    px = capi.DevicePrefix(dm, None, logR, 2 * n, profiles=profs)
    try:
        nodes = np.array([px.root(k)[0] for k in range(n)], np.int64)
        sp = np.array([px.root(k)[1] for k in range(n)]) if not len(xs[0]) else None
        seq = np.arange(n, dtype=np.int64)
        for i in range(len(xs[0])):
            nxt, sp, _ = px.extend(seq, nodes, [int(x[i]) for x in xs])
            px.release(nodes)
            nodes = np.asarray(nxt, np.int64)
        return np.asarray(sp, np.float64)
    finally:
        px.close()


def band_runs(args, em, dm, out):
    from machineboss_amd.seqpair import Envelope
    shapes = [(200, 1, 5), (200, 64, 5)] + ([] if args.quick else [(2000, 1, 2), (2000, 64, 2)])
    for size, n, reps in shapes:
        rng = np.random.RandomState(size + n)
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        profs = [np.log(rng.dirichlet([0.3] * (em.nOutTok + 1), size).astype(np.float32).astype(np.float64) + 1e-6) for _ in range(n)]
        dev = capi.DeviceProfilePairs(dm, xs, profs)
        full, tf = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
        for w in args.band:
            env = Envelope.band(size, size, w)
            dev.set_envelopes([env] * n)
            ll, tb = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
            kernel = capi.last_kernel_name()
            (_, _, llc), tc = timed(lambda: dev.counts(), 1)
            run = {"I": size, "L": size, "pairs": n, "band": w, "full_forward_rolling_s": round(tf, 6), "band_forward_rolling_s": round(tb, 6),
                   "full_over_band": round(tf / tb, 2), "band_counts_s": round(tc, 6), "reps": reps, "kernel": kernel,
                   "lattice_doubles": dev.cells(), "finite": int(np.isfinite(ll).sum()), "loglike_0": float(ll[0]), "full_loglike_0": float(full[0]),
                   "counts_loglike_equal": bool(np.array_equal(ll, llc))}
            dev.set_envelopes(None)
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1, sort_keys=True)
                f.write("\n")
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--chained-large", action="store_true")
    ap.add_argument("--band", type=int, nargs="*", metavar="W", help="sweep under bands of these half-widths (default 15 63) beside the full sweep")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.band is not None and not args.band:
        args.band = [15, 63]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pair_profile_band_bench.json" if args.band else "pair_profile_bench.json")
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    logR = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "runs": []}
    if args.band:
        band_runs(args, em, dm, out)
        dm.close()
        return
    shapes = [(200, 1, 5, 2), (200, 64, 5, 2)] + ([] if args.quick else [(2000, 1, 2, 1), (2000, 64, 2, 1)])
    for size, n, repsPairs, repsChained in shapes:
        rng = np.random.RandomState(size + n)
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        profs = [np.log(rng.dirichlet([0.3] * (em.nOutTok + 1), size).astype(np.float32).astype(np.float64) + 1e-6) for _ in range(n)]
        dev = capi.DeviceProfilePairs(dm, xs, profs)
        ll, tp = timed(lambda: dev.forward(capi.MB_ROLLING), repsPairs)
        kernel = capi.last_kernel_name()
        dev.close()
        run = {"I": size, "L": size, "pairs": n, "pairs_forward_rolling_s": round(tp, 6), "pairs_reps": repsPairs, "kernel": kernel,
               "finite": int(np.isfinite(ll).sum()), "loglike_0": float(ll[0])}
        if size > 200 and not args.chained_large:
            run["chained_error"] = "not run: pass --chained-large"
        else:
            try:
                sp, tc = timed(lambda: chained(dm, logR, xs, profs), repsChained)
                run.update(chained_prefix_fills_s=round(tc, 6), chained_reps=repsChained, chained_over_pairs=round(tc / tp, 2),
                           worst_relative_difference=float(np.max(np.abs(sp - ll) / np.maximum(1.0, np.abs(ll)))))
            except capi.MbError as e:          # (the node pool of the chained route is under the memory budget too)
                run["chained_error"] = str(e)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
