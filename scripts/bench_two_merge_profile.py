"""Two-profile sweeps against CTC-merged output profiles next to the plain two-profile sweeps (docs/profile_tapes.md, "Pairs of
profiles against a merged profile"): dnastore4 (110 states, 3 input tokens) on pairs of a random input profile of K = 200 rows and
a random output profile of L = 200 rows over A, C, G, T + blank, 1 and 64 pairs.  The same output rows are read twice: as a plain
profile (column t = output token t, mb_profile_two.hip) and CTC-merged with nCols = 4 (column c = a CSV column of token c,
mb_profile_two_merge.hip); the two score different things, and the comparison is of cost alone.  Per reading: the rolling Forward,
Viterbi with paths, and counts.

    python scripts/bench_two_merge_profile.py [--out profiles/two_merge_profile_bench.json]

Times are wall clock around synchronised calls, after one warm-up call; each figure is the mean of the repetitions stated in the
output.  The output file is rewritten after every shape.  No rate is asked of the sweep."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_merge_profile_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    colTok = np.arange(1, em.nOutTok + 1, dtype=np.int32)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "nCols": len(colTok), "runs": []}
    for size, n, reps in ((200, 1, 3), (200, 64, 3)):
        rng = np.random.RandomState(size + n)
        Bs = [soft(rng, size, em.nOutTok) for _ in range(n)]
        As = [soft(rng, size, em.nInTok) for _ in range(n)]
        run = {"K": size, "L": size, "pairs": n, "reps": reps}
        for name, ct in (("plain", None), ("merged", colTok)):
            dev = capi.DeviceProfileTwos(dm, As, Bs, colTok=ct)
            run[name + "_lattice_bytes_per_pair"] = 8 * dev.cells() // n
            ll, t = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
            run[name + "_forward_rolling_s"] = round(t, 6)
            run[name + "_kernel"] = capi.last_kernel_name()
            run[name + "_finite"] = int(np.isfinite(ll).sum())
            run[name + "_loglike_0"] = float(ll[0])
            v, t = timed(lambda: dev.viterbi(), reps)
            run[name + "_viterbi_paths_s"] = round(t, 6)
            run[name + "_viterbi_chunks"] = capi.last_launch_count()
            run[name + "_path_edges_0"] = int(v[1][1])
            c, t = timed(lambda: dev.counts(), reps)
            run[name + "_counts_s"] = round(t, 6)
            run[name + "_counts_chunks"] = capi.last_launch_count()
            dev.close()
        for what in ("forward_rolling", "viterbi_paths", "counts"):
            run[what + "_merged_over_plain"] = round(run["merged_%s_s" % what] / run["plain_%s_s" % what], 2)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
