"""Two-tape sweeps against CTC-merged profiles next to the plain two-tape sweeps (docs/profile_tapes.md, "Pairs against a merged
profile"): dnastore4 (110 states, 3 input tokens) on pairs of a random input sequence of I = 200 symbols and a random profile of
L = 200 rows over A, C, G, T + blank, 1 and 64 pairs.  The same rows are read twice: as a plain profile (column t = output token t,
mb_profile_pair.hip) and CTC-merged with nCols = 4 (column c = a CSV column of token c, mb_profile_pair_merge.hip); the two score
different things, and the comparison is of cost alone.

    python scripts/bench_pair_merge_profile.py [--out profiles/pair_merge_profile_bench.json]

Times are wall clock around synchronised calls, after one warm-up call; the repetitions of each are in the output."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_merge_profile_bench.json"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("no GPU visible")
    capi.set_device(0)
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, m.getParamDefs(True))
    dm = capi.DeviceMachine(em)
    colTok = np.arange(1, em.nOutTok + 1, dtype=np.int32)
    out = {"machine": "dnastore4", "states": em.nStates, "input_tokens": em.nInTok, "silent_levels": dm.n_levels(), "nCols": len(colTok), "runs": []}
    for size, n, reps in ((200, 1, 5), (200, 64, 5)):
        rng = np.random.RandomState(size + n)
        xs = [rng.randint(1, em.nInTok + 1, size=size).astype(np.int32) for _ in range(n)]
        profs = [np.log(rng.dirichlet([0.3] * (em.nOutTok + 1), size).astype(np.float32).astype(np.float64) + 1e-6) for _ in range(n)]
        run = {"I": size, "L": size, "pairs": n, "reps": reps}
        for name, ct in (("plain", None), ("merged", colTok)):
            dev = capi.DeviceProfilePairs(dm, xs, profs, ct)
            ll, t = timed(lambda: dev.forward(capi.MB_ROLLING), reps)
            run[name + "_forward_rolling_s"] = round(t, 6)
            run[name + "_kernel"] = capi.last_kernel_name()
            run[name + "_finite"] = int(np.isfinite(ll).sum())
            run[name + "_loglike_0"] = float(ll[0])
            dev.close()
        run["merged_over_plain"] = round(run["merged_forward_rolling_s"] / run["plain_forward_rolling_s"], 2)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    dm.close()


if __name__ == "__main__":
    main()
