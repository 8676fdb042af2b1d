"""Rates of the prefix-search node fill (mb_prefix.hip) and of whole --prefix-decode searches, beside the numpy restatement.

    python scripts/bench_decode.py [--out profiles/decode_bench.json] [--lengths 200,2000] [--batches 1,64] [--no-numpy]

Machine: tests/golden/machine/dnastore4.json (110 states).  Outputs of length L are Viterbi encodings of random inputs, so every
one of them decodes.  Per (L, batch): one `extend` of batch x nIn children of the roots (the fill rate: node fills per second and
G cells/s with 2 (L+1) S cells per node; device time from the library's events and wall time of the call), the same fills by
PrefixDP in numpy on this host (one search's worth, scaled), and a whole lock-step decode (wall time, nodes created).

The share of a fill spent in the V product: build a second library with the product left out and run the fill part against it,

    MB_BUILD_EXTRA_FLAGS=-DMB_PREFIX_SKIP_PRODUCT python -m machineboss_amd.build --force   (then keep that libmbhip.so under another name)
    MBHIP_LIBRARY=that.so python scripts/bench_decode.py --no-numpy --no-search

and compare device_ms; its cells are meaningless, only its time is read.

    python scripts/bench_decode.py --profile [--out profiles/decode_profile_bench.json]

fills the roots' children against PROFILES instead (k_prefix_fill_profile): soft versions of the same outputs, 0.86 on the encoded
symbol, 0.04 on the others and 0.02 on the blank, each jittered by up to a tenth.  Beside it the same launches through the token
kernel on the arg-max string of each profile, for a cost per row side by side.

    python scripts/bench_decode.py --merged [--out profiles/decode_merge_bench.json]

fills the roots' children against the same rows read as CTC-MERGED profiles (k_prefix_fill_merged, nCols = 4: one column per output
symbol) beside the plain profile fill on the same rows.  The figure is merged / plain at the same shape, from one session."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from machineboss_amd import boss, capi, prefixtree  # noqa: E402
from machineboss_amd.evalmachine import EvaluatedMachine  # noqa: E402
from machineboss_amd.machine import Machine  # noqa: E402


def outputs(m, n, L, seed=1):
    rng = np.random.RandomState(seed)
    syms = m.inputAlphabet()
    outs = []
    while len(outs) < n:
        ins = [[syms[k] for k in rng.randint(0, len(syms), L)] for _ in range(n)]
        outs += [o[:L] for o in boss.viterbiEncode(m, ins, "numpy") if len(o) >= L]
    return outs[:n]


def soften(em, toks, seed=2):
    rng = np.random.RandomState(seed)
    profs = []
    for y in toks:
        W = np.full((len(y), em.nOutTok + 1), 0.04)
        W[:, 0] = 0.02
        W[np.arange(len(y)), np.asarray(y, np.int64)] = 0.86
        profs.append(np.log(W * rng.uniform(0.9, 1.1, W.shape)))
    return profs


def time_children(dev, B, nIn):
    """Best of three launches that fill the nIn children of every search's root: (device ms, wall ms)."""
    roots = [dev.root(k)[0] for k in range(B)]
    seq = [k for k in range(B) for _ in range(nIn)]
    par = [roots[k] for k in range(B) for _ in range(nIn)]
    tok = [t for _ in range(B) for t in range(1, nIn + 1)]
    ch, _, _ = dev.extend(seq, par, tok)                  # warm-up
    dev.release(ch)
    best_ms, best_wall = 1e30, 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        ch, _, _ = dev.extend(seq, par, tok)
        best_wall = min(best_wall, (time.perf_counter() - t0) * 1e3)
        best_ms = min(best_ms, capi.last_device_ms())
        dev.release(ch)
    return best_ms, best_wall


def profile_rows(args, m, em, dm, R):
    S, nIn = em.nStates, em.nInTok
    rows = []
    for L in [int(x) for x in args.lengths.split(",")]:
        for B in [int(x) for x in args.batches.split(",")]:
            toks = [em.outputTokenizer.tokenize(o) for o in outputs(m, B, L)]
            profs = soften(em, toks)
            hard = [np.argmax(p[:, 1:], axis=1) + 1 for p in profs]
            dev = capi.DevicePrefix(dm, None, R, B * (1 + 3 * nIn), profs)
            p_ms, p_wall = time_children(dev, B, nIn)
            dev.close()
            dev = capi.DevicePrefix(dm, hard, R, B * (1 + 3 * nIn))
            t_ms, t_wall = time_children(dev, B, nIn)
            dev.close()
            fills = B * nIn
            row = {"L": L, "searches": B, "fills_per_launch": fills, "profile_device_ms": round(p_ms, 3), "profile_wall_ms": round(p_wall, 3),
                   "profile_us_per_row": round(p_ms * 1e3 / (L + 1), 2), "profile_fills_per_s": round(fills / (p_ms * 1e-3), 1),
                   "token_device_ms": round(t_ms, 3), "token_us_per_row": round(t_ms * 1e3 / (L + 1), 2),
                   "profile_vs_token": round(p_ms / t_ms, 2)}
            if not args.no_numpy:
                dp = prefixtree.ProfilePrefixDP(em, R)
                root = dp.fill(profs[0])[0]
                t0 = time.perf_counter()
                for t in range(1, nIn + 1):
                    dp.fill(profs[0], root, t)
                row["numpy_ms_per_fill"] = round((time.perf_counter() - t0) * 1e3 / nIn, 2)
                row["speedup_vs_numpy"] = round(row["numpy_ms_per_fill"] * fills / p_ms, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def merged_rows(args, m, em, dm, R):
    nIn = em.nInTok
    colTok = list(range(1, em.nOutTok + 1))
    rows = []
    for L in [int(x) for x in args.lengths.split(",")]:
        for B in [int(x) for x in args.batches.split(",")]:
            profs = soften(em, [em.outputTokenizer.tokenize(o) for o in outputs(m, B, L)])
            dev = capi.DevicePrefix(dm, None, R, B * (1 + 3 * nIn), profs, colTok)
            g_ms, g_wall = time_children(dev, B, nIn)
            dev.close()
            dev = capi.DevicePrefix(dm, None, R, B * (1 + 3 * nIn), profs)
            p_ms, p_wall = time_children(dev, B, nIn)
            dev.close()
            fills = B * nIn
            row = {"L": L, "searches": B, "nCols": len(colTok), "fills_per_launch": fills, "merged_device_ms": round(g_ms, 3),
                   "merged_wall_ms": round(g_wall, 3), "merged_us_per_row": round(g_ms * 1e3 / (L + 1), 2),
                   "merged_fills_per_s": round(fills / (g_ms * 1e-3), 1), "plain_device_ms": round(p_ms, 3),
                   "plain_us_per_row": round(p_ms * 1e3 / (L + 1), 2), "merged_vs_plain": round(g_ms / p_ms, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true", help="fills against profiles (k_prefix_fill_profile) beside the token kernel")
    ap.add_argument("--merged", action="store_true", help="fills against CTC-merged profiles (k_prefix_fill_merged) beside the plain profile fill")
    ap.add_argument("--out")
    ap.add_argument("--lengths", default="200,2000")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-search", action="store_true")
    args = ap.parse_args()
    m = Machine.fromFile(os.path.join(ROOT, "tests", "golden", "machine", "dnastore4.json"))
    em = EvaluatedMachine.fromMachine(m, None, useDefaults=True)
    S, nIn = em.nStates, em.nInTok
    R = prefixtree.logSumInTrans(em)
    dm = capi.DeviceMachine(em)
    rows = []
    if args.profile:
        rows = profile_rows(args, m, em, dm, R)
    elif args.merged:
        rows = merged_rows(args, m, em, dm, R)
    for L in [] if args.profile or args.merged else [int(x) for x in args.lengths.split(",")]:
        for B in [int(x) for x in args.batches.split(",")]:
            outs = outputs(m, B, L)
            toks = [em.outputTokenizer.tokenize(o) for o in outs]
            dev = capi.DevicePrefix(dm, toks, R, B * (1 + 3 * nIn))
            roots = [dev.root(k)[0] for k in range(B)]
            seq = [k for k in range(B) for _ in range(nIn)]
            par = [roots[k] for k in range(B) for _ in range(nIn)]
            tok = [t for _ in range(B) for t in range(1, nIn + 1)]
            ch, _, _ = dev.extend(seq, par, tok)                  # warm-up
            dev.release(ch)
            best_ms, best_wall = 1e30, 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                ch, _, _ = dev.extend(seq, par, tok)
                best_wall = min(best_wall, (time.perf_counter() - t0) * 1e3)
                best_ms = min(best_ms, capi.last_device_ms())
                dev.release(ch)
            dev.close()
            fills = B * nIn
            cells = fills * 2 * (L + 1) * S
            row = {"L": L, "searches": B, "fills_per_launch": fills, "device_ms": round(best_ms, 3), "wall_ms": round(best_wall, 3),
                   "fills_per_s": round(fills / (best_ms * 1e-3), 1), "gcells_per_s": round(cells / (best_ms * 1e-3) / 1e9, 4)}
            if not args.no_numpy:
                dp = prefixtree.PrefixDP(em, R)
                root = dp.fill(toks[0])[0]
                t0 = time.perf_counter()
                for t in range(1, nIn + 1):
                    dp.fill(toks[0], root, t)
                row["numpy_ms_per_fill"] = round((time.perf_counter() - t0) * 1e3 / nIn, 2)
                row["speedup_vs_numpy"] = round(row["numpy_ms_per_fill"] * fills / best_ms, 1)
            slot_bytes = 16.0 * (L + 1) * S
            if not args.no_search and B * (8 * L + 64) * slot_bytes > 100e9:
                row["decode_skipped"] = "the node pool of %d searches would not fit" % B
            elif not args.no_search:
                t0 = time.perf_counter()
                seqs, trees = prefixtree.decodeBatch(em, outs, backend="device", maxNodes=B * (8 * L + 64))
                row["decode_wall_s"] = round(time.perf_counter() - t0, 3)
                row["decode_nodes"] = int(sum(t.nFills for t in trees))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"machine": "dnastore4", "states": S, "input_tokens": nIn, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
