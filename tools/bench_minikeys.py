"""-m minikeys throughput on one MI355X: khhost.Minikeys.search over 2^--log2 consecutive candidates from --first
against tests/golden/address/unsolvedpuzzles.rmd, reported as candidates/s and valid keys/s with the VALU roofline of
the filter (one SHA-256 block per candidate).  Prints one JSON line.

Usage: python tools/bench_minikeys.py [--log2 32] [--window 16] [--per-launch-log2 30] [--warmup-log2 26]
       [--ab 3] [--cpu-log2 24]
--ab N: N alternating runs of window widths 8 and 16 in this one process (the span of --log2 each); the line then
        holds every run's rate under "ab" and the faster width's median as the value.
--cpu-log2 K: also run the reference's loop on 16 CPU threads over 2^K candidates of the same span (0 = skip) and
        report the ratio a user sees.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# Executed VALU lane-instructions per candidate in the filter (rocprofv3 --pmc SQ_INSTS_VALU x 64 / 2^30 candidates of
# one launch, profiles/minikeys/pmc_counter_collection.csv): a whole SHA-256 block is ~1450 as device/hash160.hpp
# counts it; the filter shares rounds 0..4 and W16..W19 among the candidates of a run and completes one digest word.
SHA_BLOCK_EXEC = 1233
PEAK_T = 68.2   # measured v_add_u32 / v_xor issue, 111 lane-ops/clk/CU x 256 CU x 2.4 GHz (profiles/r01_intops2.txt)


def run(M, first: str, count: int, per_launch: int) -> dict:
    t0 = time.time()
    found, st = M.search(first, count, per_launch=per_launch)
    dt = time.time() - t0
    assert st["candidates"] == count, st
    return {"seconds": round(dt, 4), "rate": count / dt, "valid": st["valid"], "found": len(found),
            "launches": st["launches"], "rescans": st["rescans"], "filter_s": st["filter_s"], "keys_s": st["keys_s"],
            "bloom_hits": st["hits"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--first", default="SRPqx8QiwnW4WNWnTVa2W5", help="the first candidate (the help text's minikey)")
    ap.add_argument("--log2", type=int, default=32, help="candidates of the measured span, as a power of two")
    ap.add_argument("--window", type=int, default=16, choices=[4, 8, 16])
    ap.add_argument("--per-launch-log2", type=int, default=30)
    ap.add_argument("--warmup-log2", type=int, default=26)
    ap.add_argument("--ab", type=int, default=0, help="N alternating runs each of window widths 8 and 16")
    ap.add_argument("--cpu-log2", type=int, default=0, help="CPU baseline over 2^K candidates on 16 threads")
    args = ap.parse_args()
    import torch  # noqa: F401  (share torch's HIP runtime, as bench.py)
    from keyhuntm1cpu_amd import khbsgs, khhost
    with open(os.path.join(REPO, "tests", "golden", "address", "unsolvedpuzzles.rmd")) as f:
        text = f.read()
    build = khbsgs.build_info()
    build["path"] = os.path.relpath(build["path"], REPO)
    count, per = 1 << args.log2, 1 << args.per_launch_log2
    widths = [8, 16] if args.ab else [args.window]
    handles, table_s = {}, {}
    for w in widths:
        t0 = time.time()
        handles[w] = khhost.Minikeys(text, window_bits=w, threads=16)
        table_s[w] = round(time.time() - t0, 3)
    runs = {w: [] for w in widths}
    for w in widths:
        if args.warmup_log2:
            run(handles[w], args.first, 1 << args.warmup_log2, per)
    for _ in range(max(1, args.ab)):
        for w in widths:
            runs[w].append(run(handles[w], args.first, count, per))
    med = {w: statistics.median(r["rate"] for r in runs[w]) for w in widths}
    best = max(widths, key=lambda w: med[w])
    r = runs[best][-1]
    rate = med[best]
    filt = count / r["filter_s"] if r["filter_s"] else 0.0
    out = {
        "metric": "Mcand/s (-m minikeys, candidates examined per second)",
        "value": round(rate / 1e6, 2),
        "unit": "Mcand/s",
        "n_gpus": 1,
        "candidates": count,
        "valid_keys_per_s": round(rate * r["valid"] / count, 1),
        "seconds": r["seconds"],
        "config": {"workload": f"-m minikeys -f tests/unsolvedpuzzles.rmd from {args.first}, 2^{args.log2} candidates",
                   "build": build, "window_bits": best, "per_launch": per, "launches": r["launches"],
                   "rescans": r["rescans"], "valid": r["valid"], "bloom_hits": r["bloom_hits"], "found": r["found"],
                   "table_build_s": table_s},
        "stages": {"filter_s": round(r["filter_s"], 4), "keys_s": round(r["keys_s"], 4),
                   "keys_share": round(r["keys_s"] / max(1e-9, r["filter_s"] + r["keys_s"]), 4)},
        "roofline": {"bound": "valu", "unit": "Tops/s", "peak": PEAK_T, "ops_per_candidate": SHA_BLOCK_EXEC,
                     "achieved_filter": round(SHA_BLOCK_EXEC * filt / 1e12, 3),
                     "frac_filter": round(SHA_BLOCK_EXEC * filt / 1e12 / PEAK_T, 4),
                     "achieved_wall": round(SHA_BLOCK_EXEC * rate / 1e12, 3),
                     "frac_wall": round(SHA_BLOCK_EXEC * rate / 1e12 / PEAK_T, 4), "kernel": "k_mini_filter"},
    }
    if args.ab:
        out["ab"] = {str(w): [round(x["rate"] / 1e6, 2) for x in runs[w]] for w in widths}
        out["ab_keys_s"] = {str(w): [round(x["keys_s"], 4) for x in runs[w]] for w in widths}
    if args.cpu_log2:
        dt, v, _ = handles[best].cpu_scan(args.first, 1 << args.cpu_log2, 16)
        cpu = (1 << args.cpu_log2) / dt
        out["cpu_baseline"] = {"threads": 16, "candidates": 1 << args.cpu_log2, "seconds": round(dt, 3),
                               "Mcand_per_s": round(cpu / 1e6, 3), "valid": v, "gpu_over_cpu": round(rate / cpu, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
