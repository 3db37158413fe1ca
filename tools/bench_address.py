"""-m address throughput (BASELINE config E): keyhunt -m address -f tests/unsolvedpuzzles.rmd on one
MI355X, sequential chunks of -n keys from 2^70 (puzzle #71's range), reported as Mkeys/s with the
VALU roofline of the hash path.  Prints one JSON line.

Usage: python tools/bench_address.py [--search 2] [--chunks 24] [--n 0x100000000] [--crypto btc|eth]
       [--mode address|xpoint|vanity] [--endo] [--targets 1Love,...|@file] [--random-targets N]
(24 chunks of 2^32 keys = three launches of eight work items per lane, two queued at a time.)
--crypto eth: keyhunt -m address -c eth -f tests/1to32.eth over the same range and chunking (--search is not read:
one Keccak-256 per key).
--mode xpoint: keyhunt -m xpoint -f tests/1to63_65.txt over the same range and chunking (--search is not read: no
hash, the first 20 bytes of x probed); --endo adds -e (x, beta*x and beta^2*x per key; keys counted once).
--mode vanity: the -m vanity search (khhost.Addr(mode="vanity")) over the same range and chunking, --search as for -m address: the
same walk and hashes, every hash tested against the targets' intervals.  --targets takes the targets separated by
commas, or @file with one per line (default: one 5-character target, 1Love); --random-targets N generates N
7-character targets from a fixed seed (about as many matches in all as one 5-character target, N times the intervals).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# 32-bit VALU operations per key, counted from the algorithms (FIPS 180-4 / RIPEMD-160 as restated in
# device/hash160.hpp): a SHA-256 compression is 64 rounds x 22 + 48 schedule
# words x 13 = 2032, a RIPEMD-160 compression 160 steps x 9 = 1440; the EC walk is ~4.5 field
# multiplies per key (x and y) at ~150 VALU each.
SHA_BLOCK, RMD_BLOCK, EC_PER_KEY = 2032, 1440, 680
OPS = {0: 2 * SHA_BLOCK + RMD_BLOCK + EC_PER_KEY,            # uncompressed: 65-byte message, 2 blocks
       1: 2 * (SHA_BLOCK + RMD_BLOCK) + EC_PER_KEY - 150,    # compressed 02 + 03 from x (no y)
       2: 4 * SHA_BLOCK + 3 * RMD_BLOCK + EC_PER_KEY}
# -c eth: one Keccak-f[1600] per key (device/keccak.hpp).  A round in 64-bit operations: theta 20 xor (column
# parities) + 5 rotate + 5 xor (D) + 25 xor (A ^ D), rho 24 rotate, chi 25 x (not, and, xor), iota 1 xor = 155, each
# two 32-bit operations (a rotation is one funnel shift per half): 310 x 24 rounds, + 16 byte swaps of x || y.
KECCAK_F = 24 * 310
OPS_ETH = KECCAK_F + 16 + EC_PER_KEY
# Executed VALU lane-instructions per key, -l both (rocprofv3 --pmc SQ_INSTS_VALU x 64 / keys of one
# 8-chunk launch, profiles/r02w/addr_valu_counter_collection.csv: 4.968e12 wave-instr x 64 / 2^35 keys;
# VALUBusy 101.5 %: the kernel is at the VALU issue ceiling).
EXEC_PER_KEY = {2: 9253.4}
# -m xpoint: no hash.  The x-only walk is ~2.5 field multiplies per key (two steps share the inverse's three) at ~150
# VALU each, + 5 byte swaps and two XXH64 of 20 bytes (~60 32-bit operations each with the 64-bit multiplies split).
# -e adds two multiplies by beta, their canonicalisations and two more probes.
OPS_X = 375 + 5 + 120
OPS_XE = OPS_X + 2 * (150 + 20) + 2 * 125
PEAK_T = 68.2   # measured v_add_u32 / v_xor issue, 111 lane-ops/clk/CU x 256 CU x 2.4 GHz (profiles/r01_intops2.txt)


def vanity_targets(args) -> str:
    """--mode vanity: the target text, one per line."""
    if args.random_targets:
        import random
        rng = random.Random(7)
        b58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
        # '1', a second character every address length has (2..P: below 2^192 as the first of 33 digits), five more
        return "".join("1" + rng.choice(b58[1:22]) + "".join(rng.choice(b58) for _ in range(5)) + "\n"
                       for _ in range(args.random_targets))
    if args.targets.startswith("@"):
        with open(args.targets[1:]) as f:
            return f.read()
    return "".join(t + "\n" for t in args.targets.split(",") if t)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", type=int, default=2, help="0 uncompress, 1 compress, 2 both (default, as keyhunt)")
    ap.add_argument("--chunks", type=int, default=24)
    ap.add_argument("--n", type=lambda s: int(s, 0), default=1 << 32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--crypto", choices=["btc", "eth"], default="btc", help="eth: -c eth over tests/1to32.eth")
    ap.add_argument("--mode", choices=["address", "xpoint", "vanity"], default="address",
                    help="xpoint: -m xpoint over tests/1to63_65.txt; vanity: -m vanity over --targets")
    ap.add_argument("--targets", default="1Love", help="--mode vanity: targets separated by commas, or @file")
    ap.add_argument("--random-targets", type=int, default=0, help="--mode vanity: N generated 7-character targets")
    ap.add_argument("--endo", action="store_true", help="-e (with --mode xpoint)")
    args = ap.parse_args()
    eth = args.crypto == "eth"
    xpoint = args.mode == "xpoint"
    vanity = args.mode == "vanity"
    if (xpoint or vanity) and eth:
        ap.error(f"--mode {args.mode} has no --crypto eth")
    if args.endo and not xpoint:
        ap.error("--endo is measured with --mode xpoint")
    search = (16 | (4 if args.endo else 0)) if xpoint else 8 if eth else args.search   # KHB_SEARCH_XPOINT, _ETH
    ops = (OPS_XE if args.endo else OPS_X) if xpoint else OPS_ETH if eth else OPS[args.search]
    targets = "1to63_65.txt" if xpoint else "1to32.eth" if eth else "unsolvedpuzzles.rmd"
    import torch  # noqa: F401  (share torch's HIP runtime, as bench.py)
    from keyhuntm1cpu_amd import khbsgs, khhost
    if vanity:
        text = vanity_targets(args)
    else:
        with open(os.path.join(REPO, "tests", "golden", "address", targets)) as f:
            text = f.read()
    build = khbsgs.build_info()                  # the line names the kernel build it measured, as bench.py's does
    build["path"] = os.path.relpath(build["path"], REPO)
    t0 = time.time()
    A = khhost.Addr(text, n_seq=args.n, threads=16, crypto=args.crypto, mode=args.mode)
    t_build = time.time() - t0
    start = 1 << 70
    cap = 1 << 18 if vanity else 4096            # vanity finds keys as it goes: room for all of them
    if args.warmup:
        A.search(start, start + args.warmup * args.n, search=search, cap=cap)
    t0 = time.time()
    found, st = A.search(start + args.warmup * args.n, start + (args.warmup + args.chunks) * args.n,
                         search=search, cap=cap)
    dt = time.time() - t0
    keys = st["keys"]
    rate = keys / dt
    kern = st["kernel_s"] / max(1, st["launches"])
    achieved = ops * keys / st["kernel_s"] / 1e12
    out = {
        "metric": "Mkeys/s (-m xpoint, keys walked and probed per second)" if xpoint else
                  "Mkeys/s (-m vanity, keys hashed and matched per second)" if vanity else
                  "Mkeys/s (-m address, keys hashed and probed per second)",
        "value": round(rate / 1e6, 2),
        "unit": "Mkeys/s",
        "n_gpus": 1,
        "keys": keys,
        "seconds": round(dt, 3),
        "search": ("xpoint -e" if args.endo else "xpoint") if xpoint else
                  "eth" if eth else ["uncompress", "compress", "both"][args.search],
        "reference_keys_per_s": round(rate * (3 if args.endo else 2 if args.search == 1 and not eth and not xpoint
                                              else 1) / 1e6, 2),
        "config": {"workload": "-m xpoint -f tests/1to63_65.txt -b 71" + (" -e" if args.endo else "") if xpoint else
                               "-m address -c eth -f tests/1to32.eth -b 71" if eth else
                               f"-m vanity ({len(text.split())} targets, first {text.split()[0]}) -b 71" if vanity else
                               "-m address -f tests/unsolvedpuzzles.rmd -b 71 (BASELINE configs[4])",
                   "build": build,
                   "targets": len(text.split()) if vanity else len(A.table()),
                   "n_seq": hex(args.n), "chunks": st["chunks"],
                   "launches": st["launches"], "bloom_hits": st["hits"], "found": len(found),
                   "table_build_s": round(t_build, 2)},
        "roofline": {"bound": "valu", "unit": "Tops/s", "achieved": round(achieved, 3), "peak": PEAK_T,
                     "frac": round(achieved / PEAK_T, 4), "ops_per_key": ops,
                     "achieved_wall": round(ops * rate / 1e12, 3),
                     "frac_wall": round(ops * rate / 1e12 / PEAK_T, 4),
                     "kernel": "k_giant_scan<xpoint>" if xpoint else "k_giant_scan<vanity>" if vanity else "k_giant_scan<address>", "kernel_ms_avg": round(kern * 1e3, 3),
                     "shader_mhz": round(st["shader_mhz"], 1)},
    }
    if vanity:
        out["config"]["intervals"] = len(A.vanity_intervals())
        out["config"]["rescans"] = st["rescans"]
    if not eth and not xpoint and not vanity and args.search in EXEC_PER_KEY:
        e = EXEC_PER_KEY[args.search]
        out["roofline"]["executed"] = {
            "valu_lane_instr_per_key": e, "valu_busy_pct": 101.5,
            "valu_lane_instr_T_per_s_wall": round(e * rate / 1e12, 3),
            "pmc_source": "profiles/r02w/addr_valu_counter_collection.csv",
            "note": "fewer executed than algorithmic ops: v_bitop3 / v_alignbit / v_add3 fuse 2-3 simple ops"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
