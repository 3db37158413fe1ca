#!/usr/bin/env python3
"""Two measurements of the kangaroo search on one MI355X, printed as one JSON line.

1. The pure walking rate in jumps/s: one full residency of the walk kernel (khb_kang_full_herd) walks --launches
   launches of --steps steps with the public key far outside the interval, so nothing is ever found, at dp_bits 16
   (a distinguished point every 65,536 jumps: the ring stays almost empty).  Two launches are kept in flight.  The herd
   is 65,536 kangaroos of the search's own making repeated to the full size: every wave holds distinct kangaroos, and
   the rate does not depend on which points walk.  Rates: by the kernels' HIP-event times and by wall time.
2. A timed solve of a 64-bit interval through khhost.Kangaroo.search, with its jumps relative to 2 sqrt(W).

--ab 16,32,64 --runs 3 measures (1) for the variant builds lib/variants/libkhbsgs_kang<L>.so
(tools/build_variant.sh kang<L> -DKHB_KANG_PER_LANE=<L>) in alternating runs, the in-tree library standing in for
the value it was built with, and records every run.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keyhuntm1cpu_amd import LIB_DIR, khbsgs, khhost  # noqa: E402

START = 1 << 100
TILE = 1 << 16


def _tile_bytes(k: khhost.Kangaroo):
    xy, d = C.create_string_buffer(64 * TILE), C.create_string_buffer(32 * TILE)
    if khhost.lib().khh_kang_make_herd(k.h, 0, TILE, xy, d):
        raise RuntimeError("khh_kang_make_herd")
    return xy.raw, d.raw


def walk_rate(lib_path: str | None, launches: int, steps: int, tile, jumps) -> dict:
    L = khbsgs.kang_per_lane(lib_path)
    herd = int(khbsgs.lib(lib_path).khb_kang_full_herd(0))
    xy, d = tile
    with khbsgs.Engine(0, lib_path=lib_path) as e:
        e.kang_load_jumps(jumps)
        reps = 16
        for first in range(0, herd, TILE * reps):
            n = min(TILE * reps, herd - first)
            r = (n + TILE - 1) // TILE
            khbsgs._check(e.L.khb_kang_store(e.h, first, n, (xy * r)[:64 * n], (d * r)[:32 * n]), e.h, e.L)
        assert e.kang_herd() == herd
        e.kang_walk(2, 16, cap=1)                                   # warm-up
        kernel_ms, n_dp = 0.0, 0
        t0 = time.perf_counter()
        e.kang_submit(steps, 16)
        for i in range(launches):
            if i + 1 < launches:
                e.kang_submit(steps, 16)
            _, st = e.kang_collect(cap=1)
            assert st.steps_walked == herd * steps
            kernel_ms += st.kernel_ms
            n_dp += st.n_dp
        wall = time.perf_counter() - t0
    jumps_made = herd * steps * launches
    return {"per_lane": L, "herd": herd, "launches": launches, "steps": steps, "jumps": jumps_made,
            "kernel_s": round(kernel_ms / 1e3, 4), "wall_s": round(wall, 4),
            "mjumps_per_s_kernel": round(jumps_made / kernel_ms / 1e3, 1),
            "mjumps_per_s_wall": round(jumps_made / wall / 1e6, 1), "dps": n_dp,
            "lib": os.path.relpath(lib_path or khbsgs.LIB_PATH)}


def solve(bits: int, herd: int, dp_bits: int, seed: int) -> dict:
    key = START + (0x9E3779B97F4A7C15 * (seed + 1)) % (1 << bits)
    with khhost.Kangaroo(khhost.pubkey(key), START, START + (1 << bits), dp_bits=dp_bits, herd=herd, seed=seed) as k:
        t0 = time.perf_counter()
        r = k.search(devices=(0,))
        wall = time.perf_counter() - t0
        out = {"bits": bits, "herd": k.herd, "dp_bits": k.dp_bits, "found": r["key"] == key, "steps": r["steps"],
               "steps_over_2_sqrt_w": round(r["steps"] / (2 * 2 ** (bits / 2)), 3), "dps": r["dps"],
               "dead": r["dead"], "lost_dps": r["lost_dps"], "launches": r["launches"], "seconds": round(wall, 3),
               "mjumps_per_s": round(r["steps"] / wall / 1e6, 1)}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--lib", default=None, help="a libkhbsgs build for the walking rate (default: the in-tree one)")
    ap.add_argument("--ab", default="", help="comma-separated KHB_KANG_PER_LANE values to compare in alternating runs")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--solve-bits", type=int, default=64, help="0 skips the timed solve")
    ap.add_argument("--solve-herd", type=int, default=1 << 21)
    ap.add_argument("--solve-dp", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    # a key 2^150 past the interval: the wild herd never meets the tame one
    with khhost.Kangaroo(khhost.pubkey(START + (1 << 150)), START, START + (1 << 64), seed=a.seed) as k:
        tile, jumps = _tile_bytes(k), k.jump_table()
    out = {"bench": "kangaroo", "build": khbsgs.build_info()}
    if a.ab:
        here = khbsgs.kang_per_lane()
        runs = []
        for _ in range(a.runs):
            for L in (int(v) for v in a.ab.split(",")):
                path = None if L == here else os.path.join(LIB_DIR, "variants", f"libkhbsgs_kang{L}.so")
                runs.append(walk_rate(path, a.launches, a.steps, tile, jumps))
        out["ab"] = runs
    else:
        out["walk"] = walk_rate(a.lib, a.launches, a.steps, tile, jumps)
    if a.solve_bits:
        out["solve"] = solve(a.solve_bits, a.solve_herd, a.solve_dp, a.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
