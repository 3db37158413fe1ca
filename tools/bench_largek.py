#!/usr/bin/env python3
"""Large -k on resident tables: build them, time S steps through khhost.Session, print one JSON line.

    python tools/bench_largek.py --k 256 [--gate-log2 L | --no-gate] [--stage1 B] [--stage0 B] [--steps S]
    python tools/bench_largek.py --k 4096 --bsgsd-example

The tables are khhost.Tables(resident=True): L2, L3 and the bPtable on the host, the level-1 bloom and its gate
built on the device by the session (khb_build_l1_resident) and kept there.  A step is one batch of chunks sized as
bench.py sizes it (eight work items per lane, at least 2^30 giant steps); the target is a key outside the range, so
every step scans its chunks whole.  The line has giant steps/s (device-counted steps over the wall time of the
timed run, which ends in the last launch's collect), the reference's keys/s (chunks x 2N over the same time), the
table and device build times, Session.resident_info, khb_build_info and the pass fractions of the stage-1 fold and
of the full gate over 2^20 seeded random x (Session.gate_probe).

--bsgsd-example starts bsgsd_amd -k K --resident as a child process, sends the two queries of the reference's
BSGSD.md example (puzzle 63 in 2^62..2^63: 7cce5efdaccf6808 in 7.551 s there; a key that is not in the range: 404
Not Found in 7.948 s) and records both times.  These are measurements, not tests.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

P63 = "0365ec2994b8cc0a20d40dd69edfe55ca32a54bcbbaa6b0ddcff36049301a54579"
P125 = "0233709eb11e0d4439a729f21c2c443dedb727528229713f0065721ba8fa46f00e"
QUERY_RANGE = "4000000000000000:8000000000000000"
REFERENCE_S = {"found": 7.551, "not_found": 7.948}      # the reference's BSGSD.md example, bsgsd -k 4096


def step_chunks(lanes: int, groups_per_item: int, cycles: int) -> int:
    """Chunks per step as bench.py chooses them: eight work items per lane, at least 2^30 giant steps."""
    fill = -(-lanes * groups_per_item // cycles)
    return max(1, (1 << 30) // (cycles * 1024), 8 * fill)


def pass_fractions(sess, n: int = 1 << 20, seed: int = 1) -> dict:
    rng = random.Random(seed)
    got = sess.gate_probe(rng.randbytes(32 * n))
    return {"x": n, "seed": seed, "stage0": sum(1 for v in got if v & 4) / n,
            "fold": sum(1 for v in got if v & 2) / n, "gate": sum(1 for v in got if v & 1) / n}


def measure(args) -> dict:
    from keyhuntm1cpu_amd import khbsgs, khhost
    threads = min(16, os.cpu_count() or 1)
    t0 = time.time()
    tables = khhost.Tables(args.n, args.k, threads=threads, gpl=4, gpu_device=args.device, resident=True,
                           gate_log2=args.gate_log2, stage1=args.stage1, stage0=args.stage0)
    t_tables = time.time() - t0
    chunks = args.chunks or step_chunks(args.lanes or khbsgs.default_lanes(args.device), khbsgs.groups_per_item(),
                                        tables.cycles)
    two_n = 2 * tables.n_low
    start = 1 << 65
    target = khhost.pubkey((1 << 200) + 12345)          # not in any scanned chunk
    t0 = time.time()
    with khhost.Session(tables, devices=[args.device], lanes=args.lanes, chunks_per_batch=chunks) as sess:
        t_open = time.time() - t0
        if args.no_gate:
            sess.set_test_hooks(use_gate=False)
        info = sess.resident_info()
        fractions = None if args.no_gate or not info[0]["gate_log2"] else pass_fractions(sess)
        if args.warmup:
            sess.run([target], start, start + (1 << 120), max_chunks=args.warmup * chunks)
        tstart = start + args.warmup * chunks * two_n
        t0 = time.time()
        res, st = sess.run([target], tstart, tstart + (1 << 120), max_chunks=args.steps * chunks)
        wall = time.time() - t0
    assert res == [None] and st["chunks"] == args.steps * chunks
    assert st["giant_steps"] == st["chunks"] * tables.cycles * 1024
    return {"metric": "giant_steps_per_s", "value": st["giant_steps"] / wall,
            "reference_keys_per_s": st["chunks"] * two_n / wall, "k": args.k, "n": args.n or "0x100000000000",
            "m": tables.m, "l1ext": tables.l1ext, "cycles": tables.cycles, "steps": args.steps,
            "warmup": args.warmup, "chunks_per_step": chunks, "wall_s": wall, "kernel_s": st["kernel_s"],
            "busy_s": st["busy_s"], "device_giant_steps_per_s": st["giant_steps"] / st["busy_s"] if st["busy_s"] else None,
            "candidates": st["candidates"], "launches": st["launches"], "shader_mhz": st["shader_mhz"],
            "gate": "off" if args.no_gate else "on", "stage1": args.stage1, "stage0": args.stage0,
            "tables_s": t_tables, "tables_baby_ms": tables.build_ms, "session_open_s": t_open,
            "build_ms": info[0]["build_ms"], "resident_info": info, "pass_fractions": fractions,
            "build_info": khbsgs.build_info()}


def bsgsd_example(args) -> dict:
    from keyhuntm1cpu_amd import BIN_DIR
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [os.path.join(BIN_DIR, "bsgsd_amd"), "-k", str(args.k), "-t", "16", "-p", str(port), "--resident", "-g",
           str(args.device)]
    if args.n:
        cmd += ["-n", args.n]
    t0 = time.time()
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    try:
        for line in p.stdout:                             # ends when the daemon exits
            lines.append(line.rstrip())
            if line.startswith("[+] Listening in"):
                break
        ready = time.time() - t0
        if p.poll() is not None:
            return {"metric": "bsgsd_example", "k": args.k, "error": "the daemon exited", "log": lines[-8:]}
        out = {"metric": "bsgsd_example", "k": args.k, "ready_s": ready, "reference_s": REFERENCE_S,
               "resident": [l for l in lines if " resident: " in l]}
        for name, pub, want in (("found", P63, "7cce5efdaccf6808"), ("not_found", P125, "404 Not Found")):
            t0 = time.time()
            with socket.create_connection(("127.0.0.1", port), timeout=600) as c:
                c.sendall(f"{pub} {QUERY_RANGE}\n".encode())
                data = b""
                while True:
                    chunk = c.recv(4096)
                    if not chunk:
                        break
                    data += chunk
            out[name] = {"seconds": time.time() - t0, "answer": data.decode(), "ok": data.decode() == want}
        return out
    finally:
        p.terminate()
        try:
            p.wait(timeout=60)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--n", default=None, help="-n (default 2^44)")
    ap.add_argument("--gate-log2", type=int, default=0, help="explicit gate size in log2 bits (default: the policy)")
    ap.add_argument("--no-gate", action="store_true", help="drop the gate after the build (the ungated kernel)")
    ap.add_argument("--stage1", type=int, default=1, help="stage-1 fold: 1 auto, 0 none, else log2 bytes")
    ap.add_argument("--stage0", type=int, default=0, help="stage-0 filter: 0 none, 1 auto, else log2 bytes")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", type=int, default=0, help="chunks per step (default: as bench.py)")
    ap.add_argument("--lanes", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--label", default=None, help="copied into the line (A/B runs)")
    ap.add_argument("--out", default=None, help="append the line to this file as well")
    ap.add_argument("--bsgsd-example", action="store_true")
    args = ap.parse_args()
    rec = bsgsd_example(args) if args.bsgsd_example else measure(args)
    if args.label:
        rec["label"] = args.label
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
