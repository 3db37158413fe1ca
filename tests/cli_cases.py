"""Transcripts of keyhunt_amd and bsgsd_amd: the argument sets of tests/test_cli_transcripts.py (no GPU: every set
ends before a device is opened) and tests/test_gpu_cli_transcripts.py, how one set is run, and the recorder of the
fixtures under tests/golden/cli/.

The fixtures are what the programs of the commit before the front-end refactor printed:

    python -m tests.cli_cases cpu <bin dir of that build>      # writes tests/golden/cli/cpu.json
    python -m tests.cli_cases gpu <bin dir of that build>      # writes tests/golden/cli/gpu.json (needs a GPU)

The gpu recorder runs every set twice and keeps a set only if both runs agree after the masks.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import socket
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLD_CLI = os.path.join(GOLD, "cli")
P63 = "0365ec2994b8cc0a20d40dd69edfe55ca32a54bcbbaa6b0ddcff36049301a54579"
P30 = "030d282cf2ff536d2c42f105d0b8588821a915dc3f9a05bd98bb23af67a2e92a5b"

# every case runs in a fresh directory holding these files and nothing else
FILES = {"63.pub": P63 + "\n", "30.pub": P30 + "\n", "66.txt": "13zb1hQbWVsc2S7ZTZnP2G4undNNpdh5so\n"}
COPIES = ["1to32.txt", "1to32.eth", "1to63_65.txt"]          # from tests/golden/address
SMALL = ["-f", "63.pub", "-n", "0x10000"]                    # valid 63-bit target, M = 256: refused after the range

CPU_CASES = {
    "help": ("keyhunt_amd", ["-h"]),
    "minikeys": ("keyhunt_amd", ["-m", "minikeys"]),
    "vanity": ("keyhunt_amd", ["-m", "vanity", "-f", "X"]),
    "xpoint_eth": ("keyhunt_amd", ["-m", "xpoint", "-c", "eth", "-f", "X", "-r", "1:1000"]),
    "rmd160_eth": ("keyhunt_amd", ["-m", "rmd160", "-c", "eth"]),
    "address_eth_endo": ("keyhunt_amd", ["-m", "address", "-c", "eth", "-e"]),
    "both_endo": ("keyhunt_amd", ["-B", "both", "-e"]),
    "both_stride": ("keyhunt_amd", ["-B", "both", "-I", "2"]),
    "check_cpu": ("keyhunt_amd", ["--check", "cpu"]),
    "resident_S": ("keyhunt_amd", ["--resident", "-S"]),
    "resident_cpu_build": ("keyhunt_amd", ["--resident", "--cpu-build"]),
    "missing_file": ("keyhunt_amd", ["-f", "missing"]),
    "no_valid_data": ("keyhunt_amd", ["-f", "66.txt", "-b", "66"]),
    "bad_geometry": ("keyhunt_amd", ["-f", "63.pub", "-b", "63", "-n", "0x10000"]),
    "range_same": ("keyhunt_amd", SMALL + ["-r", "5:5"]),
    "range_swapped": ("keyhunt_amd", SMALL + ["-r", "20:10"]),
    "range_not_hex": ("keyhunt_amd", SMALL + ["-r", "zz"]),
    "bits_300": ("keyhunt_amd", SMALL + ["-b", "300"]),
    "range_small": ("keyhunt_amd", ["-f", "63.pub", "-r", "1:2"]),
    "address_missing_file": ("keyhunt_amd", ["-m", "address", "-f", "missing", "-b", "20", "-n", "1000"]),
    "address_stride_0": ("keyhunt_amd", ["-m", "address", "-I", "0"]),
    "xpoint_missing_file": ("keyhunt_amd", ["-m", "xpoint", "-f", "missing", "-r", "1:100"]),
    "unknown_option": ("keyhunt_amd", ["-Z"]),
    "bsgsd_help": ("bsgsd_amd", ["-h"]),
    "bsgsd_resident_cpu_build": ("bsgsd_amd", ["--resident", "--cpu-build"]),
    "bsgsd_check_x": ("bsgsd_amd", ["--check", "x"]),
    "bsgsd_bad_geometry": ("bsgsd_amd", ["-n", "0x10000"]),
    "bsgsd_unknown_option": ("bsgsd_amd", ["-Z"]),
}

BSGS30 = ["-m", "bsgs", "-f", "30.pub", "-b", "30", "-n", "0x100000", "-q", "-s", "0"]
# name -> argument sets run one after the other in the same directory (one transcript each)
GPU_CASES = {
    "bsgs30": [BSGS30],
    "bsgs30_S": [BSGS30 + ["-S"], BSGS30 + ["-S"]],          # the "Writing" run, then the "Reading" run
    "address20": [["-m", "address", "-f", "1to32.txt", "-b", "20", "-n", "0x100000", "-q", "-s", "0"]],
    "eth": [["-m", "address", "-c", "eth", "-f", "1to32.eth", "-r", "1:100000", "-n", "0x100000", "-q", "-s", "0",
             "-t", "4"]],
    "xpoint": [["-m", "xpoint", "-f", "1to63_65.txt", "-r", "1:100000", "-n", "0x100000", "-q", "-s", "0", "-t", "4"]],
    "resident63": [["-m", "bsgs", "-f", "63.pub", "-r", "7cce500000000000:7cce600000000000", "-n", "0x1000000000",
                    "-k", "8", "--resident", "-q", "-s", "0"]],
}
BSGSD_ARGS = ["-n", "0x100000", "-t", "8"]                    # + -p <free port>; cut at the "Listening in" line
MASKS = [(re.compile(r"build [0-9.]+ ms"), "build <x> ms"), (re.compile(r"(Listening in 127\.0\.0\.1:)\d+"), r"\1<port>")]


def populate(cwd: str) -> None:
    for name, text in FILES.items():
        with open(os.path.join(cwd, name), "w") as f:
            f.write(text)
    for name in COPIES:
        shutil.copy(os.path.join(GOLD, "address", name), cwd)


def mask(text: str) -> str:
    for rx, to in MASKS:
        text = rx.sub(to, text)
    return text


def run(bin_dir: str, program: str, args: list, cwd: str) -> dict:
    """One run; argv[0] is the bare program name, which getopt prints in its own messages."""
    r = subprocess.run([program] + args, executable=os.path.join(bin_dir, program), cwd=cwd, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode in (0, 1), (program, args, r.returncode, r.stderr)   # anything else: stop, start nothing more
    found = os.path.join(cwd, "KEYFOUNDKEYFOUND.txt")
    return {"stdout": mask(r.stdout), "stderr": mask(r.stderr), "returncode": r.returncode,
            "keyfound": open(found).read() if os.path.exists(found) else None}


def run_cpu_case(bin_dir: str, name: str, cwd: str) -> dict:
    populate(cwd)
    program, args = CPU_CASES[name]
    return run(bin_dir, program, args, cwd)


def run_gpu_case(bin_dir: str, name: str, cwd: str) -> dict:
    """The transcripts of the case's runs and the sha256 of every table file they left."""
    populate(cwd)
    runs = [run(bin_dir, "keyhunt_amd", args, cwd) for args in GPU_CASES[name]]
    tables = {f: hashlib.sha256(open(os.path.join(cwd, f), "rb").read()).hexdigest()
              for f in sorted(os.listdir(cwd)) if f.startswith("keyhunt_bsgs_")}
    return {"runs": runs, "tables": tables}


def run_bsgsd_startup(bin_dir: str, cwd: str) -> dict:
    """bsgsd_amd in an empty directory until it listens: the output up to that line, port masked."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    log_path = os.path.join(cwd, "bsgsd.log")
    with open(log_path, "w") as log:
        p = subprocess.Popen(["bsgsd_amd"] + BSGSD_ARGS + ["-p", str(port)], executable=os.path.join(bin_dir, "bsgsd_amd"),
                             cwd=cwd, stdout=log, stderr=subprocess.STDOUT)
        try:
            t0 = time.time()
            while time.time() - t0 < 120 and p.poll() is None and "Listening in" not in open(log_path).read():
                time.sleep(0.05)
            alive = p.poll() is None
        finally:
            p.terminate()
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    text = open(log_path).read()
    assert alive and "Listening in" in text, text
    cut = text.index("\n", text.index("Listening in")) + 1
    return {"output": mask(text[:cut]), "files": sorted(f for f in os.listdir(cwd) if f != "bsgsd.log")}


def _record(kind: str, bin_dir: str) -> None:
    os.makedirs(GOLD_CLI, exist_ok=True)
    out = {}
    if kind == "cpu":
        for name in CPU_CASES:
            with tempfile.TemporaryDirectory() as d:
                out[name] = run_cpu_case(bin_dir, name, d)
    else:
        takes = []
        for _ in range(2):
            take = {}
            for name in GPU_CASES:
                with tempfile.TemporaryDirectory() as d:
                    take[name] = run_gpu_case(bin_dir, name, d)
            with tempfile.TemporaryDirectory() as d:
                take["bsgsd_startup"] = run_bsgsd_startup(bin_dir, d)
            takes.append(take)
        for name in takes[0]:
            if takes[0][name] == takes[1][name]:
                out[name] = takes[0][name]
            else:
                print("dropped (two recordings differ):", name)
    with open(os.path.join(GOLD_CLI, kind + ".json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", kind, sorted(out))


if __name__ == "__main__":
    _record(sys.argv[1], os.path.abspath(sys.argv[2]))
