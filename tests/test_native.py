"""Host-compiled checks of the device headers (fe.hpp, bloom_probe.hpp, hash160.hpp) against the
oracle: the arithmetic and hashing the kernels run, executed on the CPU (no GPU needed)."""
from __future__ import annotations

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ORACLE = os.path.join(REPO, "oracle")


SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build_and_run(src: str, tmp_path, sanitize: bool = False) -> str:
    """Compile the stand-alone program tests/native/<src> with the oracle's objects and run it; sanitize: the
    whole program (oracle objects included) under the host AddressSanitizer and UBSan."""
    subprocess.run(["make", "-s", "-C", ORACLE], check=True)
    opt = SANITIZE if sanitize else ["-O2"]
    exe = str(tmp_path / os.path.splitext(os.path.basename(src))[0])
    srcs = [os.path.join(ORACLE, f) for f in ("ora_field.c", "ora_secp.c", "ora_hash.c", "ora_bsgs.c", "ora_addr.c")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run(["gcc", *opt, "-std=gnu11", "-c", s, "-o", o], check=True)
        objs.append(o)
    subprocess.run(["g++", *opt, "-std=c++17", os.path.join(HERE, "native", src), *objs, "-o", exe, "-lm",
                    "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_launch_pipeline_on_host(tmp_path):
    """host/pipeline.hpp (the launch pipeline of -m bsgs and -m address) with a scripted fake device: FIFO order,
    queue depth, rescan parts ahead of new chunks and lo before hi, gpl-aligned cuts, draining after a submit or
    collect error, and the stop switch.  Needs neither the oracle objects nor a GPU."""
    exe = str(tmp_path / "test_pipeline_host")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "test_pipeline_host.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok", r.stdout


def test_device_math_headers_on_host(tmp_path):
    out = _build_and_run("test_device_math_host.cpp", tmp_path)
    assert "FAIL" not in out


def test_hash160_header_on_host(tmp_path):
    out = _build_and_run("test_hash160_host.cpp", tmp_path)
    assert "ok" in out


def test_confirm_header_on_host(tmp_path):
    """device/confirm.hpp (khb_check's second/third check) vs the oracle's bsgs_secondcheck: planted keys,
    the AddDirect(P, -P) special case, random candidates, every level-2/3 bloom bit set, and the directed classes
    of tests/check_cases.py (Z, K, C, D, blooms pinning every x, the U8 helpers, search_bp at 1 to 300 entries)."""
    out = _build_and_run("test_confirm_host.cpp", tmp_path)
    assert out.strip().endswith("ok"), out
    assert "oracle finds 18 at even centres, 0 at odd ones" in out, out


def test_confirm_header_on_host_sanitized(tmp_path):
    """The same stand-alone program under the host AddressSanitizer and UBSan: the 32-element batches, the bPtable
    probes at both ends of the table and the byte windows of ck_mul_g stay inside their arrays."""
    out = _build_and_run("test_confirm_host.cpp", tmp_path, sanitize=True)
    assert out.strip().endswith("ok"), out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_cli_parse_layer_on_host(tmp_path, sanitize):
    """host/cli.cpp (the option parser of keyhunt_amd and bsgsd_amd, the -r rule, -g, tokens, valid_hex) as a
    stand-alone program built from cli.cpp, u256.cpp and secp_host.cpp alone; the second run under the host
    AddressSanitizer and UBSan.  Needs neither the oracle objects nor a GPU."""
    host = os.path.join(REPO, "keyhuntm1cpu_amd", "csrc", "host")
    exe = str(tmp_path / "test_cli_host")
    subprocess.run(["g++", *(SANITIZE if sanitize else ["-O2"]), "-std=c++17", "-pthread",
                    os.path.join(HERE, "native", "test_cli_host.cpp"), *(os.path.join(host, f) for f in
                                                                         ("cli.cpp", "u256.cpp", "secp_host.cpp")),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout
