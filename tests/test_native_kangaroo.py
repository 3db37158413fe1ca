"""The kangaroo search's distinguished-point table and its distance arithmetic mod n (host/kang_host.hpp) in a
stand-alone program (tests/native/test_kang_host.cpp) built with the address and undefined-behaviour sanitizers and
run directly."""
from __future__ import annotations

import os
import random
import subprocess

import pytest

from tests import adversarial as adv

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "keyhuntm1cpu_amd", "csrc", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native_kang") / "test_kang_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "native", "test_kang_host.cpp"),
                    *(os.path.join(HOST, f) for f in ("secp_host.cpp", "u256.cpp")), "-o", out], check=True)
    return out


@pytest.mark.parametrize("n, log2_slots", [(1, 1), (5000, 1), (20000, 10), (300, 16)])
def test_dp_table_insert_growth_and_collisions(exe, n, log2_slots):
    r = subprocess.run([exe, "table", str(n), str(log2_slots)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    size, slots, grown, probes = map(int, r.stdout.split())
    assert 0 < size <= n and 2 * size <= slots
    if n >= 5000:
        assert grown >= 4 and probes > 0              # it grew from its first size and met occupied slots
        assert size < n                               # and repeated x were recognised, not stored twice
    if log2_slots == 16:
        assert grown == 0 and slots == 1 << 16


def test_distance_arithmetic_mod_n(exe, tmp_path):
    rng = random.Random(5)
    n = adv.N
    edge = [0, 1, 2, n - 1, n - 2, n // 2, n // 2 + 1, (1 << 200) - 1, 1 << 200, (1 << 64) - 1, 1 << 64, 1 << 255]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(rng.randrange(n), rng.randrange(n)) for _ in range(500)]
    pairs += [(rng.randrange(1 << 200), rng.randrange(1 << 200)) for _ in range(200)]      # what distances are
    path = tmp_path / "pairs.bin"
    path.write_bytes(b"".join(a.to_bytes(32, "big") + b.to_bytes(32, "big") for a, b in pairs))
    r = subprocess.run([exe, "modn", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(pairs)
    for (a, b), line in zip(pairs, lines):
        s, d, m = (int(v, 16) for v in line.split())
        assert (s, d, m) == ((a + b) % n, (a - b) % n, -a % n), (hex(a), hex(b))
