"""device/keccak.hpp compiled for the CPU (tests/native/test_keccak_host.cpp), the code the -c eth kernel runs, against
the tests' own Keccak (tests/eth_ref.py): random inputs and the 512 single-bit inputs.  The hash takes bytes, so the
inputs need not be points of the curve."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from tests import eth_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def test_keccak_header_on_host(tmp_path):
    exe = str(tmp_path / "test_keccak_host")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "test_keccak_host.cpp"), "-o", exe],
                   check=True)
    rng = np.random.default_rng(20)
    xy = np.concatenate([rng.integers(0, 256, size=(2000, 64), dtype=np.uint8), eth_ref.single_bit_inputs(),
                         np.zeros((1, 64), dtype=np.uint8), np.full((1, 64), 0xFF, dtype=np.uint8)])
    path = tmp_path / "points.bin"
    path.write_bytes(xy.tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split()
    want = [bytes(a).hex() for a in eth_ref.eth_addresses(xy)]
    assert len(got) == len(want) == 2514
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} addresses differ, first at input {bad[0]}"
