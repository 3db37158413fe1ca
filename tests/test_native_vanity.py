"""device/vanity.hpp compiled for the CPU (tests/native/test_vanity_host.cpp), the code the -m vanity kernels run, as
a stand-alone program built with the address and undefined-behaviour sanitizers and run directly: the bitmap build and
vanity_match against the program's own linear scan and against the tests' model (tests/vanity_ref.py), on the tables
and probe values of tests/test_gpu_vanity.py's match test."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import pytest

from tests import vanity_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native_vanity") / "test_vanity_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "native", "test_vanity_host.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("R", vr.TABLE_SIZES)
def test_vanity_header_on_host(exe, tmp_path, R):
    rng = random.Random(R)
    iv = vr.random_table(R, rng)
    vals = vr.probe_values(iv, rng)
    path = tmp_path / "case.bin"
    path.write_bytes(struct.pack("<I", R) + b"".join(vr.b20(a) for a, _ in iv) + b"".join(vr.b20(b) for _, b in iv)
                     + struct.pack("<I", len(vals)) + b"".join(vr.b20(v) for v in vals))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    T = vr.Table(iv)
    want = "".join("1" if v in T else "0" for v in vals)
    assert r.stdout.strip() == want
    assert "1" in want and "0" in want
