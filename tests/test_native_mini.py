"""device/minikey.hpp compiled for the CPU (tests/native/test_mini_host.cpp), the code the -m minikeys kernels run, as
a stand-alone program built with the address and undefined-behaviour sanitizers and run directly: the base-58 counter
against Python's integers, both message packings against hashlib, and the fixed-base k*G for window widths 4, 8 and
16 against the host's mul_g (inside the program) and the oracle's public keys (here)."""
from __future__ import annotations

import hashlib
import os
import random
import struct
import subprocess

import pytest

from tests import mini_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "keyhuntm1cpu_amd", "csrc", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native_mini") / "test_mini_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "native", "test_mini_host.cpp"),
                    *(os.path.join(HOST, f) for f in ("mini_table.cpp", "secp_host.cpp", "u256.cpp")), "-o", out],
                   check=True)
    return out


def _run(exe, tmp_path, mode, data, *extra):
    path = tmp_path / "case.bin"
    path.write_bytes(data)
    r = subprocess.run([exe, mode, str(path), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


def _digits_of(v: int) -> bytes:
    out = []
    for _ in range(21):
        v, d = divmod(v, 58)
        out.append(d)
    return bytes(reversed(out))


def test_counter(exe, tmp_path):
    """mini_add and mini_carry: carries through 1, 3 and 20 digits, offset 0, offset 2^63, 2^64 - 1, and the overflow
    report at 58^21 - 1 + 1."""
    rng = random.Random(21)
    top = mr.SPACE - 1
    cases = [(mr.value("SRPqx8QiwnW4WNWnTVa2Wz"), 1, 3),            # a carry through 1 digit
             (mr.value("SRPqx8QiwnW4WNWnTVazzz"), 1, 60),           # through 3
             (mr.value("S1zzzzzzzzzzzzzzzzzzzu"), 6, 58 * 58 + 5),  # through 20
             (mr.value("S1zzzzzzzzzzzzzzzzzzzu"), 0, 0),
             (12345, 1 << 63, 1), (12345, (1 << 64) - 1, 0), (0, 0, 0), (top, 0, 0),
             (top, 1, 0), (top - 5, 6, 0), (top - 5, 5, 1), (top - (1 << 64) + 1, (1 << 64) - 1, 2),
             (top - (1 << 64) + 2, (1 << 64) - 1, 0)]
    cases += [(rng.randrange(mr.SPACE), rng.randrange(1 << 64), rng.randrange(200)) for _ in range(200)]
    data = b"".join(_digits_of(v) + struct.pack("<QI", off, steps) for v, off, steps in cases)
    lines = _run(exe, tmp_path, "add", data)
    assert len(lines) == len(cases)
    for (v, off, steps), line in zip(cases, lines):
        ok, d, ok2, d2 = line.split()
        s = v + off
        assert (ok == "1") == (s < mr.SPACE), (v, off)
        assert bytes.fromhex(d) == _digits_of(s % mr.SPACE), (v, off)
        s2 = s % mr.SPACE + steps
        assert (ok2 == "1") == (s2 < mr.SPACE), (v, off, steps)
        assert bytes.fromhex(d2) == _digits_of(s2 % mr.SPACE), (v, off, steps)


@pytest.mark.parametrize("alphabet", [mr.ALPHABET, mr.ALPHABET[::-1], bytes(range(0xC6, 0x100)).decode("latin-1")],
                         ids=["default", "reversed", "high-bytes"])
def test_packings(exe, tmp_path, alphabet):
    """Both message shapes, the filter's head-word path, mini_valid and mini_key against hashlib on the strings."""
    assert len(alphabet) == 58 and len(set(alphabet)) == 58
    rng = random.Random(7)
    vals = [0, mr.SPACE - 1] + [rng.randrange(mr.SPACE) for _ in range(300)]
    if alphabet == mr.ALPHABET:
        first, count, _ = mr.SPANS[2]
        vals += [mr.value(first) + o for o in mr.valid_offsets(first, count)]       # some valid ones
    data = alphabet.encode("latin-1") + b"".join(_digits_of(v) for v in vals)
    lines = _run(exe, tmp_path, "pack", data)
    assert len(lines) == len(vals)
    n_valid = 0
    for v, line in zip(vals, lines):
        s = mr.string(v, alphabet).encode("latin-1")
        h23, h22, ok, key = line.split()
        assert h23 == hashlib.sha256(s + b"?").hexdigest() and h22 == hashlib.sha256(s).hexdigest() == key
        assert (ok == "1") == (hashlib.sha256(s + b"?").digest()[0] == 0)
        n_valid += ok == "1"
    if alphabet == mr.ALPHABET:
        assert n_valid >= 38


@pytest.mark.parametrize("w", [4, 8, 16])
def test_fixed_base_multiplication(exe, tmp_path, ora, w):
    good, bad = mr.directed_scalars(w)
    rng = random.Random(w)
    rnd = [rng.randrange(1, mr.N) for _ in range(500)]
    ks = good + bad + rnd
    lines = _run(exe, tmp_path, "mul", b"".join(k.to_bytes(32, "big") for k in ks), str(w))
    assert len(lines) == len(ks)
    for k, line in zip(ks, lines):
        if k in bad:
            assert line == "1", hex(k)
        else:
            assert line.startswith("0 "), hex(k)
    for k, line in list(zip(ks, lines))[:len(good)] + list(zip(ks, lines))[-20:]:     # the program compared them all
        assert bytes.fromhex(line.split()[1]) == ora.pubkey(k).be64(), hex(k)          # with mul_g; these also here
