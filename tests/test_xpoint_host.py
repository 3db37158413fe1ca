"""CPU checks of -m xpoint (keyhunt.cpp:3005-3062, 6454-6552): the C++ host (libkhhost) against a model of a few lines
(the first 20 bytes of big-endian x; beta and lambda as constants; the oracle for points and for the bloom over 20-byte
values): the target loader and its bloom, the confirmation of a hit, the refusal of a search whose flag does not match
the handle, device/xpoint.hpp compiled for the CPU, and the CLI's refusals.  Every comparison is exact."""
from __future__ import annotations

import os
import random
import subprocess

import pytest

from keyhuntm1cpu_amd import khhost

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE      # keyhunt.cpp:584
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72    # keyhunt.cpp:582
SEARCH_XPOINT, SEARCH_ENDO, SEARCH_ETH, KIND_X = 16, 4, 8, 32                   # include/khbsgs.h


def x20(x: int) -> bytes:
    return x.to_bytes(32, "big")[:20]


def lam(e: int, k: int) -> int:
    return k * pow(LAMBDA, e, N) % N


def _xy(ora, k: int) -> tuple[int, int]:
    b = ora.pubkey(k).be64()
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")


def test_model_constants(ora):
    """beta and lambda are cube roots of one, and lambda*(x, y) = (beta*x, y): the model's own footing."""
    assert pow(BETA, 3, P) == 1 and BETA != 1 and pow(LAMBDA, 3, N) == 1 and LAMBDA != 1
    for k in (1, 2, 0xDEADBEEF):
        x, y = _xy(ora, k)
        for e in (1, 2):
            assert _xy(ora, lam(e, k)) == (pow(BETA, e, P) * x % P, y)


def _oracle_bloom(ora, values, extra_counted=0):
    """The oracle's target bloom over 20-byte values (its 40-hex line loader), sized as if extra_counted more lines
    had been counted (lines longer than 20 characters that it omits)."""
    text = "\n".join([v.hex() for v in values] + ["z" * 41] * extra_counted) + "\n"
    O = ora.AddrTable(text)
    assert O.n == len(values)
    out = (O.bloom_bytes(), int(O.bloom().bits), int(O.bloom().hashes), O.table())
    O.close()
    return out


def test_loader_same_entry_for_the_three_forms(ora):
    """64, 66 and 130 hex of one key give the same table entry, the first 20 bytes of x (for 130 hex a deliberate
    deviation from keyhunt.cpp:6524-6528, see include/khhost.h); the two prefix characters of a 66-hex line are not
    checked (05 here, and an 03 for a key whose y is even)."""
    k = 0x1234567
    x, y = _xy(ora, k)
    forms = [f"{x:064x}", f"{2 + (y & 1):02x}{x:064x}", f"04{x:064x}{y:064x}", f"05{x:064X}", f"{3 - (y & 1):02x}{x:064x}"]
    for f in forms:
        A = khhost.Addr(f + "\n", n_seq=1 << 16, threads=2, mode="xpoint")
        assert A.table() == [x20(x)] and A.skipped() == 0 and A.counted() == 1
        assert A.bloom() == _oracle_bloom(ora, [x20(x)])[:3]
        A.close()


def test_loader_lines(ora):
    """forceReadFileXPoint's rules: the first token decides, so a comment after it is not read; lines are trimmed; a
    non-hex token, a 65-hex token and a 40-character token are counted (40 or more characters) and skipped; blank and
    short lines are not counted.  As in the reference, as many lines are read from the top as were counted: here 7 of
    the 9, so the short line and the target after it are never reached."""
    xs = [_xy(ora, k) for k in (3, 5, 7, 11)]
    text = "\n".join([f"{xs[0][0]:064x} # puzzle three",                # comment after the token
                      f"  \t02{xs[1][0]:064x}\t: subtracted 40 \r",      # trimmed; ':' and tab end the token
                      "",                                                # blank: not counted, read as line 3, skipped
                      "g" * 64,                                          # not hex: counted, skipped
                      "a" * 65,                                          # 65 hex: counted, skipped
                      "b" * 40,                                          # 40 hex: counted, skipped (no such length)
                      f"04{xs[2][0]:064x}{xs[2][1]:064x}",               # uncompressed
                      "short",                                           # not counted and never read
                      f"{xs[3][0]:064x}"]) + "\n"                        # counted, but past the lines that are read
    A = khhost.Addr(text, n_seq=1 << 16, threads=2, mode="xpoint")
    accepted = [x20(xs[0][0]), x20(xs[1][0]), x20(xs[2][0])]
    assert A.counted() == 7
    assert A.table() == sorted(accepted)
    assert A.skipped() == 4
    bf, bits, h, table = _oracle_bloom(ora, accepted, extra_counted=4)
    assert A.bloom() == (bf, bits, h)
    assert b"".join(A.table()) == table
    A.close()


def test_loader_bloom_past_the_floor(ora):
    """10,001 targets, the first size past initBloomFilter's 10,000-entry floor: the bloom bytes equal the oracle's
    bloom over the same 20-byte values, and it is larger than the floor's."""
    rng = random.Random(5)
    vals = [rng.getrandbits(256) % P for _ in range(10001)]
    A = khhost.Addr("\n".join(f"{v:064x}" for v in vals) + "\n", n_seq=1 << 16, threads=2, mode="xpoint")
    want = [x20(v) for v in vals]
    assert A.counted() == 10001 and A.skipped() == 0
    bf, bits, h, table = _oracle_bloom(ora, want)
    assert A.bloom() == (bf, bits, h)
    assert b"".join(A.table()) == table
    assert bits > _oracle_bloom(ora, want[:3])[1]
    A.close()


def test_confirm_xpoint_kinds(ora):
    """A planted beta^e * x is confirmed from the walked key k as lambda^e * k mod n, the key whose point has the
    planted x; other e, other keys and values not in the table give nothing."""
    ks = [0x6000000123, 0x6000000456, 0x6000000789]
    planted = [pow(BETA, e, P) * _xy(ora, ks[e])[0] % P for e in range(3)]
    A = khhost.Addr("\n".join(f"{v:064x}" for v in planted) + "\n", n_seq=1 << 16, threads=2, mode="xpoint")
    for e in range(3):
        r = A.confirm(ks[e], KIND_X | e << 2)
        assert r == (lam(e, ks[e]), False)
        assert _xy(ora, r[0])[0] == planted[e]
        for other in range(3):
            if other != e:
                assert A.confirm(ks[e], KIND_X | other << 2) is None
        assert A.confirm(ks[e] + 1, KIND_X | e << 2) is None
    assert A.confirm(ks[0], KIND_X | 3 << 2) is None           # no such e
    for kind in (0, 1, 2, 16):                                 # an xpoint table holds no hash160 and no ETH address
        assert A.confirm(ks[0], kind) is None
    A.close()
    B = khhost.Addr("00" * 20 + "\n", n_seq=1 << 16, threads=2)
    assert B.confirm(ks[0], KIND_X) is None                    # nor a BTC table an x
    B.close()


def test_confirm_has_no_sign_fixup(ora):
    """A target given as 03 + x is found by the walked key whichever parity that key's y has: the reference prints the
    walked key (keyhunt.cpp:3013-3017), so k and n - k each confirm as themselves."""
    seen = set()
    for k in (0x6000000001, 0x6000000002, 0x6000000003, 0x6000000004, 0x6000000005, 0x6000000006):
        x, y = _xy(ora, k)
        seen.add(y & 1)
        A = khhost.Addr(f"03{x:064x}\n", n_seq=1 << 16, threads=2, mode="xpoint")
        assert A.confirm(k, KIND_X) == (k, False)
        assert A.confirm(N - k, KIND_X) == (N - k, False)
        A.close()
    assert seen == {0, 1}


@pytest.mark.parametrize("mode,search", [("xpoint", 2), ("address", SEARCH_XPOINT), ("xpoint", SEARCH_XPOINT | 1),
                                         ("xpoint", SEARCH_XPOINT | SEARCH_ETH), ("xpoint", SEARCH_ETH),
                                         ("address", SEARCH_XPOINT | SEARCH_ENDO)])
def test_mismatched_search_is_an_error(mode, search):
    """A search flag that does not match the handle's targets is refused with a message before any device is
    opened; it is never a silent empty search."""
    text = f"{1:064x}\n" if mode == "xpoint" else "00" * 20 + "\n"
    A = khhost.Addr(text, n_seq=1 << 16, threads=2, mode=mode)
    with pytest.raises(khhost.KhhError) as e:
        A.search(1, 1 << 16, search=search, lanes=256)
    msg = str(e.value)
    assert "[-1]" in msg and "xpoint" in msg.lower()
    A.close()


def test_python_binding_arguments():
    with pytest.raises(ValueError):
        khhost.Addr(f"{1:064x}\n", n_seq=1 << 16, mode="xpoint", crypto="eth")
    with pytest.raises(ValueError):
        khhost.Addr(f"{1:064x}\n", n_seq=1 << 16, mode="vanity")
    A = khhost.Addr("00" * 20 + "\n", n_seq=1 << 16, threads=2)
    assert A.mode == "address"
    A.close()


def test_x_be20_header_on_host(tmp_path):
    """device/xpoint.hpp under g++ (tests/native/test_xpoint_host.cpp), the code the kernel runs, over zero, the 256
    single-bit x values and p - 1: each of the top 160 bits flips exactly its own bit of the 20 bytes, the low 96
    bits change nothing."""
    exe = str(tmp_path / "test_xpoint_host")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "test_xpoint_host.cpp"), "-o", exe],
                   check=True)
    xs = [0] + [1 << b for b in range(256)] + [P - 1]
    path = tmp_path / "xs.bin"
    path.write_bytes(b"".join(x.to_bytes(32, "big") for x in xs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(l, 16) for l in r.stdout.split()]
    assert len(got) == 258
    assert got[0] == 0
    for b in range(256):
        assert got[1 + b] == ((1 << (b - 96)) if b >= 96 else 0), b
    assert got[257] == (P - 1) >> 96 == int.from_bytes(x20(P - 1), "big")


def _cli(args, cwd):
    from keyhuntm1cpu_amd import BIN_DIR
    exe = os.path.join(BIN_DIR, "keyhunt_amd")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=60)


def test_cli_xpoint_with_eth_is_refused(tmp_path):
    r = _cli(["-m", "xpoint", "-c", "eth", "-f", os.path.join(GOLD, "address", "1to63_65.txt"), "-r", "1:1000"],
             tmp_path)
    assert r.returncode == 1
    assert "[+] Mode xpoint\n" in r.stdout
    assert "[E] -c eth is valid only with -m address" in r.stderr
    assert "Hit" not in r.stdout and not (tmp_path / "KEYFOUNDKEYFOUND.txt").exists()


def test_cli_vanity_is_still_refused(tmp_path):
    r = _cli(["-m", "vanity", "-f", os.path.join(GOLD, "address", "1to63_65.txt"), "-r", "1:1000"], tmp_path)
    assert r.returncode == 1
    assert "-m xpoint; -m minikeys and -m vanity remain (mode vanity is not available)" in r.stderr
    r = _cli(["-m", "minikeys"], tmp_path)
    assert r.returncode == 1 and "(mode minikeys is not available)" in r.stderr
