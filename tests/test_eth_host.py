"""CPU checks of -m address -c eth (keyhunt.cpp:4783-4789, 2989-3002, 6374-6450): the tests' own Keccak
(tests/eth_ref.py) pinned against hashlib, the empty-message digest and the reference's tests/1to32.eth; then the C++
host (libkhhost) against it: the address hash, the target loader and its bloom, the confirmation of a hit, and the
refusal of a search whose flag does not match the handle.  Every comparison is exact."""
from __future__ import annotations

import hashlib
import json
import os
import random

import numpy as np
import pytest

from keyhuntm1cpu_amd import khhost
from tests import eth_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SEARCH_ETH, KIND_ETH = 8, 16             # include/khbsgs.h KHB_SEARCH_ETH, KHB_ADDR_KIND_ETH


def _text(name: str) -> str:
    with open(os.path.join(GOLD, "address", name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLD, "puzzle_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture_addresses():
    lines = [l.strip() for l in _text("1to32.eth").splitlines() if l.strip()]
    assert len(lines) == 32 and all(len(l) == 42 and l.startswith("0x") for l in lines)
    return [bytes.fromhex(l[2:]) for l in lines]


# ---- the model, pinned independently of the product ----
def test_model_with_sha3_pad_equals_hashlib():
    rng = random.Random(1)
    for ln in (0, 1, 64, 135, 136, 137, 300):
        for _ in range(3):
            m = bytes(rng.getrandbits(8) for _ in range(ln))
            assert eth_ref.keccak256(m, 0x06) == hashlib.sha3_256(m).digest(), ln


def test_model_keccak256_of_empty_message():
    assert eth_ref.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"


def test_model_reproduces_reference_fixture(ora, keys, fixture_addresses):
    for n in range(1, 33):
        xy = ora.pubkey(int(keys[str(n)]["key"], 16)).be64()
        assert eth_ref.eth_address(xy) == fixture_addresses[n - 1], n


# ---- libkhhost ----
def test_host_eth_address_matches_model(ora, keys):
    rng = random.Random(8)
    ks = [int(keys[str(n)]["key"], 16) for n in range(1, 33)] + [rng.randrange(1, N) for _ in range(1000)]
    xy = [ora.pubkey(k).be64() for k in ks]
    want = eth_ref.eth_addresses(np.frombuffer(b"".join(xy), dtype=np.uint8))
    for i, p in enumerate(xy):
        assert khhost.eth_address(p) == want[i].tobytes(), i
        assert khhost.pubkey(ks[i]) == p


def test_loader_reads_reference_fixture(fixture_addresses):
    A = khhost.Addr(_text("1to32.eth"), n_seq=1 << 16, threads=2, crypto="eth")
    assert A.table() == sorted(fixture_addresses)
    assert A.skipped() == 0
    A.close()


def _hex_lines_bloom(ora, values, extra_counted=0):
    """The oracle's target bloom over 20-byte values (its 40-hex line loader), sized as if extra_counted more lines
    had been counted (lines longer than 20 characters that it omits)."""
    text = "\n".join([v.hex() for v in values] + ["z" * 41] * extra_counted) + "\n"
    O = ora.AddrTable(text)
    assert O.n == len(values)
    out = (O.bloom_bytes(), int(O.bloom().bits), int(O.bloom().hashes), O.table())
    O.close()
    return out


def test_loader_quirks(ora):
    """forceReadFileAddressEth: 40 hex without a prefix, upper case, a 41-character line (omitted), a 42-character
    line whose two leading characters are not 0x (accepted: they are not looked at), a non-hex line (omitted), and
    surrounding blanks trimmed."""
    rng = random.Random(4)
    v = [bytes(rng.getrandbits(8) for _ in range(20)) for _ in range(5)]
    text = "\n".join([v[0].hex(),                       # 40 hex
                      v[1].hex().upper(),               # upper case
                      "0" + v[2].hex(),                 # 41 characters: omitted
                      "zz" + v[3].hex(),                # 42 characters, the prefix is not looked at
                      "0x" + "g" * 40,                  # 42 characters, not hex: omitted
                      "g" * 40,                         # 40 characters, not hex: omitted
                      "  \t0x" + v[4].hex().upper()[:20] + v[4].hex()[20:] + " \r",   # mixed case, trimmed
                      "short"]) + "\n"                  # not counted; the counted lines are used up before it
    A = khhost.Addr(text, n_seq=1 << 16, threads=2, crypto="eth")
    accepted = [v[0], v[1], v[3], v[4]]
    assert A.table() == sorted(accepted)
    assert A.skipped() == 3
    bf, bits, h, table = _hex_lines_bloom(ora, accepted, extra_counted=3)
    assert A.bloom() == (bf, bits, h)
    assert b"".join(A.table()) == table
    A.close()


def test_loader_bloom_sized_by_counted_lines(ora):
    """More than 10,000 targets: initBloomFilter sizes the bloom by the lines of 40 or more characters, the omitted
    ones included (keyhunt.cpp:6387-6409, 6559-6576).  12,000 prefixed addresses and 3,000 41-character lines give
    the oracle's bloom for 15,000 counted lines holding the 12,000 values, byte for byte."""
    rng = random.Random(5)
    vals = [bytes(rng.getrandbits(8) for _ in range(20)) for _ in range(12000)]
    lines = ["0x" + v.hex() for v in vals]
    for i in range(3000):
        lines.insert(4 * i, "f" * 41)
    A = khhost.Addr("\n".join(lines) + "\n", n_seq=1 << 16, threads=2, crypto="eth")
    assert len(A.table()) == 12000 and A.skipped() == 3000
    bf, bits, h, table = _hex_lines_bloom(ora, vals, extra_counted=3000)
    assert A.bloom() == (bf, bits, h)
    assert b"".join(A.table()) == table
    small = _hex_lines_bloom(ora, vals)
    assert bits > small[1]
    A.close()


def test_confirm_eth_kind(keys):
    A = khhost.Addr(_text("1to32.eth"), n_seq=1 << 16, threads=2, crypto="eth")
    for n in (1, 7, 20, 32):
        k = int(keys[str(n)]["key"], 16)
        assert A.confirm(k, KIND_ETH) == (k, False)
        assert A.confirm(k + 1, KIND_ETH) is None       # not a puzzle key
    assert A.confirm(N - 3, KIND_ETH) is None           # the negated point's address is another one: never negated
    for kind in (0, 1, 2):                              # an ETH table holds no hash160
        assert A.confirm(3, kind) is None
    A.close()
    B = khhost.Addr(_text("1to32.rmd"), n_seq=1 << 16, threads=2)
    assert B.confirm(3, KIND_ETH) is None               # nor a BTC table an ETH address
    B.close()


@pytest.mark.parametrize("crypto,search", [("btc", SEARCH_ETH), ("eth", 0), ("eth", 1), ("eth", 2),
                                           ("eth", SEARCH_ETH | 4), ("eth", SEARCH_ETH | 1), ("btc", SEARCH_ETH | 4)])
def test_mismatched_search_is_an_error(crypto, search):
    """A search flag that does not match the handle's targets is refused with a message before any device is
    opened; it is never a silent empty search."""
    A = khhost.Addr(_text("1to32.eth" if crypto == "eth" else "1to32.rmd"), n_seq=1 << 16, threads=2, crypto=crypto)
    with pytest.raises(khhost.KhhError) as e:
        A.search(1, 1 << 16, search=search, lanes=256)
    msg = str(e.value)
    assert "[-1]" in msg and ("eth" in msg.lower())
    A.close()
