"""GPU parity for -m address -c eth (keyhunt.cpp:2776-2780, 2989-3002, 4783-4789): the Keccak kernel of libkhbsgs
through its C ABI, the libkhhost search driver and the CLI, against the tests' own Keccak (tests/eth_ref.py, pinned
on the CPU by tests/test_eth_host.py).  Every comparison is exact: each address, each bloom byte, each bloom hit
{job, group, t, kind}, each recovered key, each printed line."""
from __future__ import annotations

import json
import os
import random
import subprocess

import numpy as np
import pytest

from keyhuntm1cpu_amd import khhost
from tests import eth_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2**256 - 2**32 - 977
SEARCH_ETH, SEARCH_ENDO, KIND_ETH = 8, 4, 16      # include/khbsgs.h


def _text(name: str) -> str:
    with open(os.path.join(GOLD, "address", name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLD, "puzzle_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


def _load(eng, A: khhost.Addr):
    bf, bits, h = A.bloom()
    eng.load_addr_bloom(bf, bits, h)
    eng.load_giant_table(A.giant_table())
    offs, gpl = A.lane_offsets()
    eng.load_lane_offsets(offs, gpl)


def _eth_text(addresses) -> str:
    return "\n".join("0x" + bytes(a).hex() for a in addresses) + "\n"


def _bloom_passes(ora, addresses_in_bloom, probes) -> list[bool]:
    """bloom_check of each probe in the oracle's target bloom over the same 20-byte values (the bloom
    tests/test_eth_host.py shows the ETH loader builds)."""
    O = ora.AddrTable("\n".join(bytes(a).hex() for a in addresses_in_bloom) + "\n")
    out = [O.bloom_check(bytes(p)) for p in probes]
    O.close()
    return out


def test_eth_address_kernel_matches_model(eng, ora):
    """khb_hash160(kind = 3): the 512 single-bit inputs (every lane, half and bit of the serialisation), zeros,
    p - 1 in both coordinates and 3,000 random points of the curve; a third of their addresses are the loaded
    targets, so the bloom byte is checked both ways."""
    rng = random.Random(12)
    pts = [ora.pubkey(rng.randrange(1, N)).be64() for _ in range(3000)]
    edge = bytes(64) + (P - 1).to_bytes(32, "big") * 2
    xy = eth_ref.single_bit_inputs().tobytes() + edge + b"".join(pts)
    want = eth_ref.eth_addresses(np.frombuffer(xy, dtype=np.uint8))
    assert len(want) == 3514
    targets = [want[i] for i in range(0, len(want), 3)]
    A = khhost.Addr(_eth_text(targets), n_seq=1 << 16, crypto="eth")
    _load(eng, A)
    passes = _bloom_passes(ora, targets, want)
    got = eng.hash160(3, xy)
    bad = [i for i in range(len(want)) if got[i][0] != want[i].tobytes()]
    assert not bad, f"{len(bad)} addresses differ, first at input {bad[0]}"
    assert [g[1] for g in got] == [1 if p else 0 for p in passes]
    assert sum(passes) >= len(targets)
    A.close()


@pytest.mark.parametrize("gpl,n_jobs", [(1, 1), (4, 1), (1, 5)])
def test_eth_hits_match_model(eng, ora, gpl, n_jobs):
    """16 groups per job from a base, ~3,000 of the walked keys' addresses planted as targets: the device's hit set
    {job, group, t, kind} equals {points of khb_addr_dump whose model address passes the loaded bloom}, every kind
    KHB_ADDR_KIND_ETH.  (1, 5): 80 work items, one full wave and a partial one."""
    ngroups = 16
    base = 0x6000000000 + 1 + gpl
    centres = [khhost.pubkey(base + 1024 * ngroups * j + 512) for j in range(n_jobs)]
    probe = khhost.Addr(_text("1to32.eth"), n_seq=1024 * ngroups, gpl=gpl, crypto="eth")
    _load(eng, probe)
    xy = b"".join(eng.addr_dump(c, 0, ngroups) for c in centres)
    probe.close()
    assert xy[:64] == khhost.pubkey(base)                      # point t of group g of job j is key base + ...
    addrs = eth_ref.eth_addresses(np.frombuffer(xy, dtype=np.uint8))
    npts = 1024 * ngroups * n_jobs
    assert len(addrs) == npts
    rng = random.Random(100 * gpl + n_jobs)
    picks = rng.sample(range(npts), 3000)
    targets = [addrs[i] for i in picks]
    A = khhost.Addr(_eth_text(targets), n_seq=1024 * ngroups, gpl=gpl, crypto="eth")
    _load(eng, A)
    passes = _bloom_passes(ora, targets, addrs)
    want = sorted((i // (1024 * ngroups), (i // 1024) % ngroups, i % 1024, KIND_ETH) for i in range(npts) if passes[i])
    assert len(want) >= 3000
    hits, st = eng.addr_scan(b"".join(centres), 0, ngroups, SEARCH_ETH)
    assert st.giant_steps == npts
    assert sorted(hits) == want
    # the host confirms exactly the planted keys
    conf = [A.confirm(base + 1024 * ngroups * j + 1024 * g + t, kind) for j, g, t, kind in hits]
    assert sorted(r[0] for r in conf if r) == sorted(base + i for i in picks)
    A.close()


def test_eth_search_with_stride():
    """-I 3: chunks of 2^14 keys base + c * 2^14 + 3 t; the planted keys of three chunks are found, each once."""
    n_seq, stride = 1 << 14, 3
    base = 0x7000000000 + 5
    rng = random.Random(33)
    picks = [base + c * n_seq + stride * t for c in range(3) for t in rng.sample(range(n_seq), 40)]
    picks = sorted(set(picks + [base, base + 2 * n_seq + stride * (n_seq - 1)]))   # + the first and last key walked
    text = _eth_text(khhost.eth_address(khhost.pubkey(k)) for k in picks)
    A = khhost.Addr(text, n_seq=n_seq, stride=stride, gpl=4, crypto="eth")
    found, st = A.search(base, base + 3 * n_seq, search=SEARCH_ETH, lanes=4096)
    assert sorted(k for k, _, _ in found) == sorted(picks)
    assert all(not c and a == khhost.eth_address(khhost.pubkey(k)) for k, c, a in found)
    assert st["chunks"] == 3 and st["keys"] == 3 * n_seq
    A.close()


@pytest.mark.parametrize("hit_cap", [0, 16])
def test_eth_search_puzzles(keys, hit_cap):
    """tests/1to32.eth over [1, 2^24): exactly puzzle keys 1..24, uncompressed flag, their addresses; with a
    16-entry hit ring the overflow rescans (by chunks, then by group ranges) find the same keys once each."""
    A = khhost.Addr(_text("1to32.eth"), n_seq=1 << 20, crypto="eth")
    if hit_cap:
        A.set_hit_capacity(hit_cap)
    found, st = A.search(1, 1 << 24, search=SEARCH_ETH, lanes=65536)
    want = [int(keys[str(n)]["key"], 16) for n in range(1, 25)]
    assert sorted(k for k, _, _ in found) == sorted(want)
    lines = [l.strip() for l in _text("1to32.eth").splitlines() if l.strip()]
    for k, c, a in found:
        assert not c and "0x" + a.hex() == lines[want.index(k)]
    assert st["chunks"] == 16 and st["keys"] == 1 << 24
    assert (st["rescans"] > 0) == bool(hit_cap)
    A.close()


def _cli(args, cwd):
    from keyhuntm1cpu_amd import BIN_DIR
    exe = os.path.join(BIN_DIR, "keyhunt_amd")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_cli_eth_range(tmp_path, keys):
    """keyhunt_amd -m address -c eth -f tests/1to32.eth -r 1:100000 (chunks of 2^20 keys, so exactly the range is
    scanned): writekeyeth's lines (keyhunt.cpp:6023-6051) on stdout and in KEYFOUNDKEYFOUND.txt for puzzle keys
    1..20, the keys below 0x100000, in key order."""
    r = _cli(["-m", "address", "-c", "eth", "-f", os.path.join(GOLD, "address", "1to32.eth"), "-r", "1:100000",
              "-n", "0x100000", "-q", "-s", "0", "-t", "4"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "[+] Setting search for ETH adddress.\n" in r.stdout
    lines = [l.strip() for l in _text("1to32.eth").splitlines() if l.strip()]
    ks = [int(keys[str(n)]["key"], 16) for n in range(1, 33)]
    inside = [n for n in range(32) if ks[n] < 0x100000]
    assert inside == list(range(20))
    out, file = "", ""
    for n in inside:
        out += f"\n Hit!!!! Private Key: {ks[n]:x}\naddress: {lines[n]}\n"
        file += f"Private Key: {ks[n]:x}\naddress: {lines[n]}\n"
    assert out in r.stdout
    assert r.stdout.count("Hit!!!!") == 20
    assert r.stdout.rstrip().endswith("End")
    with open(tmp_path / "KEYFOUNDKEYFOUND.txt") as f:
        assert f.read() == file


def test_cli_eth_ignores_l_for_hashing(tmp_path, keys):
    """-l compress with -c eth: accepted, and the same address is found (one Keccak per point whatever -l says)."""
    r = _cli(["-m", "address", "-c", "eth", "-l", "compress", "-f", os.path.join(GOLD, "address", "1to32.eth"),
              "-r", "1:1000", "-n", "0x1000", "-q", "-s", "0", "-t", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("Hit!!!!") == 12               # puzzle keys 1..12 are below 0x1000
    assert f" Hit!!!! Private Key: {int(keys['12']['key'], 16):x}\n" in r.stdout


def test_cli_eth_with_endomorphism_is_refused(tmp_path):
    r = _cli(["-m", "address", "-c", "eth", "-e", "-f", os.path.join(GOLD, "address", "1to32.eth"), "-r", "1:1000"],
             tmp_path)
    assert r.returncode == 1
    assert "[E] -c eth does not work with -e" in r.stderr and "does not own the address" in r.stderr
    assert "Hit" not in r.stdout and not (tmp_path / "KEYFOUNDKEYFOUND.txt").exists()


def test_cli_eth_with_rmd160_mode_is_refused(tmp_path):
    r = _cli(["-m", "rmd160", "-c", "eth", "-f", os.path.join(GOLD, "address", "1to32.eth"), "-r", "1:1000"], tmp_path)
    assert r.returncode == 1
    assert "[E] -c eth is valid only with -m address" in r.stderr
    assert "Hit" not in r.stdout and not (tmp_path / "KEYFOUNDKEYFOUND.txt").exists()


@pytest.mark.parametrize("search", [SEARCH_ETH | SEARCH_ENDO, SEARCH_ETH | 1, SEARCH_ETH | 2])
def test_eth_scan_rejects_combined_flags(eng, keys, search):
    """khb_addr_scan takes KHB_SEARCH_ETH exactly: with -e or -l bits it is KHB_EINVAL, and nothing is queued."""
    from keyhuntm1cpu_amd.khbsgs import KhbError
    A = khhost.Addr(_text("1to32.eth"), n_seq=1 << 14, gpl=4, crypto="eth")
    _load(eng, A)
    with pytest.raises(KhbError) as e:
        eng.addr_scan(khhost.pubkey(1 + 512), 0, 16, search)
    assert "invalid argument" in str(e.value)
    hits, st = eng.addr_scan(khhost.pubkey(1 + 512), 0, 16, SEARCH_ETH)     # the context is still usable
    below = sorted(k for k in (int(keys[str(n)]["key"], 16) for n in range(1, 33)) if k <= 1 << 14)
    assert len(below) == 14
    assert sorted(1 + 1024 * g + t for _, g, t, _ in hits if A.confirm(1 + 1024 * g + t, KIND_ETH)) == below
    A.close()
