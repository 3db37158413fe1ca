"""GPU parity for -m xpoint (keyhunt.cpp:3005-3062): the xpoint kernels of libkhbsgs through its C ABI, the libkhhost
search driver and the CLI, against a model of a few lines (the first 20 bytes of big-endian x, beta and lambda as
constants, the oracle for points and for the bloom over 20-byte values).  Every comparison is exact: each 20 bytes,
each bloom byte, each bloom hit {job, group, t, kind}, each recovered key, each printed line."""
from __future__ import annotations

import json
import os
import random
import subprocess

import pytest

from keyhuntm1cpu_amd import khhost

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE      # keyhunt.cpp:584
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72    # keyhunt.cpp:582
SEARCH_XPOINT, SEARCH_ENDO, SEARCH_ETH, KIND_X = 16, 4, 8, 32                   # include/khbsgs.h
FIXTURE = os.path.join(GOLD, "address", "1to63_65.txt")


def x20(x: int) -> bytes:
    return x.to_bytes(32, "big")[:20]


def lam(e: int, k: int) -> int:
    return k * pow(LAMBDA, e, N) % N


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLD, "puzzle_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture_text():
    with open(FIXTURE) as f:
        return f.read()


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


def _x_text(xs) -> str:
    return "\n".join(f"{x:064x}" for x in xs) + "\n"


def _bloom_passes(ora, values_in_bloom, probes) -> list[bool]:
    """bloom_check of each probe in the oracle's target bloom over the same 20-byte values (the bloom
    tests/test_xpoint_host.py shows the xpoint loader builds)."""
    O = ora.AddrTable("\n".join(bytes(v).hex() for v in values_in_bloom) + "\n")
    out = [O.bloom_check(bytes(p)) for p in probes]
    O.close()
    return out


def test_x_be20_kernel_matches_model(eng, ora):
    """khb_hash160(kind = 4): the 256 single-bit x (every word, byte and bit of the serialisation; the low 96 change
    nothing), zero, p - 1 and 3,000 random points of the curve; every third x is a loaded target, so the 20 bytes
    and the bloom byte are checked both ways."""
    rng = random.Random(12)
    pts = [ora.pubkey(rng.randrange(1, N)).be64() for _ in range(3000)]
    xs = [1 << b for b in range(256)] + [0, P - 1] + [int.from_bytes(p[:32], "big") for p in pts]
    xy = b"".join(x.to_bytes(32, "big") + bytes(32) for x in xs[:258]) + b"".join(pts)
    want = [x20(x) for x in xs]
    assert len(want) == 3258
    target_xs = sorted(set(xs[0::3]))
    A = khhost.Addr(_x_text(target_xs), n_seq=1 << 16, mode="xpoint")
    _load(eng, A)
    passes = _bloom_passes(ora, [x20(x) for x in target_xs], want)
    got = eng.hash160(4, xy)
    bad = [i for i in range(len(want)) if got[i][0] != want[i]]
    assert not bad, f"{len(bad)} values differ, first at input {bad[0]}"
    assert [g[1] for g in got] == [1 if p else 0 for p in passes]
    assert all(passes[i] for i in range(0, len(xs), 3)) and not all(passes)
    A.close()


def _walked_x(eng, centres, ngroups, gpl) -> list[int]:
    """x of every walked point from khb_addr_dump (the x,y walk), in (job, group, t) order."""
    probe = khhost.Addr(_x_text([1]), n_seq=1024 * ngroups, gpl=gpl, mode="xpoint")
    _load(eng, probe)
    xy = b"".join(eng.addr_dump(c, 0, ngroups) for c in centres)
    probe.close()
    return [int.from_bytes(xy[64 * i:64 * i + 32], "big") for i in range(len(xy) // 64)]


@pytest.mark.parametrize("gpl,n_jobs", [(1, 1), (4, 1), (1, 5)])
def test_xpoint_hits_match_model(eng, ora, gpl, n_jobs):
    """16 groups per job from a base, 3,000 of the walked x planted as 64-hex targets: the device's hit set {job,
    group, t, kind} equals {points of khb_addr_dump whose first 20 bytes of x pass the loaded bloom}, every kind
    KHB_ADDR_KIND_X, so the x-only walk's x are the x,y walk's bit for bit.  (1, 5): 80 work items, one full wave
    and a partial one."""
    ngroups = 16
    base = 0x6000000000 + 1 + gpl
    centres = [khhost.pubkey(base + 1024 * ngroups * j + 512) for j in range(n_jobs)]
    xs = _walked_x(eng, centres, ngroups, gpl)
    npts = 1024 * ngroups * n_jobs
    assert len(xs) == npts
    assert xs[0] == int.from_bytes(khhost.pubkey(base)[:32], "big")     # point t of group g of job j is key base + ...
    rng = random.Random(100 * gpl + n_jobs)
    picks = rng.sample(range(npts), 3000)
    A = khhost.Addr(_x_text(xs[i] for i in picks), n_seq=1024 * ngroups, gpl=gpl, mode="xpoint")
    _load(eng, A)
    passes = _bloom_passes(ora, [x20(xs[i]) for i in picks], [x20(x) for x in xs])
    want = sorted((i // (1024 * ngroups), (i // 1024) % ngroups, i % 1024, KIND_X) for i in range(npts) if passes[i])
    assert len(want) >= 3000
    hits, st = eng.addr_scan(b"".join(centres), 0, ngroups, SEARCH_XPOINT)
    assert st.giant_steps == npts
    assert sorted(hits) == want
    # the host confirms exactly the planted keys
    conf = [A.confirm(base + 1024 * ngroups * j + 1024 * g + t, kind) for j, g, t, kind in hits]
    assert sorted(r[0] for r in conf if r) == sorted(base + i for i in picks)
    assert all(not r[1] for r in conf if r)
    A.close()


def test_xpoint_endomorphism_hits_match_model(eng, ora):
    """-e at gpl 4: a third of the 3,000 plants are x, a third beta*x, a third beta^2*x of walked points.  The hit set
    equals the model's over the three values of every point, the kinds carry e, and the confirmed keys are
    lambda^e * k mod n."""
    ngroups, gpl = 16, 4
    base = 0x6100000000 + 7
    centre = khhost.pubkey(base + 512)
    xs = _walked_x(eng, [centre], ngroups, gpl)
    npts = 1024 * ngroups
    rng = random.Random(77)
    picks = rng.sample(range(npts), 3000)
    planted = [pow(BETA, n % 3, P) * xs[i] % P for n, i in enumerate(picks)]
    A = khhost.Addr(_x_text(planted), n_seq=1024 * ngroups, gpl=gpl, mode="xpoint")
    _load(eng, A)
    probes = [x20(pow(BETA, e, P) * x % P) for x in xs for e in range(3)]
    passes = _bloom_passes(ora, [x20(v) for v in planted], probes)
    want = sorted((0, i // 1024, i % 1024, KIND_X | e << 2) for i in range(npts) for e in range(3) if passes[3 * i + e])
    assert len(want) >= 3000
    assert {k for _, _, _, k in want} == {KIND_X, KIND_X | 4, KIND_X | 8}
    hits, st = eng.addr_scan(centre, 0, ngroups, SEARCH_XPOINT | SEARCH_ENDO)
    assert st.giant_steps == npts
    assert sorted(hits) == want
    conf = [A.confirm(base + 1024 * g + t, kind) for _, g, t, kind in hits]
    assert sorted(r[0] for r in conf if r) == sorted(lam(n % 3, base + i) for n, i in enumerate(picks))
    assert all(not r[1] for r in conf if r)
    found_x = sorted(int.from_bytes(khhost.pubkey(r[0])[:32], "big") for r in conf if r)
    assert found_x == sorted(planted)
    A.close()


def test_xpoint_search_with_stride():
    """-I 3: chunks of 2^14 keys base + c * 2^14 + 3 t; the planted keys of three chunks are found, each once."""
    n_seq, stride = 1 << 14, 3
    base = 0x7000000000 + 5
    rng = random.Random(33)
    picks = [base + c * n_seq + stride * t for c in range(3) for t in rng.sample(range(n_seq), 40)]
    picks = sorted(set(picks + [base, base + 2 * n_seq + stride * (n_seq - 1)]))   # + the first and last key walked
    text = "\n".join(khhost.pubkey(k)[:32].hex() for k in picks) + "\n"
    A = khhost.Addr(text, n_seq=n_seq, stride=stride, gpl=4, mode="xpoint")
    found, st = A.search(base, base + 3 * n_seq, search=SEARCH_XPOINT, lanes=4096)
    assert sorted(k for k, _, _ in found) == sorted(picks)
    assert all(not c and a == khhost.pubkey(k)[:20] for k, c, a in found)
    assert st["chunks"] == 3 and st["keys"] == 3 * n_seq
    A.close()


@pytest.mark.parametrize("hit_cap", [0, 16])
def test_xpoint_search_puzzles(keys, fixture_text, hit_cap):
    """tests/1to63_65.txt (64 compressed puzzle pubkeys) over [1, 2^24): exactly puzzle keys 1..24, compressed false,
    the first 20 bytes of their x; 16 chunks of 2^20 keys.  With a 16-entry hit ring the overflow rescans (by chunks,
    then by group ranges) find the same keys once each."""
    A = khhost.Addr(fixture_text, n_seq=1 << 20, mode="xpoint")
    assert A.counted() == 64 and A.skipped() == 0 and len(A.table()) == 64
    if hit_cap:
        A.set_hit_capacity(hit_cap)
    found, st = A.search(1, 1 << 24, search=SEARCH_XPOINT, lanes=65536)
    want = [int(keys[str(n)]["key"], 16) for n in range(1, 25)]
    assert sorted(k for k, _, _ in found) == sorted(want)
    lines = [l.strip() for l in fixture_text.splitlines() if l.strip()]
    for k, c, a in found:
        assert not c and a.hex() == lines[want.index(k)][2:42]
    assert st["chunks"] == 16 and st["keys"] == 1 << 24
    assert (st["rescans"] > 0) == bool(hit_cap)
    A.close()


def _cli(args, cwd):
    from keyhuntm1cpu_amd import BIN_DIR
    exe = os.path.join(BIN_DIR, "keyhunt_amd")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_cli_xpoint_range(tmp_path, keys, ora):
    """keyhunt_amd -m xpoint -f tests/1to63_65.txt -r 1:100000 -n 0x100000 (chunks of 2^20 keys, so exactly the range
    is scanned): writekey(false, key)'s four lines (keyhunt.cpp:5989-6021: the uncompressed key, its address and
    hash160) on stdout and in KEYFOUNDKEYFOUND.txt for puzzle keys 1..20, the keys below 0x100000, in key order."""
    r = _cli(["-m", "xpoint", "-f", FIXTURE, "-r", "1:100000", "-n", "0x100000", "-q", "-s", "0", "-t", "4"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "[+] Mode xpoint\n" in r.stdout
    assert "[+] Allocating memory for 64 elements: 0.00 MB\n" in r.stdout
    assert "[+] Bloom filter for 64 elements.\n" in r.stdout
    assert "[+] Sorting data ... done! 64 values were loaded and sorted\n" in r.stdout
    ks = [int(keys[str(n)]["key"], 16) for n in range(1, 33)]
    inside = [n for n in range(32) if ks[n] < 0x100000]
    assert inside == list(range(20))
    out, file = "", ""
    for n in inside:
        pt = ora.pubkey(ks[n])
        rmd = ora.pub_hash160(pt, False)
        four = (f"Private Key: {ks[n]:x}\npubkey: 04{pt.be64().hex()}\nAddress {ora.rmd_to_address(rmd)}\n"
                f"rmd160 {rmd.hex()}\n")
        out += "\nHit! " + four
        file += four
    assert out in r.stdout
    assert r.stdout.count("Hit!") == 20
    assert r.stdout.rstrip().endswith("End")
    with open(tmp_path / "KEYFOUNDKEYFOUND.txt") as f:
        assert f.read() == file


@pytest.mark.parametrize("search", [SEARCH_XPOINT | 1, SEARCH_XPOINT | SEARCH_ETH])
def test_xpoint_scan_rejects_combined_flags(eng, keys, fixture_text, search):
    """khb_addr_scan takes KHB_SEARCH_XPOINT alone or with -e: with -l bits or KHB_SEARCH_ETH it is KHB_EINVAL, nothing
    is queued and the context still scans afterwards."""
    from keyhuntm1cpu_amd.khbsgs import KhbError
    A = khhost.Addr(fixture_text, n_seq=1 << 14, gpl=4, mode="xpoint")
    _load(eng, A)
    with pytest.raises(KhbError) as e:
        eng.addr_scan(khhost.pubkey(1 + 512), 0, 16, search)
    assert "invalid argument" in str(e.value)
    hits, st = eng.addr_scan(khhost.pubkey(1 + 512), 0, 16, SEARCH_XPOINT)     # the context is still usable
    below = sorted(k for k in (int(keys[str(n)]["key"], 16) for n in range(1, 46)) if k <= 1 << 14)
    assert len(below) == 14
    assert all(kind == KIND_X for _, _, _, kind in hits)
    assert sorted(1 + 1024 * g + t for _, g, t, _ in hits if A.confirm(1 + 1024 * g + t, KIND_X)) == below
    A.close()
