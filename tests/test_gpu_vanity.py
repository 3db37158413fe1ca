"""GPU parity for -m vanity: the match stage (khb_vanity_match), the six vanity kernels through khb_addr_scan and the
libkhhost search driver, against the tests' model (tests/vanity_ref.py) with the oracle for points and
hash160s.  Every comparison is exact: each match byte, each hit {job, group, t, kind}, each found key."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd import khhost
from tests import vanity_ref as vr

pytestmark = pytest.mark.gpu
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE      # keyhunt.cpp:584
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72    # keyhunt.cpp:582
SEARCH_ENDO, SEARCH_ETH, SEARCH_XPOINT, SEARCH_VANITY = 4, 8, 16, 32            # include/khbsgs.h


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


def _table_bytes(iv):
    return [(vr.b20(a), vr.b20(b)) for a, b in iv]


def _form_hashes(ora, pts, endo: bool):
    """hash160 of every form of every point (x, y): {(e, form): [20 bytes per point]}, form 0/1 = compressed with
    prefix 02/03, 2 = uncompressed (x_e, y), 3 = uncompressed (x_e, p - y) (-e only), x_e = beta^e x."""
    out = {}
    for e in range(3 if endo else 1):
        xs = [pow(BETA, e, P) * x % P for x, _ in pts]
        for form in range(4 if endo else 3):
            if form < 2:
                msgs, n = b"".join(bytes([2 + form]) + x.to_bytes(32, "big") for x in xs), 33
            else:
                msgs = b"".join(b"\x04" + x.to_bytes(32, "big") + (y if form == 2 else P - y).to_bytes(32, "big")
                                for x, (_, y) in zip(xs, pts))
                n = 65
            raw = ora.hash160_many(msgs, n)
            out[e, form] = [raw[20 * i:20 * i + 20] for i in range(len(pts))]
    return out


# ---------------------------------------------------------------------------------------------- 1: the match stage
@pytest.mark.parametrize("R", vr.TABLE_SIZES)
def test_vanity_match_kernel(eng, R):
    rng = random.Random(R)
    iv = vr.random_table(R, rng)
    vals = vr.probe_values(iv, rng)
    eng.load_vanity(_table_bytes(iv))
    got = eng.vanity_match(b"".join(vr.b20(v) for v in vals))
    T = vr.Table(iv)
    want = bytes(1 if v in T else 0 for v in vals)
    bad = [i for i in range(len(vals)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {len(vals)} differ, first {vals[bad[0]]:040x}: device {got[bad[0]]}"
    assert 0 < sum(want) < len(want)


def test_vanity_load_and_match_errors():
    from keyhuntm1cpu_amd.khbsgs import Engine, KhbError, KHB_EINVAL, KHB_ESTATE
    with Engine(0, lanes=16384) as e:
        with pytest.raises(KhbError) as x:
            e.vanity_match(bytes(20))
        assert x.value.code == KHB_ESTATE                      # before any load
        a, b, c, d = (vr.b20(v) for v in (100, 200, 300, 400))
        for bad in ([], [(b, a)], [(c, d), (a, b)], [(a, c), (b, d)], [(a, b), (b, c)]):
            with pytest.raises(KhbError) as x:                 # n = 0, lo > hi, unsorted, overlapping, hi == next lo
                e.load_vanity(bad)
            assert x.value.code == KHB_EINVAL, bad
        with pytest.raises(KhbError) as x:
            e.vanity_match(bytes(20))
        assert x.value.code == KHB_ESTATE                      # a refused load leaves no table
        e.load_vanity([(a, b), (vr.b20(201), c)])              # touching intervals are a valid table
        assert e.vanity_match(b"".join(vr.b20(v) for v in (99, 100, 200, 201, 300, 301))) == bytes([0, 1, 1, 1, 1, 0])


# ------------------------------------------------------------------------------------ 2: hit sets of the six kernels
_walks: dict = {}


def _walk(eng, ora, gpl, n_jobs):
    """The walked points of a shape (khb_addr_dump) and their hashes from the oracle, computed once per shape."""
    if (gpl, n_jobs) not in _walks:
        ngroups = 16
        base = 0x5A00000000 + 3 + gpl
        centres = [khhost.pubkey(base + 1024 * ngroups * j + 512) for j in range(n_jobs)]
        A = khhost.Addr("1\n", n_seq=1024 * ngroups, gpl=gpl, mode="vanity")
        eng.load_giant_table(A.giant_table())
        offs, g = A.lane_offsets()
        eng.load_lane_offsets(offs, g)
        xy = b"".join(eng.addr_dump(c, 0, ngroups) for c in centres)
        pts = [(int.from_bytes(xy[64 * i:64 * i + 32], "big"), int.from_bytes(xy[64 * i + 32:64 * i + 64], "big"))
               for i in range(len(xy) // 64)]
        assert pts[0] == ora.pubkey(base).xy()
        _walks[gpl, n_jobs] = (A, centres, pts, _form_hashes(ora, pts, endo=(gpl, n_jobs) == (1, 1)))
    A, centres, pts, hashes = _walks[gpl, n_jobs]
    eng.load_giant_table(A.giant_table())
    offs, g = A.lane_offsets()
    eng.load_lane_offsets(offs, g)
    return centres, pts, hashes


@pytest.mark.parametrize("gpl,n_jobs,search", [(g, j, s) for g, j in [(1, 1), (4, 1), (1, 5)] for s in (0, 1, 2)]
                         + [(1, 1, 2 | SEARCH_ENDO)])
def test_vanity_hits_match_model(eng, ora, gpl, n_jobs, search):
    """16 groups per job; targets = the first three characters of the addresses of 40 sampled (point, form) pairs.
    The device's set {job, group, t, kind} equals the (point, form) pairs whose hash lies in the model's intervals.
    (1, 5): 80 work items, one full wave and a ragged one.  -e runs at shape (1, 1)."""
    endo = bool(search & SEARCH_ENDO)
    ngroups = 16
    centres, pts, hashes = _walk(eng, ora, gpl, n_jobs)
    npts = len(pts)
    assert npts == 1024 * ngroups * n_jobs
    forms = {0: [2], 1: [0, 1], 2: [0, 1, 2]}[search & 3] if not endo else [0, 1, 2, 3]
    kinds = [(e, f) for e in range(3 if endo else 1) for f in forms]
    rng = random.Random(1000 * gpl + 10 * n_jobs + search)
    targets = sorted({vr.address(hashes[kinds[n % len(kinds)]][i])[:3]
                      for n, i in enumerate(rng.sample(range(npts), 40))})
    iv = vr.merged(targets)
    T = vr.Table(iv)
    want = sorted((i // (1024 * ngroups), (i // 1024) % ngroups, i % 1024, f | e << 2)
                  for (e, f) in kinds for i in range(npts) if hashes[e, f][i] in T)
    assert want and {k for _, _, _, k in want} == {f | e << 2 for e, f in kinds}
    assert len(want) < 1 << 16                                  # far under the ring's 2^18
    eng.load_vanity(_table_bytes(iv))
    hits, st = eng.addr_scan(b"".join(centres), 0, ngroups, search | SEARCH_VANITY)
    assert st.giant_steps == npts and st.n_cand == len(want)
    assert sorted(hits) == want


# -------------------------------------------------------------------------------------------- 3: invalid combinations
@pytest.mark.parametrize("search", [SEARCH_VANITY | SEARCH_ETH, SEARCH_VANITY | SEARCH_XPOINT,
                                    SEARCH_VANITY | SEARCH_XPOINT | SEARCH_ENDO, SEARCH_VANITY | 3])
def test_vanity_scan_rejects_combined_flags(eng, ora, search):
    from keyhuntm1cpu_amd.khbsgs import KhbError, KHB_EINVAL
    centres, pts, hashes = _walk(eng, ora, 4, 1)
    iv = vr.merged(["1A"])
    eng.load_vanity(_table_bytes(iv))
    with pytest.raises(KhbError) as x:
        eng.addr_scan(centres[0], 0, 16, search)
    assert x.value.code == KHB_EINVAL
    hits, st = eng.addr_scan(centres[0], 0, 16, SEARCH_VANITY | 0)           # nothing was queued: this one runs
    T = vr.Table(iv)
    assert sorted(hits) == sorted((0, i // 1024, i % 1024, 2) for i in range(len(pts)) if hashes[0, 2][i] in T)


def test_vanity_scan_needs_a_table():
    from keyhuntm1cpu_amd.khbsgs import Engine, KhbError, KHB_ESTATE
    A = khhost.Addr("1\n", n_seq=1024 * 16, gpl=4, mode="vanity")
    with Engine(0, lanes=16384) as e:
        e.load_giant_table(A.giant_table())
        offs, g = A.lane_offsets()
        e.load_lane_offsets(offs, g)
        with pytest.raises(KhbError) as x:
            e.addr_scan(khhost.pubkey(1 + 512), 0, 16, SEARCH_VANITY | 2)
        assert x.value.code == KHB_ESTATE
    A.close()


# --------------------------------------------------------------------------------- 4, 5: through the host library
def _expected_found(ora, keys, targets, search):
    """{(key, compressed, address)} the forms of `search` imply for the scanned keys: with the compressed forms the
    key of either parity (key or n - key), with -e the lambda multiples and the negated uncompressed points."""
    endo = bool(search & SEARCH_ENDO)
    pts = [ora.pubkey(k).xy() for k in keys]
    hashes = _form_hashes(ora, pts, endo)
    T = vr.Table(vr.merged(targets))
    forms = {0: [2], 1: [0, 1], 2: [0, 1, 2]}[search & 3]
    if endo:
        forms = forms + ([3] if 2 in forms else [])
    out = set()
    for (e, f), hs in hashes.items():
        if f not in forms:
            continue
        for k, (x, y), h in zip(keys, pts, hs):
            if h not in T:                                      # a superset of startswith (tests/test_vanity_host.py)
                continue
            a = vr.address(h)
            if not any(a.startswith(t) for t in targets):
                continue
            K = k * pow(LAMBDA, e, N) % N
            if f < 2:
                K = K if (y & 1) == f else N - K
            elif f == 3:
                K = N - K
            out.add((K, f < 2, a))
    return out


@pytest.mark.parametrize("search", [2, 2 | SEARCH_ENDO])
def test_vanity_search_matches_oracle(ora, search):
    """2^15 consecutive keys in four chunks, two 3-character prefixes of addresses inside the range, -l both, once
    with -e: the found (key, compressed, address) set equals the oracle's under startswith."""
    base, n = 0x7B00000000 + 11, 1 << 15
    keys = list(range(base, base + n))
    targets = [vr.address(ora.pub_hash160(ora.pubkey(base + 1000), True))[:3],
               vr.address(ora.pub_hash160(ora.pubkey(base + 20000), False))[:3]]
    want = _expected_found(ora, keys, targets, search)
    assert (base + 1000, True) in {(k, c) for k, c, _ in want} and (base + 20000, False) in {(k, c) for k, c, _ in want}
    A = khhost.Addr("\n".join(targets) + "\n", n_seq=1 << 13, gpl=4, mode="vanity")
    found, st = A.search(base, base + n, search=search, lanes=16384, cap=1 << 14)
    got = [(k, c, vr.address(r)) for k, c, r in found]
    assert len(got) == len(set(got)) and set(got) == want
    assert st["chunks"] == 4 and st["keys"] == n and st["rescans"] == 0
    A.close()


def test_vanity_search_overflow(ora):
    """Target "1": every hash matches.  4,096 keys, -l compress: 8,192 hits against a ring of 3,000, so the chunk is
    rescanned in halves down to single groups (2,048 hits each); every key and every n - key comes back once."""
    base, n = 0x7C00000000 + 5, 4096
    A = khhost.Addr("1\n", n_seq=n, gpl=1, mode="vanity")
    A.set_hit_capacity(3000)
    found, st = A.search(base, base + n, search=1, lanes=16384, cap=1 << 14)
    want = sorted([k for k in range(base, base + n)] + [N - k for k in range(base, base + n)])
    assert sorted(k for k, _, _ in found) == want
    assert all(c for _, c, _ in found) and st["rescans"] == 3 and st["keys"] == n
    for k, _, r in found[:32]:
        assert r == ora.pub_hash160(ora.pubkey(k), True)
    A.close()
