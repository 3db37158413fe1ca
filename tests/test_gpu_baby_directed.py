"""Directed small-shape GPU tests of the baby-step table build: k_giant_scan<kBaby> (k_baby.hip, device/baby_point.hpp)
under khb_build_baby and khb_build_l1_resident (khb_tables.hip), called through Engine.build_baby and
Engine.build_l1_resident with chosen limits, null levels, bloom geometries, gate sizes and work shapes.

The expected value of every launch is tests/baby_ref.baby_build_ref, which tests/test_baby_ref_cpu.py pins to the
CPU-built tables and to the oracle.  Every comparison is of whole buffers, byte for byte.

The contexts are loaded as the host's GPU build loads them: the stride-1 table Gn[k] = k * G (k = 1..512) with 1024 * G,
and lane offsets (m * gpl * 1024) * G.  Job centres are unrelated random keys in [2^200, n - 2^40), asserted to keep
every group's centre further than 1,536 from a multiple of n and every walked key nonzero mod n, so no group is
degenerate (those are scan_group's, tests/test_gpu_addr_adversarial.py); one set has the product's consecutive centres
k * job_keys + 513, for which the exact condition is asserted instead (centre 513 is closer than 1,536 to 0, and no
centre is +-k * G, k <= 512, or +-1024 * G).

The bPtable: the model's records of ic < min(m3, total) must be equal.  With m3 > total the call copies 16 * m3 bytes
back from a device buffer it allocated and never cleared, so bytes 16 * total .. 16 * m3 of the host buffer are
overwritten with whatever that device memory held: nothing is asserted about them (include/khbsgs.h promises a record
for every ic < m3 of the jobs given, and nothing for an m3 beyond them)."""
from __future__ import annotations

import contextlib
import itertools
import random

import numpy as np
import pytest

from keyhuntm1cpu_amd import khbsgs
from keyhuntm1cpu_amd.khbsgs import TABLE_GATE, TABLE_L1, Engine, KhbError
from tests import adversarial as adv
from tests import baby_ref
from tests.helpers import _popcount, lane_offsets

pytestmark = pytest.mark.gpu
N = adv.N
ALL = ("l1", "l2", "l3", "bp", "gate")
JOBS, GPJ = 5, 6                       # 5 jobs x 6 groups: with 4 groups per lane every job's last lane is two short
JK = GPJ * 1024                        # job_keys
TOTAL = JOBS * JK                      # 30,720 walked points
LANES = 16384
GLG = 18                               # the general cases' gate: 2^18 bits, 35 % (lo) and 11 % (hi) full at 30,720 x


def geom(bits: int, hashes: int) -> tuple:
    return (bits + 7) // 8, bits, hashes


G_PLAIN = [geom(3461, 20), geom(2049, 20), geom(599, 20)]       # 433, 257 and 75 bytes: all odd


def differ(got: bytes, want: bytes, what: str) -> None:
    """assert got == want, with a report that stays small for buffers of megabytes."""
    if got == want:
        return
    if len(got) != len(want):
        pytest.fail(f"{what}: {len(got)} bytes for {len(want)}")
    d = np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
    i = int(d[0])
    pytest.fail(f"{what}: {len(d)} of {len(want)} bytes differ, the first at {i}: got {got[i:i + 8].hex()} "
                f"want {want[i:i + 8].hex()}")


class World:
    """What the cases share: the table, lane offsets, centre points and the model's Points by (centre keys, groups)."""

    def __init__(self, ora):
        self.ora = ora
        gen = ora.AddrGen(1)
        try:
            self.raw = gen.table()
        finally:
            gen.close()
        self.cache = {}
        rng = random.Random("baby directed")
        self.keys = [rng.randrange(2**200, N - 2**40) for _ in range(67)]

    def offsets(self, gpl: int, gpj: int) -> bytes:
        n = (gpj + gpl - 1) // gpl
        return bytes(64) + b"".join(self.ora.pubkey(m * gpl * 1024).be64() for m in range(1, n))

    def centres(self, keys) -> bytes:
        k = ("c", tuple(keys))
        if k not in self.cache:
            pts = {c: self.ora.pubkey(c).be64() for c in set(keys)}
            self.cache[k] = b"".join(pts[c] for c in keys)
        return self.cache[k]

    def points(self, keys, gpj: int) -> baby_ref.Points:
        k = ("p", tuple(keys), gpj)
        if k not in self.cache:
            self.cache[k] = baby_ref.Points(self.ora, keys, gpj)
        return self.cache[k]

    def ref(self, keys, gpj, limits, geoms, lg=0, probes=0, bp=True) -> dict:
        k = ("r", tuple(keys), gpj, tuple(limits), tuple(geoms), lg, probes, bp)
        if k not in self.cache:
            self.cache[k] = baby_ref.baby_build_ref(self.ora, list(keys), gpj, *limits, geoms, lg, probes, bp,
                                                    pts=self.points(keys, gpj))
        return self.cache[k]


@pytest.fixture(scope="module")
def world(ora):
    w = World(ora)
    yield w
    w.cache.clear()
    baby_ref._runs.clear()


def assert_no_degenerate_group(keys, gpj: int, product: bool = False) -> None:
    for c in keys:
        first = (c - 512) % N
        assert first != 0 and first + gpj * 1024 <= N, "a walked key is 0 mod n"
        for j in range(gpj):
            r = (c + 1024 * j) % N
            if product:      # the exact condition: the group's centre is none of +-k * G (k <= 512), +-1024 * G
                assert min(r, N - r) > 512 and min(r, N - r) != 1024
            else:
                assert min(r, N - r) > 1536


@contextlib.contextmanager
def baby_engine(world, lanes: int, gpl: int, gpj: int):
    with Engine(0, lanes=lanes) as e:
        e.load_giant_table(world.raw)
        e.load_lane_offsets(world.offsets(gpl, gpj), gpl)
        yield e


def same(out: dict, ref: dict, want, m3: int, total: int, geoms=None) -> None:
    assert not out["incomplete"] and out["kernel_ms"] > 0
    for k in ("l1", "l2", "l3", "gate"):
        if k in want:
            differ(out[k], ref[k], k)
        else:
            assert out[k] is None
    if "bp" in want:
        n = min(m3, total)
        assert len(out["bp"]) == 16 * m3
        differ(out["bp"][:16 * n], ref["bp"], "bp")        # bytes 16 n .. 16 m3: see the module's docstring
    else:
        assert out["bp"] is None
    for l, g in enumerate(geoms or ()):
        if f"l{l + 1}" in want and g[1] % 8:
            last = np.frombuffer(out[f"l{l + 1}"], dtype=np.uint8).reshape(256, g[0])[:, -1]
            assert not (last >> (g[1] % 8)).any(), f"padding bits of level {l + 1}"


# ------------------------------------------------------------------------------------------ 1. limits
_L = [1, 1023, 1024, 1025, JK - 1, JK, JK + 1, 3 * JK + 517, TOTAL - 1, TOTAL, TOTAL + 5000]
LIMITS = [(_L[i], _L[(i + 4) % 11], _L[(i + 7) % 11]) for i in range(11)]
LIMITS.append((JK + 1, JK + 1025, 2 * JK - 1))         # all end inside job 1: jobs 2..4 take the early-out
LIMITS.append((TOTAL + 5000,) * 3)                     # nothing past the walk is written


def test_limit_launches_cover_what_they_should():
    for lvl in range(3):
        assert {lim[lvl] for lim in LIMITS[:11]} == set(_L)              # every level gets every value
        assert any(lim[lvl] == max(lim) and lim.count(max(lim)) == 1 for lim in LIMITS)    # ... is the largest once
        assert any(lim[lvl] == min(lim) and lim.count(min(lim)) == 1 for lim in LIMITS)    # ... and the smallest
    assert any(lim[2] > lim[0] for lim in LIMITS)                        # m3 > l1ext
    assert all(JK < v <= 2 * JK for v in LIMITS[11])


@pytest.mark.parametrize("limits", LIMITS, ids=lambda lim: "-".join(map(str, lim)))
def test_limits(world, limits):
    """The four independent limits of baby_point (l1ext, m2, m3 and the gate's, which is l1ext), each at 1, around a
    group's end, around a job's end, inside job 3, around the walk's end and past it.  The bPtable's host buffer goes
    in filled with 0xa5."""
    keys = world.keys[:JOBS]
    assert_no_degenerate_group(keys, GPJ)
    ref = world.ref(keys, GPJ, limits, G_PLAIN, GLG, 3)
    with baby_engine(world, LANES, 4, GPJ) as e:
        out = e.build_baby(world.centres(keys), GPJ, *limits, G_PLAIN, ALL, GLG, 3, fill=0xA5)
    same(out, ref, ALL, limits[2], TOTAL, G_PLAIN)


# ------------------------------------------------------------------------------------------ 2. null levels
NULL_LIMITS = (JK + 1, 1025, TOTAL - 1)          # m3 the largest: bp without l3 and l3 without bp both key on it
SUBSETS = [s for r in range(6) for s in itertools.combinations(ALL, r)]


@pytest.fixture(scope="module")
def all_five(world):
    keys = world.keys[:JOBS]
    with baby_engine(world, LANES, 4, GPJ) as e:
        out = e.build_baby(world.centres(keys), GPJ, *NULL_LIMITS, G_PLAIN, ALL, GLG, 3)
    same(out, world.ref(keys, GPJ, NULL_LIMITS, G_PLAIN, GLG, 3), ALL, NULL_LIMITS[2], TOTAL, G_PLAIN)
    return out


@pytest.mark.parametrize("part", range(4))
def test_null_levels(world, all_five, part):
    """Every subset of the five outputs, eight per case (the empty one, the gate alone, bp without l3 and l3 without
    bp among them): what a subset returns equals the same buffers of the launch that asked for all five."""
    assert len(SUBSETS) == 32 and () in SUBSETS and ("gate",) in SUBSETS and ("bp",) in SUBSETS and ("l3",) in SUBSETS
    keys = world.keys[:JOBS]
    with baby_engine(world, LANES, 4, GPJ) as e:
        for want in SUBSETS[part::4]:
            geoms = [g if f"l{l + 1}" in want else None for l, g in enumerate(G_PLAIN)]
            out = e.build_baby(world.centres(keys), GPJ, *NULL_LIMITS, geoms, want, GLG if "gate" in want else 0, 3)
            same(out, all_five, want, NULL_LIMITS[2], TOTAL, G_PLAIN)


# ------------------------------------------------------------------------------------------ 3. bloom geometry
# Levels 1, 2, 3 receive 120, 74 and 24 points per sub-bloom on average; each geometry is sized for a fill of 20 to
# 80 % (1 - exp(-hashes * points / bits)), asserted from the model.  bytes_per_sub mod 4: 0 (512, 128, 4096, 32, 256),
# 1 (257, 17, 1025), 2 (6, 430), 3 (23, 75); bits mod 8: 0, 1 and 7; powers of two (wrap = 0): 4096, 256; 2^k + 1:
# 2049, 129, 8193; 2^k - 1: 1023, 32767, 2047; hashes 1, 2, 20, 255.
GEOM_LIMITS = (TOTAL, 3 * JK + 517, JK + 1)
GEOM_CASES = {
    "pow2": [geom(4096, 20), geom(2049, 20), geom(1023, 20)],
    "h255-h1-h2": [geom(32767, 255), geom(129, 1), geom(47, 2)],
    "h1-h2-h255": [geom(183, 1), geom(256, 2), geom(8193, 255)],
    "odd-bytes": [geom(3433, 20), geom(2047, 20), geom(599, 20)],
    "two-bits": [geom(3461, 20), geom(2049, 20), (1, 2, 1)],       # the degenerate extra: 2 bits, 1 byte, 1 hash
}


def test_geometry_list_covers_what_it_should():
    gs = [g for case in GEOM_CASES.values() for g in case]
    assert {g[0] % 4 for g in gs} == {0, 1, 2, 3} and {g[1] % 8 for g in gs} >= {0, 1, 7}
    assert {g[2] for g in gs} == {1, 2, 20, 255}
    for k in (12, 8):
        assert geom(1 << k, 20)[:2] in {g[:2] for g in gs} and (1 << 64) % (1 << k) == 0      # wrap = 0
    assert {2049, 129, 8193, 1023, 32767, 2047} <= {g[1] for g in gs}
    assert all(len(set(case)) == 3 for case in GEOM_CASES.values())


def geometry_ref(world, name: str) -> dict:
    keys = world.keys[:JOBS]
    ref = world.ref(keys, GPJ, GEOM_LIMITS, GEOM_CASES[name], GLG, 3)
    for l, g in enumerate(GEOM_CASES[name]):
        lvl = f"l{l + 1}"
        assert ref["subs"][lvl] == set(range(256)), "the points must reach every sub-bloom, 0 and 255 included"
        if g[1] > 2:
            assert 0.2 <= ref["fill"][lvl] <= 0.8, (name, lvl, ref["fill"][lvl])
    return ref


@pytest.mark.parametrize("name", list(GEOM_CASES))
def test_bloom_geometry(world, name):
    """Three different geometries for the three levels in one launch, through the word-aligned build and its repack.
    The repack copies the sub-blooms in order, so bytes it copies too many of one are overwritten by the next: only
    the last sub-bloom's would show, behind the buffer's end, where Engine.build_baby keeps guard bytes and raises
    when they come back changed."""
    keys, geoms = world.keys[:JOBS], GEOM_CASES[name]
    ref = geometry_ref(world, name)
    with baby_engine(world, LANES, 4, GPJ) as e:
        out = e.build_baby(world.centres(keys), GPJ, *GEOM_LIMITS, geoms, ALL, GLG, 3, fill=0xFF)
    same(out, ref, ALL, GEOM_LIMITS[2], TOTAL, geoms)


def bloom_has(bf: bytes, g: tuple, ora, x: int) -> bool:
    nb, bits, hashes = g
    xb = x.to_bytes(32, "big")
    a = ora.xxh64(xb, baby_ref.SEED)
    b = ora.xxh64(xb, a)
    for i in range(hashes):
        p = ((a + b * i) & baby_ref.M64) % bits
        if not (bf[xb[0] * nb + (p >> 3)] >> (p & 7)) & 1:
            return False
    return True


@pytest.mark.parametrize("name", list(GEOM_CASES))
def test_packed_layout(world, ora, name):
    """The same geometries through khb_build_l1_resident, each as the level-1 bloom with the limit it was sized for:
    the packed layout (with an odd byte count neighbouring sub-blooms share words), the gate beside it with 1, 2 and 3
    probes (one probe: the device image has every hi word set), the device popcounts, and the probe's answers: 1 for
    every model x below the limit, the model's bits for 20,000 random x."""
    keys = world.keys[:JOBS]
    ref = geometry_ref(world, name)
    pts = ref["points"]
    rng = random.Random(name)
    others = [rng.randrange(1, adv.P) for _ in range(20000)]
    others_be = b"".join(x.to_bytes(32, "big") for x in others)
    with baby_engine(world, LANES, 4, GPJ) as e:
        for l, (g, limit) in enumerate(zip(GEOM_CASES[name], GEOM_LIMITS)):
            lg, probes = (18, 20, 16)[l], l + 1
            assert e.build_l1_resident(world.centres(keys), GPJ, limit, *g, gate_log2=lg, gate_probes=probes) > 0
            want = ref[f"l{l + 1}"]
            differ(e.resident_read(TABLE_L1), want, f"packed L1 {g}")
            assert e.resident_popcount(TABLE_L1) == _popcount(want)
            gate = np.frombuffer(baby_ref.gate_ref(pts, limit, lg, probes), dtype="<u4").copy()
            if probes == 1:
                gate[1::2] = 0xFFFFFFFF
            got = e.resident_read(TABLE_GATE)
            differ(got, gate.tobytes(), f"gate 2^{lg} x {probes}")
            if probes == 1:
                assert (np.frombuffer(got, dtype="<u4")[1::2] == 0xFFFFFFFF).all()
            assert e.resident_popcount(TABLE_GATE) == _popcount(gate.tobytes())
            n = min(limit, TOTAL)
            assert e.probe(b"".join(pts.xb[:n])) == b"\1" * n
            assert e.probe(others_be) == bytes(bloom_has(want, g, ora, x) for x in others)


# ------------------------------------------------------------------------------------------ 4. gate
@pytest.mark.parametrize("lg", [13, 20])
def test_gate_probes(world, lg):
    """1, 2 and 3 probes through khb_build_baby, at the smallest gate (128 blocks for 1,025 x, eight x per block) and at
    2^20 bits for 18,949 x; l1ext is sized so that the model's gate is between 1 % and 80 % full (a saturated gate
    hides wrong positions).  The gate takes ic < l1ext only, while level 2 beside it takes every point."""
    keys = world.keys[:JOBS]
    limits = ({13: 1025, 20: 3 * JK + 517}[lg], TOTAL, 1)
    want = ("l1", "l2", "gate")
    with baby_engine(world, LANES, 4, GPJ) as e:
        for probes in (1, 2, 3):
            ref = world.ref(keys, GPJ, limits, G_PLAIN, lg, probes, False)
            assert 0.01 <= _popcount(ref["gate"]) / (1 << lg) <= 0.8
            out = e.build_baby(world.centres(keys), GPJ, *limits, G_PLAIN, want, lg, probes, fill=0xFF)
            same(out, ref, want, limits[2], TOTAL, G_PLAIN)
            assert out["gate"] != world.ref(keys, GPJ, (TOTAL, TOTAL, 1), G_PLAIN, lg, probes, False)["gate"]


# ------------------------------------------------------------------------------------------ 5. work shape
SHAPE_LIMITS = (TOTAL - 1, JK + 1, 3 * JK + 517)


@pytest.mark.parametrize("lanes,gpl", [(LANES, 4), (LANES, 1), (LANES, 2), (LANES, 8), (256, 4), (256, 1), (0, 4)],
                         ids=lambda v: str(v))
def test_work_shapes_give_the_same_bytes(world, lanes, gpl):
    """One input through seven shapes: 1, 2, 4 and 8 groups per lane (8: one short lane per job), one workgroup, and
    the default lanes with 10 items for a quarter of a million lanes.  Each equals the model, so all are equal."""
    keys = world.keys[:JOBS]
    ref = world.ref(keys, GPJ, SHAPE_LIMITS, G_PLAIN, GLG, 3)
    with baby_engine(world, lanes, gpl, GPJ) as e:
        if lanes == 0:
            assert e.lanes() > JOBS * GPJ
        out = e.build_baby(world.centres(keys), GPJ, *SHAPE_LIMITS, G_PLAIN, ALL, GLG, 3)
    same(out, ref, ALL, SHAPE_LIMITS[2], TOTAL, G_PLAIN)


@pytest.mark.parametrize("gpl", [1, 4])
def test_single_job(world, gpl):
    keys = world.keys[:1]
    limits = (JK, JK - 1, 1025)
    ref = world.ref(keys, GPJ, limits, G_PLAIN, GLG, 2)
    with baby_engine(world, LANES, gpl, GPJ) as e:
        out = e.build_baby(world.centres(keys), GPJ, *limits, G_PLAIN, ALL, GLG, 2)
    same(out, ref, ALL, limits[2], JK, G_PLAIN)


def test_product_centres(world):
    """The product's consecutive centres k * job_keys + 513 (key ic + 1; job 0 starts on G itself)."""
    keys = [k * JK + 513 for k in range(JOBS)]
    assert_no_degenerate_group(keys, GPJ, product=True)
    limits = (TOTAL, 3 * JK + 517, JK + 1)
    ref = world.ref(keys, GPJ, limits, G_PLAIN, GLG, 3)
    assert ref["points"].xs[:2] == [world.ora.pubkey(1).xy()[0], world.ora.pubkey(2).xy()[0]]
    with baby_engine(world, LANES, 4, GPJ) as e:
        out = e.build_baby(world.centres(keys), GPJ, *limits, G_PLAIN, ALL, GLG, 3)
    same(out, ref, ALL, limits[2], TOTAL, G_PLAIN)


def test_ragged_last_wave(world):
    """67 jobs x 3 groups at one group per lane: 201 items, three full waves and one of nine lanes."""
    keys, gpj = world.keys, 3
    assert_no_degenerate_group(keys, gpj)
    total = 67 * gpj * 1024
    limits = (total - 1025, 40 * gpj * 1024 + 1, total)
    geoms = [geom(23003, 20), geom(13999, 20), geom(40009, 20)]
    ref = world.ref(keys, gpj, limits, geoms, 20, 3)
    assert all(0.2 <= f <= 0.8 for f in ref["fill"].values()), ref["fill"]
    with baby_engine(world, LANES, 1, gpj) as e:
        out = e.build_baby(world.centres(keys), gpj, *limits, geoms, ALL, 20, 3)
    same(out, ref, ALL, limits[2], total, geoms)


def test_many_handouts_per_wave(world):
    """One workgroup (4 waves) takes 5,400 items of one group, more than 21 hand-outs of 64 per wave.  The jobs cycle
    through the 30 group centres of the other cases, so the model walks 30 groups; the bPtable takes a record of
    every one of the 5.5 million points, so an item that is skipped or walked twice shows there (and in the walked
    count behind KHB_EINCOMPLETE)."""
    n_jobs, lanes = 5400, 256
    assert n_jobs > 20 * 64 * (lanes // 64)
    centres30 = [c + 1024 * j for c in world.keys[:JOBS] for j in range(GPJ)]
    assert_no_degenerate_group(centres30, 1)
    keys = [centres30[i % 30] for i in range(n_jobs)]
    total = n_jobs * 1024
    limits = (3 * 1024 + 517, total, total)
    geoms = [geom(599, 20), geom(347, 2), None]
    want = ("l1", "l2", "bp", "gate")
    ref = world.ref(keys, 1, limits, geoms, 13, 3)
    with baby_engine(world, lanes, 1, 1) as e:
        out = e.build_baby(world.centres(keys), 1, *limits, geoms, want, 13, 3, fill=0xA5)
    same(out, ref, want, limits[2], total, geoms)


# ------------------------------------------------------------------------------------------ 6. context state
def load_bsgs_tables(e, bs, gpl: int) -> None:
    bf, nb, bits, h = bs.bloom_concat(1)
    e.load_bloom(bf, nb, bits, h)
    e.load_giant_table(bs.giant_table())
    e.load_lane_offsets(lane_offsets(bs, gpl, (bs.cycles + gpl - 1) // gpl), gpl)


@pytest.fixture(scope="module")
def bs32(ora):
    b = ora.Bsgs("0x100000000", 1)     # M = 65,536, 64 groups per chunk (tests/test_gpu_scan.py)
    yield b
    b.close()


def scan_jobs(ora, bs32):
    tgt = ora.pubkey(0x2000000000123457)
    starts = [bs32.chunk_start(0x2000000000000000 + c * (1 << 33), tgt) for c in range(4)]
    ref = sorted((j, a) for j, st in enumerate(starts) for a in bs32.scan(st, 0, bs32.cycles)[0])
    return b"".join(st.be64() for st in starts), ref


def test_scan_build_scan(world, ora, bs32):
    """scan, build_baby, the same scan on one context.  The scan's epilogue leaves slot 0's counters zero and says
    so; the build dirties them (work-item cursor, walked groups) and must take that word back, or the second scan
    starts on the build's counters: its candidates and giant_steps equal the first scan's and the oracle's."""
    centres, ref = scan_jobs(ora, bs32)
    keys = world.keys[:JOBS]
    with Engine(0, lanes=LANES) as e:
        load_bsgs_tables(e, bs32, 4)
        c1, d1, s1 = e.scan(centres, 0, bs32.cycles)
        assert sorted(c1) == ref and ref and not d1 and s1.giant_steps == 4 * bs32.cycles * 1024
        e.load_giant_table(world.raw)
        e.load_lane_offsets(world.offsets(4, GPJ), 4)
        out = e.build_baby(world.centres(keys), GPJ, *SHAPE_LIMITS, G_PLAIN, ALL, GLG, 3)
        same(out, world.ref(keys, GPJ, SHAPE_LIMITS, G_PLAIN, GLG, 3), ALL, SHAPE_LIMITS[2], TOTAL, G_PLAIN)
        load_bsgs_tables(e, bs32, 4)
        c2, d2, s2 = e.scan(centres, 0, bs32.cycles)
        assert sorted(c2) == ref and not d2 and (s2.n_cand, s2.giant_steps) == (s1.n_cand, s1.giant_steps)


def code_of(call) -> int:
    with pytest.raises(KhbError) as err:
        call()
    return err.value.code


def test_refused_calls_leave_the_resident_tables(world):
    """KHB_EINVAL for a bits / bytes pair that does not match, hashes = 0, gate_log2 = 12, four probes and (resident)
    l1ext = 0, from both build calls: the refusals come before anything is dropped, so a resident level-1 bloom and
    gate installed before stay readable and unchanged."""
    keys = world.keys[:JOBS]
    c = world.centres(keys)
    g = G_PLAIN[0]
    bad = [dict(g=(g[0], g[1] + 8, g[2])), dict(g=(g[0], g[1], 0)), dict(lg=12), dict(probes=4)]
    with baby_engine(world, LANES, 4, GPJ) as e:
        e.build_l1_resident(c, GPJ, TOTAL, *g, gate_log2=13, gate_probes=3)
        before = e.resident_read(TABLE_L1), e.resident_read(TABLE_GATE)
        differ(before[0], world.ref(keys, GPJ, (TOTAL, 1, 1), [g, None, None], 13, 3, False)["l1"], "resident L1")
        for b in bad:
            gg, lg, probes = b.get("g", g), b.get("lg", 13), b.get("probes", 3)
            assert code_of(lambda: e.build_l1_resident(c, GPJ, TOTAL, *gg, gate_log2=lg, gate_probes=probes)) == \
                khbsgs.KHB_EINVAL, b
            assert code_of(lambda: e.build_baby(c, GPJ, TOTAL, 1, 1, [gg, None, None], ("l1", "gate"), lg, probes)) == \
                khbsgs.KHB_EINVAL, b
            assert (e.resident_read(TABLE_L1), e.resident_read(TABLE_GATE)) == before
        assert code_of(lambda: e.build_l1_resident(c, GPJ, 0, *g, gate_log2=13, gate_probes=3)) == khbsgs.KHB_EINVAL
        assert (e.resident_read(TABLE_L1), e.resident_read(TABLE_GATE)) == before
        assert e.resident_popcount(TABLE_L1) == _popcount(before[0])


def test_state_and_busy_refusals(world, ora, bs32):
    """KHB_ESTATE from both build calls while no lane offsets are loaded; KHB_EBUSY from both while a submission is
    pending, which is then collected whole."""
    keys = world.keys[:JOBS]
    c, g = world.centres(keys), G_PLAIN[0]
    centres, ref = scan_jobs(ora, bs32)
    with Engine(0, lanes=LANES) as e:
        e.load_giant_table(world.raw)
        assert code_of(lambda: e.build_baby(c, GPJ, TOTAL, 1, 1, [g, None, None], ("l1",))) == khbsgs.KHB_ESTATE
        assert code_of(lambda: e.build_l1_resident(c, GPJ, TOTAL, *g)) == khbsgs.KHB_ESTATE
        load_bsgs_tables(e, bs32, 4)
        e.submit(centres, 0, bs32.cycles)
        try:
            assert code_of(lambda: e.build_baby(c, GPJ, TOTAL, 1, 1, [g, None, None], ("l1",))) == khbsgs.KHB_EBUSY
            assert code_of(lambda: e.build_l1_resident(c, GPJ, TOTAL, *g)) == khbsgs.KHB_EBUSY
        finally:
            cands, degen, st = e.collect()
        assert sorted(cands) == ref and not degen and st.giant_steps == 4 * bs32.cycles * 1024
