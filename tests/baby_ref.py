"""A model of the baby-step table build (khb_build_baby / khb_build_l1_resident, device/baby_point.hpp), test
infrastructure.  It restates what the build must write from include/khbsgs.h alone:

  * the walked point (job, j, t) is (centre_key[job] - 512 + 1024 j + t) * G with ic = job * groups_per_job * 1024 +
    1024 j + t; its x comes from curve arithmetic on Python integers, stepping by G from ora.pubkey of the run's first
    key (walk_xs: adversarial.add, or the same affine addition with the inverses of many runs taken in one batch);
  * bloom level l holds, for ic < limit[l], bits ((a + b i) mod 2^64) mod bits, i < hashes, of sub-bloom x >> 248, with
    a = xxh64(x_be32, seed) and b = xxh64(x_be32, a) by ora.xxh64 (pinned to the Python xxhash in
    tests/test_oracle_pins.py), bit p at bit p & 7 of byte p >> 3;
  * the bPtable record of ic < m3 is x bytes 16..21, two zero bytes and ic as 8 little-endian bytes at 16 ic;
  * the gate holds tests/helpers.gate_bits of every x with ic < l1ext.

256 sub-blooms of bytes_per_sub bytes back to back are one byte string whose bit sub * bytes_per_sub * 8 + p is bit p
of sub-bloom sub, so the concatenation khb_build_baby returns and the packed layout khb_build_l1_resident writes are
the same bytes.  tests/test_baby_ref_cpu.py pins the model to the CPU-built tables and to the oracle."""
from __future__ import annotations

import numpy as np

from tests import adversarial as adv
from tests.helpers import gate_bits

P, N = adv.P, adv.N
SEED = 0x59F2815B16F81798
M64 = 2**64 - 1
GROUP = 1024
CHAINS = 512          # runs stepped side by side in walk_xs, their inverses taken in one batch

_G = None
_runs: dict = {}      # (first key, count) -> Run, shared by every model of a test session


def generator(ora):
    global _G
    if _G is None:
        _G = ora.pubkey(1).xy()
    return _G


def walk_slow(ora, key0: int, count: int) -> list:
    """x of key0 * G, (key0 + 1) * G, ...: adversarial.add stepping by G from ora.pubkey(key0)."""
    g, pt, out = generator(ora), ora.pubkey(key0).xy(), []
    for _ in range(count):
        out.append(pt[0])
        pt = adv.add(pt, g)
    return out


def walk_xs(ora, key0: int, count: int) -> list:
    """The same list as walk_slow.  The count keys are cut into up to CHAINS runs, each anchored by ora.pubkey at its
    first key and stepped by G with adversarial.add's formulas; one step of all runs shares one modular inversion
    (the product of the dx, inverted once and unrolled).  A step with a zero dx (a run standing on +-G) is done with
    adversarial.add itself."""
    if count <= 2 * CHAINS:
        return walk_slow(ora, key0, count)
    gx, gy = g = generator(ora)
    length = -(-count // CHAINS)
    starts = list(range(0, count, length))
    pts = [ora.pubkey(key0 + s).xy() for s in starts]
    cols = [[] for _ in starts]
    for step in range(length):
        for c, pt in zip(cols, pts):
            c.append(pt[0])
        if step == length - 1:
            break
        dx =[(gx - pt[0]) % P for pt in pts]
        if not all(dx):
            pts = [adv.add(pt, g) for pt in pts]
            continue
        pre, acc = [], 1
        for d in dx:
            pre.append(acc)
            acc = acc * d % P
        acc = pow(acc, -1, P)
        nxt = [None] * len(pts)
        for i in range(len(pts) - 1, -1, -1):
            x1, y1 = pts[i]
            s = (gy - y1) * (acc * pre[i] % P) % P
            acc = acc * dx[i] % P
            x3 = (s * s - x1 - gx) % P
            nxt[i] = (x3, (s * (x1 - x3) - y1) % P)
        pts = nxt
    return [x for c in cols for x in c][:count]


class Run:
    """count consecutive keys from key0: x, its bytes and the two hashes of every point."""

    def __init__(self, ora, key0: int, count: int):
        assert 0 < key0 % N and key0 % N + count <= N, "a walked key is 0 mod n"
        self.xs = walk_xs(ora, key0 % N, count)
        self.xb = [x.to_bytes(32, "big") for x in self.xs]
        a = [ora.xxh64(b, SEED) for b in self.xb]
        self.a = np.array(a, dtype=np.uint64)
        self.b = np.array([ora.xxh64(b, s) for b, s in zip(self.xb, a)], dtype=np.uint64)
        self.sub = np.array([b[0] for b in self.xb], dtype=np.uint64)


def run_of(ora, key0: int, count: int) -> Run:
    r = _runs.get((key0, count))
    if r is None:
        r = _runs[key0, count] = Run(ora, key0, count)
    return r


class Points:
    """Every walked point of a build in ic order: job k walks the groups_per_job * 1024 keys from centre_keys[k] - 512.
    Jobs with the same centre share one Run."""

    def __init__(self, ora, centre_keys, groups_per_job: int):
        self.centre_keys, self.groups_per_job = list(centre_keys), groups_per_job
        self.job_keys = groups_per_job * GROUP
        self.total = self.job_keys * len(self.centre_keys)
        runs = [run_of(ora, c - 512, self.job_keys) for c in self.centre_keys]
        self.xs = [x for r in runs for x in r.xs]
        self.xb = [b for r in runs for b in r.xb]
        self.a = np.concatenate([r.a for r in runs])
        self.b = np.concatenate([r.b for r in runs])
        self.sub = np.concatenate([r.sub for r in runs])


def bloom_positions(a: int, b: int, bits: int, hashes: int) -> list:
    """bloom_add's bit positions of one x on Python integers."""
    return [((a + b * i) & M64) % bits for i in range(hashes)]


def bloom_level(pts: Points, limit: int, geom) -> bytes:
    """256 sub-blooms of geom = (bytes_per_sub, bits, hashes) back to back, holding every point with ic < limit.
    bloom_positions over numpy uint64 (a + b i wraps mod 2^64 there as it must)."""
    nb, bits, hashes = geom
    assert nb == (bits + 7) // 8
    n = min(limit, pts.total)
    flags = np.zeros(256 * nb * 8, dtype=np.uint8)
    a, b, base = pts.a[:n], pts.b[:n], pts.sub[:n] * np.uint64(nb * 8)
    with np.errstate(over="ignore"):
        for i in range(hashes):
            flags[(base + (a + b * np.uint64(i)) % np.uint64(bits)).astype(np.intp)] = 1
    return np.packbits(flags, bitorder="little").tobytes()


def bloom_level_slow(pts: Points, limit: int, geom) -> bytes:
    """bloom_level on Python integers alone."""
    nb, bits, hashes = geom
    out = bytearray(256 * nb)
    for ic in range(min(limit, pts.total)):
        for p in bloom_positions(int(pts.a[ic]), int(pts.b[ic]), bits, hashes):
            out[pts.xb[ic][0] * nb + (p >> 3)] |= 1 << (p & 7)
    return bytes(out)


def bp_records_slow(pts: Points, m3: int) -> bytes:
    """The records the build writes: those of ic < min(m3, total), at 16 ic."""
    return b"".join(pts.xb[ic][16:22] + b"\0\0" + ic.to_bytes(8, "little") for ic in range(min(m3, pts.total)))


def bp_records(pts: Points, m3: int) -> bytes:
    """bp_records_slow, the bytes laid out with numpy."""
    n = min(m3, pts.total)
    rec = np.zeros((n, 16), dtype=np.uint8)
    rec[:, :6] = np.frombuffer(b"".join(pts.xb[:n]), dtype=np.uint8).reshape(n, 32)[:, 16:22]
    rec[:, 8:] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    return rec.tobytes()


def gate_ref(pts: Points, limit: int, gate_log2: int, probes: int) -> bytes:
    out = bytearray((1 << gate_log2) // 8)
    for x in pts.xs[:min(limit, pts.total)]:
        for p in gate_bits(gate_log2, probes, x):
            out[p >> 3] |= 1 << (p & 7)
    return bytes(out)


def baby_build_ref(ora, centre_keys, groups_per_job: int, l1ext: int, m2: int, m3: int, geoms, gate_log2: int = 0,
                   gate_probes: int = 0, want_bp: bool = False, pts: Points | None = None) -> dict:
    """What one build writes.  centre_keys: the centre key of every job; the four limits are l1ext, m2, m3 and the
    gate's, which is l1ext; geoms: (bytes_per_sub, bits, hashes) of levels 1..3, None for a level that is not built;
    gate_log2 0 = no gate.  pts: the Points of (centre_keys, groups_per_job) when the caller already has them.
    Returns {"l1", "l2", "l3", "gate", "bp": bytes or None, "fill": the set fraction of all bits of each built level,
    "subs": per level the sub-blooms that received a point, "points": the Points}.  "bp" is the records of
    ic < min(m3, total) alone: the build writes nothing else."""
    if pts is None:
        pts = Points(ora, centre_keys, groups_per_job)
    assert pts.centre_keys == list(centre_keys) and pts.groups_per_job == groups_per_job
    out = {"points": pts, "fill": {}, "subs": {}, "gate": None, "bp": None}
    for name, limit, geom in zip(("l1", "l2", "l3"), (l1ext, m2, m3), geoms):
        out[name] = None
        if geom is not None:
            bf = out[name] = bloom_level(pts, limit, geom)
            out["fill"][name] = int.from_bytes(bf, "little").bit_count() / (256 * geom[1])
            out["subs"][name] = {int(s) for s in np.unique(pts.sub[:min(limit, pts.total)])}
    if gate_log2:
        out["gate"] = gate_ref(pts, l1ext, gate_log2, gate_probes)
    if want_bp:
        out["bp"] = bp_records(pts, m3)
    return out
