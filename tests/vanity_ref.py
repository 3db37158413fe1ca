"""The tests' own model of -m vanity, independent of the C++: Base58Check with hashlib, the match rule (the printed
address begins with the target) and the interval rule.

Interval rule: a target s of z >= 1 '1' characters followed by the digits r gives, for every address length L, the
interval from s padded to L with '1' to s padded to L with 'z', intersected with the 25-byte values that have exactly
z leading zero bytes, [2^(8(24-z)), 2^(8(25-z)) - 1], both ends shifted right by 32 bits (the checksum), kept when not
empty.  A target of '1' characters alone is also the prefix of every address with more leading '1's, so the exact-z
cut would lose matches (interval_ends' e - 1 below the lowest interval of "1" still begins with "1"); for such a
target the cut is "at least z leading zero bytes", [0, 2^(8(25-z)) - 1]."""
from __future__ import annotations

import bisect
import hashlib

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def b58check(payload: bytes) -> str:
    d = payload + hashlib.sha256(hashlib.sha256(payload).digest()).digest()[:4]
    zeros = len(d) - len(d.lstrip(b"\0"))
    v, s = int.from_bytes(d, "big"), ""
    while v:
        v, r = divmod(v, 58)
        s = B58[r] + s
    return "1" * zeros + s


def address(h: bytes | int) -> str:
    if isinstance(h, int):
        h = h.to_bytes(20, "big")
    return b58check(b"\0" + h)


def value(s: str) -> int:
    v = 0
    for c in s:
        v = v * 58 + B58.index(c)
    return v


def intervals_of(s: str) -> list[tuple[int, int]]:
    """The closed intervals of hash160 values (as integers) of one target; [] when it is not accepted."""
    if not 1 <= len(s) <= 29 or s[0] != "1" or any(c not in B58 for c in s):
        return []
    z = len(s) - len(s.lstrip("1"))
    if z > 25:
        return []
    all_ones = z == len(s)
    bottom = 0 if all_ones else 1 << 8 * (24 - z) if z <= 24 else None
    top = (1 << 8 * (25 - z)) - 1
    if bottom is None:
        return []
    out = []
    for L in range(len(s), 37):
        lo, hi = value(s + "1" * (L - len(s))), value(s + "z" * (L - len(s)))
        lo, hi = max(lo, bottom), min(hi, top)
        if lo <= hi:
            out.append((lo >> 32, hi >> 32))
    return out


def merged(targets) -> list[tuple[int, int]]:
    """All targets' intervals sorted, disjoint, touching ones joined."""
    iv = sorted(i for t in targets for i in intervals_of(t))
    out: list[list[int]] = []
    for lo, hi in iv:
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(a, b) for a, b in out]


class Table:
    """Range membership in a merged table, by bisection (the linear scan's answer)."""

    def __init__(self, intervals):
        self.iv = list(intervals)
        self.los = [a for a, _ in self.iv]

    def __contains__(self, h) -> bool:
        if not isinstance(h, int):
            h = int.from_bytes(h, "big")
        i = bisect.bisect_right(self.los, h) - 1
        return i >= 0 and h <= self.iv[i][1]


def startswith_any(h, targets) -> bool:
    a = address(h)
    return any(a.startswith(t) for t in targets)


def b20(v: int) -> bytes:
    return v.to_bytes(20, "big")


# ---- directed inputs for the device match (tests/test_gpu_vanity.py) and its host build (tests/test_native_vanity.py)
TABLE_SIZES = (1, 2, 3, 1000, 1537)     # the binary search's small and non-power-of-two shapes
TOP = (1 << 160) - 1


def random_table(R: int, rng) -> list[tuple[int, int]]:
    """R sorted, disjoint intervals of mixed widths: single values, narrower than a 16-bit bucket, half a gap, up to
    one short of the next interval and touching it; from R = 2 the first starts at 0 and from R = 3 the last ends at
    2^160 - 1 (buckets 0x0000 and 0xffff)."""
    a = sorted(rng.sample(range(1 << 40), R))
    a = [(v << 120) | rng.getrandbits(120) for v in a]
    if R >= 2:
        a[0] = 0
    out = []
    for i, lo in enumerate(a):
        gap = (a[i + 1] if i + 1 < R else TOP + 1) - lo
        kind = i % 5
        width = (0, rng.getrandbits(100), gap // 2, gap - 2, gap - 1)[kind]
        out.append((lo, lo + min(width, gap - 1)))
    if R >= 3:
        out[-1] = (out[-1][0], TOP)
    if R == 1:
        lo = (0x1234 << 144) | rng.getrandbits(140)
        out = [(lo, lo + rng.getrandbits(130))]
    return out


def probe_values(iv, rng, n_random: int = 3000) -> list[int]:
    vals = []
    for lo, hi in iv:
        vals += [lo - 1, lo, hi, hi + 1]
        vals.append((lo & ~0xFF) | ((lo + 0x5A) & 0xFF))            # only the last byte changed
        vals.append((lo & ~0xFFFFFFFF) | ((lo ^ 0x9E3779B1) & 0xFFFFFFFF))   # only the last word changed
        for b in {lo >> 144, hi >> 144}:
            vals += [b << 144, (b << 144) | rng.getrandbits(144), (b << 144) | ((1 << 144) - 1)]    # its buckets
            vals += [((b - 1) << 144) | rng.getrandbits(144), ((b + 1) << 144) | rng.getrandbits(144)]   # neighbours
    for b in (0, 0xFFFF):
        vals += [(b << 144) | rng.getrandbits(144) for _ in range(50)]
    vals += [0, TOP]
    vals += [rng.getrandbits(160) for _ in range(n_random)]
    return [v for v in vals if 0 <= v <= TOP]
