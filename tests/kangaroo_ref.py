"""Python model of the kangaroo walk's step rule (device/kangaroo.hpp) on big integers, built on
tests/adversarial.py's point addition, and a model of the whole search for small intervals.

A herd is a list of (x, y, d); jumps are [(s_j, (x_j, y_j))] with (x_j, y_j) = s_j * G.  Kangaroo i is tame for even i
(its point is d * G) and wild for odd i (Q + d * G).
"""
from __future__ import annotations

import random

from tests import adversarial as adv

NJ = 32
M256 = (1 << 256) - 1
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)


def mul(k: int, pt=G):
    """k * pt by double and add; None is the point at infinity."""
    r = None
    while k:
        if k & 1:
            r = adv.add(r, pt)
        pt = adv.add(pt, pt)
        k >>= 1
    return r


def pick(jumps, x: int) -> tuple[int, bool]:
    """The jump of a kangaroo at x, and whether the x == J_j.x rule chose it."""
    j = x & 31
    if jumps[j][1][0] == x:
        return (j + 1) & 31, True
    return j, False


def is_dp(x: int, dp: int) -> bool:
    return ((x >> 32) & ((1 << dp) - 1)) == 0


def step(jumps, roo):
    """One jump of (x, y, d): the new (x, y, d) and whether the second choice was taken."""
    x, y, d = roo
    j, second = pick(jumps, x)
    s, J = jumps[j]
    p = adv.add((x, y), J)
    assert p is not None
    return (p[0], p[1], (d + s) & M256), second


def walk(jumps, herd, steps: int, dp: int):
    """`steps` jumps of every kangaroo: (final herd, [(i, x, d)] in the order met: step by step, ascending i,
    second choices)."""
    herd = list(herd)
    dps, seconds = [], 0
    for _ in range(steps):
        for i, roo in enumerate(herd):
            herd[i], sec = step(jumps, roo)
            seconds += sec
            if is_dp(herd[i][0], dp):
                dps.append((i, herd[i][0], herd[i][2]))
    return herd, dps, seconds


def random_herd(n: int, seed: int, q=None, bits: int = 64):
    """n kangaroos with random distances below 2^bits: d * G for even i, q + d * G for odd i (q = None: all tame
    points, which is all the step rule sees)."""
    rng = random.Random(seed)
    herd = []
    for i in range(n):
        d = rng.randrange(1, 1 << bits)
        p = mul(d)
        if q is not None and i & 1:
            p = adv.add(q, p)
        herd.append((p[0], p[1], d))
    return herd


def solve_model(jumps, herd, pub, start: int, dp: int, max_steps: int):
    """The search on the model alone, without replacing merged kangaroos: the key, or None within max_steps jumps in
    all, and the jumps made."""
    table = {}
    herd = list(herd)
    made = 0
    while made + len(herd) <= max_steps:
        for i, roo in enumerate(herd):
            herd[i], _ = step(jumps, roo)
            x, _, d = herd[i]
            if not is_dp(x, dp):
                continue
            kind = i & 1
            if x in table and table[x][0] != kind:
                dt, dw = (table[x][1], d) if kind else (d, table[x][1])
                for c in ((dt - dw) % adv.N, (-dt - dw) % adv.N):
                    key = (start + c) % adv.N
                    if key and mul(key) == pub:
                        return key, made + i + 1
            table.setdefault(x, (kind, d))
        made += len(herd)
    return None, made
