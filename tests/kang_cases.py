"""Directed herds for the kangaroo walk's step rule, for any jump table (test infrastructure).

Plain Python on tests/kangaroo_ref.py (the model of the step rule) and tests/adversarial.py (curve arithmetic and the
finders of the field classes A, B, C, D and Y); nothing here imports the library under test.  A jump table is
[(s_j, (x_j, y_j))] as everywhere; a kangaroo is (x, y, d).

  fixed_table    a table with J_j.x & 31 == j for every j, so a kangaroo at +-J_j takes the second choice for every j,
                 the wrap 31 -> 0 included
  predecessors   the points from which one step arrives exactly at a chosen point
  arriving, dp_points, near_jump
                 start points whose first step lands on a field-class point, on an x whose word 1 is at an edge of the
                 distinguished-point test, or whose dx = J_j.x - x is tiny or just below p
  edge_herd      one herd of about 2 L + 5 kangaroos that holds all of them in one lane and in the partial last lane
  cheap_herd, trajectory
                 a large herd for one point addition per kangaroo, and the model's states step by step, which the tests
                 of stores, reads, growth and queued launches cut their expectations from
"""
from __future__ import annotations

import random

from tests import adversarial as adv
from tests import kangaroo_ref as kr

P = adv.P
CLASSES = "ABCDY"
CLASS_POINTS = 8                       # class points tried per class; at least MIN_REACHABLE must have a predecessor
MIN_REACHABLE = 3
DP_WORDS = (0, 0x80000000, 1, 0xFFFF0000)           # word 1 of the x a dp_points start arrives at
CARRY_DISTANCES = ((1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1, (1 << 224) - 1, (1 << 256) - 1, 1 << 255)


def fixed_table(first: int = 1001):
    """32 jumps with J_j.x & 31 == j and distinct x: k * G walked upward from k = first, the first hit per residue."""
    out = [None] * kr.NJ
    k, pt = first, kr.mul(first)
    while any(e is None for e in out):
        j = pt[0] & 31
        if out[j] is None:
            out[j] = (k, pt)
        k, pt = k + 1, adv.add(pt, kr.G)
    assert len({x for _, (x, _) in out}) == kr.NJ
    return out


def predecessors(jumps, target):
    """All (j, S) with S = target - J_j and pick(S.x) == (j, False): one step from S arrives exactly at target."""
    out = []
    for j, (_, J) in enumerate(jumps):
        s = adv.add(target, adv.neg(J))
        if s is not None and kr.pick(jumps, s[0]) == (j, False):
            out.append((j, s))
    return out


def arriving(jumps, cls: str, n: int = CLASS_POINTS, seed: int = 3):
    """[(start, target)]: for each of adv.class_points(cls, n, seed) that has a predecessor, its first one.  A target
    has one with probability 1 - (31/32)^32 = 0.64."""
    out = []
    for target in adv.class_points(cls, n, seed):
        pre = predecessors(jumps, target)
        if pre:
            out.append((pre[0][1], target))
    return out


def dp_points(jumps, seed: int = 5):
    """[(word, start, target)] for word in DP_WORDS: target is a curve point whose x has word 1 == word (a random x
    with that word forced, lifted) and start a predecessor of it."""
    rng = random.Random(f"dp{seed}")
    out = []
    for word in DP_WORDS:
        while True:
            x = rng.randrange(P) & ~(0xFFFFFFFF << 32) | (word << 32)
            target = adv.lift_x(x, rng.randrange(2)) if x < P else None
            pre = predecessors(jumps, target) if target else []
            if pre:
                out.append((word, pre[0][1], target))
                break
    return out


def near_jump(jumps, j: int, sign: int):
    """(point, dx): a curve point next to J_j.x that picks jump j, dx = J_j.x - x mod p.  sign > 0: x below J_j.x, so
    dx = 32 t + e is tiny; sign < 0: x above it, so dx = p - (32 t + e') is just below p; t >= 1 the smallest with x
    on the curve.  e = (J_j.x - j) mod 32 and e' = (-e) mod 32 keep x & 31 == j; with fixed_table() both are 0 and
    x = J_j.x -+ 32 t."""
    jx = jumps[j][1][0]
    e = (jx - j) % 32
    t = 1
    while True:
        x = jx - e - 32 * t if sign > 0 else jx + (-e) % 32 + 32 * t
        assert 0 <= x < P
        pt = adv.lift_x(x, t & 1)
        if pt is not None and kr.pick(jumps, x) == (j, False):
            return pt, (jx - x) % P
        t += 1


def cheap_herd(n: int, seed: int):
    """n kangaroos (d0 + i * s) * G with random 64-bit d0 and 40-bit s: one point addition each."""
    rng = random.Random(f"herd{seed}")
    d, s = rng.randrange(1 << 63, 1 << 64), rng.randrange(1 << 39, 1 << 40)
    pt, inc = kr.mul(d), kr.mul(s)
    herd = []
    for _ in range(n):
        herd.append((pt[0], pt[1], d))
        pt, d = adv.add(pt, inc), d + s
    return herd


def trajectory(jumps, herd, steps: int):
    """(states, seconds): states[t] is the herd after t steps (states[0] the herd itself), seconds[t][i] whether
    kangaroo i took the second choice in step t + 1.  kr.step is what kr.walk runs, kangaroo by kangaroo."""
    states, seconds = [list(herd)], []
    for _ in range(steps):
        moved = [kr.step(jumps, roo) for roo in states[-1]]
        states.append([m[0] for m in moved])
        seconds.append([m[1] for m in moved])
    return states, seconds


def points_of(states, t0: int, t1: int, dp: int, n: int | None = None):
    """The distinguished points [(i, x, d)] of steps t0 + 1 .. t1 of the first n kangaroos, in kr.walk's order."""
    return [(i, x, d) for t in range(t0 + 1, t1 + 1) for i, (x, _, d) in enumerate(states[t][:n]) if kr.is_dp(x, dp)]


def edge_herd(jumps, per_lane: int, seed: int = 7):
    """(herd, marks): a herd of 2 L + 5 kangaroos (more lanes when L is too small for the list) whose lane 1 holds,
    from its first slot on, every directed start and whose partial last lane holds five more; the rest is random.
    marks: {name: [indices]} with the names "class" (points of classes A B C D Y as start points), "arriving:<cls>",
    "near" (near_jump for j in {0, 31}, both signs), "jump" (+-J_j for j in {0, 30, 31}), "dp:<word>" and "carry"
    (the distances of CARRY_DISTANCES).  Every arriving class must have MIN_REACHABLE starts."""
    L = per_lane
    rng = random.Random(f"edge{seed}")
    special, marks = [], {}

    def put(name, pt, d=None):
        marks.setdefault(name, []).append(len(special))
        special.append((pt[0], pt[1], rng.randrange(1, 1 << 64) if d is None else d))

    for cls in CLASSES:
        for pt in adv.class_points(cls, 2, seed):
            put("class", pt)
    extra = []
    for cls in CLASSES:
        arr = arriving(jumps, cls)
        assert len(arr) >= MIN_REACHABLE, (cls, len(arr))
        for start, _ in arr[:MIN_REACHABLE]:
            put(f"arriving:{cls}", start)
        extra.append(arr[-1][0])
    for j in (0, 31):
        for sign in (+1, -1):
            put("near", near_jump(jumps, j, sign)[0])
    for j in (0, 30, 31):
        J = jumps[j][1]
        put("jump", J)
        put("jump", adv.neg(J))
    dps = dp_points(jumps)
    for word, start, _ in dps:
        put(f"dp:{word:#x}", start)
    lanes = 2 + max(0, (len(special) - 1) // L)          # full lanes: lane 0 random, the directed ones from lane 1 on
    n = lanes * L + 5
    herd = cheap_herd(n, seed)
    marks = {k: [L + i for i in v] for k, v in marks.items()}
    herd[L:L + len(special)] = special
    # the partial last lane: the wrap's kangaroo, a tiny dx, a class-B arrival, a 32-bit distinguished point, and
    # one random kangaroo
    last = n - 5
    tail = [("jump", adv.neg(jumps[31][1])), ("near", near_jump(jumps, 0, +1)[0]), ("arriving:B", extra[1]),
            ("dp:0x0", dps[0][1])]
    for k, (name, pt) in enumerate(tail):
        herd[last + k] = (pt[0], pt[1], rng.randrange(1, 1 << 64))
        marks[name].append(last + k)
    # distances whose add carries through 1, 2, 4, 7 and all 8 words (the last wraps mod 2^256), and 2^255: on random
    # kangaroos of lane 0, on directed ones of lane 1 and in the last lane
    at = [1, 2, 3, 4, 5, 6, L + 1, L + len(special) - 1, n - 1, n - 5, marks["jump"][0], marks["arriving:A"][0]]
    marks["carry"] = at
    for k, i in enumerate(at):
        herd[i] = (herd[i][0], herd[i][1], CARRY_DISTANCES[k % len(CARRY_DISTANCES)])
    assert all(adv.on_curve((x, y)) and 0 <= d < 1 << 256 for x, y, d in herd)
    return herd, marks
