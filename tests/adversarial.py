"""Directed inputs for the rare-carry, canonicalisation and degenerate paths (test infrastructure).

Four things live here, all on Python integers (P, K, limbs, value come from tests/field_model.py):

  * secp256k1 affine arithmetic and finders of curve points whose x (or y) falls in a class that the
    lazy field arithmetic of csrc/device/fe_asm.hpp treats specially;
  * the limb-level model of that arithmetic by the names its users know (MODEL, m_mul .. m_canon, flags): thin
    names over tests/field_model.py, which holds the model of the header as it computes today and the integer
    definition of every raw lazy value.  The model chooses operands, certifies that each one arithmetically
    requires the branch it is aimed at, and is what the raw-mode GPU tests compare the device's value with;
    field_model.check pins it to the integers;
  * planting: start points such that a chosen step of a chosen group of the walk lands on a chosen point,
    the reference's rule for a group's centre, a reference of one -m address group from a centre (degenerate
    groups included) and of one launch of a job as the library splits it over lanes;
  * second_check_ref: bsgs_secondcheck / bsgs_thirdcheck with a report of what each of the 32 slots of every
    batch did (tests/check_cases.py holds the directed cases that use it).
"""
from __future__ import annotations

import random

from tests.field_model import EXACT, K, M32, P, device, limbs, value  # noqa: F401
from tests.field_model import canon as m_canon, propagate as _propagate  # noqa: F401

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GROUP = 1024
HALF = 512

# ---------------------------------------------------------------------------------- curve arithmetic


def inv(a: int) -> int:
    """The inverse mod p, and 0 for 0 as the reference's ModInv (a^(p-2))."""
    a %= P
    return pow(a, -1, P) if a else 0


def on_curve(pt) -> bool:
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - x * x * x - 7) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def add(p1, p2):
    """Affine addition; None is the point at infinity."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    x1, y1 = p1
    x2, y2 = p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        s = 3 * x1 * x1 * inv(2 * y1) % P
    else:
        s = (y2 - y1) * inv(x2 - x1) % P
    x3 = (s * s - x1 - x2) % P
    return x3, (s * (x1 - x3) - y1) % P


def sqrt(v: int):
    """v^((p+1)/4) (p = 3 mod 4), or None when v is no square."""
    r = pow(v % P, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def cbrt(a: int):
    """a^((p+2)/9) (p = 7 mod 9: its cube is a^((p-1)/3) * a), or None when a is no cube."""
    r = pow(a % P, (P + 2) // 9, P)
    return r if pow(r, 3, P) == a % P else None


def lift_x(x: int, odd: int = 0):
    y = sqrt(x * x * x + 7)
    if y is None:
        return None
    return (x, y if (y & 1) == odd else P - y)


# ------------------------------------------------------------------------------------- point finders
# class A: x < K                  the lazy product leaves the reduction as x + p (top word ffffffff)
# class B: K <= x < K + 2^40      the reduction's rare branch and its fold of a wrap past 2^256
# class C: x mod 2^96 < 2^33      the rare branch (carry out of limb 2 of the second fold)
# class D: 2^256 - 2^224 <= x < p top word ffffffff with a canonical value
# class Y: y < K

def in_class(cls: str, pt) -> bool:
    x, y = pt
    if cls == "A":
        return x < K
    if cls == "B":
        return K <= x < K + 2**40
    if cls == "C":
        return x % 2**96 < 2**33 and x >= K + 2**40
    if cls == "D":
        return 2**256 - 2**224 <= x < P
    if cls == "Y":
        return y < K
    raise ValueError(cls)


def class_values(cls: str, seed: int = 0):
    """An endless stream of field values (not necessarily x of a point) of class A, B, C or D."""
    rng = random.Random(f"{cls}{seed}")
    i = 0
    while True:
        if cls == "A":
            v = i if i < 64 else rng.randrange(K)
        elif cls == "B":
            v = K + i if i < 64 else K + rng.randrange(2**40)
        elif cls == "C":
            v = (rng.randrange(1, 2**160) << 96) | rng.randrange(2**33)
        elif cls == "D":
            v = P - 1 - i if i < 64 else (M32 << 224) | rng.randrange(2**224)
        else:
            raise ValueError(cls)
        i += 1
        if v < P:
            yield v


def class_points(cls: str, n: int, seed: int = 0) -> list:
    """n distinct curve points of the class, the same for the same seed."""
    out = []
    if cls == "Y":
        y = 0
        while len(out) < n:
            x = cbrt(y * y - 7)
            if x is not None:
                out.append((x, y))
            y += 1
        return out
    seen = set()
    for k, v in enumerate(class_values(cls, seed)):
        if v in seen:
            continue
        seen.add(v)
        pt = lift_x(v, k & 1)
        if pt is not None:
            out.append(pt)
            if len(out) == n:
                return out


# ------------------------------------------------ the limb-level model of device/fe_asm.hpp, by its old names
# tests/field_model.py holds the model (device) and the integer definition of every raw value (lazy).

def _product_op(op: int):
    def model(a: int, b: int = 0):
        r, f = device(op, a, b)
        return r, f["c3"], f["wrap"]
    return model


m_mul, m_sqr, m_sqr_add = _product_op(0), _product_op(1), _product_op(6)


def m_sub(a: int, b: int):
    """fm_sub(a < 2^256, b < p) -> (value, sub_b2)."""
    r, f = device(3, a, b)
    return r, f["sub_b2"]


def m_add_lazy(a: int, b: int):
    """fm_add_lazy(a < p, b < 2^256) -> (value, lazy_c2)."""
    r, f = device(5, a, b)
    return r, f["lazy_c2"]


# field self-test op numbers (include/khbsgs.h khb_field_op) -> model
MODEL = {0: m_mul, 1: m_sqr, 3: m_sub, 5: m_add_lazy, 6: m_sqr_add}


def flags(op: int, a: int, b: int) -> dict:
    r = MODEL[op](a, b)
    if op in (0, 1, 6):
        return {"c3": r[1], "wrap": r[2]}
    return {"sub_b2": r[1]} if op == 3 else {"lazy_c2": r[1]}


def random_operands(op: int, rng: random.Random):
    """An ordinary operand pair within the op's contract (fe_asm.hpp)."""
    if op in (0, 1):
        return rng.randrange(2**256), rng.randrange(2**256)
    if op == 3:
        return rng.randrange(2**256), rng.randrange(P)
    if op == 5:
        return rng.randrange(P), rng.randrange(2**256)
    return rng.randrange(2**256), rng.randrange(2**256)


# --------------------------------------------------------------------------------- operand generators

def directed_operands(op: int, flag: str, n: int, seed: int = 0) -> list:
    """n operand pairs (a, b) of op that need the branch `flag` by the model.  Candidates are built so that
    the exact result has the shape the branch fires on and kept only when the model's flag is set."""
    rng = random.Random(f"{op}{flag}{seed}")
    out = []
    if op in (0, 1, 6):
        vals = class_values("B" if flag == "wrap" else "C", seed)
        while len(out) < n:
            v = next(vals)
            if op == 0:
                a = rng.randrange(1, P)
                if rng.random() < 0.25:
                    a = P + rng.randrange(1, K)     # a lazy operand >= p
                b = v * inv(a) % P
            elif op == 1:
                a = sqrt(v)
                if a is None:
                    continue
                a, b = (P - a if rng.random() < 0.5 else a), 0
            else:
                b = rng.randrange(2**256)
                a = sqrt(v - b)
                if a is None:
                    continue
            if flags(op, a, b)[flag] and (flag == "wrap" or not flags(op, a, b)["wrap"]):
                out.append((a, b))
        return out
    if op == 3:
        # a < b and (a - b) mod 2^64 < K: adding p back borrows out of limb 1.  d = a - b + 2^256.
        while len(out) < n:
            shape = len(out) % 4
            d = rng.randrange(2**256) & ~(2**64 - 1) | rng.randrange(K)
            if shape == 1:
                d &= ~(M32 << 64)                  # limb 2 zero: the borrow runs on into limb 3
            elif shape == 2:
                d &= ~((2**96 - 1) << 64)          # limbs 2..4 zero
            elif shape == 3:
                d = (1 << 255) | (d & (2**64 - 1)) # limbs 2..6 zero
            lo = 2**256 - d
            if lo >= P:
                continue
            b = rng.randrange(lo, P)
            a = b + d - 2**256
            if flags(3, a, b)[flag]:
                out.append((a, b))
        return out
    if op == 5:
        # a + b = 2^256 + s with s mod 2^64 >= 2^64 - K: folding the carry carries out of limb 1
        while len(out) < n:
            shape = len(out) % 4
            a = rng.randrange(2**200, P)
            s = rng.randrange(a) & ~(2**64 - 1) | (2**64 - 1 - rng.randrange(K))
            if shape == 1:
                s |= M32 << 64                     # limb 2 all ones: the carry runs on into limb 3
            elif shape == 2:
                s |= (2**96 - 1) << 64
            elif shape == 3:
                s |= (2**160 - 1) << 64
            if s >= a:
                continue
            b = s + 2**256 - a
            if flags(5, a, b)[flag]:
                out.append((a, b))
        return out
    raise ValueError(op)


# ------------------------------------------------------------------------------------------ planting

def be64(pt) -> bytes:
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def table_points(raw: bytes) -> list:
    """The 513 affine points of a giant table (GSn[0..511], _2GSn), x||y big-endian."""
    return [(int.from_bytes(raw[64 * i:64 * i + 32], "big"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "big"))
            for i in range(len(raw) // 64)]


def group_offset(ora, bs, g: int):
    """g * _2GSn as helpers.lane_offsets builds it: -(g * 2048 * M) * G."""
    if g == 0:
        return None
    return ora.negation(ora.pubkey(g * 2048 * bs.m)).xy()


def step_of(i: int, sign: int) -> int:
    """The step t of a group at which C + sign * GSn[i] stands (t = 512 is C itself: i = -1)."""
    if i < 0:
        return HALF
    return HALF - 1 - i if sign < 0 else HALF + 1 + i


def planted_cases():
    """(i, sign) of the 14 planted steps: i in {511, 510, 509, 3, 2, 1, 0} with both signs where the step has
    both (C + GSn[511] is not part of a group), and the centre itself (i = -1)."""
    cases = [(511, -1)]
    for i in (510, 509, 3, 2, 1, 0):
        cases += [(i, -1), (i, +1)]
    return cases + [(-1, 0)]


def centre_for(Q, i: int, sign: int, gsn: list):
    """The centre C with C + sign * GSn[i] == Q (i = -1: C = Q)."""
    if i < 0:
        return Q
    return add(Q, gsn[i]) if sign < 0 else add(Q, neg(gsn[i]))


def start_for(centre, g: int, ora, bs):
    """startP such that group g's centre, startP + g * _2GSn, is `centre`."""
    return add(centre, neg(group_offset(ora, bs, g)))


def ref_centre(ora, bs, start, g: int):
    """The reference's centre of group g of a job that starts at `start`: AddDirect(startP, g * _2GSn) with
    ModInv(0) = 0 (so it also defines the collapsed add); group 0 is startP itself.  An ora.Point."""
    sp = ora.Point.of(*start)
    if g == 0:
        return sp
    return ora.add_direct(sp, ora.Point.of(*group_offset(ora, bs, g)))


def add_direct_ref(p1, p2, inverse=None):
    """AddDirect(p1, p2) (SECP256K1.cpp:242-265) on integers: s = (p2.y - p1.y) * inverse, x = s^2 - p1.x - p2.x,
    y = (p2.x - x) * s - p2.y, with inverse = ModInv(p2.x - p1.x) unless given (a batch's inverse), and ModInv(0) = 0.
    Returns (point, collapsed): collapsed when p2.x == p1.x.  The operands need not be on the curve."""
    dx = (p2[0] - p1[0]) % P
    if inverse is None:
        inverse = inv(dx)
    s = (p2[1] - p1[1]) * inverse % P
    x = (s * s - p1[0] - p2[0]) % P
    return (x, ((p2[0] - x) * s - p2[1]) % P), dx == 0


def addr_group_ref(centre, gn: list):
    """One -m address group from its centre C with the table Gn[0..511], _2Gn (keyhunt.cpp:2586-2711):
    pts[t] = C - Gn[511 - t] (t < 512), C (t = 512), C + Gn[t - 513] (t > 512) as x||y, the next centre C + _2Gn
    (AddDirect's formulas with the batch's inverse, keyhunt.cpp:3986-3999) and whether the group is degenerate.
    The 513 inverses come from one batch inversion, so they are all 0 when any dx is 0 (C = +-Gn[k] or +-_2Gn:
    IntGroup.cpp:36-58 with ModInv(0) = 0), and y follows the walk's own formulas, which give the reference's
    value with such an inverse too: (x - Gn.x) * s' + Gn.y with s' = (Gn.y + C.y) * inv for C - Gn[i]
    (keyhunt.cpp:2628-2641), (Gn.x - x) * s - Gn.y with s = (Gn.y - C.y) * inv for C + Gn[i] (2611-2624).  C need
    not be on the curve (the centre after a degenerate group is not)."""
    cx, cy = centre
    dx = [(g[0] - cx) % P for g in gn]
    degenerate = not all(dx)
    inverse = [0] * len(dx)
    if not degenerate:
        pre = [1]
        for d in dx:
            pre.append(pre[-1] * d % P)
        acc = inv(pre[-1])
        for i in range(len(dx) - 1, -1, -1):
            inverse[i] = acc * pre[i] % P
            acc = acc * dx[i] % P

    def minus(i):
        gx, gy = gn[i]
        s = (gy + cy) * inverse[i] % P
        x = (s * s - cx - gx) % P
        return x, ((x - gx) * s + gy) % P

    def plus(i):
        return add_direct_ref(centre, gn[i], inverse[i])[0]

    out = [minus(HALF - 1 - t) for t in range(HALF)] + [centre] + [plus(t) for t in range(HALF - 1)]
    return b"".join(be64(p) for p in out), plus(HALF), degenerate


def addr_lanes_ref(start, gn: list, offs: list, gpl: int, ngroups: int, cache: dict | None = None):
    """One launch of one -m address job as the library lays it out (scan_kernels.hpp, scan_group): lane m walks
    groups [m * gpl, min((m + 1) * gpl, ngroups)) from AddDirect(start, offs[m]) with ModInv(0) = 0 (lane 0 from
    start itself; offs[m] = (m * gpl) * _2Gn), each group handing its next centre on to the following one.  Returns
    (x||y of the ngroups groups, the set of degenerate records the kernel emits): (m * gpl) | 0x80000000 for a lane
    add that collapses (start = +-offs[m]), g for every degenerate group.  Centres that are no longer on the curve
    are integers like any other.  cache: {centre: addr_group_ref(centre, gn)}, shared between calls with one gn."""
    xy, records = [], set()
    for m in range((ngroups + gpl - 1) // gpl):
        c = start
        if m:
            c, collapsed = add_direct_ref(start, offs[m])
            if collapsed:
                records.add((m * gpl) | 0x80000000)
        for g in range(m * gpl, min((m + 1) * gpl, ngroups)):
            if cache is None:
                ref = addr_group_ref(c, gn)
            else:
                ref = cache.get(c)
                if ref is None:
                    ref = cache[c] = addr_group_ref(c, gn)
            xy.append(ref[0])
            if ref[2]:
                records.add(g)
            c = ref[1]
    return b"".join(xy), records


# ------------------------------------------------------------------- the second / third check, per slot

def bp_search(bp: bytes, xb: bytes):
    """bsgs_searchbinary (keyhunt.cpp:3748-3773) transcribed: bp holds 16-byte entries (value[6], pad[2], index
    u64 LE), the key is bytes 16..22 of xb.  The index of the entry the loop lands on, or None."""
    n = len(bp) // 16
    lo, hi, half, current = 0, n, n, 0
    while half >= 1:
        half = (hi - lo) // 2
        e = 16 * (current + half)
        v, k = bp[e:e + 6], xb[16:22]
        if k == v:
            return int.from_bytes(bp[e + 8:e + 16], "little")
        if k < v:
            hi = hi - half
        else:
            lo = lo + half
        current = lo
    return None


def second_check_ref(tabs: dict, base: int, a: int, target) -> dict:
    """bsgs_secondcheck / bsgs_thirdcheck (keyhunt.cpp:4271-4368, oracle/ora_bsgs.c) on Python integers, reporting
    what every slot did.  tabs: the four constants m_double, m2_double, m3_value, m3_double (any width below 2^256,
    sums modulo 2^256 as the device's U8), amp2 / amp3 / bptable as bytes, and "bs", the oracle geometry whose
    (possibly altered) level-2 and level-3 sub-blooms answer membership.  k*G is the oracle's, 0 giving (0, 0);
    AddDirect is add_direct_ref with inverse(0) = 0.  target: (x, y).
    Returns key (or None), l2_hits, l3_hits, bp_hits, xs2 (the 32 second-check x), xs3 {i2: the 32 third-check x of
    every third check entered} and zero, the (level, slot) of every batch element with dx == 0."""
    import ctypes as C
    from oracle import ora
    bs, L, W = tabs["bs"], ora.lib(), 2**256
    amp2, amp3, bp = table_points(tabs["amp2"]), table_points(tabs["amp3"]), tabs["bptable"]
    res = {"key": None, "l2_hits": 0, "l3_hits": 0, "bp_hits": 0, "xs2": None, "xs3": {}, "zero": []}

    def member(level, x):
        xb = x.to_bytes(32, "big")
        return bool(L.ora_bloom_check(C.byref(bs.bloom(level, xb[0])), xb, 32))

    def minus_base(k):                     # target - k*G by AddDirect(target, Negation(k*G))
        bx, by = ora.pubkey(k).xy()
        return add_direct_ref(target, (bx, (P - by) % P))[0]

    def batch(q, tab, level):
        xs = []
        for i in range(32):
            pt, collapsed = add_direct_ref(q, tab[i])
            xs.append(pt[0])
            if collapsed:
                res["zero"].append((level, i))
        return xs

    def third(base1, i2):
        base2 = (base1 + i2 * tabs["m2_double"]) % W
        q = minus_base(base2)
        xs = res["xs3"][i2] = batch(q, amp3, 3)
        for i in range(32):
            ci = (i * tabs["m3_double"] + tabs["m3_value"]) % W
            if member(3, xs[i]):
                res["l3_hits"] += 1
                j = bp_search(bp, xs[i].to_bytes(32, "big"))
                if j is not None:
                    res["bp_hits"] += 1
                    for key in ((ci + j + 1) % W, (ci - j - 1) % W):
                        key = (key + base2) % W
                        if ora.pubkey(key).xy()[0] == target[0]:
                            return key
            elif q[0] == amp3[i][0]:
                return (ci + base2) % W
        return None

    base1 = (base + a * tabs["m_double"]) % W
    xs2 = res["xs2"] = batch(minus_base(base1), amp2, 2)
    for i2 in range(32):
        if member(2, xs2[i2]):
            res["l2_hits"] += 1
            res["key"] = third(base1, i2)
            if res["key"] is not None:
                break
    return res
