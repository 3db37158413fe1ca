"""Operands aimed at each rare condition of fm_reduce_V's second fold in csrc/device/fe_asm.hpp (test infrastructure;
used by test_field_fold2_model.py and test_gpu_field_directed.py).

After the chain R = sum_i lo64(V_i) 2^(32i) + Lw8 2^256 the device keeps R9, the carry out of R8, as a lane mask
(r9) and folds R8 alone: m = R8 977 + (R1:R0) in one 64-bit multiply-add (carry-out o), R1' = hi(m) + R8,
R2' = R2 + carry (carry-out c2).  A wave in which any lane has a V carry-out (ov), r9, o or c2 redoes the fold in its
general form for all its lanes.  tests/field_model.py's device() (f_op here) does that per operand and returns the raw
lazy value with the flags: path ("fast" or "general"), r9, o, c2 as the device computes them (on R before the carry
fix), and ov.  The device has one rare branch, so "general" stands for every reason to take it.

Operands.  Each generator keeps an operand only when the model raises exactly the flags asked for.
  op 6 (a^2 + w): every flag, by the choice of w for an a whose square has a chosen high half: w sets all of Lw.
  op 0: r9 through H_7 in 2^32 - 979 .. 2^32 - 978 (field_reduce._with_high).  o and c2 through the multiplier
        b = 2^255 + 1 and an even a = 2e: the product is e 2^256 + 2e, so H = e, L = 2e and S = e (K + 2), whose low
        96 bits are solved for e and whose high limbs (the V carry-outs) are free.
  op 1: r9 as op 0.  o and c2 through the root a = 2^255 + d, d < 2^128: a^2 = (2^254 + d) 2^256 + d^2, so
        S = d^2 + K d + 2^254 K, a quadratic in d solved mod 2^96 by lifting bit by bit; limb 3 of d is free (ov).
  Not reached for ops 0 and 1: o together with c2 (it needs R8 >= 2^32 - 976, and these families have R8 < 2^31), and
  r9 together with o or c2 (the general fold's concern, covered by op 6's generators and field_reduce's classes).
fm_add_lazy (op 5) and fm_sub (op 3) keep their carry into limb 2 in a lane mask as well; device() models that form
and adversarial.directed_operands provides their classes (lazy_c2, sub_b2)."""
from __future__ import annotations

import random

from tests import adversarial as adv
from tests import field_reduce as fr
from tests.field_model import K, M32, M64, M256, P  # noqa: F401
from tests.field_model import device as f_op

M96 = 2**96 - 1
R9_H7 = (2**32 - 979, 2**32 - 978)       # H_7 that brings R8 to the brink without a V carry-out


# ------------------------------------------------------------------------------------- operands

FLAGS = ("r9", "o", "c2", "ov")


def has_exactly(f: dict, want) -> bool:
    """The model's flags are exactly `want` (a subset of FLAGS; ov stands for any V carry-out)."""
    return all((bool(any(f[k])) if k == "ov" else bool(f[k])) == (k in want) for k in FLAGS)


def _low96_target(want, R8: int, rng: random.Random) -> int:
    """Low three words of R that raise o and / or c2 (as asked) for a top word near R8, or random ones."""
    if "o" in want:
        lo = M64 - rng.randrange(max(1, 977 * R8 // 2))
    elif "c2" in want:
        lo = ((M32 - rng.randrange(1, max(2, R8 // 2))) << 32) | rng.randrange(2**31)
    else:
        return rng.randrange(2**96)
    r2 = M32 if "c2" in want else rng.randrange(2, 2**32 - 2000)
    return (r2 << 64) | lo


def _high_half(want, rng: random.Random) -> int:
    """A high half H for the flags: quiet limbs, H_7 chosen for r9 or for o with c2, limbs 1..6 for ov."""
    h = [fr._quiet_limb(rng) for _ in range(8)]
    if "r9" in want:
        h[7] = rng.choice(R9_H7)
    elif "o" in want and "c2" in want:
        h[7] = rng.randrange(2**32 - 1953, 2**32 - 979)
    if "ov" in want:
        for i in rng.sample(range(1, 7), rng.randrange(1, 3)):
            h[i] = rng.randrange(fr.H_ALWAYS, 2**32)
    return adv.value(h)


def sqr_add_with(want, n: int, seed: int = 0) -> list:
    """n operand pairs (a, w) of op 6 with exactly the flags `want`: a for the high half, w for Lw."""
    want = frozenset(want)
    rng = random.Random(f"fold2-6{sorted(want)}{seed}")
    out = []
    while len(out) < n:
        ab = fr._with_high(1, _high_half(want, rng), rng)
        if not ab:
            continue
        a = ab[0]
        L, H = (a * a) & M256, (a * a) >> 256
        lw = rng.randrange(2**256)
        R8 = ((lw + H * K) >> 256) & M32                      # within a carry of the chain's
        lw = (lw & ~M96) | ((_low96_target(want, R8, rng) - H * K) & M96)
        w = (lw - L) & M256
        if has_exactly(f_op(6, a, w)[1], want):
            out.append((a, w))
    return out


def _r9_with(op: int, want, n: int, rng: random.Random) -> list:
    out = []
    while len(out) < n:
        ab = fr._with_high(op, _high_half(want, rng), rng)
        if ab and has_exactly(f_op(op, *ab)[1], want):
            out.append(ab)
    return out


def mul_with(want, n: int, seed: int = 0) -> list:
    """n operand pairs of op 0 with exactly the flags `want` (module docstring for the families)."""
    want = frozenset(want)
    rng = random.Random(f"fold2-0{sorted(want)}{seed}")
    if "r9" in want:
        return _r9_with(0, want, n, rng)
    inv = pow(K + 2, -1, 2**96)
    out = []
    while len(out) < n:
        e = _high_half(want, rng) & (2**255 - 1)               # H = e < 2^255; its limbs carry the ov
        R8 = (e * (K + 2)) >> 256
        e = (e & ~M96) | ((_low96_target(want, R8, rng) * inv) & M96)
        a, b = 2 * e, 2**255 + 1
        if has_exactly(f_op(0, a, b)[1], want):
            out.append((a, b))
    return out


def sqr_with(want, n: int, seed: int = 0) -> list:
    """n operands (a, 0) of op 1 with exactly the flags `want` (module docstring for the families)."""
    want = frozenset(want)
    rng = random.Random(f"fold2-1{sorted(want)}{seed}")
    if "r9" in want:
        return _r9_with(1, want, n, rng)
    R8 = (2**254 * K) >> 256
    out = []
    while len(out) < n:
        T = _low96_target(want, R8, rng) & ~1                  # d (d + K) is even
        d = rng.randrange(2)
        for k in range(1, 96):                                 # d^2 + K d = T mod 2^(k+1), one bit at a time
            if (d * d + K * d - T) >> k & 1:
                d |= 1 << k
        d |= (rng.randrange(fr.H_ALWAYS, 2**32) if "ov" in want else fr._quiet_limb(rng)) << 96
        a = 2**255 + d
        if has_exactly(f_op(1, a, 0)[1], want):
            out.append((a, 0))
    return out


WITH = {0: mul_with, 1: sqr_with, 6: sqr_add_with}
# the classes per op: each flag alone, each with a V carry-out, and (op 6) o together with c2
CLASSES = {op: [("r9",), ("o",), ("c2",), ("r9", "ov"), ("o", "ov"), ("c2", "ov")] for op in (0, 1)}
CLASSES[6] = CLASSES[0] + [("o", "c2")]


def directed(op: int, n: int, seed: int = 0) -> dict:
    """{class: n operand pairs} for every class of the op."""
    return {c: WITH[op](c, n, seed) for c in CLASSES[op]}
