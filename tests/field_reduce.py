"""Operands aimed at the carry-out branch of the per-limb reduction of csrc/device/fe_asm.hpp (fm_reduce_V)
(test infrastructure; used by test_field_reduce_model.py and test_gpu_field_directed.py).

The reduction folds S = Lw + Lw8 2^256 + H (2^32 + 977) (L, H the halves of the 512-bit product, Lw = L or
L + w) through V_i = 977 H_i + (H_i : Lw_i), one 64-bit multiply-add per limb.  V_i can pass 2^64; the
device keeps the low 64 bits, records the carry-out per lane (ov_i), runs its chain R on the truncated
values and, when any lane of a wave carried, adds ov_i back at word i + 2 of R.  tests/field_model.py models
that (v_op here is its device()) and gives ov_i from the integers alone (expected_ov)."""
from __future__ import annotations

import math
import random

from tests import adversarial as adv
from tests.field_model import K, M32, M64, M256, P, expected_ov  # noqa: F401
from tests.field_model import device as v_op
# V_i = H_i K + Lw_i >= 2^64: always for H_i >= 2^32 - 976, never for H_i <= 2^32 - 978, and for
# H_i = 2^32 - 977 (H_i K = 2^64 - 977^2) exactly when Lw_i >= 977^2.
H_ALWAYS = 2**32 - 976
EDGE = (2**32 - 979, 2**32 - 978, 2**32 - 977, 2**32 - 976)


# ------------------------------------------------------------------------------------- operands

def _with_high(op: int, H: int, rng: random.Random):
    """(a, b) of op whose 512-bit product has the high half H, or None.  op 0: t = H 2^256 + 2^256 - 1 rounded
    down to a multiple of a random b > H moves only the low half; ops 1 and 6: the integer square root of such
    a t, which may borrow one from H (the caller checks)."""
    t = (H << 256) | M256
    if op == 0:
        if H + 2 >= 2**256:
            return None
        b = rng.randrange(H + 1, 2**256)
        a = t // b
        return (a, b) if a < 2**256 and (a * b) >> 256 == H else None
    a = math.isqrt(t)
    if (a * a) >> 256 != H:
        return None
    return a, (rng.randrange(2**256) if op == 6 else 0)


def _quiet_limb(rng: random.Random) -> int:
    return rng.randrange(2, 2**32 - 2000)


def one_limb(op: int, i: int, n: int, seed: int = 0) -> list:
    """n operand pairs whose V mad carries out in limb i and in no other."""
    rng = random.Random(f"one{op}{i}{seed}")
    out = []
    while len(out) < n:
        h = [_quiet_limb(rng) for _ in range(8)]
        h[i] = rng.randrange(H_ALWAYS, 2**32)
        ab = _with_high(op, adv.value(h), rng)
        if ab and expected_ov(op, *ab) == [int(k == i) for k in range(8)]:
            out.append(ab)
    return out


_NEAR_P, _ALL = [0] + [1] * 7, [1] * 8
# the carry-outs of all_limbs' named operands, by hand: H = 2^256 - 2^33 - 1956 (- 1957, - 1958) for the
# products near p^2, so H_0 stays under the threshold; H = 2^256 - 2 for (2^256-1)^2
NAMED_OV = {0: [_NEAR_P, _NEAR_P, _ALL], 1: [_NEAR_P, _NEAR_P, _ALL], 6: [_NEAR_P, _NEAR_P, _ALL, _NEAR_P]}


def all_limbs(op: int, n: int) -> list:
    """Operands near 2^256 and p, whose every upper limb is all ones: the named ones first ((p-1)^2,
    (p-1)(p-2), (2^256-1)^2, and for op 6 the addend 2^256-1), then (2^256-1-x)(2^256-1-y) with x + y < 900.
    All eight mads carry out, except that the products of values just below p have H_0 = 2^32 - 1956 or so,
    under the threshold: limbs 1..7 carry there (NAMED_OV)."""
    named = {0: [(P - 1, P - 1), (P - 1, P - 2), (M256, M256)],
             1: [(P - 1, 0), (P - 2, 0), (M256, 0)],
             6: [(P - 1, M256), (P - 2, M256), (M256, M256), (P - 1, 0)]}[op]
    rng = random.Random(f"all{op}")
    out = list(named)
    while len(out) < n:
        x, y = rng.randrange(450), rng.randrange(450)
        out.append((M256 - x, M256 - y) if op == 0 else (M256 - x, rng.randrange(2**256) if op == 6 else 0))
    return out


def edge(op: int, n: int, seed: int = 0) -> list:
    """n operand pairs with one H_i in EDGE (2^32 - 979 .. 2^32 - 976), the limb and the value cycling; the other
    limbs stay clear of the threshold.  Returns [(a, b, i, H_i)]."""
    rng = random.Random(f"edge{op}{seed}")
    out = []
    while len(out) < n:
        i, hv = len(out) % 8, EDGE[(len(out) // 8) % 4]
        h = [_quiet_limb(rng) for _ in range(8)]
        h[i] = hv
        ab = _with_high(op, adv.value(h), rng)
        if ab:
            out.append(ab + (i, hv))
    return out


def with_second_fold(flag: str, n: int, seed: int = 0) -> list:
    """n operand pairs of op 6 (a^2 + w) that carry out of a V mad and also need the second fold's rare branch:
    flag "c3" (carry into limb 3, no wrap) or "wrap" (c3 and the fold of a wrap past 2^256).  a is chosen for
    the high half of a^2, w for the value a^2 + w reduces to (a class C / class B value of adversarial.py);
    kept when the model raises exactly the flags asked for.  Op 0 has mul_with_c3; the combinations of op 1 and the
    wrap of op 0 are not aimed at (they would need a square root, or a product, with both a chosen high half and
    chosen low words)."""
    rng = random.Random(f"fold{flag}{seed}")
    vals = adv.class_values("B" if flag == "wrap" else "C", seed)
    out = []
    while len(out) < n:
        h = [_quiet_limb(rng) for _ in range(8)]
        for i in rng.sample(range(8), rng.randrange(1, 4)):
            h[i] = rng.randrange(H_ALWAYS, 2**32)
        ab = _with_high(1, adv.value(h), rng)
        if not ab:
            continue
        a = ab[0]
        w = (next(vals) - a * a) % P
        for ww in (w, w + P):
            if ww >= 2**256:
                continue
            f = v_op(6, a, ww)[1]
            if any(f["ov"]) and f["c3"] == 1 and f["wrap"] == (1 if flag == "wrap" else 0):
                out.append((a, ww))
                break
    return out


def mul_with_c3(n: int, seed: int = 0) -> list:
    """n operand pairs of op 0 that carry out of the V mads and need c3 (no wrap): a = 2^256 - 1 - x with
    x < 2^128 and b = 2^256 - 1, so H = 2^256 - 2 - x (limbs 4..7 all ones: their mads carry) and L = 1 + x.  The low
    three words of S = L + H K are (1 - 2K - (K - 1) x) mod 2^96; x is solved for a value r of them in the top 2^32
    of 2^96 (K - 1 = 16 (2^28 + 61), so r = 1 - 2K mod 16), which the second fold's addend (top ~ 2^32, times K)
    carries out of.  Every pair is checked against the model's flags; the search is bounded."""
    rng = random.Random(f"mulc3{seed}")
    odd_inv = pow((K - 1) // 16, -1, 2**92)
    out = []
    for _ in range(64 * n):
        if len(out) == n:
            break
        r = 2**96 - 1 - rng.randrange(2**32)
        r -= (r - (1 - 2 * K)) % 16
        x = ((1 - 2 * K - r) // 16 * odd_inv) % 2**92 | (rng.randrange(2**36) << 92)
        a, b = M256 - x, M256
        f = v_op(0, a, b)[1]
        if f["ov"][4:] == [1] * 4 and f["c3"] == 1 and f["wrap"] == 0:
            out.append((a, b))
    assert len(out) == n, len(out)
    return out
