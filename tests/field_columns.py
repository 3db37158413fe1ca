"""Operands aimed at the edge conditions of the forward-carried columns of csrc/device/fe_asm.hpp's 512-bit products
(fm_mul512x and the cross sum of fm_sqr512x), and the bound that says which columns are masked (test infrastructure;
used by test_field_columns_model.py and test_gpu_field_directed.py).  The column model itself is
tests/field_model.py's (cols_mul, cols_cross, cols_sqr, product); this is what it does:

Column K accumulates in one 64-bit pair S that starts as {lo = hi(S of column K-1), hi = cw of column K-1}, where cw
counts the carries out of the pair.  The first product of a column is added without a carry count.  That is exact
while the seed is at most 2^33 - 2 (a product is at most 2^64 - 2^33 + 1): always behind a column of one or two
products, not always behind one of three or more -- columns 3..13 of a product and 6..10 of the cross sum
(unsafe_columns works the bound out).  There the device keeps the first product's carry-out as a lane mask and, in a
wave where any lane has one, adds the dropped carries back at word K + 2 (fm_fix_cols).  The model does the same: it
drops the carry, counts on from the smaller value, records the drop (first[K]) and adds the bits back at the end; in
every other column it asserts that the first product fits.  t[K] = lo(S); column 14 leaves t[14] and t[15].
cols_mul / cols_cross return the 16 words with, per column, the final pair's high word, the count, the unreduced
total and the drop, so that a generator can certify what an operand does.  The squaring's tail (diagonal + doubled
cross sum) is the device's one carry chain, which is plain integer addition: cols_sqr returns 2 cross + diagonal.

Operand families (each returns (a, b) pairs for khb_field_op 0; for ops 1 and 6 the first operand is used):
  all_ones        both operands 2^256 - 1: every column at its maximum carry count, ten of the eleven masks set
  low_ones        the first n limbs all ones, n = 1..8: each number of carries 0..n-1 in the widest column
  single_limbs    x 2^(32i) and y 2^(32j) for every (i, j): columns of one product, zero seeds, column 14
  full_high       hi(S_K) = 0xffffffff with cw_K > 0 at a chosen column K, certified by the model: the largest seed
                  a count of 1 can hand on.  A column of two products cannot do that, so K runs over the columns
                  of three or more: 2..12 for the product and 5..9 for the cross sum.
  first_drop      the first product of masked column K, and of no other, drops its carry
  near_p          operands within a few units of p, 2^256 and 2^255"""
from __future__ import annotations

import random

from tests import adversarial as adv
from tests.field_model import K, M32, M64, M256, MUL_MASKED, P, PMAX, SQR_MASKED  # noqa: F401
from tests.field_model import cols_cross, cols_mul, cols_sqr  # noqa: F401
from tests.field_model import cross_products as _cross_products, mul_products as _mul_products

MUL_FULL_COLS = tuple(range(2, 13))
SQR_FULL_COLS = tuple(range(5, 10))


def unsafe_columns(counts) -> list:
    """The columns whose first product can overflow its seed, for columns of counts[K] products: an upper bound of
    what column K-1 hands on, floor(total / 2^32) with every product at its maximum, against 2^64 - PMAX."""
    v, out = 0, []
    for k, n in enumerate(counts):
        if n and v + PMAX > M64:
            out.append(k)
        v = (n * PMAX + v) >> 32
    return out


# ------------------------------------------------------------------------------------- operands

def all_ones() -> list:
    return [(M256, M256)]


def low_ones() -> list:
    return [(2**(32 * n) - 1, 2**(32 * n) - 1) for n in range(1, 9)]


def single_limbs(seed: int = 0) -> list:
    """x 2^(32i), y 2^(32j) for every (i, j), x and y all ones for the first pass and random words after it."""
    rng = random.Random(f"columns-single{seed}")
    out = []
    for x, y in ((M32, M32), (rng.randrange(1, 2**32), rng.randrange(1, 2**32))):
        out += [(x << (32 * i), y << (32 * j)) for i in range(8) for j in range(8)]
    return out


def is_full_high(op: int, a: int, b: int, k: int) -> bool:
    _, hi, cw, _, _ = cols_mul(a, b) if op == 0 else cols_cross(a)
    return hi[k] == M32 and cw[k] > 0


def drops(op: int, a: int, b: int) -> list:
    """The masked columns whose first product drops its carry (op 0: a*b; ops 1, 6: the cross sum of a)."""
    first = (cols_mul(a, b) if op == 0 else cols_cross(a))[4]
    return [k for k, d in enumerate(first) if d]


def full_high(op: int, k: int, n: int, seed: int = 0) -> list:
    """n operands whose column k ends with hi(S_k) = 0xffffffff and cw_k > 0 (op 0: a*b; ops 1, 6: the cross sum of a).
    One limb is solved for: the one whose product with the column's first limb enters at column k and in no earlier
    column (for k > 7 the limbs of a below k - 7 are zero, so that the solved limb 7 meets nothing before column k).
    The column's total is linear in it, and the window [c 2^64 + (2^32 - 1) 2^32, (c + 1) 2^64) is 2^32 wide, wider
    than the step.  Kept only when the model certifies the condition."""
    assert k in (MUL_FULL_COLS if op == 0 else SQR_FULL_COLS)
    rng = random.Random(f"columns-full{op}{k}{seed}")
    lo = max(0, k - 7)                    # the solved limb is b[k - lo] (op 0) or a[k - lo] (cross sum)
    out = []
    while len(out) < n:
        A = [rng.randrange(2**31, 2**32) if i >= lo else 0 for i in range(8)]
        B = [rng.randrange(2**31, 2**32) for _ in range(8)]
        if op == 0:
            B[k - lo] = 0
            base = cols_mul(adv.value(A), adv.value(B))[3][k]
        else:
            A[k - lo] = 0
            base = cols_cross(adv.value(A))[3][k]
        nprod = len((_mul_products(A, B) if op == 0 else _cross_products(A))[k])
        c = rng.randrange(1, nprod - 1)   # the count to reach: at most nprod - 2 with the top word full
        v = -((base - (c << 64) - (M32 << 32)) // A[lo])
        if not 0 < v <= M32:
            continue
        if op == 0:
            B[k - lo] = v
        else:
            A[k - lo] = v
        a, b = adv.value(A), (adv.value(B) if op == 0 else rng.randrange(2**256))
        if is_full_high(op, a, b, k):
            out.append((a, b))
    return out


def first_drop(op: int, k: int, n: int, seed: int = 0) -> list:
    """n operands whose column k, and no other, drops the carry of its first product.  The two limbs of that product
    are all ones and every other limb lies in [0xe0000000, 0xffff0000): no other first product comes within 2^48 of
    2^64, and column k-1 (three or more products of at least 0.76 2^64) hands on a count of 2 or more."""
    assert k in (MUL_MASKED if op == 0 else SQR_MASKED)
    rng = random.Random(f"columns-drop{op}{k}{seed}")
    lo = max(0, k - 7)
    out = []
    while len(out) < n:
        A = [rng.randrange(0xE0000000, 0xFFFF0000) for _ in range(8)]
        B = [rng.randrange(0xE0000000, 0xFFFF0000) for _ in range(8)]
        A[lo] = M32
        if op == 0:
            B[k - lo] = M32
        else:
            A[k - lo] = M32
        a, b = adv.value(A), (adv.value(B) if op == 0 else rng.randrange(2**256))
        if drops(op, a, b) == [k]:
            out.append((a, b))
    return out


def near_p(seed: int = 0) -> list:
    rng = random.Random(f"columns-p{seed}")
    vals = [P - 2, P - 1, P, P + 1, P + K - 1, M256 - 1, M256, 2**255 - 1, 2**255, 2**255 + 1, K, K - 1, 1, 0]
    out = [(x, y) for x in vals for y in vals[:7]]
    out += [(P - rng.randrange(2**40), P - rng.randrange(2**40)) for _ in range(16)]
    return out


def directed(op: int, per_col: int = 4, seed: int = 0) -> list:
    """Every family for the op, as one list of (a, b)."""
    out = all_ones() + low_ones() + single_limbs(seed) + near_p(seed)
    for k in (MUL_FULL_COLS if op == 0 else SQR_FULL_COLS):
        out += full_high(op, k, per_col, seed)
    for k in (MUL_MASKED if op == 0 else SQR_MASKED):
        out += first_drop(op, k, per_col, seed)
    return out
