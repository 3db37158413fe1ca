"""The column model of tests/field_model.py against Python integers, and field_columns' directed operands: the model's 16
words are a*b / a*a, the masked columns are exactly those whose first product can overflow its seed, every directed
operand sets the condition it is named for, and every mask and every column that can end with a full high word and a
carry count has operands of its own."""
from __future__ import annotations

import random

import pytest

from tests import adversarial as adv
from tests import field_columns as fc
from tests import field_model as fm


def _operands():
    rng = random.Random(1401)
    ops = fc.all_ones() + fc.low_ones() + fc.single_limbs(1) + fc.near_p(1)
    ops += [(rng.randrange(2**256), rng.randrange(2**256)) for _ in range(500)]
    words = (0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF)
    ops += [(adv.value([rng.choice(words) for _ in range(8)]), adv.value([rng.choice(words) for _ in range(8)]))
            for _ in range(500)]
    return ops


def test_model_is_the_product():
    for a, b in _operands():
        t, hi, cw, _, first = fc.cols_mul(a, b)
        assert adv.value(t) == a * b and max(first) <= 1
        assert max(cw) <= 7 and cw[0] == cw[14] == 0
        c = fc.cols_cross(a)
        assert 2 * adv.value(c[0]) + sum(x * x << (64 * i) for i, x in enumerate(adv.limbs(a))) == a * a
        assert all(c[2][k] == 0 for k in (0, 1, 2, 12, 13, 14))
        assert adv.value(fc.cols_sqr(a)) == a * a
        for op in (0, 1, 6):
            assert fm.product(op, a, b)[0] ==(a * b if op == 0 else a * a)


def test_all_ones_reaches_every_maximum():
    # column k of (2^256 - 1)^2 holds min(k, 14 - k) + 1 products of (2^32 - 1)^2 and carries once less than that,
    # counted or, for the first product of a masked column, dropped; ten of the eleven masks are set
    _, _, cw, _, first = fc.cols_mul(*fc.all_ones()[0])
    assert [c + d for c, d in zip(cw, first)] == [min(k, 14 - k) for k in range(15)]
    assert [k for k in range(15) if first[k]] == list(range(3, 13))
    _, _, cw, _, first = fc.cols_cross(fc.all_ones()[0][0])
    assert [c + d for c, d in zip(cw, first)] == \
        [max(0, len(range(max(0, k - 7), (k - 1) // 2 + 1)) - 1) for k in range(15)]
    assert [k for k in range(15) if first[k]] == [6, 8, 10]


def test_masked_columns_are_the_unsafe_ones():
    assert fc.unsafe_columns([min(k, 14 - k) + 1 for k in range(15)]) == list(fc.MUL_MASKED)
    assert fc.unsafe_columns([len(range(max(0, k - 7), (k - 1) // 2 + 1)) for k in range(15)]) == list(fc.SQR_MASKED)


@pytest.mark.parametrize("op", [0, 1])
def test_first_drop_operands(op):
    for k in (fc.MUL_MASKED if op == 0 else fc.SQR_MASKED):
        ops = fc.first_drop(op, k, 4, seed=5)
        assert len(ops) == 4
        for a, b in ops:
            assert fc.drops(op, a, b) == [k]
            assert fm.product(op, a, b)[0] ==(a * b if op == 0 else a * a)


def test_low_ones_reach_each_count():
    # the widest column of (2^(32n) - 1)^2 is n - 1, with n products: n - 1 carries, counted or dropped
    for n, (a, b) in enumerate(fc.low_ones(), 1):
        _, _, cw, _, first = fc.cols_mul(a, b)
        assert cw[n - 1] + first[n - 1] == n - 1
    assert {max(fc.cols_mul(a, b)[2]) for a, b in fc.low_ones()} == set(range(7))


def test_single_limbs_cover_every_column():
    ops = fc.single_limbs(2)
    assert len(ops) == 128
    for n, (a, b) in enumerate(ops):
        i, j = (n % 64) // 8, n % 8
        t, hi, cw, total, first = fc.cols_mul(a, b)
        assert not any(cw) and not any(first) and adv.value(t) == a * b
        assert [k for k in range(15) if total[k]] in ([i + j], [i + j, i + j + 1])    # the product and its seed
    assert {(n % 64) // 8 + n % 8 for n in range(128)} == set(range(15))


@pytest.mark.parametrize("op", [0, 1])
def test_full_high_operands(op):
    cols = fc.MUL_FULL_COLS if op == 0 else fc.SQR_FULL_COLS
    for k in cols:
        ops = fc.full_high(op, k, 4, seed=5)
        assert len(ops) == 4
        for a, b in ops:
            assert fc.is_full_high(op, a, b, k)
            assert fm.product(op, a, b)[0] ==(a * b if op == 0 else a * a)


def test_directed_lists():
    for op in (0, 1, 6):
        ops = fc.directed(op, 4, seed=9)
        assert all(0 <= a < 2**256 and 0 <= b < 2**256 for a, b in ops)
        assert len(ops) >= 64
