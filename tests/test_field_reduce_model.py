"""The per-limb reduction of fe_asm.hpp (V_i = 977 H_i + (H_i : Lw_i), carry-outs added back at word i + 2)
as the limb model of tests/field_model.py against the integer definition of the lazy value (field_model.lazy):
the raw value and the c3 / wrap / ov flags must be equal for ops 0, 1, 6 on 100,000 random operands and on
every directed class of tests/field_reduce.py, and each directed operand must raise the carry-out flags it is
aimed at."""
from __future__ import annotations

import random

import pytest

from tests import adversarial as adv
from tests import field_model as fm
from tests import field_reduce as fr

OPS = (0, 1, 6)


def _same(op, a, b):
    return fm.check(op, a, b)[1]          # value, c3, wrap, ov equal the integers'; < 2^256; congruent


@pytest.mark.parametrize("op", OPS)
def test_random_operands(op):
    rng = random.Random(2000 + op)
    for _ in range(100000):
        _same(op, *adv.random_operands(op, rng))


@pytest.mark.parametrize("op", OPS)
def test_one_limb(op):
    for i in range(8):
        for a, b in fr.one_limb(op, i, 64, seed=1):
            assert _same(op, a, b)["ov"] == [int(k == i) for k in range(8)]


@pytest.mark.parametrize("op", OPS)
def test_all_limbs(op):
    ops = fr.all_limbs(op, 64)
    named = fr.NAMED_OV[op]
    for k, (a, b) in enumerate(ops):
        assert _same(op, a, b)["ov"] == (named[k] if k < len(named) else [1] * 8), (op, k)


@pytest.mark.parametrize("op", OPS)
def test_threshold_edge(op):
    """H_i = 2^32 - 979, - 978: no carry; - 976: carry; - 977: carry exactly when Lw_i >= 977^2."""
    seen = set()
    for a, b, i, hv in fr.edge(op, 128, seed=1):
        ov = _same(op, a, b)["ov"]
        t = a * b if op == 0 else a * a
        assert (t >> (256 + 32 * i)) & adv.M32 == hv
        lw = (((t & fr.M256) + (b if op == 6 else 0)) >> (32 * i)) & adv.M32
        want = {fr.EDGE[0]: 0, fr.EDGE[1]: 0, fr.EDGE[2]: int(lw >= 977 * 977), fr.EDGE[3]: 1}[hv]
        assert ov == [want if k == i else 0 for k in range(8)], (op, i, hex(hv), ov)
        seen.add((hv, want))
    assert {(fr.EDGE[0], 0), (fr.EDGE[1], 0), (fr.EDGE[2], 1), (fr.EDGE[3], 1)} <= seen


@pytest.mark.parametrize("flag", ["c3", "wrap"])
def test_carry_out_with_second_fold(flag):
    for a, w in fr.with_second_fold(flag, 64, seed=1):
        f = _same(6, a, w)
        assert any(f["ov"]) and f["c3"] == 1 and f["wrap"] == int(flag == "wrap")


def test_mul_carry_out_with_c3():
    for a, b in fr.mul_with_c3(64, seed=1):
        f = _same(0, a, b)
        assert f["ov"][4:] == [1] * 4 and f["c3"] == 1 and f["wrap"] == 0
