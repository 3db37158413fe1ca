"""The model of the one-mad second fold (tests/field_fold2.py) against field_reduce.v_reduce, the model of the general
fold that the device's raw value was pinned to before: equal on every directed class of field_fold2, on the classes
of field_reduce and on 10^5 random operands per op, of which at most 1 in 10^4 may leave the fast path (so a model
that sends everything through the general fold fails).  fm_add_lazy / fm_sub with their carry in a lane mask equal
adversarial.MODEL on its lazy_c2 / sub_b2 classes and on random operands.  No GPU."""
from __future__ import annotations

import random

import pytest

from tests import adversarial as adv
from tests import field_fold2 as ff
from tests import field_reduce as fr


@pytest.mark.parametrize("op", [0, 1, 6])
def test_directed_classes(op):
    for want, ops in ff.directed(op, 24, seed=1).items():
        assert len(ops) == 24
        for a, b in ops:
            v, f = ff.f_op(op, a, b)
            assert ff.has_exactly(f, want) and f["path"] == "general", (op, want, f)
            assert v == fr.v_op(op, a, b)[0], (op, want, hex(a), hex(b))
            assert v % adv.P == adv.EXACT[op](a, b) and v < 2**256


@pytest.mark.parametrize("op", [0, 1, 6])
def test_existing_classes(op):
    ops = [ab for i in range(8) for ab in fr.one_limb(op, i, 16, seed=5)]
    ops += fr.all_limbs(op, 64) + [e[:2] for e in fr.edge(op, 256, seed=5)]
    if op == 0:
        ops += fr.mul_with_c3(16, seed=5)
    if op == 6:
        ops += fr.with_second_fold("c3", 16, seed=5) + fr.with_second_fold("wrap", 16, seed=5)
    ops += adv.directed_operands(op, "c3", 16, seed=5) + adv.directed_operands(op, "wrap", 16, seed=5)
    r9 = 0
    for a, b in ops:
        v, f = ff.f_op(op, a, b)
        ref, g = fr.v_op(op, a, b)
        assert v == ref and f["ov"] == g["ov"], (op, hex(a), hex(b))
        assert f["path"] == "general" or not (any(g["ov"]) or g["c3"])
        r9 += f["r9"] and not any(f["ov"])
    assert r9 > 0          # edge holds operands with R9 = 1 and no V carry-out


@pytest.mark.parametrize("op", [0, 1, 6])
def test_random_operands_take_the_fast_path(op):
    rng = random.Random(600 + op)
    n, slow = 100_000, 0
    for _ in range(n):
        a, b = adv.random_operands(op, rng)
        v, f = ff.f_op(op, a, b)
        assert v == fr.v_op(op, a, b)[0], (op, hex(a), hex(b))
        slow += f["path"] != "fast"
    assert slow * 10_000 <= n, slow


@pytest.mark.parametrize("op,flag,model", [(5, "lazy_c2", ff.f_add_lazy), (3, "sub_b2", ff.f_sub)])
def test_mask_carry_of_add_lazy_and_sub(op, flag, model):
    rng = random.Random(610 + op)
    ops = adv.directed_operands(op, flag, 256, seed=7)
    assert all(model(a, b)[1] == 1 for a, b in ops)
    ops += [adv.random_operands(op, rng) for _ in range(20_000)]
    for a, b in ops:
        assert model(a, b) == adv.MODEL[op](a, b), (op, hex(a), hex(b))
        assert model(a, b)[0] % adv.P == adv.EXACT[op](a, b)
