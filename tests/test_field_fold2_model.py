"""The model of the one-mad second fold (tests/field_model.py's device) against the integer definition of the lazy
value (field_model.lazy): equal on every directed class of field_fold2, on the classes of field_reduce and on 10^5
random operands per op, of which at most 1 in 10^4 may leave the fast path (so a model that sends everything through
the general fold fails).  fm_add_lazy / fm_sub with their carry in a lane mask equal their integer definitions on
adversarial's lazy_c2 / sub_b2 classes and on random operands, and adversarial.MODEL is the same model.  No GPU."""
from __future__ import annotations

import random

import pytest

from tests import adversarial as adv
from tests import field_fold2 as ff
from tests import field_model as fm
from tests import field_reduce as fr


@pytest.mark.parametrize("op", [0, 1, 6])
def test_directed_classes(op):
    for want, ops in ff.directed(op, 24, seed=1).items():
        assert len(ops) == 24
        for a, b in ops:
            v, f = fm.check(op, a, b)
            assert ff.has_exactly(f, want) and f["path"] == "general", (op, want, f)
            assert adv.MODEL[op](a, b) == (v, f["c3"], f["wrap"])


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
        v, f = fm.check(op, a, b)
        g = fm.lazy(op, a, b)[1]
        assert f["path"] == "general" or not (any(g["ov"]) or g["c3"])
        r9 += f["r9"] and not any(f["ov"])
    assert r9 > 0          # edge holds operands with R9 = 1 and no V carry-out


@pytest.mark.parametrize("op", [0, 1, 6])
def test_random_operands_take_the_fast_path(op):
    rng = random.Random(600 + op)
    n, slow = 100_000, 0
    for _ in range(n):
        a, b = adv.random_operands(op, rng)
        slow += fm.check(op, a, b)[1]["path"] != "fast"
    assert slow * 10_000 <= n, slow


@pytest.mark.parametrize("op,flag", [(5, "lazy_c2"), (3, "sub_b2")],
                         ids=["5-lazy_c2-f_add_lazy", "3-sub_b2-f_sub"])      # the ids these cases have always had
def test_mask_carry_of_add_lazy_and_sub(op, flag):
    rng = random.Random(610 + op)
    ops = adv.directed_operands(op, flag, 256, seed=7)
    assert all(fm.device(op, a, b)[1][flag] == 1 for a, b in ops)
    ops += [adv.random_operands(op, rng) for _ in range(20_000)]
    for a, b in ops:
        v, f = fm.check(op, a, b)
        assert adv.MODEL[op](a, b) == (v, f[flag]), (op, hex(a), hex(b))
