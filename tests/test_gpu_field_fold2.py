"""fm_mul / fm_sqr / fm_sqr_add (khb_field_op 0, 1, 6) on operands aimed at each rare condition of the one-mad second
fold (tests/field_fold2.py: r9, o, c2, each alone and with a V carry-out, and o with c2 for op 6), and fm_add_lazy /
fm_sub (ops 5, 3) on the operands whose carry into limb 2, now a lane mask, is set (adversarial's lazy_c2 / sub_b2).
The batches are test_gpu_field_reduce's: one fully directed wave, waves with one directed lane at a moving place,
waves with none, a partial last wave with a directed operand in its last lane.  The canonical result equals the
Python integer; the raw result (op | KHB_FIELD_OP_RAW) equals the model of the general fold bit for bit, filler
included, so a lane gets the same value whether or not its wave took the rare branch.  The file is also meant for a
KHB_RARE_FORCE build (every wave takes every rare branch): profiles/r09_fold2/rare.txt."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd.khbsgs import FIELD_OP_RAW as RAW
from tests import adversarial as adv
from tests import field_fold2 as ff
from tests import field_reduce as fr
from tests.test_gpu_field_reduce import _batches, _be, _ints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


def _directed(op: int) -> list:
    """64 operands of every class, interleaved so that the fully directed wave holds all of them."""
    if op in (5, 3):
        ops = adv.directed_operands(op, "lazy_c2" if op == 5 else "sub_b2", 256, seed=9)
        assert all(ff.MODEL[op](a, b)[1] == 1 for a, b in ops)
        return ops
    classes = list(ff.directed(op, 64, seed=9).values())
    return [c[k] for k in range(64) for c in classes]


def _reference(op: int, a: int, b: int) -> int:
    """The raw value the parent's code returned: the general fold's model (ops 0, 1, 6), adversarial's (5, 3)."""
    return fr.v_op(op, a, b)[0] if op in (0, 1, 6) else adv.MODEL[op](a, b)[0]


@pytest.mark.parametrize("op", [0, 1, 6, 5, 3])
def test_field_ops_second_fold(eng, op):
    directed = _directed(op)
    rng = random.Random(90 + op)
    for ops, where in _batches(op, directed, rng):
        ab, bb = _be(a for a, _ in ops), _be(b for _, b in ops)
        canon = _ints(eng.field_op(op, ab, bb))
        raw = _ints(eng.field_op(op | RAW, ab, bb))
        exact = [adv.EXACT[op](a, b) for a, b in ops]
        model = [ff.MODEL[op](a, b)[0] for a, b in ops]
        assert model == [_reference(op, a, b) for a, b in ops]
        bad = [i for i in range(len(ops)) if canon[i] != exact[i]]
        assert not bad, (op, "canonical", bad[:8], [i in where for i in bad[:8]])
        bad = [i for i in range(len(ops)) if raw[i] != model[i]]
        assert not bad, (op, "raw", bad[:8], [i in where for i in bad[:8]])
