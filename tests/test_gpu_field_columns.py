"""fm_mul / fm_sqr / fm_sqr_add (khb_field_op 0, 1, 6) on operands aimed at the forward-carried columns of the
512-bit products (tests/field_columns.py): both operands all ones, the first n limbs all ones, single-limb operands
at every pair of places, columns that end with a full high word and a carry count, operands near p, and the first
product of each masked column dropping its carry, alone and, with the reduction's operands of
tests/field_reduce.py in the same waves, next to V carry-outs.  The batches are test_gpu_field_reduce's: one fully
directed wave, waves with one directed lane at a moving place, waves with none, a partial last wave with a directed
operand in its last lane.  The canonical result equals the Python integer; the raw result (op | KHB_FIELD_OP_RAW)
equals tests/field_fold2.py's model, the parent's lazy value, bit for bit, filler included, so a lane gets the same
value whether or not its wave took a rare branch.  The file is also meant for a KHB_RARE_FORCE build (every wave takes
every rare branch): profiles/r10_columns/rare.txt."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd.khbsgs import FIELD_OP_RAW as RAW
from tests import adversarial as adv
from tests import field_columns as fc
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
    """Every family of field_columns for the op, then operands whose V mads carry out (all limbs, and one limb each),
    interleaved with first-product drops so that the fully directed wave holds both kinds."""
    ops = fc.directed(op, 4, seed=9)
    masked = fc.MUL_MASKED if op == 0 else fc.SQR_MASKED
    assert {k for a, b in ops for k in fc.drops(op, a, b)} == set(masked)
    carry = fr.all_limbs(op, 8) + [fr.one_limb(op, i, 1, seed=4)[0] for i in range(8)]
    assert all(any(fr.expected_ov(op, a, b)) for a, b in carry)
    drop = [fc.first_drop(op, k, 1, seed=13)[0] for k in masked]
    mixed = [x for pair in zip(carry, drop * 2) for x in pair]
    ops = mixed + ops
    assert 96 <= len(ops) <= 2048 + 95
    return ops


@pytest.mark.parametrize("op", [0, 1, 6])
def test_field_ops_columns(eng, op):
    directed = _directed(op)
    rng = random.Random(140 + op)
    for ops, where in _batches(op, directed, rng):
        ab, bb = _be(a for a, _ in ops), _be(b for _, b in ops)
        canon = _ints(eng.field_op(op, ab, bb))
        raw = _ints(eng.field_op(op | RAW, ab, bb))
        exact = [adv.EXACT[op](a, b) for a, b in ops]
        model = [ff.MODEL[op](a, b)[0] for a, b in ops]
        assert all(fc.t_op(op, a, b) == (a * b if op == 0 else a * a) for a, b in ops)
        bad = [i for i in range(len(ops)) if canon[i] != exact[i]]
        assert not bad, (op, "canonical", bad[:8], [i in where for i in bad[:8]])
        bad = [i for i in range(len(ops)) if raw[i] != model[i]]
        assert not bad, (op, "raw", bad[:8], [i in where for i in bad[:8]])
