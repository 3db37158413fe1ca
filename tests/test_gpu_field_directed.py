"""The field ops of fe_asm.hpp (khb_field_op 0 mul, 1 sqr, 6 sqr_add, 5 add_lazy, 3 sub) on operands aimed at each rare
condition, three families of them:

  carry_out    the carry-out of the reduction's V mads (tests/field_reduce.py): a carry in exactly one limb i for every
               i, in all limbs (products near p^2 and 2^512, the addend 2^256 - 1), H_i on either side of the
               threshold, and a carry together with the second fold's c3 (ops 0 and 6) and with c3 and the wrap (op 6;
               op 1's combinations and op 0's wrap are not aimed at);
  second_fold  each rare condition of the one-mad second fold (tests/field_fold2.py: r9, o, c2, each alone and with a V
               carry-out, and o with c2 for op 6), and fm_add_lazy / fm_sub on the operands whose carry into limb 2, a
               lane mask, is set (adversarial's lazy_c2 / sub_b2);
  columns      the forward-carried columns of the 512-bit products (tests/field_columns.py): both operands all ones,
               the first n limbs all ones, single-limb operands at every pair of places, columns that end with a full
               high word and a carry count, operands near p, and the first product of each masked column dropping its
               carry, alone and next to V carry-outs in the same waves.

Every family goes out in the same two batches: one fully directed wave, waves with one directed lane at a moving place,
waves with none, a partial last wave with a directed operand in its last lane.  The canonical result equals the Python
integer; the raw result (op | KHB_FIELD_OP_RAW) equals the limb model of tests/field_model.py bit for bit, filler
included, so a lane gets the same value whether or not its wave took a rare branch; and the model equals the integer
definition of the lazy value.  The file is also meant for a KHB_RARE_FORCE build, where every wave takes every rare
branch: tools/build_variant.sh with LIBDIR=1 and -DKHB_RARE_FORCE=1, then KHB_LIB_DIR=<that directory> pytest -m gpu on
this file (profiles/r10_columns/rare.txt, profiles/field_layer/README.md)."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd.khbsgs import FIELD_OP_RAW as RAW
from tests import adversarial as adv
from tests import field_columns as fc
from tests import field_fold2 as ff
from tests import field_model as fm
from tests import field_reduce as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


def _be(vals) -> bytes:
    return b"".join(v.to_bytes(32, "big") for v in vals)


def _ints(raw: bytes) -> list:
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


def _batches(op: int, directed: list, rng: random.Random):
    """Two batches with random filler.  The first (4,096 = 64 waves): wave 0 has all 64 lanes directed, waves
    1..31 exactly one directed lane each, at a lane that moves from wave to wave, waves 32..63 none.  The second
    (4,059: its last wave is partial) takes the rest at random places of its first 32 waves and one in its last
    lane; the waves between hold none."""
    first = [adv.random_operands(op, rng) for _ in range(4096)]
    where1 = list(range(64)) + [64 * w + (7 * w + 3) % 64 for w in range(1, 32)]
    for k, i in enumerate(where1):
        first[i] = directed[k]
    rest = directed[len(where1):]
    assert 2 <= len(rest) <= 2048
    n2 = 4096 - 37
    second = [adv.random_operands(op, rng) for _ in range(n2)]
    where2 = [n2 - 1] + rng.sample(range(2048), len(rest) - 1)
    for k, i in enumerate(where2):
        second[i] = rest[k]
    return (first, set(where1)), (second, set(where2))


def _check(eng, op: int, directed: list, seed: int):
    rng = random.Random(seed)
    for ops, where in _batches(op, directed, rng):
        ab, bb = _be(a for a, _ in ops), _be(b for _, b in ops)
        canon = _ints(eng.field_op(op, ab, bb))
        raw = _ints(eng.field_op(op | RAW, ab, bb))
        exact = [adv.EXACT[op](a, b) for a, b in ops]
        model = [fm.check(op, a, b)[0] for a, b in ops]       # the model, pinned to the integer definition
        bad = [i for i in range(len(ops)) if canon[i] != exact[i]]
        assert not bad, (op, "canonical", bad[:8], [i in where for i in bad[:8]])
        bad = [i for i in range(len(ops)) if raw[i] != model[i]]
        assert not bad, (op, "raw", bad[:8], [i in where for i in bad[:8]])


def _directed_carry_out(op: int) -> list:
    """Every class, 64 operands each, interleaved so that the fully directed wave holds all of them."""
    classes = [fr.one_limb(op, i, 64, seed=3) for i in range(8)]
    classes.append(fr.all_limbs(op, 64))
    classes.append([e[:2] for e in fr.edge(op, 64, seed=3)])
    if op == 0:
        classes.append(fr.mul_with_c3(64, seed=3))
    if op == 6:
        classes.append(fr.with_second_fold("c3", 64, seed=3))
        classes.append(fr.with_second_fold("wrap", 64, seed=3))
    assert all(len(c) >= 64 for c in classes)
    return [c[k] for k in range(64) for c in classes]


def _directed_second_fold(op: int) -> list:
    """64 operands of every class, interleaved so that the fully directed wave holds all of them."""
    if op in (5, 3):
        flag = "lazy_c2" if op == 5 else "sub_b2"
        ops = adv.directed_operands(op, flag, 256, seed=9)
        assert all(fm.device(op, a, b)[1][flag] == 1 for a, b in ops)
        return ops
    classes = list(ff.directed(op, 64, seed=9).values())
    return [c[k] for k in range(64) for c in classes]


def _directed_columns(op: int) -> list:
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
def test_field_ops_carry_out(eng, op):
    directed = _directed_carry_out(op)
    assert all(any(fr.expected_ov(op, a, b)) or (a, b) in [e[:2] for e in fr.edge(op, 64, seed=3)]
               for a, b in directed)
    _check(eng, op, directed, 60 + op)


@pytest.mark.parametrize("op", [0, 1, 6, 5, 3])
def test_field_ops_second_fold(eng, op):
    _check(eng, op, _directed_second_fold(op), 90 + op)


@pytest.mark.parametrize("op", [0, 1, 6])
def test_field_ops_columns(eng, op):
    _check(eng, op, _directed_columns(op), 140 + op)
