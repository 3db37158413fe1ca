"""The model of the baby-step table build (tests/baby_ref.py) pinned on the CPU: its walk against adversarial.add and
the oracle's k * G, its numpy bit arithmetic against Python integers, and whole tables against the CPU-built
khhost.Tables and the oracle's Bsgs at -n 0x40000000 -k 1 (m = 32,768) and -k 33 (l1ext > m, the overshoot)."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd import khhost
from tests import adversarial as adv
from tests import baby_ref


def test_walk_equals_single_steps_and_the_oracle(ora):
    rng = random.Random(41)
    for key0, count in ((1, 3000), (rng.randrange(2**200, adv.N - 2**40), 2500), (adv.N - 4000, 3999)):
        xs = baby_ref.walk_xs(ora, key0, count)
        assert xs == baby_ref.walk_slow(ora, key0, count)
        for i in (0, 1, 2, count // 2, count - 1):
            assert xs[i] == ora.pubkey(key0 + i).xy()[0]
    # a run that meets -G in the middle of a batch of runs (the step from -G is the point at infinity, which no
    # build may walk: the run ends on -G)
    xs = baby_ref.walk_xs(ora, adv.N - 2000, 2000)
    assert xs[-1] == ora.pubkey(1).xy()[0] and xs == baby_ref.walk_slow(ora, adv.N - 2000, 2000)


def test_bit_arithmetic_equals_python_integers(ora):
    rng = random.Random(43)
    pts = baby_ref.Points(ora, [rng.randrange(2**200, adv.N - 2**40) for _ in range(2)], 1)
    for geom in ((1, 2, 1), (5, 33, 2), (17, 129, 20), (16, 128, 255), (433, 3461, 20)):
        for limit in (1, 1025, 2048, 5000):
            assert baby_ref.bloom_level(pts, limit, geom) == baby_ref.bloom_level_slow(pts, limit, geom), (geom, limit)
    for m3 in (1, 1025, 2048, 5000):
        assert baby_ref.bp_records(pts, m3) == baby_ref.bp_records_slow(pts, m3)
    # a + b i wraps 2^64 for most i, and the wrap changes the position unless bits divides 2^64
    a, b = int(pts.a[0]), int(pts.b[0])
    wraps = [i for i in range(20) if a + b * i >= 2**64]
    assert wraps and any(((a + b * i) & baby_ref.M64) % 3461 != (a + b * i) % 3461 for i in wraps)


@pytest.mark.parametrize("k", [1, 33])
def test_model_equals_the_cpu_built_tables_and_the_oracle(ora, k):
    t = khhost.Tables("0x40000000", k, threads=8)
    o = ora.Bsgs("0x40000000", k, 8)
    try:
        assert (t.m, t.m2, t.m3, t.l1ext) == (o.m, o.m2, o.m3, o.l1ext) and t.m == 32768 * k
        assert (t.l1ext > t.m) == (k == 33)
        gpj = 16                                   # jobs of 16,384 consecutive keys, the product's centres
        n_jobs = -(-t.l1ext // (gpj * 1024))
        centres = [j * gpj * 1024 + 513 for j in range(n_jobs)]
        geoms = [t.bloom_concat(l)[1:] for l in (1, 2, 3)]
        gate, lg = t.gate()
        ref = baby_ref.baby_build_ref(ora, centres, gpj, t.l1ext, t.m2, t.m3, geoms, lg, t.gate_probes(), True)
        assert ref["points"].xs[0] == ora.pubkey(1).xy()[0]          # key ic + 1
        for l in (1, 2, 3):
            assert ref[f"l{l}"] == t.bloom_concat(l)[0], l
            assert (ref[f"l{l}"],) + tuple(geoms[l - 1]) == o.bloom_concat(l), l
        assert lg >= 13 and ref["gate"] == gate
        bp = ref["bp"]
        recs = sorted((bp[16 * i:16 * i + 6], int.from_bytes(bp[16 * i + 8:16 * i + 16], "little"))
                      for i in range(t.m3))
        assert all(bp[16 * i + 6:16 * i + 8] == b"\0\0" for i in range(t.m3))
        assert recs == t.bptable()
    finally:
        t.close()
        o.close()
