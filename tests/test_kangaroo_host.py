"""The kangaroo search's host side without a GPU: the jump table against the oracle, khh_kang_cpu_walk against the
Python model of the step rule (tests/kangaroo_ref.py), and a 24-bit interval solved through khh_kang_cpu_walk and the
real distinguished-point table."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khhost
from tests import adversarial as adv
from tests import kangaroo_ref as kr

START, END = 0x1000000, 0x2000000          # a 24-bit interval
SEED = 3


def _kang(key, **kw):
    return khhost.Kangaroo(khhost.pubkey(key), START, END, seed=kw.pop("seed", SEED), **kw)


def test_jump_table(ora):
    with _kang(START + 0x654321) as k, _kang(START + 5) as same, _kang(START + 5, seed=SEED + 1) as other:
        jt = k.jump_table()
        assert len(jt) == 32
        w = (END - START).bit_length()
        for s, (x, y) in jt:
            assert 1 <= s < 1 << ((w + 1) // 2 + 1)
            assert ora.pubkey(s).be64() == x.to_bytes(32, "big") + y.to_bytes(32, "big")
        assert len({x for _, (x, _) in jt}) == 32
        assert same.jump_table() == jt                    # the seed alone decides the table
        assert other.jump_table() != jt


@pytest.mark.parametrize("bits", [16, 24, 63, 64, 65, 130, 200])
def test_jump_distance_bound_by_width(bits):
    start = 1 << 20
    with khhost.Kangaroo(khhost.pubkey(start + 12345), start, start + (1 << bits), seed=1) as k:
        w = bits + 1
        assert k.width_bits == w
        assert all(1 <= s < 1 << ((w + 1) // 2 + 1) for s, _ in k.jump_table())
        assert k.herd << k.dp_bits <= 1 << max(w // 2 - 2, 1)


def test_widths_outside_the_accepted_range_are_refused():
    pub = khhost.pubkey(77)
    for start, end in ((0, (1 << 16) - 1), (0, (1 << 200) + 1), (5, 5), (9, 3), (1, adv.N + 1)):
        with pytest.raises(ValueError):
            khhost.Kangaroo(pub, start, end)
    khhost.Kangaroo(pub, 0, 1 << 16).close()
    khhost.Kangaroo(pub, 0, 1 << 200).close()


@pytest.fixture(scope="module")
def walked():
    """A few hundred kangaroos x 50 steps on the model, once: (jumps, herd, {dp: (final, dps, seconds)})."""
    with _kang(START + 0x654321) as k:
        jumps, herd = k.jump_table(), k.make_herd(300)
    return jumps, herd, {dp: kr.walk(jumps, herd, 50, dp) for dp in (0, 4)}


@pytest.mark.parametrize("dp", [0, 4])
def test_cpu_walk_matches_the_model(walked, dp):
    jumps, herd, ref = walked
    final, dps, seconds = ref[dp]
    with _kang(START + 0x654321) as k:
        got_final, got_dps, got_seconds = k.cpu_walk(herd, 50, dp)
    assert got_final == final
    assert got_dps == dps                                 # the same order too: step by step, ascending kangaroo
    assert got_seconds == seconds
    assert len(dps) == (300 * 50 if dp == 0 else len(dps)) and len(dps) > 0


def test_herd_is_tame_and_wild(ora):
    key = START + 0x654321
    with _kang(key) as k:
        herd = k.make_herd(40)
    q = kr.mul(key - START)
    w = END - START
    for i, (x, y, d) in enumerate(herd):
        p = kr.mul(d)
        assert (x, y) == (adv.add(q, p) if i & 1 else p)
        assert (1 <= d < w) if i & 1 else (w // 2 <= d < w // 2 + w)


MAX_STEPS = 400_000


@pytest.mark.parametrize("key", [START, END - 1, START + 0x654321], ids=["start", "end-1", "middle"])
def test_24_bit_interval_is_solved(key):
    with _kang(key) as k:
        jumps, herd = k.jump_table(), k.make_herd()
        # the case is a fair one only if the model alone finds the key within the same budget
        mkey, _ = kr.solve_model(jumps, herd, adv_pub(key), START, k.dp_bits, MAX_STEPS)
        assert mkey == key
        r = k.search(devices=(), max_steps=MAX_STEPS)
    assert r["key"] == key
    assert 0 < r["steps"] <= MAX_STEPS and r["dps"] > 0 and r["launches"] >= 1 and r["lost_dps"] == 0


def adv_pub(key):
    b = khhost.pubkey(key)
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")


def test_key_outside_the_interval_is_not_found():
    # far outside: the wild kangaroos start 2^60 away from the tame ones and jump less than 2^15 at a time.  (A key
    # just past an end can still be met and, being verified, is reported.)
    with _kang(END + (1 << 60)) as k:
        r = k.search(devices=(), max_steps=100_000)
    assert r["key"] is None
    assert 0 < r["steps"] <= 100_000


def test_merged_kangaroos_are_counted_and_replaced():
    key = START + 0x654321
    with _kang(key) as k:
        herd = k.make_herd()
        planted = herd[:3]
        planted[2] = herd[0]                              # kangaroo 2 walks in kangaroo 0's footsteps: both tame
        k.plant(planted)
        k.keep_herd()
        r = k.search(devices=(), max_steps=len(herd))     # one launch of one step; dp_bits is 0 for this width
        assert k.dp_bits == 0 and r["launches"] == 1 and r["key"] is None
        assert r["dead"] == 1
        final = k.final_herd()
        stepped, _, _ = k.cpu_walk(herd[:1], 1)
    assert final[0] == stepped[0]                         # the earlier one walks on
    x, y, d = final[2]
    assert final[2] != final[0] and (x, y) == kr.mul(d)   # the later one is a fresh tame kangaroo
    w = END - START
    assert w // 2 <= d < w // 2 + w


def test_ring_overflow_costs_points_not_correctness():
    key = START + 0x654321
    with _kang(key) as k:
        k.set_ring_capacity(100)                          # far below the 1,024 points of a one-step launch
        r = k.search(devices=(), max_steps=MAX_STEPS * 4)
    assert r["key"] == key and r["lost_dps"] > 0
