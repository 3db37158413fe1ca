"""GPU parity for the kangaroo walk (k_kang_walk through khb_kang_* and khhost.Kangaroo) against the Python model of
the step rule (tests/kangaroo_ref.py): every ring entry, every final state and every counter is compared exactly.
With L = khb_kang_per_lane() the herds are 64 L + 5 kangaroos (one full wave and a partial lane) and 320 L + 5 (which
crosses a block); each herd's model walk is computed once and shared."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khbsgs, khhost
from tests import adversarial as adv
from tests import kangaroo_ref as kr

pytestmark = pytest.mark.gpu

START, END = 1 << 44, (1 << 44) + (1 << 40)      # a 40-bit interval
KEY = START + 0x9A3C5E7F11
SEED = 11


def _sizes():
    L = khbsgs.kang_per_lane()
    return [64 * L + 5, 256 * L + 64 * L + 5]


@pytest.fixture(scope="module")
def kang():
    k = khhost.Kangaroo(khhost.pubkey(KEY), START, END, seed=SEED)
    yield k
    k.close()


@pytest.fixture(scope="module")
def models(kang):
    """{n: (herd, after 3 steps, its points at dp 0, after K = 10^5 // n steps, all K steps' points at dp 0, K)}."""
    jumps = kang.jump_table()
    out = {}
    for n in _sizes():
        herd = kang.make_herd(n)
        k_steps = max(4, 100_000 // n)
        after3, dps3, _ = kr.walk(jumps, herd, 3, 0)
        after_k, dps_rest, _ = kr.walk(jumps, after3, k_steps - 3, 0)
        out[n] = (herd, after3, dps3, after_k, dps3 + dps_rest, k_steps)
    return out


@pytest.mark.parametrize("which", [0, 1], ids=["wave+5", "block+wave+5"])
def test_step_parity(kang, models, which):
    n = _sizes()[which]
    herd, after3, dps3, _, _, _ = models[n]
    kang.load_herd(herd)
    assert kang.read_herd() == herd
    dps, st = kang.walk(3, 0)
    assert st["n_dp"] == 3 * n == len(dps) and not st["dp_overflow"]
    assert st["steps_walked"] == 3 * n
    assert sorted(dps) == sorted(dps3)
    assert kang.read_herd() == after3


@pytest.mark.parametrize("which", [0, 1], ids=["wave+5", "block+wave+5"])
def test_distinguished_points(kang, models, which):
    n = _sizes()[which]
    herd, _, _, after_k, dps_all, k_steps = models[n]
    assert n * k_steps <= 100_000 + 4 * n
    want = sorted(p for p in dps_all if kr.is_dp(p[1], 4))
    assert len(want) > 50                                   # about n K / 16
    kang.load_herd(herd)
    dps, st = kang.walk(k_steps, 4)
    assert all(i < n for i, _, _ in dps)                    # an empty trailing slot never reports
    assert sorted(dps) == want and st["n_dp"] == len(want)
    assert st["steps_walked"] == n * k_steps
    assert kang.read_herd() == after_k


def _seed_with_fixed_point():
    """A seed whose table has a j with J_j.x mod 32 == j (about two tables in three), found on the CPU."""
    for seed in range(100, 200):
        k = khhost.Kangaroo(khhost.pubkey(KEY), START, END, seed=seed)
        jt = k.jump_table()
        js = [j for j, (_, (x, _)) in enumerate(jt) if x & 31 == j]
        if js:
            return k, jt, js[0]
        k.close()
    raise AssertionError("no seed with a fixed jump in 100 tables")


def test_second_choice_rule():
    k, jt, j = _seed_with_fixed_point()
    with k:
        L = khbsgs.kang_per_lane()
        n = 64 * L + 5
        herd = k.make_herd(n)
        jx, jy = jt[j][1]
        herd[L + 3] = (jx, jy, 5)                           # J_j and -J_j in lane 1, otherwise random
        herd[2 * L - 2] = (jx, adv.P - jy, 7)
        assert kr.pick(jt, jx) == ((j + 1) & 31, True)
        want, dps_want, seconds = kr.walk(jt, herd, 1, 0)
        assert seconds == 2
        k.load_herd(herd)
        dps, st = k.walk(1, 0)
        assert st["second_choice"] == 2
        got = k.read_herd()
        assert got[L:2 * L] == want[L:2 * L]                # the whole lane: a zero dx would have poisoned its batch
        assert got == want and sorted(dps) == sorted(dps_want)


def test_distance_carries(kang):
    L = khbsgs.kang_per_lane()
    n = 64 * L + 5
    herd = kang.make_herd(n)
    planted = {1: (1 << 32) - 1, L + 2: (1 << 64) - 1, 2 * L + 3: (1 << 128) - 1, n - 1: (1 << 224) - 1}
    for i, d in planted.items():
        herd[i] = (herd[i][0], herd[i][1], d)
    want, _, _ = kr.walk(kang.jump_table(), herd, 1, 0)
    kang.load_herd(herd)
    kang.walk(1, 0)
    got = kang.read_herd()
    for i in planted:
        assert got[i] == want[i], i
    assert got == want


def test_ring_overflow(kang, models):
    n = _sizes()[0]
    herd, after3, dps3, _, _, _ = models[n]
    kang.load_herd(herd)
    kang.set_ring_capacity(16)
    try:
        dps, st = kang.walk(3, 0)
    finally:
        kang.set_ring_capacity(1 << 18)
    assert st["dp_overflow"] == 1
    assert st["n_dp"] == 3 * n                              # the counter goes on counting
    assert len(dps) == 16 and set(dps) <= set(dps3)         # the first 16 entries are real points
    assert st["steps_walked"] == 3 * n
    assert kang.read_herd() == after3                       # the walk itself is not affected


def test_argument_checks(kang):
    jt = kang.jump_table()
    herd = kang.make_herd(10)

    def einval(f, *a):
        with pytest.raises(khbsgs.KhbError) as e:
            f(*a)
        assert e.value.code == khbsgs.KHB_EINVAL

    with khbsgs.Engine(0) as e:
        einval(e.kang_submit, 1, 0)                         # no jumps
        dup = list(jt)
        dup[9] = dup[4]
        einval(e.kang_load_jumps, dup)                      # duplicate J.x
        einval(e.kang_submit, 1, 0)                         # still no jumps
        e.kang_load_jumps(jt)
        einval(e.kang_submit, 1, 0)                         # no herd
        e.kang_store(herd)
        einval(e.kang_submit, 0, 0)                         # steps == 0
        einval(e.kang_submit, 1, 33)                        # dp_bits > 32
        einval(e.kang_store, herd, 11)                      # a store that would leave a gap
        with pytest.raises(khbsgs.KhbError) as none:        # nothing was launched by any of them
            e.kang_collect()
        assert none.value.code == khbsgs.KHB_ESTATE
        assert e.kang_read() == herd
        dps, st = e.kang_walk(1, 32)                        # dp_bits = 32 is accepted
        assert st.steps_walked == 10 and st.n_dp == len(dps)


@pytest.mark.parametrize("key, devices", [(KEY, (0,)), (KEY, (0, 0)), (START, (0,)), (END - 1, (0,))],
                         ids=["middle", "two-herds", "start", "end-1"])
def test_end_to_end_40_bit(key, devices):
    with khhost.Kangaroo(khhost.pubkey(key), START, END, seed=SEED) as k:
        r = k.search(devices=devices)
    print(f"40-bit solve: steps {r['steps']} = {r['steps'] / (2 * 2 ** 20):.2f} x 2 sqrt(W), dps {r['dps']}, "
          f"dead {r['dead']}, launches {r['launches']}, {r['seconds']:.2f} s")
    assert r["key"] == key
    assert r["steps"] > 0 and r["launches"] >= 1


def test_end_to_end_key_outside():
    with khhost.Kangaroo(khhost.pubkey(END + (1 << 80)), START, END, seed=SEED) as k:
        budget = 6 * k.herd
        r = k.search(devices=(0,), max_steps=budget)
    assert r["key"] is None
    assert 0 < r["steps"] <= budget
