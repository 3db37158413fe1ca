"""Directed GPU tests of the kangaroo walk's state and edges (k_kang_walk, k_kang_scatter, k_kang_gather and the
khb_kang_* calls, through khbsgs.Engine) against the Python model of the step rule (tests/kangaroo_ref.py) on the herds
of tests/kang_cases.py.  Every comparison is exact.  A kangaroo whose (x, y, d) is silently wrong fails no end-to-end
search (its points give keys that fail verification), so these compare the whole state: stores and reads at first > 0,
growth of a herd that is not empty, two launches in flight with a store queued behind them, herds of 1 to 256 L + 1
kangaroos, the second choice's wrap 31 -> 0, the distinguished-point test at 31 and 32 bits, field-edge x as start and
as arrival, tiny and near-p dx, and the distance's wrap mod 2^256.

The jump table is kang_cases.fixed_table() throughout.  One model trajectory of 256 L + 7 kangaroos over 3 steps
(about 49,000 point additions) is computed once and every size, store and growth case is cut from it; the other herds
are a few hundred kangaroos."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khbsgs
from tests import adversarial as adv
from tests import kang_cases as kc
from tests import kangaroo_ref as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return khbsgs.kang_per_lane()


@pytest.fixture(scope="module")
def jumps():
    return kc.fixed_table()


@pytest.fixture(scope="module")
def big(jumps, L):
    """(states, seconds) of cheap_herd(256 L + 7) over 3 steps; read only."""
    return kc.trajectory(jumps, kc.cheap_herd(256 * L + 7, 21), 3)


@pytest.fixture(scope="module")
def edges(jumps, L):
    """(herd, marks, states, seconds) of the edge herd over 4 steps; read only."""
    herd, marks = kc.edge_herd(jumps, L)
    return (herd, marks) + kc.trajectory(jumps, herd, 4)


def _engine(jumps):
    e = khbsgs.Engine(0, lanes=256)
    e.kang_load_jumps(jumps)
    return e


def _stats(st):
    return st.steps_walked, st.n_dp, st.second_choice, st.dp_overflow


# ------------------------------------------------------------------------------------------ edges of the step
@pytest.mark.parametrize("dp", [0, 16, 31, 32])
def test_step_edges(jumps, L, edges, dp):
    herd, marks, states, seconds = edges
    n = len(herd)
    assert n == 2 * L + 5
    with _engine(jumps) as e:
        done = 0
        e.kang_store(herd)
        assert e.kang_read() == herd
        for steps in (1, 3):
            want, want_dps, want_sec = kr.walk(jumps, states[done], steps, dp)
            assert want == states[done + steps]
            dps, st = e.kang_walk(steps, dp)
            got = e.kang_read()
            assert got[L:2 * L] == want[L:2 * L]           # the directed lane first: one bad dx poisons its batch
            assert got == want
            assert sorted(dps) == sorted(want_dps) and len(dps) == len(want_dps)
            assert _stats(st) == (steps * n, len(want_dps), want_sec, 0)
            if done == 0:
                assert want_sec == 7                       # +-J_0, +-J_30, +-J_31 and the last lane's -J_31
                hit = {i for i, _, _ in dps}
                if dp == 0:
                    assert len(dps) == n
                if dp in (31, 32):
                    assert hit == {i for i, (x, _, _) in enumerate(want) if (x >> 32) & 0xFFFFFFFF == 0} | (
                        set(marks["dp:0x80000000"]) if dp == 31 else set())
                    assert hit >= set(marks["dp:0x0"]) and len(marks["dp:0x0"]) == 2
                    assert not hit & set(marks["dp:0x1"] + marks["dp:0xffff0000"])
                if dp == 16:
                    assert hit >= set(marks["dp:0x0"] + marks["dp:0x80000000"] + marks["dp:0xffff0000"])
                    assert not hit & set(marks["dp:0x1"])
                for i in marks["carry"]:                   # the distance add, the wrap mod 2^256 included
                    assert got[i][2] == (herd[i][2] + jumps[kr.pick(jumps, herd[i][0])[0]][0]) % (1 << 256)
            done += steps


# ------------------------------------------------------------------------------------------------ herd sizes
def _sizes(L):
    return [1, 2, L - 1, L, L + 1, 256 * L, 256 * L + 1]


@pytest.mark.parametrize("which", range(7), ids=["1", "2", "L-1", "L", "L+1", "256L", "256L+1"])
def test_herd_sizes(jumps, L, big, which):
    n = _sizes(L)[which]
    states, seconds = big
    with _engine(jumps) as e:
        e.kang_store(states[0][:n])
        assert e.kang_herd() == n and e.kang_read() == states[0][:n]
        dps, st = e.kang_walk(2, 0)
        assert _stats(st) == (2 * n, 2 * n, sum(sum(s[:n]) for s in seconds[:2]), 0)
        assert sorted(dps) == sorted(kc.points_of(states, 0, 2, 0, n))
        assert e.kang_read() == states[2][:n]
        # forget, then a herd of 5 in the state that was sized for n: only 5 walk and only 5 can be read
        e.kang_store([])
        assert e.kang_herd() == 0
        five = states[1][100:105]
        e.kang_store(five)
        dps, st = e.kang_walk(1, 0)
        assert _stats(st) == (5, 5, 0, 0)
        assert sorted(dps) == sorted((i, x, d) for i, (x, _, d) in enumerate(states[2][100:105]))
        assert e.kang_herd() == 5 and e.kang_read() == states[2][100:105]
        with pytest.raises(khbsgs.KhbError) as err:
            e.kang_read(0, 6)
        assert err.value.code == khbsgs.KHB_EINVAL
        with pytest.raises(khbsgs.KhbError) as err:
            e.kang_read(5, 1)
        assert err.value.code == khbsgs.KHB_EINVAL


# ------------------------------------------------------------------------------------- partial store and read
def test_partial_store_and_read(jumps, L, big):
    states, _ = big
    n = 3 * L + 7
    fresh = kc.cheap_herd(16, 33)
    with _engine(jumps) as e:
        e.kang_store(states[0][:n])
        e.kang_walk(2, 0)
        want = list(states[2][:n])
        assert e.kang_read() == want
        k = 0
        for first, count in [(0, 1), (L - 1, 1), (L, 1), (2 * L + 3, 1), (n - 1, 1), (L - 2, 5)]:
            roos = fresh[k:k + count]
            k += count
            e.kang_store(roos, first=first)
            want[first:first + count] = roos
            assert e.kang_herd() == n
            assert e.kang_read(first, count) == roos
        assert len(set(want)) == n and e.kang_read() == want
        windows = [(0, 1), (L - 1, 1), (L, 1), (2 * L + 3, 1), (n - 1, 1), (L - 2, 5), (1, n - 1), (L - 1, 2 * L + 2),
                   (63, 130), (n - 6, 6)]
        for first, count in windows:
            assert e.kang_read(first, count) == want[first:first + count], (first, count)
        assert e.kang_read(L + 5) == want[L + 5:]
        after, want_dps, _ = kr.walk(jumps, want, 2, 0)
        dps, st = e.kang_walk(2, 0)
        assert sorted(dps) == sorted(want_dps) and _stats(st) == (2 * n, 2 * n, 0, 0)
        assert e.kang_read() == after


# ----------------------------------------------------------------------------------------------------- growth
def test_growth_keeps_the_walked_herd(jumps, L, big):
    states, _ = big
    n = 256 * L + 7
    with _engine(jumps) as e:
        e.kang_store(states[0][:10])
        e.kang_walk(2, 0)
        e.kang_store(states[0][10:], first=10)             # more than one block of lanes: a wider stride
        assert e.kang_herd() == n
        got = e.kang_read()
        assert got[:10] == states[2][:10]                  # still the walked ones
        assert got[10:] == states[0][10:]
        want = states[3][:10] + states[1][10:]
        dps, st = e.kang_walk(1, 0)
        assert _stats(st) == (n, n, 0, 0)
        assert sorted(dps) == sorted((i, x, d) for i, (x, _, d) in enumerate(want))
        assert e.kang_read() == want


def test_growth_within_the_stride_and_by_one(jumps, L, big):
    """Appending inside the allocated lanes, and a growth that crosses the block by a single kangaroo."""
    states, _ = big
    with _engine(jumps) as e:
        e.kang_store(states[0][:L + 3])
        e.kang_walk(1, 0)
        e.kang_store(states[0][L + 3:256 * L], first=L + 3)            # fills the first block exactly
        e.kang_walk(1, 0)
        e.kang_store(states[0][256 * L:256 * L + 1], first=256 * L)    # one more: lane 256, a second block
        want = states[2][:L + 3] + states[1][L + 3:256 * L] + states[0][256 * L:256 * L + 1]
        assert e.kang_read() == want
        dps, st = e.kang_walk(1, 0)
        want = states[3][:L + 3] + states[2][L + 3:256 * L] + states[1][256 * L:256 * L + 1]
        assert _stats(st) == (256 * L + 1, 256 * L + 1, 0, 0)
        assert sorted(dps) == sorted((i, x, d) for i, (x, _, d) in enumerate(want))
        assert e.kang_read() == want


# ------------------------------------------------------------------------------------- two launches in flight
@pytest.mark.parametrize("ring", [None, 16], ids=["ring-default", "ring-16"])
def test_two_launches_in_flight(jumps, L, edges, ring):
    herd, marks, states, seconds = edges
    n = len(herd)
    a, b = 1, 3
    r = L + 7                                              # replaced behind both launches
    fresh = kc.cheap_herd(1, 44)[0]
    default = 1 << 18
    with _engine(jumps) as e:
        assert int(e.L.khb_kang_ring_capacity(e.h)) == default
        e.kang_store(herd)
        if ring:
            e.kang_set_ring_capacity(ring)
        e.kang_submit(a, 0)
        if ring:
            e.kang_set_ring_capacity(default)              # of later launches: the first keeps its 16
        e.kang_submit(b, 0)
        with pytest.raises(khbsgs.KhbError) as err:
            e.kang_submit(1, 0)
        assert err.value.code == khbsgs.KHB_EBUSY
        e.kang_store([fresh], first=r)
        first_want = kc.points_of(states, 0, a, 0)
        second_want = kc.points_of(states, a, a + b, 0)
        sec_a = sum(map(sum, seconds[:a]))
        sec_b = sum(map(sum, seconds[a:a + b]))
        assert sec_a == 7 and sec_a != sec_b
        dps, st = e.kang_collect(default if ring else None)        # room for more than the launch's ring kept
        if ring:
            assert _stats(st) == (a * n, a * n, sec_a, 1)
            assert len(dps) == ring == len(set(dps)) and set(dps) <= set(first_want)
        else:
            assert _stats(st) == (a * n, a * n, sec_a, 0)
            assert sorted(dps) == sorted(first_want)
        dps, st = e.kang_collect()
        assert _stats(st) == (b * n, b * n, sec_b, 0)
        assert sorted(dps) == sorted(second_want)
        assert sum(i == r for i, _, _ in dps) == b         # the points of the kangaroo replaced afterwards
        with pytest.raises(khbsgs.KhbError) as err:
            e.kang_collect(default)
        assert err.value.code == khbsgs.KHB_ESTATE
        want = list(states[a + b])
        want[r] = fresh
        assert e.kang_read() == want
        assert adv.on_curve(fresh[:2])
