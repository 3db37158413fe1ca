"""tests/kang_cases.py without a GPU: every constructed case has the property its name claims, by the Python model of
the step rule alone (tests/kangaroo_ref.py), and the directed herds that need no fixed_table() go through the host's
restatement of the rule (khhost.Kangaroo.cpu_walk, with that handle's own jump table) and must give the model's final
herd, distinguished points and second-choice count."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khhost
from tests import adversarial as adv
from tests import kang_cases as kc
from tests import kangaroo_ref as kr

P = adv.P
START, END = 1 << 44, (1 << 44) + (1 << 40)
KEY = START + 0x9A3C5E7F11
SEED = 11
L = 64                                  # the herds' lane width here; the GPU module asks the library


@pytest.fixture(scope="module")
def fixed():
    return kc.fixed_table()


@pytest.fixture(scope="module")
def handle():
    k = khhost.Kangaroo(khhost.pubkey(KEY), START, END, seed=SEED)
    yield k
    k.close()


@pytest.fixture(scope="module", params=["fixed", "seeded"])
def jumps(request, fixed, handle):
    return fixed if request.param == "fixed" else handle.jump_table()


def _one_step(jumps, pt):
    (x, y, _), second = kr.step(jumps, (pt[0], pt[1], 0))
    return (x, y), second


def test_fixed_table(fixed):
    assert len(fixed) == 32 and len({x for _, (x, _) in fixed}) == 32
    assert min(s for s, _ in fixed) == 1001
    for j, (s, J) in enumerate(fixed):
        assert J[0] & 31 == j and kr.mul(s) == J
        for pt in (J, adv.neg(J)):                         # +-J_j takes the second choice, 31 wraps to 0
            assert kr.pick(fixed, pt[0]) == ((j + 1) & 31, True)
    assert kr.pick(fixed, fixed[31][1][0]) == (0, True)
    # the first hit per residue: no smaller k >= 1001 has that residue
    pt, seen = kr.mul(1001), {}
    for k in range(1001, max(s for s, _ in fixed) + 1):
        seen.setdefault(pt[0] & 31, k)
        pt = adv.add(pt, kr.G)
    assert [seen[j] for j in range(32)] == [s for s, _ in fixed]


def test_predecessors(jumps):
    target = kr.mul(0xC0FFEE)
    n = 0
    for k in range(40):
        for j, s in kc.predecessors(jumps, target):
            assert adv.on_curve(s) and kr.pick(jumps, s[0]) == (j, False)
            assert _one_step(jumps, s) == (target, False)
            n += 1
        # and nothing is left out: a predecessor by any jump is in the list
        for j, (_, J) in enumerate(jumps):
            s = adv.add(target, adv.neg(J))
            if s is not None and s[0] & 31 == j and s[0] != J[0]:
                assert (j, s) in kc.predecessors(jumps, target)
        target = adv.add(target, kr.G)
    assert n > 10                                          # about one per target


@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_arriving_lands_in_its_class(jumps, cls):
    arr = kc.arriving(jumps, cls)
    assert kc.MIN_REACHABLE <= len(arr) <= kc.CLASS_POINTS, (cls, len(arr))
    points = adv.class_points(cls, kc.CLASS_POINTS, 3)
    for start, target in arr:
        assert target in points and adv.in_class(cls, target)
        assert adv.on_curve(start) and _one_step(jumps, start) == (target, False)


def test_dp_points_verdicts(jumps):
    dps = kc.dp_points(jumps)
    assert [w for w, _, _ in dps] == [0, 0x80000000, 1, 0xFFFF0000]
    want = {0: (True, True, True), 0x80000000: (True, True, False), 1: (False, False, False),
            0xFFFF0000: (True, False, False)}
    for word, start, target in dps:
        assert adv.on_curve(target) and (target[0] >> 32) & 0xFFFFFFFF == word
        assert _one_step(jumps, start) == (target, False)
        assert tuple(kr.is_dp(target[0], dp) for dp in (16, 31, 32)) == want[word], hex(word)
        assert kr.is_dp(target[0], 0)


@pytest.mark.parametrize("j", [0, 31])
@pytest.mark.parametrize("sign", [+1, -1])
def test_near_jump_dx(jumps, j, sign):
    pt, dx = kc.near_jump(jumps, j, sign)
    jx = jumps[j][1][0]
    assert adv.on_curve(pt) and kr.pick(jumps, pt[0]) == (j, False)
    assert dx == (jx - pt[0]) % P
    small = dx if sign > 0 else P - dx
    assert 32 <= small < 32 * 64 and (dx < 1 << 11) == (sign > 0)
    e = (jx - j) % 32 if sign > 0 else (j - jx) % 32
    assert small % 32 == e
    for t in range(1, small // 32):                        # the smallest t: nothing nearer is on the curve
        assert adv.lift_x(jx - e - 32 * t if sign > 0 else jx + e + 32 * t) is None


def test_near_jump_on_the_fixed_table_is_a_multiple_of_32(fixed):
    for j in (0, 31):
        assert kc.near_jump(fixed, j, +1)[1] % 32 == 0
        assert (P - kc.near_jump(fixed, j, -1)[1]) % 32 == 0


def test_cheap_herd_and_trajectory(fixed):
    herd = kc.cheap_herd(40, 1)
    assert len({x for x, _, _ in herd}) == 40
    for x, y, d in herd[:3] + herd[-2:]:
        assert (x, y) == kr.mul(d)
    states, seconds = kc.trajectory(fixed, herd, 3)
    for t in (1, 3):
        final, dps, sec = kr.walk(fixed, herd, t, 2)
        assert states[t] == final and sum(map(sum, seconds[:t])) == sec
        assert kc.points_of(states, 0, t, 2) == dps
    assert kc.points_of(states, 1, 3, 0, 7) == kr.walk(fixed, states[1][:7], 2, 0)[1]


def test_edge_herd_holds_what_it_names(jumps):
    herd, marks = kc.edge_herd(jumps, L)
    n = len(herd)
    assert n == 2 * L + 5
    assert all(adv.on_curve((x, y)) for x, y, _ in herd)
    directed = sorted(i for k, v in marks.items() if k != "carry" for i in v)
    assert len(set(directed)) == len(directed)
    assert all(L <= i < 2 * L or n - 5 <= i < n - 1 for i in directed)       # one lane, and the partial last one
    assert sum(i >= n - 5 for i in directed) == 4
    assert len(marks["class"]) == 10 and len(marks["near"]) == 5 and len(marks["jump"]) == 7
    for c, cls in enumerate(kc.CLASSES):
        for i in marks["class"][2 * c:2 * c + 2]:
            assert adv.in_class(cls, herd[i][:2])
        assert len(marks[f"arriving:{cls}"]) >= kc.MIN_REACHABLE
    after, _, seconds = kr.walk(jumps, herd, 1, 0)
    for cls in kc.CLASSES:
        for i in marks[f"arriving:{cls}"]:
            assert adv.in_class(cls, after[i][:2])
    # the second choices: +-J_j with J_j.x & 31 == j, which is all seven with fixed_table()
    want = sum(herd[i][0] & 31 == j for i in marks["jump"] for j in (0, 30, 31) if herd[i][0] == jumps[j][1][0])
    assert seconds == want
    if all(J[0] & 31 == j for j, (_, J) in enumerate(jumps)):
        assert seconds == 7
    # the distinguished points of the first step at 32 bits are exactly the arrivals with word 1 == 0, at 31 bits
    # the 0x80000000 one as well, at 16 bits the 0xFFFF0000 one too
    at = {dp: {i for i, (x, _, _) in enumerate(after) if kr.is_dp(x, dp)} for dp in (16, 31, 32)}
    # (a class-A arrival has x < 2^32 + 977 and a class-C one x mod 2^96 < 2^33, so their word 1 is 0 or 1: those
    # with 0 are such points of their own)
    small = {i for cls in "AC" for i in marks[f"arriving:{cls}"] if (after[i][0] >> 32) & 0xFFFFFFFF == 0}
    assert at[32] == set(marks["dp:0x0"]) | small and len(at[32]) == 2 + len(small)
    assert at[31] == at[32] | set(marks["dp:0x80000000"]) and len(at[31]) == 3 + len(small)
    assert at[16] >= at[31] | set(marks["dp:0xffff0000"]) and not at[16] & set(marks["dp:0x1"])
    # the distances: every carry length, the wrap mod 2^256 on a kangaroo that moves
    assert sorted({herd[i][2] for i in marks["carry"]}) == sorted(kc.CARRY_DISTANCES)
    wrapped = [i for i in marks["carry"] if herd[i][2] == (1 << 256) - 1]
    assert len(wrapped) == 2 and all(after[i][2] < 1 << 64 for i in wrapped)


@pytest.mark.parametrize("dp", [0, 16, 31, 32])
def test_cpu_walk_on_the_edge_herd(handle, dp):
    jumps = handle.jump_table()
    herd, marks = kc.edge_herd(jumps, L)
    for steps in (1, 4):
        want, dps, seconds = kr.walk(jumps, herd, steps, dp)
        got, got_dps, got_seconds = handle.cpu_walk(herd, steps, dp)
        assert got == want and got_dps == dps and got_seconds == seconds
        assert len(dps) == (steps * len(herd) if dp == 0 else len(dps))
    if dp >= 31:                                           # the planted ones are among the first step's points
        first = {i for i, _, _ in handle.cpu_walk(herd, 1, dp)[1]}
        assert first >= set(marks["dp:0x0"]) and not first & set(marks["dp:0x1"] + marks["dp:0xffff0000"])
        assert (marks["dp:0x80000000"][0] in first) == (dp == 31)


@pytest.mark.parametrize("n", [1, 2, L - 1, L, L + 1])
def test_cpu_walk_small_herds(handle, n):
    jumps = handle.jump_table()
    herd = kc.cheap_herd(n, 2)
    want, dps, seconds = kr.walk(jumps, herd, 2, 0)
    assert handle.cpu_walk(herd, 2, 0) == (want, dps, seconds)
