"""tests/adversarial.py checked on the CPU: the point finders, the limb model of fe_asm.hpp's lazy arithmetic
against Python big integers, the operand generators (every operand must need its branch), planting against
the oracle's walk, and the -m address group reference against the oracle's.  Exact equality throughout."""
from __future__ import annotations

import random

import pytest

from tests import adversarial as adv

P, K = adv.P, adv.K
OPS = (0, 1, 3, 5, 6)
DIRECTED = ((0, "c3"), (0, "wrap"), (1, "c3"), (1, "wrap"), (6, "c3"), (6, "wrap"), (3, "sub_b2"), (5, "lazy_c2"))


@pytest.fixture(scope="module")
def bs32(ora):
    b = ora.Bsgs("0x100000000", 1)
    yield b
    b.close()


def test_curve_arithmetic():
    g = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
         0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
    assert adv.on_curve(g) and not adv.on_curve((g[0], g[1] + 1))
    g2 = adv.add(g, g)
    assert g2[0] == 0xC6047F9441ED7D6D3045406E95C07CD85C778E4B8CEF3CA7ABAC09B95C709EE5 and adv.on_curve(g2)
    assert adv.add(g2, adv.neg(g)) == g and adv.add(g, adv.neg(g)) is None and adv.add(None, g) == g
    assert adv.add(adv.add(g2, g), g) == adv.add(g2, g2)
    assert adv.sqrt(9) in (3, P - 3) and adv.sqrt(g[0]**3 + 7) in (g[1], P - g[1])
    assert adv.cbrt(27) is not None and pow(adv.cbrt(27), 3, P) == 27
    assert P % 9 == 7 and P % 4 == 3
    assert sum(adv.cbrt(a) is None for a in range(2, 200)) > 100      # two thirds of all values are no cubes
    assert adv.inv(0) == 0 and adv.inv(5) * 5 % P == 1


@pytest.mark.parametrize("cls", ["A", "B", "C", "D", "Y"])
def test_point_classes(cls):
    pts = adv.class_points(cls, 12, seed=3)
    assert len(pts) >= 8 and len(set(pts)) == len(pts)
    for pt in pts:
        assert adv.on_curve(pt) and adv.in_class(cls, pt), (cls, pt)
    assert pts == adv.class_points(cls, 12, seed=3)
    if cls == "D":
        assert all(pt[0] >> 224 == 0xFFFFFFFF for pt in pts)


def test_known_small_points():
    """The issue's census: 101 of the x in [0, 200) and 113 of the 200 x below p are on the curve, and
    0x1000003d0 / 0x1000003d2 straddle K."""
    assert sum(adv.lift_x(x) is not None for x in range(200)) == 101
    assert all(adv.lift_x(x) is not None for x in (1, 2, 3, 4, 6, 8))
    assert sum(adv.lift_x(P - 1 - i) is not None for i in range(200)) == 113
    assert adv.lift_x(0x1000003D0) is not None and adv.lift_x(0x1000003D2) is not None
    assert 0x1000003D0 < K < 0x1000003D2


@pytest.mark.parametrize("op", OPS)
def test_model_is_congruent_and_lazy(op):
    """100,000 seeded random operand pairs within the op's contract: congruent, < 2^256, and fm_canon of it is
    the canonical value."""
    rng = random.Random(1000 + op)
    model, exact = adv.MODEL[op], adv.EXACT[op]
    for _ in range(100000):
        a, b = adv.random_operands(op, rng)
        r = model(a, b)[0]
        e = exact(a, b)
        assert 0 <= r < 2**256 and r % P == e and adv.m_canon(r) == e, (op, a, b)


@pytest.mark.parametrize("op", OPS)
def test_no_flag_on_random_operands(op):
    rng = random.Random(2000 + op)
    for _ in range(10000):
        a, b = adv.random_operands(op, rng)
        assert not any(adv.flags(op, a, b).values()), (op, a, b)


@pytest.mark.parametrize("op,flag", DIRECTED)
def test_directed_operands_need_their_branch(op, flag):
    n = 256 if op in (0, 1, 6) else 64
    ops = adv.directed_operands(op, flag, n, seed=1)
    assert len(ops) == n and len(set(ops)) == n
    for a, b in ops:
        assert a < 2**256 and b < 2**256
        if op == 3:
            assert b < P
        if op == 5:
            assert a < P
        assert adv.flags(op, a, b)[flag] == 1, (op, flag, a, b)
        r = adv.MODEL[op](a, b)[0]
        assert r < 2**256 and adv.m_canon(r) == adv.EXACT[op](a, b)
    assert ops == adv.directed_operands(op, flag, n, seed=1)


def test_sub_and_lazy_add_shapes_run_the_long_chain():
    """The directed fm_sub / fm_add_lazy operands include borrows / carries that run through limbs 2..6."""
    for a, b in adv.directed_operands(3, "sub_b2", 8):
        assert a < b
    long_sub = [(a - b) % 2**256 >> 64 & (2**160 - 1) for a, b in adv.directed_operands(3, "sub_b2", 8)]
    assert 0 in long_sub
    long_add = [(a + b) % 2**256 >> 64 & (2**160 - 1) for a, b in adv.directed_operands(5, "lazy_c2", 8)]
    assert 2**160 - 1 in long_add


@pytest.mark.parametrize("op", [0, 1, 6])
def test_class_a_and_b_results(op):
    """A product whose canonical value v is below K leaves the reduction as v + p (a lazy value >= p with top
    word ffffffff); v in [K, K + 2^40) always takes the rare branch and its wrap fold and comes out as v.  Both
    for every product whose first fold L + H*K reaches 2^257 (see below): of random operands, all."""
    rng = random.Random(3000 + op)
    for cls in ("A", "B"):
        vals = adv.class_values(cls, 9)
        done = 0
        while done < 500:
            v = next(vals)
            if op == 0:
                a = rng.randrange(1, P)
                b = v * adv.inv(a) % P
            else:
                b = rng.randrange(2**256) if op == 6 else 0
                a = adv.sqrt(v - b)
                if a is None:
                    continue
                a = P - a if done & 1 else a
            t = a * b if op == 0 else a * a + b
            if (t % 2**256) + (t >> 256) * K < 2**257:
                # v + m*p with the first fold L + H*K below 2^257 can be v itself or 2^256 + (v - K): nothing
                # is left to fold (1 * 1 = 1; 2^128 squares to 2^256 = K exactly).  No other product is.
                continue
            r, c3, wrap = adv.MODEL[op](a, b)
            if cls == "A":
                assert r == v + P and r >> 224 == 0xFFFFFFFF and not wrap, (op, v)
            else:
                assert r == v and c3 and wrap, (op, v)
            done += 1


def test_class_c_values_take_the_rare_branch():
    rng = random.Random(5)
    vals = adv.class_values("C", 2)
    for _ in range(2000):
        v = next(vals)
        if v < K + 2**40:
            continue
        a = rng.randrange(1, P)
        r, c3, wrap = adv.m_mul(a, v * adv.inv(a) % P)
        assert c3 and not wrap and r == v


@pytest.mark.parametrize("cls", ["A", "B", "C", "D"])
def test_planted_points_appear_in_the_oracle_walk(ora, bs32, cls):
    gsn = adv.table_points(bs32.giant_table())
    cases = adv.planted_cases()
    assert sorted(adv.step_of(i, s) for i, s in cases) == \
        [0, 1, 2, 508, 509, 510, 511, 512, 513, 514, 515, 516, 1022, 1023]
    pts = adv.class_points(cls, len(cases), seed=11)
    for k, ((i, sign), Q) in enumerate(zip(cases, pts)):
        g = k % 4
        centre = adv.centre_for(Q, i, sign, gsn)
        start = adv.start_for(centre, g, ora, bs32)
        assert adv.on_curve(start)
        assert adv.ref_centre(ora, bs32, start, g).xy() == centre
        _, xs, _ = bs32.scan(ora.Point.of(*start), 0, g + 1, want_x=True)
        a = 1024 * g + adv.step_of(i, sign)
        assert xs[32 * a:32 * a + 32] == Q[0].to_bytes(32, "big"), (cls, i, sign, g)
        # the one-group walk from the reference centre gives the same group
        _, x1, _ = bs32.scan(adv.ref_centre(ora, bs32, start, g), 0, 1, want_x=True)
        assert x1 == xs[32 * 1024 * g:]


def test_addr_group_reference_matches_oracle(ora):
    gen = ora.AddrGen(1)
    O = ora.AddrTable("00" * 20 + "\n")
    try:
        gn = adv.table_points(gen.table())
        for key in (0x123456789ABCDEF0123, adv.N - 5000):
            _, _, ref = gen.group(O, key, 2, want_xy=True)
            centre = ora.pubkey(key + 512).xy()
            got, nxt, degenerate = adv.addr_group_ref(centre, gn)
            assert got == ref and not degenerate
            assert nxt == ora.pubkey(key + 512 + 1024).xy()
    finally:
        gen.close()
        O.close()


# ------------------------------------------------------------ the -m address model's degenerate branch

@pytest.fixture(scope="module")
def addr_gen(ora):
    gen = ora.AddrGen(1)
    O = ora.AddrTable("00" * 20 + "\n")
    yield gen, O, adv.table_points(gen.table())
    gen.close()
    O.close()


SPECIAL_K = (0, 1, 2, 509, 510, 511)


def _degenerate_keys():
    """[(first key of the group, its centre as a signed multiple of G)]: centre = (key + 512) * G on +-_2Gn and on
    +-Gn[k]; the oracle takes keys >= n as they are."""
    rows = [(512, 1024), (adv.N - 1536, -1024)]
    for k in SPECIAL_K:
        rows += [(adv.N - k - 513, -(k + 1)), (adv.N + k - 511, k + 1)]
    return rows


def test_addr_group_reference_matches_oracle_on_degenerate_centres(ora, addr_gen):
    """Centres on +-Gn[k] and +-_2Gn: every inverse of the batch is 0, and the model's x||y equal the oracle's group
    byte for byte on all 1024 points; the centre is the only true point of such a group.  Ordinary centres
    (near n as well) are not degenerate and unchanged."""
    gen, O, gn = addr_gen
    for key, c in _degenerate_keys():
        centre = ora.pubkey(c % adv.N).xy()
        row = gn[512] if abs(c) == 1024 else gn[abs(c) - 1]
        assert centre == (row if c > 0 else adv.neg(row))
        _, _, ref = gen.group(O, key, 2, want_xy=True)
        got, nxt, degenerate = adv.addr_group_ref(centre, gn)
        assert degenerate and got == ref, (key, c)
        assert got[64 * 512:64 * 513] == adv.be64(centre)
        # every other point: s = 0, so x = -(C.x + Gn.x) and y = +-Gn.y, and the next centre likewise
        assert got[:64] == adv.be64(((-centre[0] - gn[511][0]) % P, gn[511][1]))
        assert got[-64:] == adv.be64(((-centre[0] - gn[510][0]) % P, P - gn[510][1]))
        assert nxt == ((-centre[0] - gn[512][0]) % P, P - gn[512][1])
        true = sum(got[64 * t:64 * t + 64] == ora.pubkey((key + t) % adv.N).be64() for t in range(1024)
                   if (key + t) % adv.N)
        assert true == 1
    for key in (0x123456789ABCDEF0123, 1, 513, adv.N - 5000, adv.N - 1537, adv.N - 1535):
        _, _, ref = gen.group(O, key, 2, want_xy=True)
        got, nxt, degenerate = adv.addr_group_ref(ora.pubkey(key + 512).xy(), gn)
        assert got == ref and not degenerate and nxt == ora.pubkey((key + 1536) % adv.N).xy(), key


def test_add_direct_reference_matches_oracle(ora, addr_gen):
    """AddDirect on integers against the oracle's: ordinary operands, and p2.x == p1.x (ModInv(0) = 0), which is
    the collapsed lane-offset add (start = +-offs[m]) and the next-centre add of a group centred on +-_2Gn."""
    _, _, gn = addr_gen
    g2 = gn[512]
    a, b = ora.pubkey(0xABCDEF).xy(), ora.pubkey(0x1234567).xy()
    cases = [(a, b, False), (a, a, True), (a, adv.neg(a), True), (g2, g2, True), (adv.neg(g2), g2, True),
             (ora.pubkey(3 * 1024).xy(), ora.pubkey(3 * 1024).xy(), True),
             (ora.negation(ora.pubkey(4096)).xy(), ora.pubkey(4096).xy(), True),
             ((5, 7), b, False)]                                        # an operand off the curve
    for p1, p2, collapsed in cases:
        got, c = adv.add_direct_ref(p1, p2)
        assert c == collapsed
        assert got == ora.add_direct(ora.Point.of(*p1), ora.Point.of(*p2)).xy(), (p1, p2)
        if collapsed:
            assert got == ((-p1[0] - p2[0]) % P, P - p2[1])
    # the next centre of a group on +-_2Gn is that add with the batch's inverse, 0
    for c in (g2, adv.neg(g2)):
        assert adv.addr_group_ref(c, gn)[1] == ora.add_direct(ora.Point.of(*c), ora.Point.of(*g2)).xy()
    assert adv.add_direct_ref(a, b, 0)[0] == ((-a[0] - b[0]) % P, P - b[1])


def _offs(ora, gpl: int, n: int) -> list:
    return [None] + [ora.pubkey(m * gpl * 1024).xy() for m in range(1, n)]


@pytest.mark.parametrize("gpl", [1, 4])
def test_addr_lanes_reference(ora, addr_gen, gpl):
    """addr_lanes_ref on an ordinary start equals the oracle's groups walked one by one (6 groups: a short last lane
    at 4 groups per lane) and reports nothing; on starts that collapse it is pinned against the oracle group by
    group wherever a group's centre is still the key's own point."""
    gen, O, gn = addr_gen
    base = 0x7123456789ABCDEF
    offs = _offs(ora, gpl, 6)
    cache = {}
    xy, rec = adv.addr_lanes_ref(ora.pubkey(base + 512).xy(), gn, offs, gpl, 6, cache)
    assert rec == set() and len(cache) == 6
    for g in range(6):
        assert xy[65536 * g:65536 * (g + 1)] == gen.group(O, base + 1024 * g, 2, want_xy=True)[2], g
    assert adv.addr_lanes_ref(ora.pubkey(base + 512).xy(), gn, offs, gpl, 6) == (xy, rec)
    # group 0 on Gn[0]: reported; at one group per lane the later lanes restart from exact offsets, at four the
    # chain goes on from a centre off the curve and no later group of the lane is the oracle's
    key = adv.N - 511
    xy, rec = adv.addr_lanes_ref(gn[0], gn, offs, gpl, 4)
    assert rec == {0}
    exact = [xy[65536 * g:65536 * (g + 1)] == gen.group(O, key + 1024 * g, 2, want_xy=True)[2] for g in range(4)]
    assert exact == ([True] * 4 if gpl == 1 else [True, False, False, False])
    centres = [(int.from_bytes(xy[65536 * g + 32768:][:32], "big"), int.from_bytes(xy[65536 * g + 32800:][:32], "big"))
               for g in range(4)]
    assert [adv.on_curve(c) for c in centres] == ([True] * 4 if gpl == 1 else [True, False, False, False])
    # start = offs[1]: the lane add collapses (m * gpl | 0x80000000) and lane 1 walks from (-2x, -y)
    n = 2 * gpl
    xy, rec = adv.addr_lanes_ref(offs[1], gn, offs, gpl, n)
    assert 0x80000000 | gpl in rec and rec - {0x80000000 | gpl} == ({0} if gpl == 1 else set())
    o = offs[1]
    assert xy[65536 * gpl + 32768:][:64] == adv.be64(((-2 * o[0]) % P, P - o[1]))
    xy2, rec2 = adv.addr_lanes_ref(adv.neg(offs[1]), gn, offs, gpl, n)
    assert 0x80000000 | gpl in rec2
    assert xy2[65536 * gpl + 32768:][:64] == adv.be64(((-2 * o[0]) % P, P - o[1]))


def test_oracle_batch_helpers(ora):
    """hash160_many and AddrTable.bloom_check_many are loops over the single calls."""
    rng = random.Random(4)
    msgs = [bytes(rng.randrange(256) for _ in range(33)) for _ in range(50)]
    assert ora.hash160_many(b"".join(msgs), 33) == b"".join(ora.hash160(m) for m in msgs)
    h = [ora.hash160(m) for m in msgs]
    with ora.AddrTable("\n".join(x.hex() for x in h[::2]) + "\n") as O:
        got = O.bloom_check_many(b"".join(h))
        assert list(got) == [1 if O.bloom_check(x) else 0 for x in h] and all(got[::2]) and not all(got)


# ------------------------------------------------------- adv.second_check_ref, the per-slot model of the check

@pytest.fixture(scope="module")
def check_tabs(ora):
    from tests import check_cases as cc
    bs, tabs = cc.oracle_tables(ora)
    yield cc, bs, tabs
    bs.close()


def _pin(cc, bs, tabs, cases):
    """The model's key equals the oracle's bsgs_secondcheck on every case; the models are returned."""
    out = []
    for c in cases:
        r = cc.model(bs, tabs, c)
        assert r["key"] == bs.secondcheck(c.start, c.a, c.target), c.name
        out.append(r)
    return out


def test_check_model_on_random_families(ora, check_tabs):
    cc, bs, tabs = check_tabs
    cases = cc.r_cases(ora, bs)
    res = _pin(cc, bs, tabs, cases)
    found = [r for r in res if r["key"] is not None]
    assert len(found) >= 48 and sum(r["bp_hits"] for r in res) >= 32
    special = [r for c, r in zip(cases, res) if "special" in c.name]
    assert all(len(r["zero"]) == 1 and r["zero"][0][0] == 3 for r in special)       # Q' == -AMP3[i], that slot alone
    # the same families with every level-2 / level-3 bit set
    with cc.saved_blooms(bs, fill=0xFF):
        res = _pin(cc, bs, tabs, cases[:6] + cases[48:51] + cases[-3:])
        assert all(r["l2_hits"] == 32 and r["l3_hits"] == 1024 for r in res[-3:])
    assert bs.bloom_concat(2) == tabs["l2"] and bs.bloom_concat(3) == tabs["l3"]


def test_check_model_on_directed_cases(ora, check_tabs):
    """Classes Z, K and C with the geometry's constants: the model's key is the oracle's, every Z case reaches the
    dx == 0 element it is aimed at, and the other 31 x of that batch are plain point addition."""
    cc, bs, tabs = check_tabs
    amp = {2: adv.table_points(tabs["amp2"]), 3: adv.table_points(tabs["amp3"])}
    res = _pin(cc, bs, tabs, cc.k_cases(ora, bs) + cc.c_cases(ora, bs))
    assert [r["key"] is not None for r in res] == [False] * 5 + [True] * 18
    assert _pin(cc, bs, tabs, [cc.wrap_case(ora, bs)])[0]["key"] is None     # the oracle's sums wrap at 2^256 too
    assert all(r["bp_hits"] >= 1 for r in res[5:])
    z2, z3 = cc.z2_cases(ora, bs), cc.z3_cases(ora, bs)
    assert all(r["l2_hits"] == 0 for r in _pin(cc, bs, tabs, z3))      # unpinned: slot 0 does not enter
    with cc.saved_blooms(bs):
        cc.pin_z3_entry(ora, bs, tabs, z3)
        cc.pin_batches(ora, bs, tabs, z2 + z3, skip_zero=True)
        res = _pin(cc, bs, tabs, z2 + z3)
    for c, r in zip(z2 + z3, res):
        level, slot = cc.z_slot(c)
        assert r["zero"] == [(level, slot)], c.name
        xs = r["xs2"] if level == 2 else r["xs3"][0]
        base2 = c.start + c.a * 2 * bs.m
        q = adv.add(c.target.xy(), adv.neg(ora.pubkey(base2).xy()))
        for i in range(32):
            if i != slot:
                assert xs[i] == adv.add(q, amp[level][i])[0], (c.name, i)
        assert xs[slot] == (-2 * q[0]) % P                            # inverse 0: s = 0, x = -q.x - amp.x
        if level == 2:
            assert (r["key"], r["l2_hits"], r["l3_hits"]) == (None, 31, 31 * 32), c.name
        else:                      # the reference returns base2 + (2i+1) m3 here, the key being base2 - (2i+1) m3
            assert r["key"] == base2 + (2 * slot + 1) * bs.m3 and (r["l2_hits"], r["l3_hits"]) == (1, slot), c.name
            assert ora.pubkey(r["key"]).xy()[0] != c.target.xy()[0]


def test_check_model_equal_bptable_keys(ora, check_tabs):
    """Runs of three equal 6-byte keys: the oracle's bsgs_searchbinary lands on the run's member that its probe
    order 128, 64 / 192, ... reaches first, the one with the most trailing zero bits.  Observed split: the key at
    an even centre p is found (p is that member), at an odd p it is lost (p - 1 or p + 1 is) - 18 found, 18 lost.
    The model's transcription of the loop agrees case by case."""
    cc, bs, tabs = check_tabs
    cases = cc.d_cases(ora, bs)
    assert all(r["key"] is not None for r in _pin(cc, bs, tabs, cases))
    with cc.equal_key_runs(ora, bs):
        t = cc.current_tabs(bs, tabs)
        raw = t["bptable"]
        assert [raw[16 * i:16 * i + 6] for i in range(256)] == sorted(raw[16 * i:16 * i + 6] for i in range(256))
        assert raw != tabs["bptable"] and [raw[16 * i + 8:16 * i + 16] for i in range(256)] == \
            [tabs["bptable"][16 * i + 8:16 * i + 16] for i in range(256)]
        res = _pin(cc, bs, t, cases)
    assert cc.bptable_raw(bs) == tabs["bptable"]
    for c, r in zip(cases, res):
        p = int(c.name[3:-1])
        assert (r["key"] is not None) == (p % 2 == 0) and r["bp_hits"] == 1, c.name


def test_check_model_table_of_200(ora, check_tabs):
    """The bPtable cut to 200 entries (class T; the oracle's table size is fixed, so no oracle here): with distinct
    keys the model finds every planted key, as any correct search must; with the runs it finds some and loses
    others, and never reports a key whose point is not the target."""
    cc, bs, tabs = check_tabs
    cases = cc.t_cases(ora, bs)
    cut = dict(tabs, bptable=tabs["bptable"][:16 * cc.T_ENTRIES], m3=cc.T_ENTRIES)
    assert all(cc.model(bs, cut, c)["key"] is not None for c in cases)
    with cc.equal_key_runs(ora, bs):
        res = [cc.model(bs, cc.t_tabs(bs, tabs), c) for c in cases]
    found = [r["key"] for r in res if r["key"] is not None]
    assert 0 < len(found) < len(cases)
    assert all(ora.pubkey(r["key"]).xy()[0] == c.target.xy()[0] for c, r in zip(cases, res) if r["key"] is not None)
    print("class T:", len(found), "of", len(cases), "found")


def test_check_model_pins_every_slot(ora, check_tabs):
    """Level-2 and level-3 blooms that hold exactly the model's 32 + 32 x 32 x of four candidates: those give 32
    and 1024 hits, four unrelated candidates none; the oracle finds nothing for any of them."""
    cc, bs, tabs = check_tabs
    pinned, other = cc.nothing_cases(ora, 4, 0x70696e), cc.nothing_cases(ora, 4, 0x6f7468)
    with cc.saved_blooms(bs, fill=0):
        cc.pin_batches(ora, bs, tabs, pinned)
        res = _pin(cc, bs, tabs, pinned + other)
    assert [(r["l2_hits"], r["l3_hits"]) for r in res] == [(32, 1024)] * 4 + [(0, 0)] * 4
    assert bs.bloom_concat(2) == tabs["l2"] and bs.bloom_concat(3) == tabs["l3"]


def test_bp_search_equals_the_oracle_at_every_table_size(ora):
    """adv.bp_search against the oracle's bsgs_searchbinary on sorted tables of 1 to 300 entries with runs of equal
    keys: every key of the table, its neighbours, and keys below and above all.  The landed index, not just found."""
    rng = random.Random(0x6270)
    landed_elsewhere = 0
    for n in range(1, 301):
        keys = sorted(rng.randrange(1, 2**48 - 1) for _ in range(n))
        for _ in range(n // 6):                                       # runs of two to four equal keys
            p = rng.randrange(n)
            for q in range(p, min(n, p + rng.randrange(2, 5))):
                keys[q] = keys[p]
        keys.sort()
        tab = b"".join(k.to_bytes(6, "big") + b"\0\0" + (n - 1 - i).to_bytes(8, "little") for i, k in enumerate(keys))
        probes = set(keys) | {k + 1 for k in keys} | {k - 1 for k in keys} | {0, 2**48 - 1}
        for k in probes:
            xb = bytes(16) + k.to_bytes(6, "big") + bytes(10)
            got = adv.bp_search(tab, xb)
            assert got == ora.searchbinary(tab, xb), (n, k)
            assert (got is not None) == (k in keys), (n, k)
        landed_elsewhere += len(set(keys)) < n
    assert landed_elsewhere > 200


def test_bp_search_is_the_reference_loop():
    """adv.bp_search on small tables by hand: every entry of a table of distinct keys is found (entry 0 by the
    last probe, the one with half == 0), equal keys give the probe order's first member."""
    def tab(keys):
        return b"".join(k.to_bytes(6, "big") + b"\0\0" + i.to_bytes(8, "little") for i, k in enumerate(keys))

    def xb(k):
        return bytes(16) + k.to_bytes(6, "big") + bytes(10)
    assert adv.bp_search(tab([5]), xb(5)) == 0 and adv.bp_search(tab([5]), xb(6)) is None
    keys = [10, 20, 30, 40, 50, 60, 70, 80]
    assert [adv.bp_search(tab(keys), xb(k)) for k in keys] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert adv.bp_search(tab(keys), xb(35)) is None
    assert adv.bp_search(tab([10, 20, 20, 20, 50, 60, 70, 80]), xb(20)) == 2      # probes 4, 2
    assert adv.bp_search(tab([10, 20, 30, 40, 40, 40, 70, 80]), xb(40)) == 4      # probes 4
