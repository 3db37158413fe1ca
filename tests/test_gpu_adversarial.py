"""Directed GPU tests for the paths random inputs reach with probability 2^-30 or less (tests/adversarial.py):
the rare carries of the lazy field arithmetic, the canonicalisation of a lazy x >= p in the gated kernels,
degenerate groups through the product path, and -m address on points with extreme coordinates.  Expected
values are Python big integers or the oracle; every comparison is exact."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd.khbsgs import FIELD_OP_RAW as RAW
from tests import adversarial as adv
from tests.helpers import gate_bits, gate_pass, lane_offsets

pytestmark = pytest.mark.gpu

P, K = adv.P, adv.K
GPL, NGROUPS, NJOBS = 4, 4, 64   # one work item per job, one wave per launch
LG, PROBES = 16, 3
CONFIGS = ((False, 0, 0), (True, 0, 0), (True, 12, 0), (True, 12, 10))   # gate, stage-1 fold, stage-0 filter
CLASSES = ("A", "B", "C", "D")


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bs32(ora):
    b = ora.Bsgs("0x100000000", 1)       # M = 65536, 64 groups per chunk (as test_gpu_scan.py)
    yield b
    b.close()


def _be(vals) -> bytes:
    return b"".join(v.to_bytes(32, "big") for v in vals)


def _ints(raw: bytes) -> list:
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


# ------------------------------------------------------------------------------------ a. field ops

def _batches(op: int, directed: list, rng: random.Random):
    """Two batches of operand pairs with random filler.  The first (4,096 = 64 waves): wave 0 has all 64 lanes
    directed, waves 1..63 exactly one directed lane each, at a lane that moves from wave to wave.  The second
    (4,059: its last wave is partial) takes the rest at random places, one of them in its last lane."""
    assert len(directed) >= 64 + 63 + 2
    first = [adv.random_operands(op, rng) for _ in range(4096)]
    where1 = list(range(64)) + [64 * w + (7 * w + 3) % 64 for w in range(1, 64)]
    for k, i in enumerate(where1):
        first[i] = directed[k]
    rest = directed[len(where1):]
    n2 = 4096 - 37
    second = [adv.random_operands(op, rng) for _ in range(n2)]
    where2 = [n2 - 1] + rng.sample(range(n2 - 1), len(rest) - 1)
    for k, i in enumerate(where2):
        second[i] = rest[k]
    return (first, set(where1)), (second, set(where2))


@pytest.mark.parametrize("op", [0, 1, 6, 3, 5])
def test_field_ops_directed(eng, op):
    """fm_mul / fm_sqr / fm_sqr_add with 256 operands that need fm_reduce_T's rare branch (c3) and 256 that
    need its wrap fold as well; fm_sub / fm_add_lazy with 160 that need theirs.  The canonical result equals
    the Python integer; the raw result (op | KHB_FIELD_OP_RAW) equals the limb model bit for bit on directed
    operands and filler alike, so the model's flags mean on the GPU what they mean in the model."""
    if op in (0, 1, 6):
        c3 = adv.directed_operands(op, "c3", 256, seed=2)
        wrap = adv.directed_operands(op, "wrap", 256, seed=2)
        assert all(adv.flags(op, a, b) == {"c3": 1, "wrap": 0} for a, b in c3)
        assert all(adv.flags(op, a, b) == {"c3": 1, "wrap": 1} for a, b in wrap)
        directed = [x for pair in zip(c3, wrap) for x in pair]
    else:
        flag = "sub_b2" if op == 3 else "lazy_c2"
        directed = adv.directed_operands(op, flag, 160, seed=2)
        assert all(adv.flags(op, a, b)[flag] == 1 for a, b in directed)
    rng = random.Random(40 + op)
    for ops, where in _batches(op, directed, rng):
        assert all(any(adv.flags(op, a, b).values()) == (i in where) for i, (a, b) in enumerate(ops))
        ab, bb = _be(a for a, _ in ops), _be(b for _, b in ops)
        canon = _ints(eng.field_op(op, ab, bb))
        raw = _ints(eng.field_op(op | RAW, ab, bb))
        exact = [adv.EXACT[op](a, b) for a, b in ops]
        model = [adv.MODEL[op](a, b)[0] for a, b in ops]
        bad = [i for i in range(len(ops)) if canon[i] != exact[i]]
        assert not bad, (op, "canonical", bad[:8], [i in where for i in bad[:8]])
        bad = [i for i in range(len(ops)) if raw[i] != model[i]]
        assert not bad, (op, "raw", bad[:8], [i in where for i in bad[:8]])


def test_field_op_raw_is_refused_where_it_means_nothing(eng):
    from keyhuntm1cpu_amd.khbsgs import KhbError
    x = _be([5])
    for op in (2, 4, 7):
        with pytest.raises(KhbError):
            eng.field_op(op | RAW, x, x)
    assert _ints(eng.field_op(3 | RAW, _be([5]), _be([2**64]))) == [adv.m_sub(5, 2**64)[0]]


# ------------------------------------------------------- b / c. the product kernels: shared framework

def _l1_bits(nb: int, bits: int, hashes: int, xb: bytes, ora) -> list:
    """Bit indices in the concatenated level-1 bloom of bloom_add(&bloom_bP[x[0]], x, 32) (bloom.cpp)."""
    a = ora.xxh64(xb, 0x59F2815B16F81798)
    b = ora.xxh64(xb, a)
    return [8 * nb * xb[0] + ((a + b * i) & 0xFFFFFFFFFFFFFFFF) % bits for i in range(hashes)]


class World:
    """The dense synthetic level-1 bloom and the random three-probe gate of test_gate_candidates_exact, both
    forced to contain every planted x of every class, and the ordinary jobs all cases share."""

    def __init__(self, ora, bs):
        self.ora, self.bs = ora, bs
        self.gsn = adv.table_points(bs.giant_table())
        _, self.nb, self.bits, self.hashes = bs.bloom_concat(1)
        rng = random.Random(7)
        bf = bytearray(sum(1 << k for k in range(8) if rng.random() < 0.97) for _ in range(256 * self.nb))
        fill = 0.5 ** (1.0 / PROBES)
        gate = bytearray(sum(1 << k for k in range(8) if rng.random() < fill) for _ in range((1 << LG) // 8))
        # the planted jobs: class -> [(start, g, t, Q)]
        self.planted = {}
        for cls in CLASSES:
            rows = []
            for k, ((i, sign), Q) in enumerate(zip(adv.planted_cases(), adv.class_points(cls, 14, seed=21))):
                g = k % NGROUPS
                start = adv.start_for(adv.centre_for(Q, i, sign, self.gsn), g, ora, bs)
                rows.append((start, g, adv.step_of(i, sign), Q))
                for b in _l1_bits(self.nb, self.bits, self.hashes, Q[0].to_bytes(32, "big"), ora):
                    bf[b >> 3] |= 1 << (b & 7)
                for b in gate_bits(LG, PROBES, Q[0]):
                    gate[b >> 3] |= 1 << (b & 7)
            self.planted[cls] = rows
        self.bf, self.gate = bytes(bf), bytes(gate)
        self.ordinary = []                       # [(start, l1 list, gate list)]
        for c in range(NJOBS - 14):
            st = bs.chunk_start(0x3000000000000000 + c * (1 << 33), ora.pubkey(0xABCDEF0123 + 977 * c)).xy()
            self.ordinary.append((st,) + self.reference(st)[1:])

    def reference(self, start):
        """(x of the job's groups, steps that pass the level-1 bloom, steps that also pass the gate): every group
        walked on its own by the oracle from its reference centre (adv.ref_centre)."""
        ora, bs = self.ora, self.bs
        xs = b""
        for g in range(NGROUPS):
            _, x, _ = bs.scan(adv.ref_centre(ora, bs, start, g), 0, 1, want_x=True)
            xs += x
        l1, gt = [], []
        for a in range(NGROUPS * 1024):
            xb = xs[32 * a:32 * a + 32]
            if all((self.bf[b >> 3] >> (b & 7)) & 1 for b in _l1_bits(self.nb, self.bits, self.hashes, xb, ora)):
                l1.append(a)
                if gate_pass(self.gate, LG, PROBES, int.from_bytes(xb, "big")):
                    gt.append(a)
        return xs, l1, gt


@pytest.fixture(scope="module")
def world(ora, bs32):
    return World(ora, bs32)


def _load(eng, bs, world):
    eng.load_bloom(world.bf, world.nb, world.bits, world.hashes)
    eng.load_giant_table(bs.giant_table())
    eng.load_lane_offsets(lane_offsets(bs, GPL, (NGROUPS + GPL - 1) // GPL), GPL)


def _unload(eng, bs):
    eng.set_gate_stage1(1)                     # KHB_GATE_STAGE1_AUTO, the library default
    eng.set_gate_stage0(0)
    eng.load_gate(None)
    bf, nb, bits, h = bs.bloom_concat(1)
    eng.load_bloom(bf, nb, bits, h)


def _run_configs(eng, world, centres: bytes, njobs: int):
    """[(config, per-job sorted candidates, degenerate records, stats)] for the four kernel configurations."""
    out = []
    for use_gate, stage1, stage0 in CONFIGS:
        eng.set_gate_stage1(stage1)
        eng.set_gate_stage0(stage0)
        eng.load_gate(world.gate if use_gate else None, LG, PROBES)
        assert eng.gate_stages() == (4 if use_gate else 0) | (2 if use_gate and stage1 else 0) | \
            (1 if use_gate and stage0 else 0)
        got, degen, st = eng.scan(centres, 0, NGROUPS)
        per_job = [[] for _ in range(njobs)]
        for job, a in got:
            per_job[job].append(a)
        out.append(((use_gate, stage1, stage0), [sorted(x) for x in per_job], degen, st))
    return out


@pytest.mark.parametrize("cls", CLASSES)
def test_planted_x_through_the_product_kernels(eng, bs32, ora, world, cls):
    """One wave of 64 jobs of 4 groups; 14 of them have a step of one group land on a curve point whose x is of
    the class (A: the lazy x is x + p, which x_out must canonicalise before the gate reads its low word; B and C:
    the x itself comes out of fm_reduce_T's rare branch, with and without the wrap fold; D: top word ffffffff with
    a canonical x, x_out's branch taken for nothing).  Steps 0, 1, 2, 508..516, 1022 and 1023, in groups 0..3."""
    rows = world.planted[cls]
    slots = {(4 * k + 1) % NJOBS: k for k in range(len(rows))}
    assert len(slots) == 14
    jobs, it = [], iter(world.ordinary)
    for j in range(NJOBS):
        if j in slots:
            start = rows[slots[j]][0]
            jobs.append((start,) + world.reference(start))
        else:
            st, l1, gt = next(it)
            jobs.append((st, None, l1, gt))
    assert sum(1 for j in jobs if j[1] is None) >= 16
    centres = b"".join(adv.be64(j[0]) for j in jobs)
    try:
        _load(eng, bs32, world)
        for j, k in slots.items():
            start, g, t, Q = rows[k]
            xs = jobs[j][1]
            a = 1024 * g + t
            assert xs[32 * a:32 * a + 32] == Q[0].to_bytes(32, "big")
            assert a in jobs[j][2] and a in jobs[j][3]            # forced into the bloom and the gate
            assert eng.dump_x(adv.be64(start), 0, NGROUPS) == xs, (cls, j)
        for cfg, per_job, degen, st in _run_configs(eng, world, centres, NJOBS):
            ref = [j[3] if cfg[0] else j[2] for j in jobs]
            for j, k in slots.items():
                a = 1024 * rows[k][1] + rows[k][2]
                assert a in per_job[j], (cls, cfg, "planted x lost", j, a, hex(rows[k][3][0]))
            bad = [j for j in range(NJOBS) if per_job[j] != ref[j]]
            assert not bad, (cls, cfg, bad, [j in slots for j in bad])
            assert not degen and st.n_degenerate == 0
            assert st.giant_steps == NJOBS * NGROUPS * 1024
    finally:
        _unload(eng, bs32)


def _degenerate_starts(ora, bs, gsn) -> list:
    """Start points of the degenerate jobs: group g in {0, 1, 3} centred on +-GSn[k] for the half stream's
    special indices k (the unstored P_0, the i > 2 boundary, the peeled step, the rebuilt P_510), on +-_2GSn
    (k = 512: g2x == cx), and startP = +-jg * _2GSn (the centre add collapses).  _2GSn as group 1's centre would
    need the point at infinity as startP and is left out; starts that two rules share (GSn[511] in group 1 is
    -GSn[511] in group 0) are taken once."""
    starts = []
    for g in (0, 1, 3):
        for k in (0, 1, 2, 509, 510, 511, 512):
            for pt in (gsn[k], adv.neg(gsn[k])):
                starts.append(adv.start_for(pt, g, ora, bs))
    for jg in (1, 3):
        o = adv.group_offset(ora, bs, jg)
        starts += [o, adv.neg(o)]
    out = []
    for st in starts:
        if st is not None and st not in out:
            out.append(st)
    return out


def test_degenerate_groups_through_the_product_kernels(eng, bs32, ora, world):
    """Every degenerate group is walked from its exact reference centre with inverse 0 and reported, in the
    ungated kernel and the three gated ones (walk_group_g_half); a collapsed centre add is reported as
    jg | 0x80000000.  The report is computed here from the centres alone."""
    gsn = world.gsn
    starts = _degenerate_starts(ora, bs32, gsn)
    assert len(starts) == 41 and all(adv.on_curve(st) for st in starts)
    table_x = {p[0] for p in gsn}
    assert len(table_x) == 513
    jobs, expect = [], []
    it = iter(world.ordinary)
    for j in range(NJOBS):
        if j % 3 != 2 and j - j // 3 < len(starts):      # 41 degenerate jobs, 23 ordinary ones between them
            start = starts[j - j // 3]
            _, l1, gt = world.reference(start)
            for g in range(NGROUPS):
                if adv.ref_centre(ora, bs32, start, g).xy()[0] in table_x:
                    expect.append((j, g))
                if g and adv.group_offset(ora, bs32, g)[0] == start[0]:
                    expect.append((j, g | 0x80000000))
        else:
            start, l1, gt = next(it)
        jobs.append((start, l1, gt))
    assert len({j for j, _ in expect}) == 41 and len(expect) > 41          # some jobs have two such groups
    assert {g for _, g in expect if g & 0x80000000} == {0x80000001, 0x80000002, 0x80000003}
    centres = b"".join(adv.be64(j[0]) for j in jobs)
    try:
        _load(eng, bs32, world)
        for cfg, per_job, degen, st in _run_configs(eng, world, centres, NJOBS):
            ref = [j[2] if cfg[0] else j[1] for j in jobs]
            bad = [j for j in range(NJOBS) if per_job[j] != ref[j]]
            assert not bad, (cfg, bad)
            assert sorted(degen) == sorted(expect), cfg
            assert st.n_degenerate == len(expect)
            assert st.giant_steps == NJOBS * NGROUPS * 1024
    finally:
        _unload(eng, bs32)


# ------------------------------------------------------------------------------------ d. -m address

def _leading_zero_points() -> list:
    """Points whose x, and points whose y, starts with one or two zero bytes."""
    rng = random.Random(33)
    out = []
    for bits in (248, 240):
        while True:
            pt = adv.lift_x(rng.randrange(2**bits), rng.randrange(2))
            if pt is not None and pt[0] >> (bits - 8):
                out.append(pt)
                break
    for bits in (248, 244):
        while True:
            pt = adv.lift_x(rng.randrange(P), 0)
            if pt is not None and min(pt[1], P - pt[1]) < 2**bits:
                out.append((pt[0], min(pt[1], P - pt[1])))
                break
    return out


def test_hash160_on_extreme_coordinates(eng, ora):
    pts = [pt for cls in ("A", "B", "C", "D", "Y") for pt in adv.class_points(cls, 8, seed=5)] + _leading_zero_points()
    assert all(adv.on_curve(pt) for pt in pts)
    xy = b"".join(adv.be64(pt) for pt in pts)
    for kind in (0, 1, 2):
        got = eng.hash160(kind, xy)
        for i, pt in enumerate(pts):
            ref = ora.x_hash160(2 + kind, pt[0]) if kind < 2 else ora.pub_hash160(ora.Point.of(*pt), False)
            assert got[i][0] == ref, (kind, i, pt)


_addr_refs: dict = {}


@pytest.mark.parametrize("gpl", [1, 4])
@pytest.mark.parametrize("cls", ["A", "B", "D", "Y"])
def test_addr_dump_on_planted_points(eng, ora, cls, gpl):
    """-m address walks (x and y) whose step t of group 0 or of group 2 is a point of the class, against curve
    arithmetic on Python integers.  With 4 groups per lane group 2 is reached through scan_group's own
    next-centre chain, with 1 through the lane offset."""
    gen = ora.AddrGen(1)
    try:
        raw = gen.table()
    finally:
        gen.close()
    gn = adv.table_points(raw)
    eng.load_giant_table(raw)
    n_off = (NGROUPS + gpl - 1) // gpl
    eng.load_lane_offsets(bytes(64) + b"".join(ora.pubkey(m * gpl * 1024).be64() for m in range(1, n_off)), gpl)
    steps = (0, 1, 511, 512, 513, 1023)
    pts = adv.class_points(cls, 2 * len(steps), seed=8)
    for k, Q in enumerate(pts):
        t, g = steps[k % len(steps)], 2 * (k // len(steps))
        if t < 512:
            centre = adv.add(Q, gn[511 - t])
        else:
            centre = Q if t == 512 else adv.add(Q, adv.neg(gn[t - 513]))
        for _ in range(g):
            centre = adv.add(centre, adv.neg(gn[512]))
        if (cls, k) not in _addr_refs:
            ref, c = b"", centre
            for _ in range(NGROUPS):
                xy, c, _ = adv.addr_group_ref(c, gn)
                ref += xy
            _addr_refs[cls, k] = ref
        ref = _addr_refs[cls, k]
        at = 64 * (1024 * g + t)
        assert ref[at:at + 64] == adv.be64(Q)
        got = eng.addr_dump(adv.be64(centre), 0, NGROUPS)
        if got != ref:
            bad = [i for i in range(NGROUPS * 1024) if got[64 * i:64 * i + 64] != ref[64 * i:64 * i + 64]]
            assert not bad, (cls, gpl, k, t, g, bad[:8])
