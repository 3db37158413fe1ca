"""Directed GPU tests of scan_group and the nine product kernels it feeds (-m address with -l 0/1/2, the same with -e,
-c eth, -m xpoint, -m xpoint -e) on the paths ordinary keys reach with probability 2^-30 or less, or never: planted
points of the coordinate classes of tests/adversarial.py, beta * x products that come out as a class value, degenerate
groups (centre on +-Gn[k] or +-_2Gn), the chain that follows one in the same lane, and the collapsed lane-offset add.

The expected value of every launch is the model's: adv.addr_lanes_ref gives the x||y of every walked point and the
degenerate records; each point is hashed here for every kind the search flag produces (the oracle's hash160, the
tests' own Keccak, the first 20 bytes of x; with -e beta^e * x and p - y) and passed through the oracle's bloom_check
over the target file the product loads.  Every comparison is exact.

Targets: every kind of every directed point, and one kind of one in PICK of all other walked points, the points of
degenerate and off-curve groups included.  (A third of the points, as first planned, would be more hits than the
quarter of the hit ring the tests allow themselves: ~100 jobs x 4,096 points / 3 > 65,536.)"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from keyhuntm1cpu_amd import khhost
from tests import adversarial as adv
from tests import eth_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
P, N, K = adv.P, adv.N, adv.K
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE      # keyhunt.cpp:584
ENDO, ETH, XPOINT = 4, 8, 16                                                    # include/khbsgs.h KHB_SEARCH_*
KIND_ETH, KIND_X = 16, 32                                                       # KHB_ADDR_KIND_*
SEARCHES = (0, 1, 2, 0 | ENDO, 1 | ENDO, 2 | ENDO, ETH, XPOINT, XPOINT | ENDO)
NGROUPS = 4
STEPS = (0, 1, 511, 512, 513, 1023)
SPECIAL_K = (0, 1, 2, 509, 510, 511)
PICK = 12
ORDINARY_BASE = 0x5000000000 + 1      # ordinary job i walks keys ORDINARY_BASE + 4096 i + [0, 1024 * groups)


def kinds_of(search: int) -> tuple:
    """khb_addr_hit.kind values the search flag produces (include/khbsgs.h)."""
    if search == ETH:
        return (KIND_ETH,)
    if search & XPOINT:
        return tuple(KIND_X | e << 2 for e in range(3 if search & ENDO else 1))
    if not search & ENDO:
        return {0: (2,), 1: (0, 1), 2: (0, 1, 2)}[search]
    forms = {0: (2, 3), 1: (0, 1), 2: (0, 1, 2, 3)}[search & 3]
    return tuple(f | e << 2 for e in range(3) for f in forms)


def values_of(ora, xy: bytes, kind: int) -> bytes:
    """The 20-byte value of kind `kind` of each x||y point of xy, back to back."""
    if kind == KIND_ETH:
        return eth_ref.eth_addresses(np.frombuffer(xy, dtype=np.uint8)).tobytes()
    n = len(xy) // 64
    e = (kind & ~KIND_X) >> 2 if kind & KIND_X else kind >> 2
    xs = [xy[64 * i:64 * i + 32] for i in range(n)]
    if e:
        b = pow(BETA, e, P)
        xs = [(int.from_bytes(x, "big") * b % P).to_bytes(32, "big") for x in xs]
    if kind & KIND_X:
        return b"".join(x[:20] for x in xs)
    form = kind & 3
    if form < 2:
        return ora.hash160_many(b"".join(bytes([2 + form]) + x for x in xs), 33)
    ys = [xy[64 * i + 32:64 * i + 64] for i in range(n)]
    if form == 3:
        ys = [((P - int.from_bytes(y, "big")) % P).to_bytes(32, "big") for y in ys]
    return ora.hash160_many(b"".join(b"\x04" + x + y for x, y in zip(xs, ys)), 65)


class Job:
    """start: the job's centre of group 0; key: its first key when it is known (start = (key + 512) * G);
    directed: [(group, t)] of its directed points."""

    def __init__(self, start, key=None, directed=()):
        self.start, self.key, self.directed = start, key, list(directed)


class World:
    """The table, the lane offsets and the caches the cases share: the model's groups by centre and the values of a
    group's points by kind (a group of an ordinary job is the same for every flag and both lane layouts)."""

    def __init__(self, ora):
        self.ora = ora
        gen = ora.AddrGen(1)
        try:
            self.raw = gen.table()
        finally:
            gen.close()
        self.gn = adv.table_points(self.raw)
        self.groups, self.lanes, self.values = {}, {}, {}

    def offsets(self, gpl: int, ngroups: int):
        n = (ngroups + gpl - 1) // gpl
        pts = [None] + [self.ora.pubkey(m * gpl * 1024).xy() for m in range(1, n)]
        return pts, bytes(64) + b"".join(adv.be64(p) for p in pts[1:])

    def model(self, start, gpl: int, ngroups: int):
        """(the x||y of each group, the degenerate records) of one job."""
        key = (start, gpl, ngroups)
        if key not in self.lanes:
            xy, rec = adv.addr_lanes_ref(start, self.gn, self.offsets(gpl, ngroups)[0], gpl, ngroups, self.groups)
            # the cache hands out one bytes object per centre, so equal groups share their values below
            per_group = [self.groups_xy(xy[65536 * g:65536 * (g + 1)]) for g in range(ngroups)]
            self.lanes[key] = (per_group, rec)
        return self.lanes[key]

    def groups_xy(self, xy: bytes) -> bytes:
        return self.values.setdefault(("xy", xy), xy)

    def group_values(self, xy: bytes, kind: int) -> bytes:
        v = self.values.get((xy, kind))
        if v is None:
            v = self.values[xy, kind] = values_of(self.ora, xy, kind)
        return v

    def ordinary(self, n: int, skip: int = 0) -> list:
        return [Job(self.ora.pubkey(ORDINARY_BASE + 4096 * i + 512).xy(), ORDINARY_BASE + 4096 * i)
                for i in range(skip, skip + n)]


@pytest.fixture(scope="module")
def world(ora):
    w = World(ora)
    yield w
    w.groups.clear()
    w.lanes.clear()
    w.values.clear()


@pytest.fixture(scope="module")
def eng():
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    yield e
    e.close()


def mix(directed: list, ordinary: list) -> list:
    """The directed jobs with the ordinary ones spread among them."""
    out, ordinary = [], list(ordinary)
    every = max(1, len(directed) // max(1, len(ordinary)))
    for i, d in enumerate(directed):
        if i % every == every // 2 and ordinary:
            out.append(ordinary.pop(0))
        out.append(d)
    return out + ordinary


class Case:
    """One addr_scan of `jobs` and the model's expectation of it."""

    def __init__(self, eng, world, jobs: list, gpl: int, ngroups: int, search: int):
        ora = world.ora
        self.jobs, self.gpl, self.ngroups, self.search = jobs, gpl, ngroups, search
        self.kinds = kinds = kinds_of(search)
        lanes_per_job = (ngroups + gpl - 1) // gpl
        assert len(jobs) >= 64 and (len(jobs) * lanes_per_job) % 64 != 0       # a ragged last wave
        models = [world.model(j.start, gpl, ngroups) for j in jobs]
        self.groups = [xy for per_group, _ in models for xy in per_group]       # (job, group) order
        self.records = [rec for _, rec in models]
        self.n_degenerate = sum(len(rec) for rec in self.records)
        npts = self.npts = 1024 * ngroups * len(jobs)
        pts = np.frombuffer(b"".join(self.groups), dtype=np.uint8).reshape(npts, 64)
        directed = np.zeros(npts, dtype=bool)
        self.directed = [(j, g, t) for j, job in enumerate(jobs) for g, t in job.directed]
        for j, g, t in self.directed:
            directed[(j * ngroups + g) * 1024 + t] = True
        picked = (pts[:, 29].astype(np.int64) * 256 + pts[:, 30]) % PICK == 0
        which = pts[:, 31] % len(kinds)
        self.vals = {k: np.frombuffer(b"".join(world.group_values(xy, k) for xy in self.groups),
                                      dtype=np.uint8).reshape(npts, 20) for k in kinds}
        targets = []
        for i, k in enumerate(kinds):
            targets += [bytes(v) for v in self.vals[k][directed | (picked & (which == i))]]
        self.targets = list(dict.fromkeys(targets))
        self.target_set = set(self.targets)
        if search == ETH:
            text, kw = "".join("0x" + v.hex() + "\n" for v in self.targets), {"crypto": "eth"}
        elif search & XPOINT:
            text, kw = "".join(v.hex() + "00" * 12 + "\n" for v in self.targets), {"mode": "xpoint"}
        else:
            text, kw = "".join(v.hex() + "\n" for v in self.targets), {}
        self.A = khhost.Addr(text, n_seq=1024 * ngroups, gpl=gpl, **kw)
        with ora.AddrTable("".join(v.hex() + "\n" for v in self.targets)) as O:
            bf, bits, h = self.A.bloom()
            assert bf == O.bloom_bytes()                   # the same target file, the same bloom
            self.expect = set()
            for k in kinds:
                passes = np.frombuffer(O.bloom_check_many(self.vals[k].tobytes()), dtype=np.uint8)
                for i in np.nonzero(passes)[0].tolist():
                    self.expect.add((i // (1024 * ngroups), (i // 1024) % ngroups, i % 1024, k))
        eng.load_addr_bloom(bf, bits, h)
        eng.load_giant_table(world.raw)
        eng.load_lane_offsets(world.offsets(gpl, ngroups)[1], gpl)
        self.ring = min(eng.candidate_capacity(), 1 << 18)          # khb_addr_hit_capacity
        hits, self.st = eng.addr_scan(b"".join(adv.be64(j.start) for j in jobs), 0, ngroups, search)
        self.hit_list, self.hits = hits, set(hits)

    def check(self):
        """What every case asserts."""
        st = self.st
        assert st.giant_steps == len(self.jobs) * self.ngroups * 1024
        assert st.n_cand == len(self.hit_list) == len(self.hits)
        assert st.n_cand < self.ring // 4
        assert 0 < len(self.hits) < self.npts * len(self.kinds)
        assert len(self.expect) >= len(self.targets)
        if self.hits != self.expect:
            lost, extra = sorted(self.expect - self.hits), sorted(self.hits - self.expect)
            assert not lost and not extra, (self.search, self.gpl, len(lost), lost[:6], len(extra), extra[:6])
        for j, g, t in self.directed:
            for k in self.kinds:
                assert (j, g, t, k) in self.hits, (self.search, self.gpl, j, g, t, k)
        assert st.n_degenerate == self.n_degenerate

    def point(self, j: int, g: int, t: int) -> bytes:
        return self.groups[j * self.ngroups + g][64 * t:64 * t + 64]

    def close(self):
        self.A.close()


# ------------------------------------------------------------------------------------------ a. planted points

def _start_for(world, Q, t: int, g: int):
    """The start of a job whose group g has Q at step t."""
    gn = world.gn
    if t < 512:
        centre = adv.add(Q, gn[511 - t])
    else:
        centre = Q if t == 512 else adv.add(Q, adv.neg(gn[t - 513]))
    for _ in range(g):
        centre = adv.add(centre, adv.neg(gn[512]))
    return centre


def endo_plants() -> list:
    """[(Q, cls, e)]: curve points Q = (beta^(3 - e) * v, y) for class A/B/C values v that are x of a curve point
    (v, y): beta^3 = 1, so Q is on the curve and the kernel's own beta^e * Q.x, beta * x or beta * (beta * x), comes
    out as v.  The limb model certifies that this product needs its branch: class A leaves the reduction as v + p
    (the fm_canon after the product), B takes the rare branch with its wrap fold, C the rare branch alone."""
    out = []
    for cls in ("A", "B", "C"):
        pts = adv.class_points(cls, 4, seed=77)
        for n, (v, y) in enumerate(pts):
            e = 1 + n % 2
            Q = (pow(BETA, 3 - e, P) * v % P, y)
            assert adv.on_curve(Q) and not adv.in_class(cls, Q)
            x = Q[0] if e == 1 else Q[0] * BETA % P          # the operand of the last product, canonical
            r, c3, wrap = adv.m_mul(x, BETA)
            assert r % P == v and adv.flags(0, x, BETA) == {"c3": c3, "wrap": wrap}
            assert {"A": r == v + P and not wrap, "B": c3 and wrap and r == v, "C": c3 and not wrap and r == v}[cls]
            out.append((Q, cls, e))
    return out


def slope_plants(gn: list) -> list:
    """[(C, Q, t, cls)]: centres C whose step t squares a slope s with s^2 = v, a class A, B or C value, so the x,y
    walk's fm_sqr(s) itself leaves v + p, takes the rare branch with the wrap fold, or the rare branch alone (its x
    comes out of the fm_sub that follows, so a planted x does not reach the reduction there).  The line of slope
    sqrt(v) through G0 = -Gn[510] (t = 1, C - Gn[510]) or Gn[510] (t = 1023, C + Gn[510]) meets the curve in two more
    points, the roots of z^2 - (s^2 - a) z + ((b - s a)^2 - 7) / a: C is one, and Q = C + G0 the mirror of the other."""
    out = []
    for cls in ("A", "B", "C"):
        vals = adv.class_values(cls, 5)
        for t in (1, 1023):
            a, b = gn[510] if t > 512 else adv.neg(gn[510])
            while True:
                v = next(vals)
                s = adv.sqrt(v)
                if s is None or v == 0:
                    continue
                prod = ((b - s * a) ** 2 - 7) * adv.inv(a) % P
                root = adv.sqrt(((v - a) ** 2 - 4 * prod) % P)
                if root is None:
                    continue
                x1 = (v - a + root) * adv.inv(2) % P
                x2 = (v - a - x1) % P
                C, R = (x1, (s * (x1 - a) + b) % P), (x2, (s * (x2 - a) + b) % P)
                if x1 in (a, x2) or not (adv.on_curve(C) and adv.on_curve(R)):
                    continue
                Q = adv.neg(R)
                assert adv.add(C, (a, b)) == Q

                def needs_branch(lazy_s):
                    r, c3, wrap = adv.m_sqr(lazy_s)
                    return {"A": r == v + P, "B": c3 and wrap and r == v, "C": c3 and not wrap and r == v}[cls]

                if not (needs_branch(s) and needs_branch(P - s)):
                    continue          # an integer square such as 1 * 1 or 2 * 2 has nothing to fold
                out.append((C, Q, t, cls))
                break
    return out


def _class_d_points(n: int) -> list:
    """Class D points whose first 20 bytes of x are not all ff: those of x = p - 1 - i are, and so are the first 20
    bytes of a lazy x + p for x < K, so as -m xpoint targets they would hide a class-A x that was not canonicalised."""
    pts = [q for q in adv.class_points("D", 64 + 2 * n, seed=31) if (q[0] >> 96) != 2**160 - 1]
    assert len(pts) >= n
    return pts[:n]


@pytest.fixture(scope="module")
def planted_jobs(world):
    """72 jobs with a point of class A, B, C, D, Y or the negation of a class-Y point (p - y < K) at step 0, 1, 511,
    512, 513 or 1023 of group 0 or of group 2, 12 with an -e plant, 6 with a slope plant, and 19 ordinary ones among
    them."""
    ypts = adv.class_points("Y", 24)
    classes = [(c, adv.class_points(c, 12, seed=31)) for c in ("A", "B", "C")] + [("D", _class_d_points(12))]
    classes += [("Y", ypts[:12]), ("negY", [adv.neg(q) for q in ypts[12:]])]
    directed = []
    for cls, pts in classes:
        for k, Q in enumerate(pts):
            assert adv.on_curve(Q) and (adv.in_class(cls, Q) if cls != "negY" else P - Q[1] < K)
            t, g = STEPS[k % 6], 2 * (k // 6)
            directed.append(Job(_start_for(world, Q, t, g), None, [(g, t)]))
    for n, (Q, cls, e) in enumerate(endo_plants()):
        t, g = STEPS[(n + n // 6) % 6], 2 * (n % 2)
        directed.append(Job(_start_for(world, Q, t, g), None, [(g, t)]))
    for n, (C, Q, t, cls) in enumerate(slope_plants(world.gn)):
        g = 2 * ((n // 2 + n) % 2)
        assert _start_for(world, Q, t, 0) == C
        directed.append(Job(_start_for(world, Q, t, g), None, [(g, t)]))
    assert len(directed) == 90
    return mix(directed, world.ordinary(19)), directed


@pytest.mark.parametrize("gpl", [1, 4])
@pytest.mark.parametrize("search", SEARCHES)
def test_planted_points_through_the_address_kernels(eng, world, planted_jobs, search, gpl):
    """109 jobs x 4 groups through one product kernel.  Group 2 is reached by scan_group's next-centre chain at 4
    groups per lane and by the lane offset at 1.  Class A: the lazy x is x + p (x_out's ungated arm, the fm_canon
    after beta * x); B and C: fm_reduce_T's rare branch inside the walk's x = s^2 - ... and inside beta * x; D: the
    top word ffffffff with nothing to do; Y and its negation: y < K and p - y < K for the uncompressed hashes and
    the -e handlers' p - y; the slope plants put v + p and the rare branch into the x,y walk's own fm_sqr.  Class C
    curve points are found directly (x = hi << 96 | lo < 2^33 is a square half the
    time), so the class is planted like the others.  The hit set equals the model's, every kind of every directed
    point is among the hits, nothing is degenerate; for kAddrX (walk_group_ax) the same jobs' khb_addr_dump (the x,y
    walk) equal the model as well, so the two walks' x agree bit for bit on the classes."""
    jobs, directed = planted_jobs
    case = Case(eng, world, jobs, gpl, NGROUPS, search)
    try:
        for j, job in enumerate(jobs):
            for g, t in job.directed:
                assert adv.on_curve((int.from_bytes(case.point(j, g, t)[:32], "big"),
                                     int.from_bytes(case.point(j, g, t)[32:], "big")))
        case.check()
        assert case.n_degenerate == 0 and case.st.n_degenerate == 0
        if search == XPOINT:
            for j, job in enumerate(jobs):
                if job.directed:
                    got = eng.addr_dump(adv.be64(job.start), 0, NGROUPS)
                    assert got == b"".join(case.groups[j * NGROUPS:(j + 1) * NGROUPS]), (gpl, j)
    finally:
        case.close()


# --------------------------------------------------------------------------------------- b. degenerate groups

def _key_job(world, start_key: int, directed_groups=()):
    """The job whose group 0 is centred on start_key * G (a signed key); None for the point at infinity."""
    if start_key % N == 0:
        return None
    return Job(world.ora.pubkey(start_key % N).xy(), (start_key - 512) % N,
               [(g, t) for g in directed_groups for t in STEPS])


def degenerate_jobs(world, gpl: int) -> tuple:
    """(jobs of 4 groups, jobs of 8 groups).  Group 0, 1 or 3 centred on +-Gn[k] for k in SPECIAL_K or on +-_2Gn
    (centre c * G: the job starts at (c - 1024 g) * G; a start that would be the point at infinity is left out and
    a start that two rules share is taken once), and starts +-offs[m], whose lane add collapses: m = 1, 3 at one
    group per lane, m = 1 with 8 groups at four.  The directed points are steps 0, 1, 511, 512, 513 and 1023 of
    the group the job is built for."""
    four, eight = [], []

    def add(to, start_key, groups):
        job = _key_job(world, start_key, groups)
        if job is None:
            return
        same = [j for j in to if j.start == job.start]
        if same:
            same[0].directed += [d for d in job.directed if d not in same[0].directed]
        else:
            to.append(job)

    for g in (0, 1, 3):
        for c in [k + 1 for k in SPECIAL_K] + [1024]:
            for sign in (1, -1):
                add(four, sign * c - 1024 * g, [g])
    if gpl == 1:
        for m in (1, 3):
            for sign in (1, -1):
                add(four, sign * 1024 * m, [m])
    else:
        for sign in (1, -1):
            add(eight, sign * 4096, [4])
    return four, eight


def _check_confirm(case, world):
    """Every hit inside a degenerate or off-curve group against khh_addr_confirm: the host recomputes the point from
    the key, so a hit on a point that is not the key's is refused; it reports a key exactly when the key's own value
    of that kind is a target (the centre of a degenerate group is a true point, and neighbouring jobs walk the same
    keys from good centres)."""
    ora = world.ora
    bad = set()
    for j, job in enumerate(case.jobs):
        if job.key is None:
            continue
        for g in range(case.ngroups):
            c = case.point(j, g, 512)
            on = adv.on_curve((int.from_bytes(c[:32], "big"), int.from_bytes(c[32:], "big")))
            if g in case.records[j] or not on:
                bad.add((j, g))
    refused = bogus = 0
    for kind in case.kinds:
        rows = [(j, g, t, (case.jobs[j].key + 1024 * g + t) % N) for j, g, t, k in case.hit_list
                if k == kind and (j, g) in bad]
        true = [ora.pubkey(key).be64() if key else bytes(64) for _, _, _, key in rows]
        own = values_of(ora, b"".join(true), kind) if rows else b""
        for i, (j, g, t, key) in enumerate(rows):
            got = case.A.confirm(key, kind)
            want = key != 0 and own[20 * i:20 * i + 20] in case.target_set
            assert (got is not None) == want, (case.search, case.gpl, j, g, t, kind)
            if case.point(j, g, t) != true[i]:
                bogus += 1
                refused += got is None
    assert bad and bogus and refused and refused >= bogus - bogus // 4     # most such keys' own values are no targets
    return bad


@pytest.mark.parametrize("gpl", [1, 4])
@pytest.mark.parametrize("search", SEARCHES)
def test_degenerate_groups_through_the_address_kernels(eng, world, search, gpl):
    """scan_group's batch inverse 0 with its emit_degen, the next-centre add with inverse 0 and the groups that
    follow it in the same lane (four groups per lane: their centres are off the curve and they are walked all the
    same), and k_giant_scan's collapsed lane-offset add.  The hit set equals the model's in every group, n_degenerate
    equals the model's record count (the address collect returns the count only), and the host refuses every hit
    on a point that is not its key's."""
    four, eight = degenerate_jobs(world, gpl)
    # 3 groups x 7 centres x 2 signs, less the point at infinity and the two shared starts
    # (+-_2Gn as the centre of group 3 / 1 both start at -2 * _2Gn; +Gn[511] in group 1 is -Gn[511] in group 0)
    assert len(four) == (41 if gpl == 1 else 39) and len(eight) == (0 if gpl == 1 else 2)
    launches = [(mix(four, world.ordinary(70 - len(four))), NGROUPS)]
    if eight:
        launches.append((mix(eight, world.ordinary(64)), 8))
    for jobs, ngroups in launches:
        case = Case(eng, world, jobs, gpl, ngroups, search)
        try:
            case.check()
            flagged = {r for rec in case.records for r in rec if r & 0x80000000}
            if ngroups == 8:
                assert flagged == {0x80000004}
                assert [0x80000004 in rec for rec in case.records] == [bool(j.directed) for j in jobs]
            else:
                # a start of +-2 * _2Gn (built for its degenerate group) collapses lane 2's add as well
                assert flagged == ({0x80000001, 0x80000002, 0x80000003} if gpl == 1 else set())
                assert all(case.records[j] for j, job in enumerate(jobs) if job.directed)
                assert not any(case.records[j] for j, job in enumerate(jobs) if not job.directed)
            bad = _check_confirm(case, world)
            if gpl == 4:      # groups after a degenerate one in the same lane
                assert any((j, g) in bad and g not in case.records[j] for j, g in bad)
        finally:
            case.close()


# ------------------------------------------------------------------------------------------------ c. the driver

@pytest.mark.parametrize("gpl", [1, 4])
def test_driver_on_a_degenerate_chunk(world, ora, gpl):
    """khh_addr_search over [512, 512 + 4096): the chunk's first centre is 1024 * G = _2Gn, so group 0 is degenerate
    (puzzle keys 514 and 1155 are in it) and at one group per lane lane 1's offset add collapses as well
    (offs[1] = _2Gn).  The found keys are the puzzle keys whose point the model's walk still holds, and the
    degenerate count is the model's record count; both come from addr_lanes_ref, and differ between the layouts
    where it says so (at one group per lane the later lanes restart from exact offsets: key 2683 of group 2)."""
    with open(os.path.join(GOLD, "puzzle_keys.json")) as f:
        puzzles = [int(v["key"], 16) for v in json.load(f).values()]
    inside = sorted(k for k in puzzles if 512 <= k < 512 + 4096)
    assert inside == [514, 1155, 2683]
    per_group, rec = world.model(ora.pubkey(1024).xy(), gpl, 4)
    xy = b"".join(per_group)
    own = [k for k in inside if xy[64 * (k - 512):64 * (k - 512) + 32] == ora.pubkey(k).be64()[:32]]
    with open(os.path.join(GOLD, "address", "1to32.rmd")) as f:
        A = khhost.Addr(f.read(), n_seq=4096, gpl=gpl)
    try:
        found, st = A.search(512, 512 + 4096, search=2, lanes=16384)
    finally:
        A.close()
    assert sorted(k for k, _, _ in found) == own
    assert st["degenerate"] == len(rec) and len(rec) >= 1
    assert st["chunks"] == 1 and st["keys"] == 4096
