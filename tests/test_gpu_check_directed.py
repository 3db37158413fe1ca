"""GPU: directed cases for the device second / third check (device/confirm.hpp through k_check / khb_check), the
paths that the random families of tests/test_gpu_check.py reach with probability about 1/2m or never.

The cases are tests/check_cases.py's.  For every candidate found, key, l2_hits, l3_hits and bp_hits equal the
per-slot model (adversarial.second_check_ref: Python integers, the oracle's k*G and blooms); where the oracle
defines the case the key also equals its bsgs_secondcheck.  The device tables are the oracle's, altered in place
where a class needs it, so the oracle, the model and the device see one geometry."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd.khbsgs import Engine
from tests import check_cases as cc

pytestmark = pytest.mark.gpu
COUNTERS = ("l2_hits", "l3_hits", "bp_hits")


@pytest.fixture(scope="module")
def ora_tables(ora):
    bs, tabs = cc.oracle_tables(ora)
    yield bs, tabs
    bs.close()


def _launch(e, cases):
    return e.check([c.target.be64() for c in cases], [(c.start, c.a, i) for i, c in enumerate(cases)])


def _reference(bs, tabs, cases, oracle=True):
    """The model of every case (tabs: what the device is loaded with, the oracle's blooms standing as loaded);
    oracle: its key equals bsgs_secondcheck too."""
    res = [cc.model(bs, tabs, c) for c in cases]
    if oracle:
        for c, r in zip(cases, res):
            assert r["key"] == bs.secondcheck(c.start, c.a, c.target), c.name
    return res


def _same(cases, got, res):
    """found / key / counters of every candidate equal the reference's."""
    assert len(got) == len(cases) == len(res)
    for c, g, r in zip(cases, got, res):
        assert g["found"] in (0, 1) and (g["key"] if g["found"] else None) == r["key"], (c.name, g, r["key"])
        assert tuple(g[k] for k in COUNTERS) == tuple(r[k] for k in COUNTERS), (c.name, g)


def _expect(bs, tabs, cases, got, oracle=True):
    res = _reference(bs, tabs, cases, oracle)
    _same(cases, got, res)
    return res


def _check(bs, tabs, cases, oracle=True):
    with Engine(0) as e:
        e.load_check_tables(**tabs)
        got = _launch(e, cases)
    return _expect(bs, tabs, cases, got, oracle)


def test_zero_dx_inside_a_batch(ora, ora_tables):
    """Class Z: Q == -AMP2[i2], Q == +AMP2[i2] (dx = dy = 0) and Q' == +AMP3[i] for slots 0, 1, 31.  The blooms
    hold, besides the geometry's, the model's other 31 x of each aimed batch (and of every third check they enter),
    so a wrong inverse in any slot next to the zero one lowers l2_hits (31) or l3_hits (31 x 32; i for the third
    check, which returns at slot i through the AddDirect(P, -P) arm, with the reference's key, not the target's)."""
    bs, tabs = ora_tables
    z2, z3 = cc.z2_cases(ora, bs), cc.z3_cases(ora, bs)
    with cc.saved_blooms(bs):
        cc.pin_z3_entry(ora, bs, tabs, z3)
        cc.pin_batches(ora, bs, tabs, z2 + z3, skip_zero=True)
        t = cc.current_tabs(bs, tabs)
        res = _check(bs, t, z2 + z3)
    for c, r in zip(z2 + z3, res):
        assert r["zero"] == [cc.z_slot(c)], c.name
    assert [(r["l2_hits"], r["l3_hits"]) for r in res] == [(31, 992)] * 6 + [(1, 0), (1, 1), (1, 31)]
    assert all(r["key"] is None for r in res[:6]) and all(r["key"] is not None for r in res[6:])


def test_degenerate_bases(ora, ora_tables):
    """Class K: start = 0 with a = 0, where base*G is (0, 0) and its negation (0, 0) again, and target == base*G,
    where the first AddDirect has dx = dy = 0.  Nothing is found, in the oracle either."""
    bs, tabs = ora_tables
    res = _check(bs, tabs, cc.k_cases(ora, bs))
    assert all(r["key"] is None for r in res)


def test_carries_through_several_limbs(ora, ora_tables):
    """Class C: start + a*2m carrying out of limbs 0..6, bases just below 2^k whose base2 and key sums carry, and a
    base that wraps past 2^256 (model only: nothing found).  Every planted key is found."""
    bs, tabs = ora_tables
    cases, wrap = cc.c_cases(ora, bs), cc.wrap_case(ora, bs)
    with Engine(0) as e:
        e.load_check_tables(**tabs)
        got = _launch(e, cases + [wrap])
    res = _expect(bs, tabs, cases, got[:-1])
    assert all(r["key"] is not None and r["bp_hits"] >= 1 for r in res)
    res = _expect(bs, tabs, [wrap], got[-1:], oracle=False)
    assert got[-1]["found"] == 0 and res[0]["key"] is None
    assert (wrap.start + wrap.a * tabs["m_double"]) >> 256 == 1


def test_wide_constants(ora, ora_tables):
    """Class W: m_double = 2^70 + 2^33 + 2 loaded in place of the geometry's, a = 0xFFFFFFFF; planted keys, the
    model's (the oracle's constants are fixed)."""
    bs, tabs = ora_tables
    t = dict(tabs, **cc.W_CONSTANTS)
    res = _check(bs, t, cc.w_cases(ora, bs), oracle=False)
    assert all(r["key"] is not None for r in res)


def test_random_families(ora, ora_tables):
    """Class R with the counters compared too (tests/test_gpu_check.py compares found and key)."""
    bs, tabs = ora_tables
    res = _check(bs, tabs, cc.r_cases(ora, bs))
    assert sum(r["key"] is not None for r in res) >= 48


def test_every_x_of_every_batch(ora, ora_tables):
    """Level-2 and level-3 blooms holding exactly the model's 32 second-check x and 32 x 32 third-check x of four
    nothing-to-find candidates: 32 and 1024 hits each, so any wrong x in any slot lowers a count; four unrelated
    candidates of the same launch give the model's counts (0)."""
    bs, tabs = ora_tables
    pinned, other = cc.nothing_cases(ora, 4, 0x70696e), cc.nothing_cases(ora, 4, 0x6f7468)
    with cc.saved_blooms(bs, fill=0):
        cc.pin_batches(ora, bs, tabs, pinned)
        t = cc.current_tabs(bs, tabs)
        with Engine(0) as e:
            e.load_check_tables(**t)
            got = _launch(e, pinned + other)
        res = _expect(bs, t, pinned + other, got)
    for g in got[:4]:
        assert (g["found"], g["l2_hits"], g["l3_hits"]) == (0, 32, 1024)
    assert [g["bp_hits"] for g in got] == [r["bp_hits"] for r in res]
    assert all((g["found"], g["l2_hits"], g["l3_hits"]) == (0, 0, 0) for g in got[4:])


def test_equal_bptable_keys(ora, ora_tables):
    """Class D: 18 runs of three equal 6-byte keys in the bPtable (centres 1, 254 and every residue mod 8 twice).
    The reference's probe sequence lands on the run's member with the most trailing zero bits, so on the same
    altered table the oracle finds the key planted at an even centre and loses the one at an odd centre: 18 found,
    18 lost (observed on the CPU, tests/test_adversarial_cpu.py).  The device must do exactly that."""
    bs, tabs = ora_tables
    cases = cc.d_cases(ora, bs)
    with cc.equal_key_runs(ora, bs):
        t = cc.current_tabs(bs, tabs)
        res = _check(bs, t, cases)
    found = [r["key"] is not None for r in res]
    assert sum(found) == 18 and found == [int(c.name[3:-1]) % 2 == 0 for c in cases]
    assert all(r["bp_hits"] == 1 for r in res)


def test_equal_keys_in_a_table_of_200(ora, ora_tables):
    """Class T: the runs of class D in a bPtable cut to 200 entries, loaded with m3 = 200.  The intervals the search
    halves are 100, 50, 25, 12 | 13, ... here, so the rounding of `half` shows (with 256 entries every interval is a
    power of two and (max - min + 1) / 2 probes the same entries).  The model's transcription of the reference's
    loop is the expected value.  The 32 keys of the overwritten entries are in no table any more (bp_hits 0); of
    the 16 at the centres the probe order keeps 7, and with the other rounding 8 of the 16 would change sides."""
    bs, tabs = ora_tables
    cases = cc.t_cases(ora, bs)
    with cc.equal_key_runs(ora, bs):
        t = cc.t_tabs(bs, tabs)
        res = _check(bs, t, cases, oracle=False)
    centre = [c.name.split("-")[1][1:] == c.name.split("-")[2][1:] for c in cases]
    assert [r["bp_hits"] for r in res] == [int(x) for x in centre]
    assert sum(r["key"] is not None for r in res) == 7 and not any(r["key"] for r, x in zip(res, centre) if not x)


def test_host_state_across_calls(ora, ora_tables):
    """khb_check's state on one Engine: the cached target upload (same count, other points; the same points
    again), growth of the target buffer past 256 (which must drop the cache), growth of the candidate buffers
    past 4096 with a ragged last workgroup, and tables reloaded between calls."""
    bs, tabs = ora_tables
    r = cc.r_cases(ora, bs, seed=0x7374617465)
    seventy = r[:40] + r[48:58] + r[64:84]
    # B: the same candidates over other points of the same count; planted ones keep a key to find
    tb = [ora.pubkey(c.start + c.a * 2 * bs.m + 12345 + 7 * i) if i < 40 else ora.pubkey(0x1234567 + i)
          for i, c in enumerate(seventy)]
    seventy_b = [c._replace(name=c.name + "-B", target=t) for c, t in zip(seventy, tb)]
    assert all(x.target.be64() != y.target.be64() for x, y in zip(seventy, seventy_b))
    # 300 targets, one candidate each
    r2 = cc.r_cases(ora, bs, seed=0x333030)
    three_hundred = (r2 + cc.r_cases(ora, bs, seed=0x333031) + cc.r_cases(ora, bs, seed=0x333032) +
                     cc.r_cases(ora, bs, seed=0x333033))[:300]
    # 4097 + 37 candidates, all over 3 targets; 8 of them have their target's key in their window
    rng = random.Random(0x66)
    keys3 = [rng.getrandbits(120) + 2**100 for _ in range(3)]
    tgt3 = [ora.pubkey(k) for k in keys3]
    planted_at = (0, 63, 64, 4095, 4096, 4097, 4132, 4133)
    cand = []
    for i in range(4097 + 37):
        k = i % 3
        if i in planted_at:
            a = rng.randrange(4096)
            cand.append((keys3[k] - a * 2 * bs.m - rng.randrange(2 * bs.m), a, k))
        else:
            cand.append((rng.getrandbits(190), rng.getrandbits(32), k))
    dense8 = r[:4] + r[-4:]

    ref_a = _reference(bs, tabs, seventy)               # computed once, compared five times
    with Engine(0) as e:
        e.load_check_tables(**tabs)
        _same(seventy, _launch(e, seventy), ref_a)                             # (a)
        res_b = _expect(bs, tabs, seventy_b, _launch(e, seventy_b))            # (b) same count, other points
        assert sum(x["key"] is not None for x in res_b) >= 36
        assert [x["key"] for x in res_b] != [x["key"] for x in ref_a]
        _same(seventy, _launch(e, seventy), ref_a)                             # (c) A again
        _same(seventy, _launch(e, seventy), ref_a)                             #     and once more: the cached path
        _expect(bs, tabs, three_hundred, _launch(e, three_hundred))            # (d) the target buffer grows
        _same(seventy, _launch(e, seventy), ref_a)                             # (e) A after the growth
        got = e.check([t.be64() for t in tgt3], cand)                          # (f) the candidate buffers grow
        assert len(got) == 4134
        for i, ((s, a, k), g) in enumerate(zip(cand, got)):                    # the oracle on all 4134: under a second
            ref = bs.secondcheck(s, a, tgt3[k])
            assert (g["key"] if g["found"] else None) == ref, i
            assert (ref is not None) == (i in planted_at) and (ref is None or ref == keys3[k]), i
        for i in list(planted_at) + list(range(1, 4134, 97)):
            s, a, k = cand[i]
            m = cc.model(bs, tabs, cc.Case(f"f-{i}", s, a, tgt3[k], "f"))
            assert tuple(got[i][c] for c in COUNTERS) == tuple(m[c] for c in COUNTERS), i
        with cc.saved_blooms(bs, fill=0xFF):                                   # (g) tables reloaded: dense blooms
            t = cc.current_tabs(bs, tabs)
            e.load_check_tables(**t)
            res = _expect(bs, t, dense8, _launch(e, dense8))
            assert all(x["l2_hits"] == 32 and x["l3_hits"] == 1024 for x in res[-4:])
        e.load_check_tables(**tabs)                                            # (h) the real ones again
        _same(seventy, _launch(e, seventy), ref_a)
