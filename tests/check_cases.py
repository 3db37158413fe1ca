"""Directed cases for the second / third check (device/confirm.hpp, k_check, khb_check): one list shared by the
CPU and the GPU tests (test infrastructure, a plain module like tests/adversarial.py).

Geometry N = 2^36, k = 1 (m = 2^18, m2 = 2^13, m3 = 2^8).  A case is (name, start, a, target, cls): the chunk
base, the giant step, the target as an oracle Point and its class.

  Z   dx == 0 inside a 32-element batch: Q == -AMP2[i2], Q == +AMP2[i2], Q' == +AMP3[i]
  K   degenerate bases: start = 0 with a = 0 (0*G is (0, 0)), target == base*G
  C   bases whose sums carry through several limbs, and a base that wraps past 2^256
  W   constants wider than one limb, loaded in place of the geometry's (checked by the model alone)
  R   the three random families of tests/test_gpu_check.py
  D   runs of three equal 6-byte keys in the bPtable
  T   the same runs in a table of 200 entries, where the binary search's halvings round (model alone)

and the helpers that alter the oracle's blooms and bPtable in place (always restored by the caller's `finally`
through the context managers here), so that the oracle, the model (adversarial.second_check_ref, which reads the
oracle's blooms) and the tables handed to the code under test stay one geometry.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import random
from collections import namedtuple

from tests import adversarial as adv

N_GEOM = "0x1000000000"        # N = 2^36: m = 2^18, m2 = 2^13, m3 = 2^8
Case = namedtuple("Case", "name start a target cls")

# W: m_double wider than one limb: the product with a = 0xFFFFFFFF carries through three limbs
WIDE_M_DOUBLE = 2**70 + 2**33 + 2


def splitmix(seed):
    s = seed
    while True:
        s = (s + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        yield z ^ (z >> 31)


def oracle_tables(ora):
    """(oracle Bsgs, everything Engine.load_check_tables takes) from the ORACLE's geometry and a GTable built from
    the oracle's ComputePublicKey, so a comparison does not route through libkhhost.  The caller closes the Bsgs."""
    bs = ora.Bsgs(N_GEOM, 1)
    # GTable: entry 256*i + b - 1 = b * 2^(8i) * G (b < 256); entry 256*i + 255 = 2^(8(i+1)) * G
    parts = []
    for i in range(32):
        for b in range(1, 257):
            parts.append(ora.pubkey(b << (8 * i)).be64())
    gt = b"".join(parts)
    tabs = {"gtable": gt, "amp2": bs.amp_table(2), "amp3": bs.amp_table(3), "l2": bs.bloom_concat(2),
            "l3": bs.bloom_concat(3), "bptable": bptable_raw(bs), "m3": bs.m3, "m_double": 2 * bs.m,
            "m2_double": 2 * bs.m2, "m3_value": bs.m3, "m3_double": 2 * bs.m3}
    return bs, tabs


def bptable_raw(bs) -> bytes:
    return b"".join(v + b"\0\0" + idx.to_bytes(8, "little") for v, idx in bs.bptable())


def current_tabs(bs, tabs: dict, **over) -> dict:
    """tabs with the oracle's blooms and bPtable as they stand now (after an alteration in place)."""
    return dict(tabs, l2=bs.bloom_concat(2), l3=bs.bloom_concat(3), bptable=bptable_raw(bs), **over)


def model(bs, tabs: dict, case: Case) -> dict:
    return adv.second_check_ref(dict(tabs, bs=bs), case.start, case.a, case.target.xy())


def random_cases(ora, bs, seed):
    """(base, a, target point, kind): planted keys across a candidate's window, the third check's
    AddDirect(P, -P) case, random candidates."""
    r = splitmix(seed)
    m, m2, m3 = bs.m, bs.m2, bs.m3
    out = []
    for _ in range(48):
        base = next(r) | ((next(r) & 0xFFFF) << 64)
        a = next(r) % 4096
        key = base + a * 2 * m + next(r) % (2 * m + 64)
        out.append((base, a, ora.pubkey(key), "planted"))
    for _ in range(16):
        base, a = next(r), next(r) % 4096
        i2, i = next(r) % 32, next(r) % 32
        key = base + a * 2 * m + i2 * 2 * m2 + i * 2 * m3 + m3
        out.append((base, a, ora.pubkey(key), "special"))
    for _ in range(32):
        base = next(r) | (next(r) << 64) | ((next(r) >> 8) << 128)
        out.append((base, next(r) & 0xFFFFFFFF, ora.pubkey(next(r) | (next(r) << 64) | (next(r) << 128)), "random"))
    return out


def r_cases(ora, bs, seed=0x636865636b34):
    return [Case(f"R-{kind}-{n}", base, a, tgt, "R") for n, (base, a, tgt, kind) in enumerate(random_cases(ora, bs, seed))]


def nothing_cases(ora, n: int, seed: int):
    """n random candidates with nothing to find."""
    rng = random.Random(seed)
    return [Case(f"N-{i}", rng.getrandbits(190), rng.getrandbits(32), ora.pubkey(rng.randrange(1, 2**250)), "N")
            for i in range(n)]


def z2_cases(ora, bs, seed=0x5a32):
    """Q == -AMP2[i2] (key = base + (2 i2 + 1) m2) and Q == +AMP2[i2] (key = base - (2 i2 + 1) m2; dx = dy = 0)."""
    rng = random.Random(seed)
    out = []
    for sign in (+1, -1):
        for i2 in (0, 1, 31):
            start, a = rng.getrandbits(70) + 2**40, rng.randrange(4096)
            key = start + a * 2 * bs.m + sign * (2 * i2 + 1) * bs.m2
            out.append(Case(f"Z2{'-' if sign > 0 else '+'}amp2[{i2}]", start, a, ora.pubkey(key), "Z2"))
    return out


def z3_cases(ora, bs, seed=0x5a33):
    """Q' == +AMP3[i] in the third check of i2 = 0: key = base2 - (2i + 1) m3 with base2 = base.  The key lies
    below the candidate's window, so the level-2 bloom does not send slot 0 into the third check by itself: the
    tests add the model's xs2[0] to the oracle's level-2 bloom (pin_z3_entry), a false positive placed by hand."""
    rng = random.Random(seed)
    out = []
    for i in (0, 1, 31):
        start, a = rng.getrandbits(70) + 2**40, rng.randrange(4096)
        key = start + a * 2 * bs.m - (2 * i + 1) * bs.m3
        out.append(Case(f"Z3+amp3[{i}]", start, a, ora.pubkey(key), "Z3"))
    return out


def z_slot(case: Case):
    """(level, slot) of the dx == 0 element a Z case is aimed at."""
    return (int(case.name[1]), int(case.name[case.name.index("[") + 1:-1]))


def k_cases(ora, bs, seed=0x4b):
    rng = random.Random(seed)
    out = [Case(f"K-zero-key{k}", 0, 0, ora.pubkey(k), "K") for k in (1, 5, 2 * bs.m + 3)]
    for a in (0, 4095):
        start = rng.getrandbits(100) + 2**64
        out.append(Case(f"K-target-is-base-a{a}", start, a, ora.pubkey(start + a * 2 * bs.m), "K"))
    return out


def c_cases(ora, bs, seed=0x43):
    """start = 2^k - 1 - d, d < 2m: start + a*2m carries out of limb k/32 - 1 through every limb below it that the
    all-ones run fills.  Second family: start = 2^k - 1 - d - a*2m, so the candidate's base is 2^k - 1 - d and it is
    base2 (i2 * 2 m2) and the final key sum that carry.  A planted key at a random offset of the window in each."""
    rng = random.Random(seed)
    out = []
    for k in (32, 64, 96, 128, 160, 192, 224):
        for a in (1, 4095):
            d = rng.randrange(2 * bs.m)
            start = 2**k - 1 - d
            key = start + a * 2 * bs.m + rng.randrange(2 * bs.m)
            out.append(Case(f"C-2^{k}-a{a}", start, a, ora.pubkey(key), "C"))
    for k in (64, 96, 160, 224):
        a, d = 4095, rng.randrange(2 * bs.m - 4 * bs.m2)
        start = 2**k - 1 - d - a * 2 * bs.m
        key = 2**k + rng.randrange(2 * bs.m - d - 1)          # past the carry, inside the window
        out.append(Case(f"C-base-below-2^{k}", start, a, ora.pubkey(key), "C"))
    return out


def wrap_case(ora, bs, seed=0x57):
    """start + a*m_double wraps past 2^256 (the device's U8 and the model are modulo 2^256); nothing to find."""
    rng = random.Random(seed)
    return Case("C-wrap", 2**256 - 1 - rng.randrange(2 * bs.m), 3, ora.pubkey(rng.randrange(1, 2**250)), "Cw")


def w_cases(ora, bs, seed=0x77):
    """Planted keys under the loaded constant m_double = WIDE_M_DOUBLE with a = 0xFFFFFFFF; limb 1 of start is all
    ones, so the product's carries meet a carry of the sum."""
    rng = random.Random(seed)
    out = []
    a = 0xFFFFFFFF
    for n in range(4):
        start = rng.getrandbits(96) | (0xFFFFFFFF << 32)
        key = start + a * WIDE_M_DOUBLE + rng.randrange(2 * bs.m)
        out.append(Case(f"W-{n}", start, a, ora.pubkey(key), "W"))
    return out


W_CONSTANTS = {"m_double": WIDE_M_DOUBLE}


# ---------------------------------------------------------------------------- the oracle's tables, altered in place

def _bloom_add(ora, bs, level: int, x: int) -> None:
    xb = x.to_bytes(32, "big")
    ora.lib().ora_bloom_add(C.byref(bs.bloom(level, xb[0])), xb, 32)


@contextlib.contextmanager
def saved_blooms(bs, fill=None):
    """Keep the oracle's level-2 and level-3 sub-blooms and put them back on exit; fill: a byte to set them to."""
    saved = []
    for lvl in (2, 3):
        for i in range(256):
            b = bs.bloom(lvl, i)
            saved.append((b, C.string_at(b.bf, b.bytes)))
            if fill is not None:
                C.memset(b.bf, fill, b.bytes)
    try:
        yield
    finally:
        for b, raw in saved:
            C.memmove(b.bf, raw, b.bytes)


def pin_batches(ora, bs, tabs: dict, cases, skip_zero: bool = False) -> None:
    """Add the model's 32 second-check x of every case to the oracle's level-2 bloom and then the 32 x of every
    third check that enters to level 3 (skip_zero: not the dx == 0 elements).  Call inside saved_blooms."""
    for level in (2, 3):
        for c in cases:
            r = model(bs, tabs, c)
            zero = set(r["zero"]) if skip_zero else set()
            batches = [r["xs2"]] if level == 2 else r["xs3"].values()
            for xs in batches:
                for i, x in enumerate(xs):
                    if (level, i) not in zero:
                        _bloom_add(ora, bs, level, x)


def pin_z3_entry(ora, bs, tabs: dict, cases) -> None:
    """The hand-placed level-2 false positive of the Z3 cases: xs2[0]."""
    for c in cases:
        _bloom_add(ora, bs, 2, model(bs, tabs, c)["xs2"][0])


D_CENTRES = (1, 254, 12, 25, 38, 51, 64, 77, 90, 103, 108, 121, 134, 147, 160, 173, 186, 199)


@contextlib.contextmanager
def equal_key_runs(ora, bs, centres=D_CENTRES):
    """Entries p - 1 and p + 1 of the oracle's bPtable get entry p's 6-byte value and keep their own index: the
    table stays sorted, with runs of three equal keys.  Restored on exit."""
    t = ora.lib().ora_bsgs_bptable(bs.h)
    saved = [(i, bytes(t[i].value)) for p in centres for i in (p - 1, p + 1)]
    try:
        for p in centres:
            for i in (p - 1, p + 1):
                C.memmove(t[i].value, bytes(t[p].value), 6)
        yield
    finally:
        for i, raw in saved:
            C.memmove(t[i].value, raw, 6)


T_ENTRIES = 200                # a bPtable size that is no power of two: the halvings round


def t_cases(ora, bs, seed=0x54):
    """For the bPtable cut to its first T_ENTRIES entries (with the equal-key runs that fit): the keys whose baby
    step is the index of entry p - 1, p and p + 1 of every run.  With 256 entries every interval the search halves
    is a power of two; with 200 they are 100, 50, 25, 12 | 13, ..., so how `half` rounds decides which member of a
    run is landed on.  Checked by the model alone (the oracle's table size is its geometry's)."""
    rng = random.Random(seed)
    table = bs.bptable()
    out = []
    for p in D_CENTRES:
        if p + 1 >= T_ENTRIES:
            continue
        for e in (p - 1, p, p + 1):
            start, a = rng.getrandbits(80) + 2**40, rng.randrange(4096)
            i2, i = rng.randrange(32), rng.randrange(32)
            key = start + a * 2 * bs.m + i2 * 2 * bs.m2 + (2 * i + 1) * bs.m3 + table[e][1] + 1
            out.append(Case(f"T-p{p}-e{e}", start, a, ora.pubkey(key), "T"))
    return out


def t_tabs(bs, tabs: dict) -> dict:
    """Call inside equal_key_runs: the altered table's first T_ENTRIES entries."""
    return dict(tabs, bptable=bptable_raw(bs)[:16 * T_ENTRIES], m3=T_ENTRIES)


def d_cases(ora, bs, centres=D_CENTRES, seed=0x44):
    """For each run centre p, the key whose baby step is entry p's index j, with both signs of +-(j + 1).  Build
    from the UNALTERED table's indices (the runs keep every entry's own index, so either works)."""
    rng = random.Random(seed)
    table = bs.bptable()
    out = []
    for p in centres:
        j = table[p][1]
        for sign in (+1, -1):
            start, a = rng.getrandbits(80) + 2**40, rng.randrange(4096)
            i2, i = rng.randrange(32), rng.randrange(32)
            key = start + a * 2 * bs.m + i2 * 2 * bs.m2 + (2 * i + 1) * bs.m3 + sign * (j + 1)
            out.append(Case(f"D-p{p}{'+' if sign > 0 else '-'}", start, a, ora.pubkey(key), "D"))
    return out
