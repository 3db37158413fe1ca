"""CPU checks of -m vanity's host side (libkhhost: host/vanity_host.cpp and the hooks in address_host.cpp) against the
tests' own model (tests/vanity_ref.py: Base58Check with hashlib, the interval rule written independently of the C++).
No GPU: targets, intervals, the hash-level match and khh_addr_confirm on keys."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd import khhost
from tests import vanity_ref as vr

TARGETS = ["1", "11", "111", "1A", "1Q", "1QL", "1R", "1z", "1abc", "1Love"]
SHORT = ["1A", "1Q", "1QL", "1z", "111"]


def _addr(targets, **kw):
    return khhost.Addr("\n".join(targets) + "\n", n_seq=1 << 16, threads=2, mode="vanity", **kw)


def _ints(iv):
    return [(int.from_bytes(a, "big"), int.from_bytes(b, "big")) for a, b in iv]


def _check_values(A, targets, table, values, ends=()):
    """The three properties of a hash value: range membership (the library's and the model's agree) is a superset of
    startswith; the two differ only at an interval end; the library's confirmation equals startswith."""
    got = A.vanity_match(b"".join(vr.b20(v) for v in values))
    ends = set(ends)
    n_in = n_match = 0
    for v, g in zip(values, got):
        inside, match = v in table, vr.startswith_any(v, targets)
        assert bool(g & 1) == inside, hex(v)
        assert bool(g & 2) == match, (hex(v), vr.address(v))
        assert inside or not match, (hex(v), vr.address(v))
        if inside != match:
            assert v in ends, (hex(v), vr.address(v))
        n_in += inside
        n_match += match
    return n_in, n_match


@pytest.mark.parametrize("targets", [[t] for t in TARGETS] + [TARGETS])
def test_intervals_equal_model(targets):
    A = _addr(targets)
    assert A.skipped() == 0 and A.counted() == len(targets)
    got = _ints(A.vanity_intervals())
    assert got == vr.merged(targets) and got
    assert all(a <= b for a, b in got) and all(got[i][1] + 1 < got[i + 1][0] for i in range(len(got) - 1))
    A.close()


@pytest.mark.parametrize("targets", [[t] for t in TARGETS] + [TARGETS])
def test_interval_ends(targets):
    A = _addr(targets)
    iv = vr.merged(targets)
    ends = [e for a, b in iv for e in (a, b)]
    values = sorted({v for e in ends for v in (e - 1, e, e + 1) if 0 <= v < 1 << 160})
    n_in, n_match = _check_values(A, targets, vr.Table(iv), values, ends)
    assert n_in >= len(set(ends)) and n_match > 0
    A.close()


def test_random_hashes():
    rng = random.Random(160)
    A = _addr(SHORT)
    iv = vr.merged(SHORT)
    values = [rng.getrandbits(160) for _ in range(100_000)]
    n_in, n_match = _check_values(A, SHORT, vr.Table(iv), values, [e for ab in iv for e in ab])
    assert n_in == n_match and 2_000 < n_match < 20_000      # four first digits of 22 that follow '1', and 1/256
    A.close()


def test_1q_deviation_matches():
    """The 34-character 1Q... addresses the reference's pairing never matches."""
    h = (vr.value("1Q" + "1" * 32) >> 32) + 1
    a = vr.address(h)
    assert len(a) == 34 and a.startswith("1Q")
    A = _addr(["1Q"])
    assert A.vanity_match(vr.b20(h)) == b"\x03"
    assert h in vr.Table(_ints(A.vanity_intervals()))
    A.close()


def test_rejected_targets():
    bad = ["3abc", "1O0l", "1" + "A" * 29, ""]
    for s in bad:
        assert not khhost.vanity_target_ok(s), s
        assert vr.intervals_of(s) == []
    for s in TARGETS + ["1" + "A" * 28]:
        assert khhost.vanity_target_ok(s), s
    with pytest.raises(ValueError):                            # the binding refuses a text without a target
        _addr(bad)
    B = _addr(bad + ["1Q"])
    assert _ints(B.vanity_intervals()) == vr.merged(["1Q"]) and B.skipped() == 3 and B.counted() == 1
    B.close()


def test_merging_and_confirm():
    targets = ["1A", "1Ab", "1Ab", "1Ac"]
    A = _addr(targets)
    got = _ints(A.vanity_intervals())
    assert got == vr.merged(["1A"]) == vr.merged(targets)       # 1Ab and 1Ac lie inside 1A
    assert A.counted() == 3
    B = _addr(["1Ab", "1Ac", "1Ab"])
    gb = _ints(B.vanity_intervals())
    assert gb == vr.merged(["1Ab", "1Ac"])
    assert all(gb[i][1] + 1 < gb[i + 1][0] for i in range(len(gb) - 1))
    assert len(gb) < len(vr.intervals_of("1Ab")) + len(vr.intervals_of("1Ac"))   # 1Abz.. + 1 = 1Ac1..: joined
    # keys: khh_addr_confirm recovers the key of each form whose address begins with 1Ab, and no other
    found = 0
    for key in range(1, 40_000):
        xy = khhost.pubkey(key)
        for comp in (True, False):
            a = khhost.rmd_to_address(khhost.hash160(xy, comp))
            assert a == vr.address(khhost.hash160(xy, comp))
            kind = (int(xy[63]) & 1) if comp else 2
            r = B.confirm(key, kind)
            if a.startswith("1Ab") or a.startswith("1Ac"):
                assert r == (key, comp)
                found += a.startswith("1Ab")
            else:
                assert r is None
        if found:
            break
    assert found, "no 1Ab address among the first 40,000 keys"
    A.close()
    B.close()


def test_vanity_handle_refuses_other_searches():
    A = _addr(["1Q"])
    for search in (8, 16, 16 | 4, 3):
        with pytest.raises(khhost.KhhError):
            A.search(1, 1 << 16, search=search, lanes=256)
    A.close()
    with pytest.raises(ValueError):
        khhost.Addr("1Q\n", n_seq=1 << 16, mode="vanity", crypto="eth")
