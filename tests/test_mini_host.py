"""khhost.Minikeys on the CPU: argument checks, the string / valid / key helpers against the tests' model
(tests/mini_ref.py) and the window table of the device's k*G against the oracle's public keys."""
from __future__ import annotations

import random

import pytest

from keyhuntm1cpu_amd import khhost
from tests import mini_ref as mr


@pytest.fixture(scope="module")
def mk():
    m = khhost.Minikeys("", window_bits=4)
    yield m
    m.close()


def test_bad_alphabets_and_widths():
    for bad in (mr.ALPHABET[:57], mr.ALPHABET + "0", mr.ALPHABET[:57] + "1", "\0" + mr.ALPHABET[1:]):
        with pytest.raises(ValueError):
            khhost.Minikeys("", alphabet=bad)
    for w in (0, 5, 32):
        with pytest.raises(ValueError):
            khhost.Minikeys("", window_bits=w)


@pytest.mark.parametrize("bad", ["SRPqx8QiwnW4WNWnTVa2W", "SRPqx8QiwnW4WNWnTVa2W5x", "TRPqx8QiwnW4WNWnTVa2W5",
                                 "SRPqx8QiwnW4WNWnTVa2W0", "SRPqx8QiwnW4WNWnTVa2Wl", "", "S" + "\0" * 21])
def test_bad_bases_are_refused(mk, bad):
    for call in (lambda: mk.valid(bad), lambda: mk.key(bad), lambda: mk.string(bad, 0), lambda: mk.search(bad, 1)):
        with pytest.raises(ValueError):
            call()


def test_span_past_the_end_is_refused_without_a_launch(mk):
    """first + count > 58^21: a ValueError before any device is opened (this test runs without a GPU)."""
    last = "S" + "z" * 21
    with pytest.raises(ValueError):
        mk.search(last, 2)
    with pytest.raises(ValueError):
        mk.search(mr.step(last, -9), 11)
    with pytest.raises(ValueError):
        mk.string(last, 1)
    assert mk.string(last, 0) == last and mk.string(mr.step(last, -9), 9) == last


def test_helpers_equal_the_model(mk):
    rng = random.Random(58)
    bases = ["SRPqx8QiwnW4WNWnTVa2W5", "SRPqx8QiwnW4WNWnTVazzz", "S1zzzzzzzzzzzzzzzzzzzu", "S" + "1" * 21]
    bases += [mr.string(rng.randrange(mr.SPACE - (1 << 64))) for _ in range(20)]
    for b in bases:
        for off in (0, 1, 57, 58, 58 ** 2, 58 ** 3 - 1, 1 << 32, (1 << 64) - 1, rng.randrange(1 << 64)):
            if mr.value(b) + off < mr.SPACE:
                assert mk.string(b, off) == mr.step(b, off)
        assert mk.key(b) == mr.key(b) and mk.valid(b) == mr.valid(b)
    first, count, _ = mr.SPANS[2]
    offs = set(mr.valid_offsets(first, count))
    assert [o for o in range(count) if mk.valid(mr.step(first, o))] == sorted(offs)
    assert mk.digits("SRPqx8QiwnW4WNWnTVa2W5") == bytes(mr.digits("SRPqx8QiwnW4WNWnTVa2W5"))


def test_custom_alphabet():
    rev = mr.ALPHABET[::-1]
    with khhost.Minikeys("", alphabet=rev, window_bits=4) as m:
        assert m.string("S" + "z" * 21, 1) == "S" + "z" * 20 + "y" == mr.step("S" + "z" * 21, 1, rev)
        b = mr.string(123456789 ** 3, rev)
        assert m.string(b, 58 ** 5 + 3) == mr.step(b, 58 ** 5 + 3, rev)
        assert m.digits(b) == bytes(mr.digits(b, rev))


@pytest.mark.parametrize("w", [4, 8])
def test_window_table(ora, w):
    with khhost.Minikeys("", window_bits=w) as m:
        t = m.table_points()
    nwin, per = 256 // w, (1 << w) - 1
    assert len(t) == 64 * nwin * per and (nwin, per) in ((64, 15), (32, 255))
    rng = random.Random(w)
    pos = {(0, 1), (0, 2), (0, per), (nwin - 1, 1), (nwin - 1, per), (1, 3), (nwin // 2, per - 1)}
    pos |= {(rng.randrange(nwin), rng.randrange(1, per + 1)) for _ in range(40)}
    for j, d in sorted(pos):
        i = j * per + d - 1
        assert t[64 * i:64 * i + 64] == ora.pubkey(d << (w * j)).be64(), (w, j, d)
