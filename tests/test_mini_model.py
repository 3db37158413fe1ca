"""The tests' model of -m minikeys (tests/mini_ref.py) pinned outside the code under test: the published Casascius
sample, the help text's minikey, and the counts of valid candidates in the spans the GPU tests use."""
from __future__ import annotations

import pytest

from tests import mini_ref as mr


def test_casascius_sample(ora):
    """The 30-character sample of the Casascius minikey format: the key rule (SHA-256 of the string) and the address
    of its uncompressed public key."""
    s = "S6c56bnXQiBjk9mqSYE7ykVQ7NzrRy"
    import hashlib
    assert hashlib.sha256(s.encode() + b"?").digest()[0] == 0
    k = int.from_bytes(hashlib.sha256(s.encode()).digest(), "big")
    assert k == 0x4C7A9640C72DC2099F23715D0C8A0D8A35F8906E3CAB61DD3F78B67BF887C9AB
    assert ora.rmd_to_address(ora.pub_hash160(ora.pubkey(k), False)) == "1CciesT23BNionJeXrbxmjc7ywfiyM4oLW"


def test_help_text_minikey():
    s = "SRPqx8QiwnW4WNWnTVa2W5"
    assert mr.valid(s)
    assert f"{mr.key(s):064x}".startswith("5fc7a3dd") and f"{mr.key(s):064x}".endswith("8225a804")
    assert mr.string(mr.value(s)) == s and mr.step(s, 0) == s


def test_counter_model():
    assert mr.step("SRPqx8QiwnW4WNWnTVazzz", 1) == "SRPqx8QiwnW4WNWnTVb111"
    assert mr.step("S1zzzzzzzzzzzzzzzzzzzu", 6) == "S21111111111111111111" + "1"
    assert mr.string(0) == "S" + "1" * 21 and mr.string(mr.SPACE - 1) == "S" + "z" * 21
    rev = mr.ALPHABET[::-1]
    assert mr.string(0, rev) == "S" + "z" * 21 and mr.value("S" + "z" * 20 + "y", rev) == 1


@pytest.mark.parametrize("first,count,want", mr.SPANS)
def test_span_counts(first, count, want):
    offs = mr.valid_offsets(first, count)
    assert len(offs) == want
    assert offs == sorted(set(offs)) and all(0 <= o < count for o in offs)


def test_fast_enumerator_agrees():
    """valid_offsets_fast against the candidate-by-candidate model: SPANS[3] (20 blocks of 58^2 from mid-block), the
    span that carries through 20 digits, another alphabet, a span inside one block and a prefix cut from the cache."""
    first, count, want = mr.SPANS[3]
    ref = mr.valid_offsets(first, count)
    assert mr.valid_offsets_fast(first, count) == ref and len(ref) == want
    assert mr.valid_offsets_fast(first, 10109) == mr.valid_offsets(first, 10109)      # cut from the longer one
    first, count, want = mr.SPANS[4]
    assert mr.valid_offsets_fast(first, count) == mr.valid_offsets(first, count)
    rev = mr.ALPHABET[::-1]
    first = mr.string(mr.value(mr.SPANS[0][0]), rev)
    assert mr.valid_offsets_fast(first, 10109, rev) == mr.valid_offsets(first, 10109, rev)
    inside = mr.step(mr.A, 58 * 58 + 7)
    assert mr.valid_offsets_fast(inside, 3000) == mr.valid_offsets(inside, 3000)
