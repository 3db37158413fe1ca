"""The tests' own model of -m minikeys, with hashlib for the two SHA-256 and the oracle for the point and its hash160.
It depends on nothing in the C++ under test.

A minikey is 'S' and 21 characters of a 58-character alphabet; the 21 characters are the digits of a counter in
[0, 58^21), the first the most significant.  valid: byte 0 of SHA-256(minikey || '?') is zero.  key: SHA-256(minikey)
read big-endian.  match: the hash160 of the key's uncompressed public key is a target."""
from __future__ import annotations

import hashlib

ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"     # the reference's Ccoinbuffer_default
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SPACE = 58 ** 21

# the spans the issue's counts were written against: (first, count, valid candidates among first .. first + count - 1)
# The first span carries through three digits at its second candidate, the last through 20 digits six steps in.  (The
# counts are the same whether a span begins at the named candidate or one after it; here it begins at it.)
A, B = "SRPqx8QiwnW4WNWnTVazzz", "S1zzzzzzzzzzzzzzzzzzzu"
SPANS = [(A, 63, 1), (A, 65, 1), (A, 10109, 38), (A, 65536, 275), (B, 10109, 48)]


def digits(s: str, alphabet: str = ALPHABET) -> list[int]:
    assert len(s) == 22 and s[0] == "S"
    return [alphabet.index(c) for c in s[1:]]


def value(s: str, alphabet: str = ALPHABET) -> int:
    v = 0
    for d in digits(s, alphabet):
        v = v * 58 + d
    return v


def string(v: int, alphabet: str = ALPHABET) -> str:
    assert 0 <= v < SPACE
    out = []
    for _ in range(21):
        v, d = divmod(v, 58)
        out.append(alphabet[d])
    return "S" + "".join(reversed(out))


def step(s: str, off: int, alphabet: str = ALPHABET) -> str:
    return string(value(s, alphabet) + off, alphabet)


def valid(s: str) -> bool:
    return hashlib.sha256(s.encode("latin-1") + b"?").digest()[0] == 0


def key(s: str) -> int:
    return int.from_bytes(hashlib.sha256(s.encode("latin-1")).digest(), "big")


_cache: dict = {}


def valid_offsets(first: str, count: int, alphabet: str = ALPHABET) -> list[int]:
    """Offsets from `first` of the valid candidates among first .. first + count - 1, ascending (computed once)."""
    k = (first, count, alphabet)
    if k not in _cache:
        v0 = value(first, alphabet)
        _cache[k] = [o for o in range(count) if valid(string(v0 + o, alphabet))]
    return _cache[k]


def valid_offsets_fast(first: str, count: int, alphabet: str = ALPHABET) -> list[int]:
    """valid_offsets for millions of candidates: the candidates of one 58^2 block share their first 20 characters, so
    that head is hashed once per block and every tail (two characters and '?') goes onto a copy() of it.  A span that
    is a prefix of one computed before is cut from it."""
    for (f, c, a), offs in _cache_fast.items():
        if (f, a) == (first, alphabet) and c >= count:
            return [o for o in offs if o < count]
    a = alphabet.encode("latin-1")
    tails = [bytes((a[i], a[j], 0x3F)) for i in range(58) for j in range(58)]
    v0 = value(first, alphabet)
    out, v, end = [], v0, v0 + count
    while v < end:
        block = v - v % BLOCK
        head = hashlib.sha256(string(block, alphabet)[:20].encode("latin-1"))
        stop = min(BLOCK, end - block)
        base = block - v0
        for t in range(v - block, stop):
            h = head.copy()
            h.update(tails[t])
            if h.digest()[0] == 0:
                out.append(base + t)
        v = block + stop
    _cache_fast[(first, count, alphabet)] = out
    return out


BLOCK = 58 * 58
_cache_fast: dict = {}


def rmd160(ora, s: str) -> bytes:
    """hash160 of the uncompressed public key of the minikey's key (0 < key < n)."""
    return ora.pub_hash160(ora.pubkey(key(s)), False)


def directed_scalars(w: int) -> tuple[list[int], list[int]]:
    """(good scalars, bad scalars) for the fixed-base multiplication of window width w."""
    nwin = 256 // w
    good = [1, 2, N - 1]
    for j in range(nwin):
        good += [1 << (w * j)]
        if j:
            good += [(1 << (w * j)) - 1]
        good += [((j * 7 + 3) % ((1 << w) - 1) + 1) << (w * j)]          # one non-zero window per position
    allmax = (1 << 256) - 1                                               # all windows at maximum is >= n: bad
    good += [allmax >> w, (allmax >> w) - (1 << 100)]                     # every window but the top at maximum
    good = [k for k in good if 0 < k < N]
    return good, [0, N, N + 1, allmax]
