"""The tests' own Keccak for -m address -c eth: Keccak-f[1600] vectorised over a batch with numpy uint64 arrays
(restated from the Keccak reference, Bertoni et al. 2011), a sponge with rate 136 that takes the pad byte as a
parameter (0x01 = Keccak-256 as Ethereum uses it, 0x06 = SHA3-256, which hashlib can check), and the address of a
public key: bytes 12..31 of keccak256(x || y).  Independent of the product code; tests/test_eth_host.py pins it
against hashlib.sha3_256, the empty-message Keccak-256 digest and the 32 lines of tests/golden/address/1to32.eth."""
from __future__ import annotations

import numpy as np

RATE = 136

_RC = np.array([
    0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B,
    0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088,
    0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089,
    0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A,
    0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008], dtype=np.uint64)


def _rho_offsets():
    """r[x][y] of the specification: (x, y) walks (1, 0) -> (y, 2x + 3y) with offsets (t + 1)(t + 2) / 2."""
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


_RHO = _rho_offsets()


def _rotl(v, n):
    n %= 64
    if n == 0:
        return v
    return (v << np.uint64(n)) | (v >> np.uint64(64 - n))


def keccak_f(state):
    """state: uint64 array [n, 25] (lane x + 5y), permuted in place and returned."""
    a = [[state[:, x + 5 * y].copy() for y in range(5)] for x in range(5)]
    for rnd in range(24):
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        b = [[None] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y] ^ d[x], _RHO[x][y])
        for x in range(5):
            for y in range(5):
                a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y])
        a[0][0] = a[0][0] ^ _RC[rnd]
    for x in range(5):
        for y in range(5):
            state[:, x + 5 * y] = a[x][y]
    return state


def keccak256_many(msgs: np.ndarray, pad: int = 0x01) -> np.ndarray:
    """Digests [n, 32] (uint8) of n messages of one length, msgs: uint8 [n, len]."""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, ln = msgs.shape
    blocks = ln // RATE + 1
    buf = np.zeros((n, blocks * RATE), dtype=np.uint8)
    buf[:, :ln] = msgs
    buf[:, ln] ^= pad
    buf[:, -1] ^= 0x80
    state = np.zeros((n, 25), dtype=np.uint64)
    for k in range(blocks):
        lanes = buf[:, k * RATE:(k + 1) * RATE].copy().view("<u8")
        state[:, :RATE // 8] ^= lanes
        keccak_f(state)
    return state[:, :4].astype("<u8").view(np.uint8).reshape(n, 32)


def keccak256(msg: bytes, pad: int = 0x01) -> bytes:
    return keccak256_many(np.frombuffer(msg, dtype=np.uint8).reshape(1, len(msg)), pad)[0].tobytes()


def eth_addresses(xy: np.ndarray) -> np.ndarray:
    """Addresses [n, 20] of n public keys x || y (uint8 [n, 64], each coordinate big-endian)."""
    return np.ascontiguousarray(keccak256_many(np.asarray(xy, dtype=np.uint8).reshape(-1, 64))[:, 12:])


def eth_address(xy: bytes) -> bytes:
    return eth_addresses(np.frombuffer(xy, dtype=np.uint8))[0].tobytes()


def single_bit_inputs() -> np.ndarray:
    """The 512 messages with exactly one bit of x || y set: every lane, half and bit of the serialisation once."""
    m = np.zeros((512, 64), dtype=np.uint8)
    for i in range(512):
        m[i, i // 8] = 1 << (i % 8)
    return m
