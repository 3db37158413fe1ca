"""The lazy field arithmetic of csrc/device/fe_asm.hpp on Python integers (test infrastructure), twice:

  * lazy(op, a, b): what the raw value of khb_field_op ops 0 (mul), 1 (sqr), 6 (sqr_add), 5 (add_lazy), 3 (sub) IS,
    as closed integer formulas with M = 2^256 and K = 2^32 + 977, and the rare-carry flags as inequalities on the
    same integers.  This is the definition every test pins the device and the limb model to.
  * device(op, a, b): one limb-level model of the header as it computes today -- forward-carried columns with
    dropped first carries, the per-limb V mads, the R chain on the truncated values, the one-mad second fold, and
    the general path (carry fix, general fold) exactly when a mask is set; ops 5 and 3 with their carry into limb 2
    as a mask.  It reports every mask, so that operand generators can certify what an operand does.

check(op, a, b) asserts that the two agree and returns the model's result."""
from __future__ import annotations

P = 2**256 - 2**32 - 977
K = 2**32 + 977                      # 2^256 mod p
M32, M64, M256 = 2**32 - 1, 2**64 - 1, 2**256 - 1
PMAX = M32 * M32
MUL_MASKED = tuple(range(3, 14))     # fm_mul512x's m[0..10]
SQR_MASKED = tuple(range(6, 11))     # fm_sqr512x's m[0..4]

# field self-test op numbers (include/khbsgs.h khb_field_op) -> the canonical value
EXACT = {0: lambda a, b: a * b % P, 1: lambda a, b: a * a % P, 3: lambda a, b: (a - b) % P,
         5: lambda a, b: (a + b) % P, 6: lambda a, b: (a * a + b) % P}


def limbs(v: int, n: int = 8) -> list:
    return [(v >> (32 * i)) & M32 for i in range(n)]


def value(w) -> int:
    return sum(x << (32 * i) for i, x in enumerate(w))


def propagate(r: list, k: int, c: int) -> int:
    """fm_propagate<K>: r[k..7] += c, carry-out returned."""
    for i in range(k, 8):
        t = r[i] + c
        r[i] = t & M32
        c = t >> 32
    return c


# ------------------------------------------------------------------------------- the integer definitions

def expected_ov(op: int, a: int, b: int) -> list:
    """The carry-out of each V mad from the integers alone: H_i K + Lw_i >= 2^64."""
    t = a * b if op == 0 else a * a
    lw = (t & M256) + (b if op == 6 else 0)
    return [int(((t >> (256 + 32 * i)) & M32) * K + ((lw >> (32 * i)) & M32) >= 2**64) for i in range(8)]


def lazy(op: int, a: int, b: int):
    """(raw lazy value, flags) of the op from the integers: c3, wrap, ov (ops 0, 1, 6), lazy_c2 (5), sub_b2 (3)."""
    if op == 5:
        s = a + b
        c = s >> 256
        return (s & M256) + c * K, {"lazy_c2": ((s & M64) + c * K) >> 64}
    if op == 3:
        d = a - b
        return (d + P if d < 0 else d), {"sub_b2": int(d < 0 and d & M64 < K)}
    t = a * b if op == 0 else a * a
    S = (t & M256) + (b if op == 6 else 0) + (t >> 256) * K
    top = S >> 256
    c3 = ((S & (2**96 - 1)) + top * K) >> 96
    r = (S & M256) + top * K
    wrap = r >> 256
    if wrap:
        r = (r & M256) + K
    return r, {"c3": c3, "wrap": wrap, "ov": expected_ov(op, a, b)}


def canon(a: int) -> int:
    """fm_canon: a + K carries out of 2^256 iff a >= p."""
    t = a + K
    return t & M256 if t >> 256 else a


# ------------------------------------------------------------------------- the device, limb by limb: products

def _columns(products, masked):
    """products[K]: the (x, y) limb pairs of column K, in the device's order; masked: the columns whose first product
    may drop a carry.  (t[0..15], hi[K], cw[K], total[K], first[K]): hi and cw are what column K hands on, total its
    unreduced sum, seed included, first the dropped carry of its first product.  Column K's pair starts as
    {lo = hi(S of column K-1), hi = cw of column K-1}; the dropped carries go back in at word K + 2 (fm_fix_cols)."""
    t, his, cws, totals, first = [], [], [], [], []
    hi = cw = 0
    for k, col in enumerate(products):
        S = (cw << 32) | hi
        cw = 0
        total = S
        drop = 0
        for n, (x, y) in enumerate(col):
            S += x * y
            total += x * y
            if n == 0:
                drop = S >> 64
                assert drop == 0 or k in masked, "an unmasked column's first product overflowed its seed"
            else:
                cw += S >> 64
            S &= M64
        t.append(S & M32)
        hi = S >> 32
        his.append(hi)
        cws.append(cw)
        totals.append(total)
        first.append(drop)
    assert cw == 0
    t.append(hi)                          # column 14's high word is t[15]
    if any(first):
        v = value(t) + sum(d << (32 * (k + 2)) for k, d in enumerate(first))
        assert v >> 512 == 0
        t = limbs(v, 16)
    return t, his, cws, totals, first


def mul_products(A, B):
    return [[(A[i], B[k - i]) for i in range(max(0, k - 7), min(k, 7) + 1)] for k in range(15)]


def cross_products(A):
    return [[(A[i], A[k - i]) for i in range(max(0, k - 7), (k - 1) // 2 + 1)] for k in range(15)]


def cols_mul(a: int, b: int):
    """fm_mul512x: (t, hi, cw, total, first) of the columns of a*b."""
    return _columns(mul_products(limbs(a), limbs(b)), MUL_MASKED)


def cols_cross(a: int):
    """The cross sum of fm_sqr512x, sum_{i<j} a_i a_j 2^(32(i+j)): (c, hi, cw, total, first); c[0] = c[15] = 0."""
    r = _columns(cross_products(limbs(a)), SQR_MASKED)
    assert r[0][0] == 0 and r[0][15] == 0
    return r


def product(op: int, a: int, b: int):
    """(the 512-bit product ops 0, 1, 6 reduce, as the columns leave it; the masked columns that dropped a carry).
    fm_sqr512x's tail, diagonal + doubled cross sum by funnel shifts and one carry chain, is plain addition."""
    if op == 0:
        t, _, _, _, first = cols_mul(a, b)
        t = value(t)
    else:
        c, _, _, _, first = cols_cross(a)
        t = sum(x * x << (64 * i) for i, x in enumerate(limbs(a))) + 2 * value(c)
    assert t == (a * b if op == 0 else a * a)
    return t, [k for k, d in enumerate(first) if d]


def cols_sqr(a: int):
    """fm_sqr512x: t = diagonal + 2 cross as 16 words."""
    return limbs(product(1, a, 0)[0], 16)


# ------------------------------------------------------------------------ the device, limb by limb: reduction

def _reduce(t: int, w: int):
    """fm_reduce_V on Lw = (t mod 2^256) + w and H = t >> 256: the raw value and the flags."""
    lw = (t & M256) + w
    Lw8, h = lw >> 256, t >> 256
    ov, R, c = [], [], 0                 # c: hi(V_{i-1}) + the chain's carry, < 2^33
    for i in range(8):
        hi = (h >> (32 * i)) & M32
        v = 977 * hi + ((hi << 32) | ((lw >> (32 * i)) & M32))
        ov.append(v >> 64)
        s = (v & M32) + c
        R.append(s & M32)
        c = ((v >> 32) & M32) + (s >> 32)
    s = Lw8 + c
    R8, r9 = s & M32, s >> 32
    assert r9 in (0, 1) and all(x in (0, 1) for x in ov)
    # common form, on R as the chain left it
    m = R8 * 977 + (R[1] << 32 | R[0])
    o, m = m >> 64, m & M64
    s = (m >> 32) + R8
    n1, c = s & M32, s >> 32
    s = R[2] + c
    n2, c2 = s & M32, s >> 32
    flags = {"path": "fast", "r9": r9, "o": o, "c2": c2, "ov": ov, "c3": 0, "wrap": 0}
    if not (any(ov) or r9 or o or c2):
        R[0], R[1], R[2] = m & M32, n1, n2
        return value(R), flags
    flags["path"] = "general"
    R += [R8, r9]
    if any(ov):                          # fm_fix_R: R[i + 2] += ov[i], one chain
        c = 0
        for i in range(8):
            s = R[i + 2] + ov[i] + c
            R[i + 2], c = s & M32, s >> 32
        assert c == 0
    assert value(R) == lw + h * K
    R8, R9 = R[8], R[9]
    assert (R9 << 32 | R8) < 3 * 2**32
    R = R[:8]
    # fm_fold2: top*977 at limb 0, top*2^32 at limb 1, the carry into limb 3 and the wrap past 2^256
    u = R8 * 977 + (((R9 * 977) & M32) << 32)
    ww = ((u >> 32) & M32) + R8
    w2 = ((ww >> 32) + R9) & M32
    s = R[0] + (u & M32)
    R[0], c = s & M32, s >> 32
    s = R[1] + (ww & M32) + c
    R[1], c = s & M32, s >> 32
    s = R[2] + w2 + c
    R[2], c3 = s & M32, s >> 32
    wrap = 0
    if c3:
        wrap = propagate(R, 3, c3)
        s = R[0] + wrap * 977
        R[0] = s & M32
        s = R[1] + wrap + (s >> 32)
        R[1] = s & M32
        propagate(R, 2, s >> 32)
    flags["c3"], flags["wrap"] = c3, wrap
    return value(R), flags


def _add_lazy(a: int, b: int):
    """fm_add_lazy(a < p, b < 2^256) with the carry into limb 2 as a mask."""
    s = a + b
    c, s = s >> 256, limbs(s & M256)
    t = s[0] + 0x3D1 * c
    s[0] = t & M32
    t = s[1] + c + (t >> 32)
    s[1], c2 = t & M32, t >> 32
    if c2:                               # the rare branch: the mask's bit, propagated from limb 2
        propagate(s, 2, 1)
    return value(s), {"lazy_c2": c2}


def _sub(a: int, b: int):
    """fm_sub(a < 2^256, b < p) with the borrow into limb 2 as a mask."""
    d = a - b
    bo, d = int(d < 0), limbs(d & M256)
    t = d[0] - (0x3D1 if bo else 0)
    d[0], br = t & M32, int(t < 0)
    t = d[1] - bo - br
    d[1], b2 = t & M32, int(t < 0)
    if b2:
        br = 1
        for i in range(2, 8):
            t = d[i] - br
            d[i], br = t & M32, int(t < 0)
    return value(d), {"sub_b2": b2}


def device(op: int, a: int, b: int):
    """(raw value, flags) as the device computes them.  Ops 0, 1, 6: path ("fast" or "general"), ov[0..7], r9, o,
    c2 (the masks, on R before the carry fix), c3, wrap (the general fold's; 0 on the fast path) and drops (the
    masked columns whose first product dropped its carry).  Op 5: lazy_c2.  Op 3: sub_b2."""
    if op == 5:
        return _add_lazy(a, b)
    if op == 3:
        return _sub(a, b)
    t, drops = product(op, a, b)
    r, flags = _reduce(t, b if op == 6 else 0)
    flags["drops"] = drops
    return r, flags


def check(op: int, a: int, b: int):
    """device() after asserting that it equals lazy() in the value and in every flag lazy() defines, and that the
    value is < 2^256 and congruent to the exact result."""
    v, f = device(op, a, b)
    r, g = lazy(op, a, b)
    assert v == r and all(f[k] == g[k] for k in g), (op, hex(a), hex(b), f, g)
    assert r < 2**256 and r % P == EXACT[op](a, b), (op, hex(a), hex(b))
    return v, f
