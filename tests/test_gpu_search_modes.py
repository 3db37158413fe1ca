"""GPU: every value of khb_addr_scan's `search` in [-2, 128) reaches the kernel it names, or is KHB_EINVAL.  One
context, gpl = 1, one job of two groups, one address bloom and one vanity table.  For one point of group 1 the 16
values any mode can derive from it are computed with the tests' models (the oracle for the point and the hash160s,
tests/eth_ref.py for the ETH address) and planted: all 16 in the bloom, the 12 hash160s in the vanity table as
one-value intervals.  The kinds a search reports at that point then name the kernel that ran: every kind a mode
computes is planted, so a permuted search -> kernel mapping shows as a missing or an extra kind.  Hits at other points
(bloom false positives) are not looked at."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khhost
from tests import eth_ref

pytestmark = pytest.mark.gpu
P = 2**256 - 2**32 - 977
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE      # keyhunt.cpp:584
ENDO, ETH, XPOINT, VANITY = 4, 8, 16, 32                                        # include/khbsgs.h KHB_SEARCH_*
BASE, GROUP, T = 0x6B00000000 + 5, 1, 777                                       # planted: key BASE + 1024 + 777

# search: the kinds reported at the planted point (kind = form | e << 2; 16 = ETH; 32 | e << 2 = the x of beta^e)
_E = {4: {2, 3, 6, 7, 10, 11}, 5: {0, 1, 4, 5, 8, 9}, 6: {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}}
EXPECTED = {
    0: {2}, 1: {0, 1}, 2: {0, 1, 2},
    4: _E[4], 5: _E[5], 6: _E[6],
    8: {16},
    16: {32}, 20: {32, 36, 40},
    32: {2}, 33: {0, 1}, 34: {0, 1, 2},                                         # the vanity values: as their BTC twins
    36: _E[4], 37: _E[5], 38: _E[6],
}


@pytest.fixture(scope="module")
def world(ora):
    """(engine, centre) with the giant table, the bloom and the vanity table loaded."""
    from keyhuntm1cpu_amd.khbsgs import Engine
    x, y = ora.pubkey(BASE + 1024 * GROUP + T).xy()
    xs = [pow(BETA, e, P) * x % P for e in range(3)]
    b32 = lambda v: v.to_bytes(32, "big")
    msgs33 = b"".join(bytes([p]) + b32(xe) for xe in xs for p in (2, 3))
    msgs65 = b"".join(b"\x04" + b32(xe) + b32(yy) for xe in xs for yy in (y, P - y))
    h33, h65 = ora.hash160_many(msgs33, 33), ora.hash160_many(msgs65, 65)
    h160 = [h[20 * i:20 * i + 20] for h in (h33, h65) for i in range(6)]
    planted = h160 + [eth_ref.eth_address(b32(x) + b32(y))] + [b32(xe)[:20] for xe in xs]
    assert len(set(planted)) == 16
    A = khhost.Addr("\n".join(v.hex() for v in planted) + "\n", n_seq=2048, gpl=1)      # 40-hex lines: 20 raw bytes
    e = Engine(0, lanes=16384)
    e.load_giant_table(A.giant_table())
    offs, gpl = A.lane_offsets()
    e.load_lane_offsets(offs, gpl)
    bf, bits, h = A.bloom()
    e.load_addr_bloom(bf, bits, h)
    e.load_vanity([(v, v) for v in sorted(h160)])
    A.close()
    yield e, khhost.pubkey(BASE + 512)
    e.close()


@pytest.mark.parametrize("search", sorted(EXPECTED))
def test_valid_search_runs_its_kernel(world, search):
    eng, centre = world
    hits, st = eng.addr_scan(centre, 0, 2, search)
    assert st.giant_steps == 2048
    kinds = {k for j, g, t, k in hits if (j, g, t) == (0, GROUP, T)}
    print(f"search {search}: kinds at the planted point {sorted(kinds)}, {len(hits)} hits in all")
    assert kinds == EXPECTED[search]


def test_invalid_search_is_einval_and_queues_nothing(world):
    from keyhuntm1cpu_amd.khbsgs import KhbError, KHB_EINVAL
    eng, centre = world
    for search in range(-2, 128):
        if search in EXPECTED:
            continue
        with pytest.raises(KhbError) as x:
            eng.addr_scan(centre, 0, 2, search)
        assert x.value.code == KHB_EINVAL, search
    hits, st = eng.addr_scan(centre, 0, 2, 2)
    assert st.giant_steps == 2048 and {k for j, g, t, k in hits if (j, g, t) == (0, GROUP, T)} == {0, 1, 2}
