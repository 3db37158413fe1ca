"""CPU: the gate policy of resident builds (Tables::resident_gate_log2 through khh_resident_gate_log2) and the
resident options that need no GPU."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khhost

MIB, GIB = 1 << 20, 1 << 30
L1EXTS = [1 << e for e in range(15, 41)] + [2129920, (1 << 34) + (1 << 20) + 7, 3 << 29]
BUDGETS = [0, 512, 1024, MIB, 100 * MIB, GIB, 33 * GIB - 1, 32 * GIB, 150 * GIB, 288 * GIB]


def test_result_is_a_valid_gate_that_fits():
    for l1ext in L1EXTS:
        for budget in BUDGETS:
            lg = khhost.resident_gate_log2(l1ext, budget)
            assert lg == 0 or 13 <= lg <= 38
            if lg:
                assert (1 << lg) >= 4 * l1ext            # at least 4 bits per x
                assert (1 << lg) // 8 <= budget          # the gate fits the budget
                assert (1 << lg) <= max(1 << 13, 2 * (l1ext << 6) - 1)   # never more than the 64-bits-per-x size


def test_starting_rule():
    """With room to spare: the smallest power of two >= 64 bits per level-1 x, capped at 2^38."""
    assert khhost.resident_gate_log2(1 << 22, 288 * GIB) == 28         # the k = 1 gate of the host policy
    assert khhost.resident_gate_log2(2129920, 288 * GIB) == 28
    assert khhost.resident_gate_log2(1 << 26, 288 * GIB) == 32
    assert khhost.resident_gate_log2(1 << 32, 288 * GIB) == 38
    assert khhost.resident_gate_log2(1 << 34, 288 * GIB) == 38         # k = 4096: 16 bits per x
    assert khhost.resident_gate_log2(1 << 36, 288 * GIB) == 38         # 4 bits per x, the last size with a gate
    assert khhost.resident_gate_log2((1 << 36) + 1, 288 * GIB) == 0
    assert khhost.resident_gate_log2(0, 288 * GIB) == 0
    # halved while it does not fit: 2^38 bits are 32 GiB
    assert khhost.resident_gate_log2(1 << 34, 32 * GIB - 1) == 37
    assert khhost.resident_gate_log2(1 << 34, 8 * GIB) == 36
    assert khhost.resident_gate_log2(1 << 34, 8 * GIB - 1) == 0        # 2^35 bits would be 2 bits per x


def test_monotone_in_the_budget():
    for l1ext in L1EXTS:
        sizes = [khhost.resident_gate_log2(l1ext, b) for b in sorted(BUDGETS)]
        assert sizes == sorted(sizes), (l1ext, sizes)


def test_monotone_in_l1ext():
    """More entries never get a smaller gate, until none fits: from there on there is none."""
    for budget in BUDGETS:
        sizes = [khhost.resident_gate_log2(l, budget) for l in sorted(L1EXTS)]
        nz = [s for s in sizes if s]
        assert nz == sorted(nz), (budget, sizes)
        if 0 in sizes:
            assert all(s == 0 for s in sizes[sizes.index(0):]), (budget, sizes)


def test_fold_is_kept_only_while_it_filters():
    """At most 32 level-1 x per 64-bit fold block (a modelled pass fraction of 47 %): k <= 32 at the default -n."""
    gib = 288 * GIB
    for k, keeps in ((1, True), (4, True), (16, True), (32, True), (64, False), (256, False), (4096, False)):
        l1ext = k << 22
        assert khhost.resident_keeps_fold(l1ext, khhost.resident_gate_log2(l1ext, gib)) is keeps, k
    assert khhost.resident_keeps_fold(32768, 38) and khhost.resident_keeps_fold(2129920, 28)
    assert not khhost.resident_keeps_fold(1 << 22, 0)          # no gate, no fold


def test_resident_needs_a_gpu_build():
    with pytest.raises(khhost.KhhError):
        khhost.Tables("0x40000000", 1, resident=True)                       # no gpu_device
    with pytest.raises(khhost.KhhError):
        khhost.Tables("0x40000000", 1, resident=True, gpu_device=0, files_dir=".")
