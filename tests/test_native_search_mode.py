"""device/scan_modes.hpp compiled for the CPU (tests/native/test_search_mode.cpp) as a stand-alone program built with
the address and undefined-behaviour sanitizers and run directly: the decoder of khb_addr_submit's `search` value over
[-2, 128) against the 15 valid values and their kernel modes written out here, and every mode predicate against a
table written out from the definitions the traits table replaced, so a row that drifts is caught without a GPU."""
from __future__ import annotations

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

BTC, ETH, XPOINT = 0, 1, 2
# search: (family, forms, endo, vanity, kernel mode of k_giant_scan)
VALID = {
    0: (BTC, 0, 0, 0, 2), 1: (BTC, 1, 0, 0, 3), 2: (BTC, 2, 0, 0, 4),
    4: (BTC, 0, 1, 0, 10), 5: (BTC, 1, 1, 0, 11), 6: (BTC, 2, 1, 0, 12),
    8: (ETH, 0, 0, 0, 13),
    16: (XPOINT, 0, 0, 0, 14), 20: (XPOINT, 0, 1, 0, 15),
    32: (BTC, 0, 0, 1, 16), 33: (BTC, 1, 0, 1, 17), 34: (BTC, 2, 0, 1, 18),
    36: (BTC, 0, 1, 1, 19), 37: (BTC, 1, 1, 1, 20), 38: (BTC, 2, 1, 1, 21),
}

# the occupancy macro of scan_args.hpp a mode is compiled for, in the order of scan_modes.hpp's Occupancy
SCAN, ADDR, ADDR_E, ADDR_ETH, ADDR_X, VANITY = range(6)
# mode: is_gated, gate_stages, is_scan, is_vanity, is_endo, is_xpoint, is_addr, addr_compressed, addr_uncompressed,
#       needs_y, is_dump, is_batched, is_xy, occupancy
PREDICATES = {
    0: (0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, SCAN),          # kScan
    1: (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, SCAN),          # kDump
    2: (0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 1, ADDR),          # kAddrU
    3: (0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, ADDR),          # kAddrC
    4: (0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, ADDR),          # kAddrB
    5: (0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, ADDR),          # kAddrDump
    6: (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, SCAN),          # kBaby
    7: (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, SCAN),          # kScanG
    8: (1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, SCAN),          # kScanG1
    9: (1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, SCAN),          # kScanG2
    10: (0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, ADDR_E),       # kAddrUE
    11: (0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, ADDR_E),       # kAddrCE
    12: (0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, ADDR_E),       # kAddrBE
    13: (0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, ADDR_ETH),     # kAddrEth
    14: (0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, ADDR_X),       # kAddrX
    15: (0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, ADDR_X),       # kAddrXE (is_endo is the BTC -e)
    16: (0, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, VANITY),       # kVanU
    17: (0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, VANITY),       # kVanC
    18: (0, 0, 0, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, VANITY),       # kVanB
    19: (0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, VANITY),       # kVanUE
    20: (0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1, VANITY),       # kVanCE
    21: (0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, VANITY),       # kVanBE
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native_search_mode") / "test_search_mode")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "native", "test_search_mode.cpp"), "-o", out],
                   check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l.split() for l in r.stdout.splitlines()]


def test_search_values(lines):
    got = {int(l[1]): l[2:] for l in lines if l[0] == "s"}
    assert sorted(got) == list(range(-2, 128))
    assert [VALID[s][4] for s in sorted(VALID)] == [2, 3, 4, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]
    for s in range(-2, 128):
        if s in VALID:
            assert tuple(int(v) for v in got[s]) == VALID[s] + (s,), s    # the fields, the mode, and the round trip
        else:
            assert got[s] == ["invalid"], s


def test_mode_predicates(lines):
    got = {int(l[1]): tuple(int(v) for v in l[2:]) for l in lines if l[0] == "m"}
    assert got == PREDICATES
