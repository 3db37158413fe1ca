"""CPU: the product's host check (khhost.Tables.secondcheck, the CHECK_HOST path) on the directed cases of
tests/check_cases.py, against the oracle's bsgs_secondcheck: classes Z (dx == 0 inside a batch), K (degenerate
bases), C (carries through several limbs, the geometry's constants) and R (the random families)."""
from __future__ import annotations

import pytest

from keyhuntm1cpu_amd import khhost
from tests import check_cases as cc


@pytest.fixture(scope="module")
def pair(ora):
    h = khhost.Tables(cc.N_GEOM, 1, threads=8)
    o = ora.Bsgs(cc.N_GEOM, 1)
    yield h, o
    h.close()
    o.close()


@pytest.mark.parametrize("cls", ["Z", "K", "C", "R"])
def test_host_check_on_directed_cases(ora, pair, cls):
    h, o = pair
    cases = {"Z": lambda: cc.z2_cases(ora, o) + cc.z3_cases(ora, o), "K": lambda: cc.k_cases(ora, o),
             "C": lambda: cc.c_cases(ora, o) + [cc.wrap_case(ora, o)], "R": lambda: cc.r_cases(ora, o)}[cls]()
    n_found = 0
    for c in cases:
        ref = o.secondcheck(c.start, c.a, c.target)
        assert h.secondcheck(c.start, c.a, c.target.be64()) == ref, c.name
        n_found += ref is not None
    if cls == "R":
        assert n_found >= 48           # of 48 planted (a few past the window's end) and 16 special
    else:
        assert n_found == {"Z": 0, "K": 0, "C": 18}[cls]
