"""The gated walk's deferred gate test (walk_gated: a step's fold and gate loads are waited for behind the next
step's products) against the oracle's x: the candidates stay exactly the gate's passers at the walk's boundaries,
in diverged waves, and with every x or no x queued.

Geometry -n 0x100000000 (64 groups per chunk, work items of 8 groups), a 2^16-bit gate with 3 probes, and an
all-ones level-1 bloom, so a candidate is exactly a giant step whose x passes the gate (helpers.gate_pass).  Every
test runs without a fold, with the 4 KiB stage-1 fold, and with the 1 KiB stage-0 filter in front of that fold.
"""
from __future__ import annotations

import random

import pytest

from tests.helpers import _fold, gate_bits, gate_pass, lane_offsets

pytestmark = pytest.mark.gpu

LG, PROBES = 16, 3
STAGES = [(0, 0), (12, 0), (12, 10)]          # (stage-1 fold, stage-0 filter), log2 bytes
GPL = 4


@pytest.fixture(scope="module")
def bs32(ora):
    b = ora.Bsgs("0x100000000", 1)
    yield b
    b.close()


@pytest.fixture(scope="module")
def eng(bs32):
    from keyhuntm1cpu_amd.khbsgs import Engine
    e = Engine(0, lanes=16384)
    _, nb, bits, hashes = bs32.bloom_concat(1)
    e.load_bloom(b"\xff" * (256 * nb), nb, bits, hashes)       # every x the gate lets through is a candidate
    e.load_giant_table(bs32.giant_table())
    n_off = (bs32.cycles + GPL - 1) // GPL
    e.load_lane_offsets(lane_offsets(bs32, GPL, n_off), GPL)
    yield e
    e.close()


def _jobs(bs, ora, n, groups, seed):
    """n chunk centres and, per job, the oracle's x of its first `groups` groups as integers (index = step)."""
    centres, xs = [], []
    for c in range(n):
        st = bs.chunk_start(0x3100000000000000 + seed * (1 << 40) + c * (1 << 33), ora.pubkey(0xFEDCBA9871 + 16 * seed + c))
        centres.append(st.be64())
        _, raw, _ = bs.scan(st, 0, groups, want_x=True)
        xs.append([int.from_bytes(raw[32 * a:32 * a + 32], "big") for a in range(groups * 1024)])
    return b"".join(centres), xs


def _scan(eng, gate, centres, n_jobs, groups, stage1, stage0):
    """The sorted candidate steps per job, and the launch's stats, of one scan behind `gate` with the given stages."""
    try:
        eng.set_gate_stage1(stage1)
        eng.set_gate_stage0(stage0)
        eng.load_gate(gate, LG, PROBES)
        assert eng.gate_stages() == 4 | (2 if stage1 else 0) | (1 if stage0 else 0)
        got, degen, st = eng.scan(centres, 0, groups)
    finally:
        eng.set_gate_stage1(1)                 # KHB_GATE_STAGE1_AUTO, the library default
        eng.set_gate_stage0(0)                 # the library default: no stage 0
        eng.load_gate(None)
    assert not degen
    assert st.n_cand == len(got) < eng.candidate_capacity()
    assert st.giant_steps == n_jobs * groups * 1024
    per_job = [[] for _ in range(n_jobs)]
    for job, a in got:
        per_job[job].append(a)
    return [sorted(x) for x in per_job], st


@pytest.fixture(scope="module")
def boundary_case(bs32, ora):
    """Two whole chunks and a gate that holds only the bits of the x at the walk's boundaries: the peeled step (index
    0), the last pair (1, 1023), the step-0 pair (511, 513), the centre (512) and the pair next to the peeled step
    (1022), in the first and last group and on both sides of a work-item boundary (groups 7 and 8)."""
    centres, xs = _jobs(bs32, ora, 2, bs32.cycles, 1)
    planted = [[1024 * g + t for g in (0, 7, 8, 63) for t in (0, 1, 511, 512, 513, 1022, 1023)] for _ in xs]
    gate = bytearray((1 << LG) // 8)
    for job, steps in enumerate(planted):
        for a in steps:
            for b in gate_bits(LG, PROBES, xs[job][a]):
                gate[b >> 3] |= 1 << (b & 7)
    gate = bytes(gate)
    ref = [[a for a, x in enumerate(job_xs) if gate_pass(gate, LG, PROBES, x)] for job_xs in xs]
    return centres, gate, planted, ref


@pytest.mark.parametrize("stage1,stage0", STAGES)
def test_boundaries(eng, bs32, boundary_case, stage1, stage0):
    centres, gate, planted, ref = boundary_case
    per_job, _ = _scan(eng, gate, centres, 2, bs32.cycles, stage1, stage0)
    for job in range(2):
        assert set(planted[job]) <= set(ref[job])
        missing = sorted(set(planted[job]) - set(per_job[job]))
        assert not missing, (job, missing)
    assert per_job == ref


@pytest.fixture(scope="module")
def ragged_case(bs32, ora):
    """Nine jobs of 62 groups (72 work items: the launch ends mid-wave, and each job's last item is two groups short)
    and a random gate with each bit set with p = 0.27: about 2 % of x pass it and about 10 % its 4 KiB fold."""
    groups = 62
    centres, xs = _jobs(bs32, ora, 9, groups, 2)
    rng = random.Random(11)
    gate = bytes(sum(1 << k for k in range(8) if rng.random() < 0.27) for _ in range((1 << LG) // 8))
    fold = _fold(gate, 12)
    ref, fold_only = [], 0
    for job_xs in xs:
        r = []
        for a, x in enumerate(job_xs):
            if gate_pass(fold, LG - 1, PROBES, x):
                if gate_pass(gate, LG, PROBES, x):
                    r.append(a)
                else:
                    fold_only += 1
            else:
                assert not gate_pass(gate, LG, PROBES, x)      # the fold is a superset of the gate
        ref.append(r)
    return centres, gate, groups, ref, fold_only / (9 * groups * 1024)


@pytest.mark.parametrize("stage1,stage0", STAGES)
def test_ragged_lanes(eng, ragged_case, stage1, stage0):
    centres, gate, groups, ref, fold_only = ragged_case
    assert 0 < sum(map(len, ref)) < eng.candidate_capacity()
    assert fold_only >= 0.05                   # x whose gate block is loaded and then fails: the deferred path
    per_job, _ = _scan(eng, gate, centres, 9, groups, stage1, stage0)
    assert per_job == ref


@pytest.fixture(scope="module")
def one_item(bs32, ora):
    return _jobs(bs32, ora, 1, 8, 3)[0]


@pytest.mark.parametrize("stage1,stage0", STAGES)
def test_dense_and_empty(eng, one_item, stage1, stage0):
    """One work item.  An all-ones gate queues both x of every step, with a drain between pending finishes; an
    all-zero gate queues nothing and the walk still completes (giant_steps, checked by _scan)."""
    per_job, _ = _scan(eng, b"\xff" * ((1 << LG) // 8), one_item, 1, 8, stage1, stage0)
    assert per_job == [list(range(8 * 1024))]
    per_job, _ = _scan(eng, bytes((1 << LG) // 8), one_item, 1, 8, stage1, stage0)
    assert per_job == [[]]
