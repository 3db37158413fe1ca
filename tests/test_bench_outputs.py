"""bench.py --dump-outputs and --full: the arrays a plain run writes after its timed steps, and what a plain line
leaves to --full."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_key_limbs_and_dump_roundtrip(tmp_path):
    """A found key is a flag and eight 32-bit limbs, most significant first, every entry exact in float64; an empty
    candidate list is a (0, 3) array."""
    sys.path.insert(0, REPO)
    import bench
    key = 0x2832ED74F2B5E35EE
    rows = bench.key_limbs([None, key, (1 << 256) - 1])
    assert rows[0] == [0.0] * 9
    assert rows[1][0] == 1.0 and sum(int(v) << (32 * (7 - i)) for i, v in enumerate(rows[1][1:])) == key
    assert rows[2][1:] == [float(0xFFFFFFFF)] * 8
    bench.dump_outputs(str(tmp_path / "d"), {"found": (rows, 9), "candidates": ([], 3), "counts": ([4, 3, 2, 1], 4)})
    f = np.load(tmp_path / "d" / "found.npy")
    assert f.dtype == np.float64 and f.tolist() == rows
    assert np.load(tmp_path / "d" / "candidates.npy").shape == (0, 3)
    assert np.load(tmp_path / "d" / "counts.npy").tolist() == [[4.0, 3.0, 2.0, 1.0]]


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    """One plain run of two small timed steps: the line has no CPU baseline and no power samples, --steps sets the
    timed steps, and the dump holds the run's counts and the last step's candidates."""
    steps, chunks = 2, 512
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--chunks",
                        str(chunks), "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["config"]["chunks_per_step"] == chunks
    assert d["cpu_baseline"] is None and d["roofline"]["power"]["available"] is False
    arrays = {n[:-4]: np.load(tmp_path / "out" / n) for n in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(arrays) == ["candidates", "counts", "found"]
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["counts"].tolist() == [[steps * chunks, steps * d["config"]["giant_steps_per_step"],
                                          d["config"]["candidates"], 0]]
    assert arrays["found"].tolist() == [[0.0] * 9]
    c = arrays["candidates"]
    assert c.shape[1] == 3 and len(c) <= d["config"]["candidates"]
    assert ((c[:, 0] >= (steps - 1) * chunks) & (c[:, 0] < steps * chunks)).all() and (c[:, 1] == 0).all()
    assert c.tolist() == sorted(c.tolist())
