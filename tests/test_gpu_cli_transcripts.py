"""keyhunt_amd and bsgsd_amd on the GPU print what they printed before the front end was refactored: the small
searches of tests/cli_cases.py, byte for byte against tests/golden/cli/gpu.json (every set was recorded twice and both
recordings agreed), and the -S table files against the recorded digests."""
from __future__ import annotations

import json
import os

import pytest

from keyhuntm1cpu_amd import BIN_DIR
from tests import cli_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(cli_cases.GOLD_CLI, "gpu.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert set(recorded) == set(cli_cases.GPU_CASES) | {"bsgsd_startup"}


@pytest.mark.parametrize("name", sorted(cli_cases.GPU_CASES))
def test_gpu_cli_transcript(name, recorded, tmp_path):
    got = cli_cases.run_gpu_case(BIN_DIR, name, str(tmp_path))
    assert got["runs"] == recorded[name]["runs"]
    assert got["tables"] == recorded[name]["tables"]
    if name == "bsgs30_S":
        assert len(got["tables"]) == 4 and "Writing" in got["runs"][0]["stdout"] and "Reading" in got["runs"][1]["stdout"]


def test_bsgsd_startup_transcript(recorded, tmp_path):
    assert cli_cases.run_bsgsd_startup(BIN_DIR, str(tmp_path)) == recorded["bsgsd_startup"]
