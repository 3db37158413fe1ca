"""keyhunt_amd and bsgsd_amd print what they printed before the front end was refactored: stdout, stderr, exit status
and KEYFOUNDKEYFOUND.txt of argument sets that end before any device is opened (tests/cli_cases.py), byte for byte
against the recordings in tests/golden/cli/cpu.json."""
from __future__ import annotations

import json
import os

import pytest

from keyhuntm1cpu_amd import BIN_DIR
from tests import cli_cases


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(cli_cases.GOLD_CLI, "cpu.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(cli_cases.CPU_CASES)


@pytest.mark.parametrize("name", sorted(cli_cases.CPU_CASES))
def test_cli_transcript(name, recorded, tmp_path):
    got = cli_cases.run_cpu_case(BIN_DIR, name, str(tmp_path))
    assert got == recorded[name]
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(list(cli_cases.FILES) + cli_cases.COPIES)
