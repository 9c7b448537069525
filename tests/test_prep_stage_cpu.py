"""The host code of a chunk's launch sequence -- front end, WinView, pre-processing chain, tap, the copy with the offset
added back, time / oscillatory, coherence, bank and Kalman launches (nmx_engine_run.inc) -- is the same for the device and
for the logic emulator.  tests/golden/prep_stage_emu.json holds what the emulator of the commit before those became
plan-built stages returned for the streams of tests/prep_stage_cases.py (tests/golden/make_fir_kernel_choice.py --emu
prep_stage_cases): the SHA-256 over the table, NaN mask and tapped windows of a batch, one process_window row and one
preprocess_window.  The same bytes: equality, no tolerance."""

import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import prep_stage_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "prep_stage_emu.json").read_text())


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_bits(emu_lib, golden, monkeypatch, name):
    got = cases.run_case(emu_lib, name, monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    assert got == golden[name]
