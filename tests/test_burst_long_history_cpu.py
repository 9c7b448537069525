"""Burst threshold histories beyond 65 536 top-K entries in the single-thread emulator (tests/emu/nmx_emu.cpp): the TILED
flavour of nmx_burst_thr_item -- nmx_merge_into_tiled with tiles of 8 entries, in the fill regime, under the fringe / pending
scheme of a full ring (h2k, h1k) and on every hop (h4k: 400 samples per hop) -- behind the sort-once fill, against the
reference-generated fixture (tests/golden/make_golden_burst_long_history.py) and the float64 restatement.  Cases and policy:
tests/burst_long_history_cases.py.  The emulator tier accepts no miss.  At the parent commit every positive case fails at
plan construction ("burst top-K list too long for the merge kernel")."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import burst_long_history_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("tag", list(cases.CASES))
def test_emulator_long_history_case(emu_lib, tag):
    assert cases.run_case(emu_lib, tag) == {}


def test_emulator_batching_gives_same_bytes(emu_lib):
    cases.batching_gives_same_bytes(emu_lib)


def test_emulator_state_travels(emu_lib):
    cases.state_travels(emu_lib)


def test_emulator_history_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_emulator_history_at_the_limit_builds(emu_lib):
    cases.at_limit_builds(emu_lib)
