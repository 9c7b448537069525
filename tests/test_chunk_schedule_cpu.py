"""The schedule of a chunk and of a batch -- which stream a launch goes to, which events say a chunk is complete, when a
host input buffer may be overwritten (Schedule, nmx_engine_sched.inc) -- is host code, the same for the device and for the
logic emulator.  tests/golden/chunk_schedule_emu.json holds what the emulator of the commit before the schedule became one
type recorded for the streams of tests/chunk_schedule_cases.py (tests/golden/make_fir_kernel_choice.py --emu
chunk_schedule_cases): the work operations in issue order, one SHA-256 over the set of work operations each of them is
ordered behind (reduced from the emulator's trace of streams, events and syncs), and the SHA-256 over everything the calls
returned.  The same operations behind the same dependencies, the same bytes: equality, no tolerance."""

import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import chunk_schedule_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "chunk_schedule_emu.json").read_text())


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.CASES)


def test_the_reduction_sees_a_lost_wait_and_a_lost_sync():
    """two streams, one event: stream 2's launch is ordered behind stream 1's only through the wait, the host's second copy
    behind both only through the sync"""
    full = "op a 1\nrecord 1 7\nwait 2 7\nop b 2\nsync 2\nop c 3\n"
    ops, deps = cases.reduce_trace(full)
    assert ops == ["a", "b", "c"]
    for lost in ("wait 2 7\n", "sync 2\n", "record 1 7\n"):
        assert cases.reduce_trace(full.replace(lost, "")) != (ops, deps), lost
    # identities do not matter, and a wait on an event never recorded contributes nothing
    assert cases.reduce_trace("op a 5\nrecord 5 1\nwait 9 1\nwait 9 4\nop b 9\nsync 9\nop c 0\n") == (ops, deps)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_schedule_and_same_bits(emu_lib, golden, monkeypatch, name):
    got = cases.run_case(emu_lib, name, monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    assert got["ops"] == golden[name]["ops"]
    assert got == golden[name]
