"""The state blob's layout -- burst ring | counts | Kalman | offsets | raw normaliser -- is one table of sections that
nmx_state_size / _export / _import / _reset walk (kStateSections, nmx_engine_abi.inc).  tests/golden/state_blob_emu.json
holds what the logic emulator of the commit before that change exported and returned for the streams of
tests/state_blob_cases.py (tests/golden/make_fir_kernel_choice.py --emu state_blob_cases): the size and the SHA-256 of the
blob after batch 1, and the SHA-256 of batch 2's rows on a fresh engine that imported it.  The same bytes: equality, no
tolerance.  Every case also asserts that reset_state + batch 1 returns batch 1's bytes."""

import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import state_blob_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "state_blob_emu.json").read_text())


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.CASES)
    assert golden["offsets_only"]["state_size"] == 56   # 2 flags + 3 floats padded to 16 bytes + 3 doubles


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_blob_and_same_rows(emu_lib, golden, monkeypatch, name):
    got = cases.run_case(emu_lib, name, monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    assert got == golden[name]
