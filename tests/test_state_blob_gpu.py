"""The state blob's layout -- burst ring | counts | Kalman | offsets | raw normaliser -- is one table of sections that
nmx_state_size / _export / _import / _reset walk (kStateSections, nmx_engine_abi.inc).  tests/golden/state_blob.json holds
what the library of the commit before that change exported and returned on the MI355X for the streams of
tests/state_blob_cases.py (tests/golden/make_fir_kernel_choice.py state_blob_cases): the size and the SHA-256 of the blob
after batch 1, and the SHA-256 of batch 2's rows on a fresh engine that imported it.  The same bytes: equality, no
tolerance.  Every case also asserts that reset_state + batch 1 returns batch 1's bytes."""

import json
from pathlib import Path

import pytest

from tests import state_blob_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "state_blob.json").read_text())


@pytest.fixture(scope="module")
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.CASES)
    assert golden["offsets_only"]["state_size"] == 56   # 2 flags + 3 floats padded to 16 bytes + 3 doubles


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_blob_and_same_rows(gpu_lib, golden, monkeypatch, name):
    got = cases.run_case(gpu_lib, name, monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    assert got == golden[name]
