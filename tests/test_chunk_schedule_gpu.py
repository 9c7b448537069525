"""Streams, events and overlap modes of a chunk and of a batch are one Schedule owned by the plan (nmx_engine_sched.inc).
tests/golden/chunk_schedule.json holds, for the smallest streams that reach every branch of it (tests/chunk_schedule_cases.py),
what the commit before that change launched in stages 1 .. 7 of every batch and the SHA-256 over everything the calls
returned: tables, NaN masks, tapped windows, one process_window row and one preprocess_window
(tests/golden/make_fir_kernel_choice.py chunk_schedule_cases).  The same kernels, the same bits: equality, no tolerance.
(Which operation is ordered behind which is pinned on the CPU tier: tests/test_chunk_schedule_cpu.py.)"""

import json
from pathlib import Path

import pytest

from tests import chunk_schedule_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "chunk_schedule.json").read_text())


@pytest.fixture(scope="module")
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_kernels_and_same_bits(gpu_lib, golden, monkeypatch, name):
    got = cases.run_case(gpu_lib, name, monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    assert got == golden[name]
