"""A chunk's front end (re-reference or offset shift), the time / oscillatory kernel, coherence and the resampler are
plan-built stages with one launcher each, and "where the next stage reads its windows" is one WinView handed from stage to
stage (FrontStage, TimeOscStage, CohStage, ResampleStage: nmx_engine.inc; run_chunk, nmx_engine_run.inc).
tests/golden/prep_stage.json holds, for the smallest streams that reach every branch of that launch sequence, what the
commit before that change launched in stages 1, 2, 3 and 7 and the SHA-256 over the table, NaN mask and tapped windows of a
batch, one process_window row and one preprocess_window (tests/golden/make_fir_kernel_choice.py prep_stage_cases).  The same
kernels on the same windows: equality, no tolerance."""

import json
from pathlib import Path

import pytest

from tests import prep_stage_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "prep_stage.json").read_text())


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
