"""Which kernels the bursts chain and the sharp-wave stage launch -- the threshold walk's schedule included -- is decided
when the plan is built (BurstStage, SharpStage: nmx_engine_plan_bursts.inc, nmx_engine_plan_state.inc).
tests/golden/burst_kernel_choice.json holds, for the smallest streams that reach every branch of those choices, what the
commit before that change launched in stages 4 and 5 after every batch and the SHA-256 of the table each batch returned
(tests/golden/make_fir_kernel_choice.py burst_kernel_choice_cases).  The same kernels on the same hops with the same
geometry: equality, no tolerance."""

import json
from pathlib import Path

import pytest

from tests import burst_kernel_choice_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "burst_kernel_choice.json").read_text())


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
