"""Which one-wave FIR kernel a plan launches is decided when the plan is built (NmxFirKernel, nmx_engine_plan_fir.inc).
tests/golden/fir_kernel_choice.json holds, for the smallest shapes that reach every kernel and every batch-size threshold
of the family, what the commit before that change launched in stages 1, 3 and 6 and the SHA-256 of the table it returned
(tests/golden/make_fir_kernel_choice.py).  The same kernels with the same geometry: equality, no tolerance."""

import json
from pathlib import Path

import pytest

from tests import fir_kernel_choice_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return json.loads((Path(__file__).parent / "golden" / "fir_kernel_choice.json").read_text())


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
