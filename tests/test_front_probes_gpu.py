"""Per-sample probes of the front end and the resampler on the MI355X (libnmx.so): the device forms the emulator never runs
-- nmx_car_tile<4> and <16>, nmx_reref_struct_tile --, the dense product on both sides of its row tile, the shift, the NaN mask,
the learned constants, and nmx_kern_resample in one-transform and polyphase form with even and odd inverse, each asserted by
name, every sample against a float64 restatement.  Cases and policy: tests/front_probe_cases.py; no miss is accepted; the
figures observed are in profiles/front_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import front_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


# ---- 1. re-reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CAR_NW4 + cases.CAR_NW16 + cases.CAR_LONG)
def test_common_average(name):
    out = cases.reref_case(None, name)
    assert set(out) - {"short"} == {"noise", "offsets", "impulse", "nosplit"} and ("short" in out) == (name in cases.CAR_LONG)
    assert set(out["nosplit"]) == {"b"} and set(out["offsets"]) == {"a", "b"}


@pytest.mark.parametrize("name", cases.STRUCT_CASES)
def test_structured_matrices(name):
    out = cases.reref_case(None, name)
    assert set(out) == {"noise", "offsets", "impulse", "nosplit"}


@pytest.mark.parametrize("name", cases.DENSE_CASES)
def test_dense_product(name):
    out = cases.reref_case(None, name)
    assert set(out) == {"noise", "offsets", "impulse", "nosplit"}


@pytest.mark.parametrize("C", [65, 129])
def test_average_of_a_window_and_of_its_stream_same_bytes(C):
    """NW = 4 over the 4600-sample range, NW = 16 over the 3100-sample range and in preprocess_window: one average, to the
    last bit."""
    cases.car_bytes_case(None, C)


@pytest.mark.parametrize("name", ["car_c13", "struct_g2"])
def test_three_chunks_store_the_bytes_of_one(name):
    cases.chunks_case(None, name)


def test_shift_in_front_of_the_notch():
    assert set(cases.shift_case(None)) == {"tap", "window"}


# ---- 2. learned constants, NaN mask ---------------------------------------------------------------------------------------
def test_learned_constants_are_the_rule_restated():
    cases.learned_case(None)


def test_nan_mask():
    cases.nanmask_case(None)


# ---- 3. resampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.RESAMPLE_CASES))
def test_resampler_through_preprocess_window(name):
    worst = cases.resample_case(None, name)
    assert {"impulse", "noise"} <= set(worst)


@pytest.mark.parametrize("with_notch", [False, True])
def test_resampler_in_a_batch_through_the_tap(with_notch):
    cases.batch_resample_case(None, with_notch)
