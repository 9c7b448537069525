"""Per-sample probes of the FIR kernels on the MI355X (libnmx.so): the channel-pair kernels of the default shapes (M = 1024 /
1536 / 2048, the fused notch + bank, the M = 4096 kernel) -- which the emulator never runs --, the one-channel forms at
their batch-size thresholds, the generic and the partitioned kernel, each asserted by name, every sample of every row
against a float64 direct convolution within four single-precision yardsticks.  Cases and policy:
tests/fir_sample_probe_cases.py; no miss is accepted; the figures observed are in profiles/fir_sample_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import fir_sample_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


# ---- band-pass bank: filter_window --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.GPU_BANK)
def test_bank_through_filter_window(name):
    worst = cases.bank_case(None, name)
    assert set(worst) == {"impulse", "noise", "constant"}


def test_bank_pair_kernel_4099_channels():
    """2050 channel pairs: chunk = 2, eight waves per workgroup, waves with two, one and no item, the last channel alone;
    an impulse at every position in either half of a pair."""
    cases.bank_case(None, "w64c_c4099", classes=("impulse", "noise"))


def test_bank_pipelined_4099_channels():
    cases.bank_case(None, "one_pp_half", classes=("impulse", "noise"))


def test_bank_pipelined_full_inverse_4096_channels():
    cases.bank_case(None, "one_pp_full", classes=("impulse", "noise"))


# ---- notch and pre-filters: preprocess_window ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.NOTCH_CASES))
def test_notch_and_pre_filters_through_preprocess_window(name):
    worst = cases.notch_case(None, name)
    assert set(worst) == {"impulse", "noise"}


# ---- the notch in batches: tap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tap_4x8", "tap_33x40", "tap_q", "tap_fused2"])
def test_notch_in_a_batch_through_the_tap(name):
    cases.tap_case(None, name)


def test_notch_persistent_form_256_channels_96_hops():
    cases.tap_case(None, "tap_qp")


def test_fused_notch_and_bank_stores_the_two_launches_window():
    """The default plan with sharp waves: the fused kernel's tapped windows against float64, and byte for byte against the
    NMX_NOTCH_SW_FUSE=0 plan's."""
    cases.tap_case(None, "tap_fused", same_as=("tap_nofuse",))


def test_a_batch_across_chunk_boundaries_stores_the_same_bytes():
    cases.tap_case(None, "tap_4x40", same_as=("tap_chunks",))
