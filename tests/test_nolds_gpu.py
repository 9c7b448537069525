"""The nolds feature (sample entropy; features/nolds.py) on the device: the cases of tests/nolds_probe_cases.py --
exact pair counts on integer-valued series at every length where the kernel's shape changes, edge values, seeded noise
and the reference-generated fixture judged entry by entry with the oracle's conditioning report, band series through
exact and through the default taps."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import nolds_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_exact_counts(n):
    cases.check_exact_counts(None, n)


def test_edge_values():
    cases.check_edge_values(None)


def test_series_limit_is_stated():
    cases.check_limit(None)


@pytest.mark.parametrize("seed", [0, 1])
def test_noise_raw(seed):
    cases.check_noise_raw(None, seed)


@pytest.mark.parametrize("W", [200, 1000])
def test_band_index_quirk(W):
    cases.check_band_index_quirk(None, W)


def test_long_window_bands():
    cases.check_long_window_bands(None)


def test_band_default_taps():
    cases.check_band_default_taps(None)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_pipeline(tag):
    cases.check_fixture_pipeline(None, tag)


@pytest.mark.parametrize("tag", ["a", "c"])
def test_fixture_direct_and_fused(tag):
    cases.check_fixture_direct(None, tag)


def test_kernel_is_reported_and_timed():
    import numpy as np

    eng = cases.engine(None, names=[f"c{i}" for i in range(4)], W=1000, bands=["low_beta"])
    x = cases.noise(9, 4, 1000 + 100 * 15).astype(np.float32)
    eng.process_batch(x, np.arange(16) * 100)
    assert "nmx_kern_nolds_sampen" in eng.kernels(10) and "bank" in eng.kernels(10)
    assert eng.timing_ms(10) > 0.0
