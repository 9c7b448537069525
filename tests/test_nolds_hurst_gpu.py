"""nolds Hurst exponent on the device: the cases of tests/nolds_hurst_cases.py -- every entry through nmx_nolds_hurst_probe,
(R/S)_n, the kept-chunk counts and H judged against the float64 restatement on the series the kernel itself read, at every
length where the scale rule or the work split changes, on every series kind; the constructed series; the
reference-generated fixture; the sample-entropy and DFA columns bit for bit."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import nolds_hurst_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_variable(monkeypatch):
    monkeypatch.delenv("NMX_NOLDS_FIT", raising=False)


@pytest.mark.parametrize("group", list(cases.GROUPS))
@pytest.mark.parametrize("W", cases.LENGTHS)
def test_kinds(W, group):
    cases.check_kinds(None, W, group, hops=2 if W <= 100 or W > 8000 else 3)


@pytest.mark.parametrize("W", [1000, 1500])   # (from the filters' 999 taps on: the tests' float64 convolution is np.convolve(..., "same"))
def test_kinds_with_bands(W):
    cases.check_kinds(None, W, "a", hops=2, bands=["low_beta", "theta"])


def test_six_hops_three_channels():
    cases.check_kinds(None, 1000, "a", hops=6)


def test_constructed_series():
    cases.check_constructed(None)


def test_two_sample_chunks():
    cases.check_two_sample_chunks(None)


def test_amplitudes():
    cases.check_amplitudes(None)


def test_long_window_bands():
    cases.check_long_window_bands(None)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_limit_length(kind):
    cases.check_limit_length(None, kind)


def test_refusals():
    cases.check_refusals(None)


def test_other_columns_unchanged_and_batch_equals_windows():
    cases.check_other_columns_unchanged(None)


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_fixture_pipeline(tag):
    cases.check_fixture_pipeline(None, tag)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_direct_and_fused(tag):
    cases.check_fixture_direct(None, tag)


def test_kernel_is_reported_and_timed():
    from tests import nolds_dfa_cases
    from tests import nolds_probe_cases as base

    names = [f"c{i}" for i in range(4)]
    eng = cases.engine(None, names=names, W=1000, bands=["low_beta"], sampen=True, dfa=True)
    x = base.noise(9, 4, 1000 + 100 * 15).astype(np.float32)
    eng.process_batch(x, np.arange(16) * 100)
    k = eng.kernels(10)
    assert "nmx_kern_nolds_hurst" in k and "nmx_kern_nolds_dfa" in k and "nmx_kern_nolds_sampen" in k and "bank" in k
    assert eng.timing_ms(10) > 0.0
    alone = cases.engine(None, names=names, W=1000, bands=["low_beta"])
    alone.process_batch(x, np.arange(16) * 100)
    assert "nmx_kern_nolds_hurst" in alone.kernels(10) and "sampen" not in alone.kernels(10) and "dfa" not in alone.kernels(10)
    assert alone.timing_ms(10) > 0.0
    without = nolds_dfa_cases.engine(None, names=names, W=1000, bands=["low_beta"], sampen=True)
    without.process_batch(x, np.arange(16) * 100)
    assert "hurst" not in without.kernels(10) and "nmx_kern_nolds_dfa" in without.kernels(10)
