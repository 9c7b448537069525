"""Time-domain, FFT and Welch features on windows up to 40 000 samples on the MI355X (libnmx.so): the persistent
long-window kernel nmx_kern_timeosc_long (nmx_timeosc_long.hip), against the reference-generated fixture
(tests/golden/make_golden_timeosc_long.py) and the float64 restatement.  Cases and policy: tests/timeosc_long_cases.py.
All cases together may accept no miss in hjorth / raw / linelength and at most 2 in fft + welch, each on a conditioning
report (the device's fast log10 / sqrt against the emulator's libm); the counts observed are in profiles/timeosc_long.md.
At the parent commit every positive case fails at plan construction."""

import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import timeosc_long_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

_ACCEPTED = {"spectral": 0}
_ROWS = {}


def _book(acc):
    assert set(acc) <= {"fft", "welch"}, acc
    _ACCEPTED["spectral"] += acc.get("fft", 0) + acc.get("welch", 0)
    assert _ACCEPTED["spectral"] <= 2, f"fft + welch misses accepted by the long-window cases so far: {_ACCEPTED}"


@pytest.mark.parametrize("tag", cases.FIXTURE_TAGS)
def test_long_window_case(tag):
    acc, rows = cases.run_case(None, tag, want_rows=True)
    _ROWS[tag] = rows
    _book(acc)


def test_16k_behind_the_notch():
    _book(cases.n16k_case(None))


def test_nan_channel():
    _book(cases.nan30k_case(None))


def test_process_equals_run():
    rows = _ROWS["d30k"] if "d30k" in _ROWS else cases.run_case(None, "d30k", want_rows=True)[1]
    cases.process_equals_run(None, rows)


def _engine(W, features, wide=False):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    s = NMSettings.get_default()
    s.reset()
    for o in (s.fft_settings, s.welch_settings):
        o.features.mean = o.features.median = o.features.std = o.features.max = True
    if wide:
        s.frequency_ranges_hz["broad"] = [4, 9000]
    return HotPathEngine(s, ["a", "b"], float(W), features=features, window=W)


def _batch(e, W, hops=5, seed=5):
    x = cases.recording(seed, W, "walk", hops=hops)
    return e.process_batch(x, np.arange(hops, dtype=np.int64) * (W // 10)).copy()


@pytest.mark.parametrize("W,wide", [(30000, False), (20000, True), (20001, True)])
def test_persistent_loop_reuses_lds_and_slab(W, wide):
    """NMX_TIMEOSC_LONG_BLOCKS=3 (read when the plan is built): ten items on three workgroups, each reusing its LDS --
    and, with the wide band, its slab of device memory -- for three or four items; bit-identical to the uncapped run.
    20 001: three subsequences of 6667 samples, an odd length (the full complex transform of each)."""
    feats = ["raw_hjorth", "return_raw", "linelength", "fft", "welch"]
    e = _engine(W, feats, wide)
    want = _batch(e, W)
    assert "nmx_kern_timeosc_long" in e.kernels(2)
    e.close()
    os.environ["NMX_TIMEOSC_LONG_BLOCKS"] = "3"
    try:
        e = _engine(W, feats, wide)
    finally:
        del os.environ["NMX_TIMEOSC_LONG_BLOCKS"]
    got = _batch(e, W)
    e.close()
    assert np.isfinite(want).all()
    np.testing.assert_array_equal(got, want)


def test_kernels_per_mode():
    """A plan whose generic layout fits launches what it launched before; the headline plan launches the long-window
    kernel and, for its sharp waves, the slab kernel."""
    e = _engine(13000, ["fft"])
    _batch(e, 13000)
    k = e.kernels(2)
    e.close()
    assert "nmx_kern_timeosc" in k and "long" not in k, k
    e = _engine(30000, ["raw_hjorth", "return_raw", "linelength", "fft", "welch", "sharpwave_analysis"])
    _batch(e, 30000)
    k2, k5 = e.kernels(2), e.kernels(5)
    e.close()
    assert "nmx_kern_timeosc_long" in k2, k2
    assert "nmx_kern_sharp_slab" in k5, k5


def test_window_above_the_limit_raises():
    cases.over_limit_raises(None)


def test_short_only_features_raise_above_16384():
    cases.short_only_features_raise(None)


def test_return_spectrum_raises():
    cases.return_spectrum_raises(None)


def test_refused_transform_length_raises():
    cases.refused_length_raises(None)
