"""The resampler's fixed padding mode (``resample_npad`` = n samples per side) on the MI355X: the cases of
tests/resample_npad_cases.py on libnmx.so -- nmx_kern_resample_npad in its one-transform form (even and odd padded
lengths, prime radices) and its long polyphase form (any q that divides n_pad, odd q included), the batch through the
tap, the stand-alone float64 Resampler with Bluestein's chirp convolution on the forward side, and the refusals.  Policy
and limits: the case module; the emulator tier with the ties of the references: test_resample_npad_cpu.py."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import resample_npad_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixed_pad_through_preprocess_window(name):
    worst = cases.run_case(None, name)
    assert {"impulse", "noise"} <= set(worst) and ("tone" in worst) == (cases.case_plan(name)["nyq_bin"] >= 0)


def test_both_modes_meet_the_same_series_at_the_shared_lengths():
    assert set(cases.both_modes_case(None)) == {"auto", 100}


@pytest.mark.parametrize("with_notch", [False, True])
def test_fixed_pad_in_a_batch_through_the_tap(with_notch):
    cases.batch_case(None, with_notch)


def test_required_windows_build():
    for W in cases.REQUIRED_WINDOWS:
        eng = cases.engine(None, {}, float(W), 1000.0, W, 2, 100)
        try:
            assert (eng.W_in, eng.W, eng.desc.resample_npad_mode, eng.desc.resample_npad) == (W, 1000, 1, 100), W
        finally:
            eng.close()


def test_refusals():
    with pytest.raises(ValueError, match=r"exceeds the padded limit of 65 536"):
        cases.engine(None, {}, 65336.0, 1000.0, 65336, 1, 101)
    with pytest.raises(ValueError, match=r"no polyphase split of the padded window \(raw window 15 818, n_pad 16 018, n_new 1 013\)"):
        cases.engine(None, {}, 15818.0, 1000.0, 15818, 1, 100)
    with pytest.raises(ValueError, match="resample_npad must be 'auto' or an int >= 0"):
        cases.engine(None, {}, 2000.0, 1000.0, 2000, 1, -1)


@pytest.mark.parametrize("fs,to,T,npad", cases.F64_SHAPES)
def test_standalone_float64(fs, to, T, npad):
    assert cases.standalone_case(None, fs, to, T, npad) <= 1.0


def test_standalone_auto_entry_forwards():
    from oracle import mne_restated
    from py_neuromodulation_amd._lib import get_library

    x = np.random.default_rng(5).standard_normal((2, 1375)) * 10 + 100
    want = mne_restated.resample(x, up=1000 / 1375, down=1.0)
    a, b = np.empty_like(want), np.empty_like(want)
    L, n = get_library(), want.shape[1]
    L.check(L.lib.nmx_resample_f64(0, x.ctypes.data, 1375, 2, 1375, 1000 / 1375, a.ctypes.data, n, n))
    L.check(L.lib.nmx_resample_f64_npad(0, x.ctypes.data, 1375, 2, 1375, 1000 / 1375, b.ctypes.data, n, n, -1))
    assert np.array_equal(a, b) and np.abs(a - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("tag", cases.STREAM_TAGS)
def test_stream_against_the_references_tables(tag):
    cases.stream_case(None, tag)
