"""Sharp waves on windows beyond 14 500 samples in the single-thread emulator (tests/emu/nmx_emu.cpp): the plan's
long-window mode and nmx_sharp_body on the whole list carve in host memory, against the reference-generated fixture
(tests/golden/make_golden_sharpwave_long.py) and the float64 restatement.  Cases and policy: tests/sharpwave_long_cases.py.
At the parent commit every positive case fails at plan construction ("window too long for the sharp-wave kernel")."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import sharpwave_long_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("tag", ["d30k", "d16k", "wide30k", "all30k"])
def test_emulator_long_window_case(emu_lib, tag):
    acc = cases.run_case(emu_lib, tag)
    assert set(acc) <= {"sharpwave"}, acc
    assert acc.get("sharpwave", 0) <= 2, acc   # (seeds chosen for 0 - 2 here: profiles/sharpwave_long.md)


def test_window_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_fixture_taps_are_the_engine_s_design():
    """The FIRs the reference used (stored halves) against the engine's own design of the same ranges."""
    from py_neuromodulation_amd import fir_design

    for tag in ("d30k", "d16k", "wide30k"):
        g, p, s, ch, cols, _ = cases.load_case(tag)
        want = cases.fixture_taps(g, tag)
        ranges = s.sharpwave_analysis_settings.filter_ranges_hz
        assert len(ranges) == len(want)
        for fr, b in zip(ranges, want):
            a = fir_design.band_pass(float(p["sfreq"]), fr[0], fr[1])
            np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=0, atol=1e-12)


def test_notch_in_front_of_long_window_sharp_waves(emu_lib):
    assert cases.notch_case(emu_lib) <= 2


@pytest.mark.parametrize("tag,kind,wide", [("default", "walk", False), ("wide", "white", True)])
def test_window_of_14000_samples_computes_what_it_did(emu_lib, tag, kind, wide):
    """A 14 000-sample window (below the long-window mode: the LDS list layout, dense and list paths) gives the rows the
    emulator gave at the commit before the long-window mode (tests/golden/sharpwave_14k_parent.npz, recorded there
    with this very recording and settings).  Bit-identical where recorded; 1e-6 relative leaves room for another
    compiler's libm.  That such plans take the launches they took before is checked on the device
    (test_sharpwave_long_gpu.py::test_kernels_per_mode)."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.stream import Stream
    from tests.helpers import load_golden

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.sharpwave_analysis = True
    if wide:
        s.sharpwave_analysis_settings.filter_ranges_hz = [[5, 5000]]
    x = cases.recording(14, 14000, kind, hops=2)
    df = Stream(14000.0, data=x, settings=s, line_noise=50, lib=emu_lib).run(x, save_csv=False)
    g = load_golden("sharpwave_14k_parent")
    assert list(df.columns) == [str(c) for c in g[f"{tag}_columns"]]
    np.testing.assert_allclose(df.to_numpy(np.float64), g[f"{tag}_values"], rtol=1e-6, atol=0)
