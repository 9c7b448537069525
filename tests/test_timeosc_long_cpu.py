"""Time-domain, FFT and Welch features on windows up to 40 000 samples in the single-thread emulator
(tests/emu/nmx_emu.cpp): the plan's long-window mode and nmx_time_osc_long_item (reached from nmx_time_osc_item, on slab
0), against the reference-generated fixture (tests/golden/make_golden_timeosc_long.py) and the float64 restatement.  Cases
and policy: tests/timeosc_long_cases.py.  The emulator tier accepts no miss in any family.  At the parent commit every
positive case fails at plan construction."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import timeosc_long_cases as cases  # noqa: E402

_ROWS = {}


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("tag", cases.FIXTURE_TAGS)
def test_emulator_long_window_case(emu_lib, tag):
    acc, rows = cases.run_case(emu_lib, tag, want_rows=True)
    _ROWS[tag] = rows
    assert acc == {}, acc


def test_emulator_16k_behind_the_notch(emu_lib):
    assert cases.n16k_case(emu_lib) == {}


def test_emulator_nan_channel(emu_lib):
    assert cases.nan30k_case(emu_lib) == {}


def test_emulator_process_equals_run(emu_lib):
    rows = _ROWS["d30k"] if "d30k" in _ROWS else cases.run_case(emu_lib, "d30k", want_rows=True)[1]
    cases.process_equals_run(emu_lib, rows)


def test_window_of_13000_samples_computes_what_it_did(emu_lib):
    """A 13 000-sample plan (the generic kernel's layout fits) gives the rows the emulator gave at the parent commit
    (tests/golden/timeosc_13k_parent.npz, recorded there with this recording and these settings).  Bit-identical where
    recorded; 1e-6 relative leaves room for another compiler's libm.  That such a plan launches what it launched before
    is checked on the device (test_timeosc_long_gpu.py::test_kernels_per_mode)."""
    from tests.helpers import load_golden

    df = cases.rows_13k(emu_lib)
    g = load_golden("timeosc_13k_parent")
    assert list(df.columns) == [str(c) for c in g["columns"]]
    np.testing.assert_allclose(df.to_numpy(np.float64), g["values"], rtol=1e-6, atol=0)


def test_window_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_short_only_features_raise_above_16384(emu_lib):
    cases.short_only_features_raise(emu_lib)


def test_return_spectrum_raises(emu_lib):
    cases.return_spectrum_raises(emu_lib)


def test_refused_transform_length_raises(emu_lib):
    cases.refused_length_raises(emu_lib)
