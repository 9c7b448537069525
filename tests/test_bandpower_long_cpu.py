"""`bandpass_filter` on windows above 16 384 samples in the single-thread emulator (tests/emu/nmx_emu.cpp): the partitioned
bank's item with the band-pass power epilogue from differenced taps (nmx_bank_ups_power, reached from nmx_bank_item), against
the reference-generated fixture (tests/golden/make_golden_bandpower_long.py) and the float64 restatement.  Cases and policy:
tests/bandpower_long_cases.py.  At the parent commit every positive case fails at plan construction (the variable is unknown
there and a 16 385-sample plan with bandpass_filter is refused)."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import bandpower_long_cases as cases  # noqa: E402


@pytest.fixture(autouse=True)
def _long_windows(monkeypatch):
    """Band-pass power (and bursts: defaults30k) above 16 384 samples are opt-in: every plan of this file is built
    with both variables on."""
    monkeypatch.setenv("NMX_LONG_BANDPOWER", "1")
    monkeypatch.setenv("NMX_LONG_BURSTS", "1")


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


_ROWS = {}


def _rows(lib, tag):
    if tag not in _ROWS:
        _ROWS[tag] = cases.run_case(lib, tag)
    return _ROWS[tag]


@pytest.mark.parametrize("tag", cases.TABLE_CASES)
def test_oracle_s_log_activities_stay_away_from_zero(tag):
    m = cases.log_margin(tag)
    print(f"{tag}: min |log10 activity| = {m:.3g}")
    assert m >= cases.LOG_MARGIN, (tag, m)


@pytest.mark.parametrize("tag", cases.TABLE_CASES)
def test_emulator_long_window_case(emu_lib, tag):
    _rows(emu_lib, tag)


def test_fixture_taps_are_the_engine_s_design():
    from py_neuromodulation_amd import fir_design

    g, p, s, _, _, _ = cases.load_case(cases.TAPS_OF[0])
    for band, b in zip(cases.TAPS_OF[1], cases.fixture_taps(g)):
        fr = s.frequency_ranges_hz[band]
        a = fir_design.band_pass_bank([(fr[0], fr[1])], float(p["sfreq"]))[0]
        np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=0, atol=1e-12)


def test_complexity_does_not_cancel_at_20_khz(emu_lib):
    """The 20 kHz white-noise plan (sigma 50, default bands, 4 hops x 2 channels): every complexity entry within 1e-5 relative
    of the float64 oracle.  Measured in the emulator: the second difference of the stored fp32 band series (the epilogue below
    the gate, tried on this plan) is 1.06e-4 off (low_beta; 78 % of the entries beyond 1e-5), mobility 2.5e-6; with the
    differenced taps complexity is 3.6e-6 off at worst and mobility 2.2e-6."""
    worst, share = cases.cancellation_case(emu_lib)
    assert worst["complexity"] <= 1e-5 and share["complexity"] == 0, (worst, share)
    assert worst["mobility"] <= 1e-5, worst


@pytest.mark.parametrize("feats", [("activity", "mobility", "complexity"), ("activity", "mobility"), ("complexity",), ("activity",)])
def test_identity_taps_pin_the_shifts_and_the_tails(emu_lib, feats):
    """(Entries whose sums the emulator's single accumulator cannot hold are left to the device tier: identity_probe.)"""
    assert cases.identity_probe(emu_lib, feats) >= 2 * 3 * 3 * len(feats)


def test_special_rows(emu_lib):
    """(The constant channel's theta entries -- a smooth 20 000-sample transient in the emulator's single accumulator -- are
    left to the device tier: special_rows.)"""
    assert cases.special_rows(emu_lib) <= 3


def test_offsets_of_1000_through_the_offset_split(emu_lib):
    """(One `bandpass` entry at 1.08 of the tolerance is accepted on its conditioning report here; the device tier accepts
    none.)"""
    acc = cases.offsets_case(emu_lib)
    assert set(acc) <= {"bandpass"} and acc.get("bandpass", 0) <= 1, acc


def test_process_window_by_window_equals_run(emu_lib):
    cases.process_equals_run(emu_lib, _rows(emu_lib, "w20k"))


def test_dropin_bandpower_equals_the_row(emu_lib):
    cases.dropin_equals_row(emu_lib, _rows(emu_lib, "w20k_nolog"))


def test_ragged_pair_of_long_lengths_carries_the_kalman_state(emu_lib):
    assert cases.ragged_pair(emu_lib) == [20000, 20001]


@pytest.mark.parametrize("bursts", [False, True])
def test_gate_is_closed_without_the_opt_in(emu_lib, monkeypatch, bursts):
    if not bursts:
        monkeypatch.delenv("NMX_LONG_BURSTS")
    cases.gate_is_closed_without_the_opt_in(emu_lib, monkeypatch.delenv)


def test_filter_window_of_a_long_plan(emu_lib):
    cases.filter_window_series(emu_lib)


@pytest.mark.parametrize("bursts", [False, True])
def test_limited_features_raise_above_16384(emu_lib, monkeypatch, bursts):
    if not bursts:
        monkeypatch.delenv("NMX_LONG_BURSTS")
    cases.limited_features_raise(emu_lib)


def test_window_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_nothing_below_the_gate_moved(emu_lib, monkeypatch):
    """An 8 kHz / 8000-sample plan: the same kernels and bytes with the variable set and unset, and the emulator's rows recorded
    at the parent commit (tests/golden/bandpower_8k_parent.npz)."""
    from tests.helpers import load_golden

    rows, _ = cases.below_the_gate(emu_lib, monkeypatch.setenv, monkeypatch.delenv)
    want = load_golden("bandpower_8k_parent")["rows"]
    assert rows.dtype == want.dtype and rows.shape == want.shape and rows.tobytes() == want.tobytes()
