"""STFT and coherence on windows above 16 384 samples in the single-thread emulator (tests/emu/nmx_emu.cpp): the STFT phase
of the long-window item (nmx_k_timeosc_long.h; its per-wave class is the device's, the emulator runs 500-sample segments
through the one-transform class) and nmx_coh_item on the long plan's window view, against the reference-generated fixture
(tests/golden/make_golden_stft_coh_long.py) and the float64 restatements.  Cases, policy and caps:
tests/stft_coh_long_cases.py.  At the parent commit every positive case fails with ValueError at plan construction (the
variables are unknown there and a 16 385-sample plan with stft or coherence is refused)."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import stft_coh_long_cases as cases  # noqa: E402


@pytest.fixture(autouse=True)
def _long_windows(monkeypatch):
    """STFT and coherence above 16 384 samples are opt-in: every plan of this file is built with both variables
    on, unless the test takes them away."""
    monkeypatch.setenv("NMX_LONG_STFT", "1")
    monkeypatch.setenv("NMX_LONG_COHERENCE", "1")


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


# ---- STFT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", cases.STFT_TAGS)
def test_emulator_long_stft_case(emu_lib, tag):
    acc, _ = _rows(emu_lib, tag)
    assert set(acc) <= {"stft"}, acc   # (the emulator tier accepts no fft / welch miss: test_timeosc_long_cpu.py)


@pytest.mark.parametrize("tag", cases.STFT_TAGS)
def test_oracle_s_own_count_of_ill_conditioned_stft_entries(tag):
    ill, entries = cases.stft_ill_conditioned(tag)
    print(f"{tag}: {ill} of {entries} stft entries hold a bin below FP32_BIN_EPS of the segment level")
    assert ill <= int(cases.STFT_CAP * entries), (tag, ill, entries)


def test_nan_samples_in_one_channel(emu_lib):
    acc, ch1, idx, _ = cases.nan_case(emu_lib)
    assert acc == {}, acc
    np.testing.assert_array_equal(ch1, _rows(emu_lib, "s30k")[1][:, idx])


def test_behind_notch_and_re_referencing(emu_lib):
    cases.notch_reref_case(emu_lib)


def test_process_window_by_window_equals_run(emu_lib):
    cases.process_equals_run(emu_lib, _rows(emu_lib, "s30k")[1])


@pytest.mark.parametrize("sfreq", [20000, 40000])
def test_bins_of_the_500_sample_segments(emu_lib, sfreq):
    cases.probe_500(emu_lib, sfreq)


def test_bins_of_the_split_segment(emu_lib):
    cases.probe_split(emu_lib)


def test_16000_sample_plan_beyond_the_generic_layout(emu_lib, monkeypatch):
    cases.stft_16000_goes_long(emu_lib, monkeypatch.setenv, monkeypatch.delenv)


# ---- coherence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c16400", "c40k", "c20k_pre"])
def test_emulator_long_coherence_case(emu_lib, tag):
    out = cases.coh_case(emu_lib, tag)
    assert out["nan"] == 0
    assert out["ill"] <= int(cases.COH_CAP * out["entries"]), out


def test_coherence_against_the_reference_s_table(emu_lib):
    out = cases.coh_fixture_case(emu_lib)
    assert out["nan"] == 0
    assert out["ill"] <= int(cases.COH_CAP * out["entries"]), out


def test_channel_constant_within_a_window(emu_lib):
    """(NaN as in the reference: coh and icoh of the pair are 0 / 0 in the last window.)"""
    out = cases.coh_case(emu_lib, "c_const")
    rows, cols = out["rows"], out["cols"]
    j = [i for i, c in enumerate(cols) if c.startswith(("coh_", "icoh_")) and "max_allfbands" not in c]
    assert np.isnan(rows[-1, j]).all() and not np.isnan(rows[:-1, j]).any()


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feature,var", [("stft", "NMX_LONG_STFT"), ("coherence", "NMX_LONG_COHERENCE")])
def test_gate_is_closed_without_the_opt_in(emu_lib, monkeypatch, feature, var):
    cases.gate_closed(emu_lib, monkeypatch.setenv, monkeypatch.delenv, feature, var)


def test_refusal_text_of_the_older_switches_is_the_parent_s(emu_lib, monkeypatch):
    cases.parent_messages(emu_lib, monkeypatch.setenv, monkeypatch.delenv)


def test_window_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_coherence_segment_above_4096_raises(emu_lib):
    cases.long_segment_raises(emu_lib)


def test_segment_without_a_split_raises(emu_lib):
    cases.no_split_raises(emu_lib)


def test_fft_return_spectrum_stays_refused(emu_lib):
    cases.fft_return_spectrum_still_raises(emu_lib)


def test_nothing_below_the_gate_moved(emu_lib, monkeypatch):
    cases.below_the_gate_emu(emu_lib, monkeypatch.setenv, monkeypatch.delenv)


# ---- one plan -------------------------------------------------------------------------------------------------------------------
def test_30_khz_defaults_with_stft_and_coherence_in_one_plan(emu_lib):
    acc, out = cases.all_in_one_plan(emu_lib)
    assert acc == {}, acc
    assert out["ill"] <= int(cases.COH_CAP * out["entries"]), out
