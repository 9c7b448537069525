"""STFT and coherence on windows above 16 384 samples on the MI355X (libnmx.so): nmx_kern_timeosc_long_stft<class> -- the
long-window time / oscillatory kernel with the STFT phase, one instantiation per segment class -- and nmx_kern_coh on the
long plan's window view, against the reference-generated fixture (tests/golden/make_golden_stft_coh_long.py) and the
float64 restatements.  Cases, policy and caps: tests/stft_coh_long_cases.py (the emulator tier asserts the float64 oracle's
own counts of ill-conditioned entries against the same caps).  Figures observed: profiles/stft_coh_long.md.  At the parent
commit every positive case raises ValueError at plan construction (the variables are unknown there)."""

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


pytestmark = pytest.mark.gpu

_ROWS = {}


def _rows(tag):
    if tag not in _ROWS:
        _ROWS[tag] = cases.run_case(None, tag)
    return _ROWS[tag]


# ---- STFT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", cases.STFT_TAGS)
def test_long_stft_case(tag):
    """(The kernel of the case's segment class is asserted inside: cases.KERNEL_OF.)"""
    _rows(tag)


def test_nan_samples_in_one_channel():
    acc, ch1, idx, _ = cases.nan_case(None)
    assert set(acc) <= {"fft", "welch"}, acc
    np.testing.assert_array_equal(ch1, _rows("s30k")[1][:, idx])


def test_behind_notch_and_re_referencing():
    cases.notch_reref_case(None)


def test_process_window_by_window_equals_run():
    cases.process_equals_run(None, _rows("s30k")[1])


@pytest.mark.parametrize("sfreq", [20000, 40000])
def test_bins_of_the_500_sample_segments(sfreq):
    cases.probe_500(None, sfreq)


def test_bins_of_the_split_segment():
    cases.probe_split(None)


def test_16000_sample_plan_beyond_the_generic_layout(monkeypatch):
    cases.stft_16000_goes_long(None, monkeypatch.setenv, monkeypatch.delenv)


def test_one_transform_class_equals_the_per_wave_class(monkeypatch):
    """NMX_LONG_STFT_PER_WAVE=0 sends 500-sample segments through the one-transform class: the same arithmetic in another
    order of barriers -- the rows agree to the policy's 1e-5."""
    from py_neuromodulation_amd.stream import Stream

    p, s, ch, cols, _ = cases.load_case("s16400")
    x = cases.case_recording(p)
    monkeypatch.setenv("NMX_LONG_STFT_PER_WAVE", "0")
    st = Stream(float(p["sfreq"]), channels=ch, settings=s, line_noise=50)
    got = st.run(x, save_csv=False).to_numpy(float)
    assert cases.K_LDS in st.data_processor.engine.kernels(2).split(" + ")
    np.testing.assert_allclose(got, _rows("s16400")[1], rtol=1e-5, atol=1e-5)


# ---- coherence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c16400", "c40k", "c20k_pre"])
def test_long_coherence_case(tag):
    assert cases.coh_case(None, tag)["nan"] == 0


def test_coherence_against_the_reference_s_table():
    assert cases.coh_fixture_case(None)["nan"] == 0


def test_channel_constant_within_a_window():
    out = cases.coh_case(None, "c_const")
    rows, cols = out["rows"], out["cols"]
    j = [i for i, c in enumerate(cols) if c.startswith(("coh_", "icoh_")) and "max_allfbands" not in c]
    assert np.isnan(rows[-1, j]).all() and not np.isnan(rows[:-1, j]).any()


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feature,var", [("stft", "NMX_LONG_STFT"), ("coherence", "NMX_LONG_COHERENCE")])
def test_gate_is_closed_without_the_opt_in(monkeypatch, feature, var):
    cases.gate_closed(None, monkeypatch.setenv, monkeypatch.delenv, feature, var)


def test_refusal_text_of_the_older_switches_is_the_parent_s(monkeypatch):
    cases.parent_messages(None, monkeypatch.setenv, monkeypatch.delenv)


def test_window_above_the_limit_raises():
    cases.over_limit_raises(None)


def test_nothing_below_the_gate_moved(monkeypatch):
    cases.below_the_gate_kernels(monkeypatch.setenv, monkeypatch.delenv)


# ---- one plan -------------------------------------------------------------------------------------------------------------------
def test_30_khz_defaults_with_stft_and_coherence_in_one_plan():
    acc, out = cases.all_in_one_plan()
    print(f"all in one: accepted {acc}, coherence accepted {out['accepted']} of {out['entries']}")
