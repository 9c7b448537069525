"""`bandpass_filter` on windows above 16 384 samples on the MI355X (libnmx.so): nmx_kern_bank_diff -- the partitioned bank
with the band-pass power epilogue from differenced taps -- against the reference-generated fixture
(tests/golden/make_golden_bandpower_long.py) and the float64 restatement.  Cases and policy: tests/bandpower_long_cases.py
(no verifier on the reference tables: no `bandpass` miss can be accepted; test_bandpower_long_cpu.py asserts the oracle's
log10 margins).  Figures observed: profiles/bandpower_long.md.  At the parent commit every positive case raises ValueError
at plan construction (the variable is unknown there)."""

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


pytestmark = pytest.mark.gpu

_ROWS = {}


def _rows(tag):
    if tag not in _ROWS:
        _ROWS[tag] = cases.run_case(None, tag)
    return _ROWS[tag]


@pytest.mark.parametrize("tag", cases.TABLE_CASES)
def test_long_window_case(tag):
    _rows(tag)


def test_complexity_does_not_cancel_at_20_khz():
    """The 20 kHz white-noise plan (sigma 50, default bands, 4 hops x 2 channels): every complexity entry within 1e-5 relative
    of the float64 oracle.  The second difference of the stored fp32 band series misses that by a factor of ten (1.06e-4,
    measured in the emulator: test_bandpower_long_cpu.py); measured here with the differenced taps: complexity 2.2e-7, mobility
    1.3e-7 (profiles/bandpower_long.md)."""
    worst, share = cases.cancellation_case(None)
    assert worst["complexity"] <= 1e-5 and share["complexity"] == 0, (worst, share)
    assert worst["mobility"] <= 1e-5, worst


@pytest.mark.parametrize("feats", [("activity", "mobility", "complexity"), ("activity", "mobility"), ("complexity",), ("activity",)])
def test_identity_taps_pin_the_shifts_and_the_tails(feats):
    assert cases.identity_probe(None, feats) == 2 * 3 * len(cases.ID_TAILS) * len(feats)


def test_kernel_of_the_long_plan_and_of_activity_alone():
    """Every long band-pass plan runs nmx_kern_bank_diff (activity alone: one series, the tail's blocks only)."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    p = cases.CASES["w20k_nolog"]
    x32 = cases.recording(p).astype(np.float32)
    rows, keys = {}, {}
    for feats in (cases.FEATS, ("activity",)):
        eng = HotPathEngine(cases.settings_of(nm, p, feats).validate(), ["ch0", "ch1"], float(p["sfreq"]))
        try:
            rows[feats] = eng.process_batch(x32, np.arange(p["hops"], dtype=np.int64) * 2000).copy()
            assert eng.kernels(3) == "nmx_kern_bank_diff", eng.kernels(3)
            keys[feats] = list(eng.keys)
        finally:
            eng.close()
    act = [i for i, k in enumerate(keys[cases.FEATS]) if "_activity_" in k]
    assert [keys[cases.FEATS][i] for i in act] == keys[("activity",)]
    # (the same y series, on frames one sample apart -- the differenced taps reach one tap further: the policy's rtol, not bytes)
    np.testing.assert_allclose(rows[cases.FEATS][:, act], rows[("activity",)], rtol=1e-5, atol=0)


def test_special_rows():
    assert cases.special_rows(None) == 0


def test_offsets_of_1000_through_the_offset_split():
    acc = cases.offsets_case(None)
    assert acc == {}, acc


def test_process_window_by_window_equals_run():
    cases.process_equals_run(None, _rows("w20k"))


def test_dropin_bandpower_equals_the_row():
    cases.dropin_equals_row(None, _rows("w20k_nolog"))


def test_ragged_pair_of_long_lengths_carries_the_kalman_state():
    assert cases.ragged_pair(None) == [20000, 20001]


@pytest.mark.parametrize("bursts", [False, True])
def test_gate_is_closed_without_the_opt_in(monkeypatch, bursts):
    if not bursts:
        monkeypatch.delenv("NMX_LONG_BURSTS")
    cases.gate_is_closed_without_the_opt_in(None, monkeypatch.delenv)


def test_filter_window_of_a_long_plan():
    cases.filter_window_series(None)


@pytest.mark.parametrize("bursts", [False, True])
def test_limited_features_raise_above_16384(monkeypatch, bursts):
    if not bursts:
        monkeypatch.delenv("NMX_LONG_BURSTS")
    cases.limited_features_raise(None)


def test_window_above_the_limit_raises():
    cases.over_limit_raises(None)


def test_nothing_below_the_gate_moved(monkeypatch):
    """An 8 kHz / 8000-sample plan (nmx_kern_bank, partitioned): the same kernels and the same bytes with the variable set
    and unset."""
    _, kernels = cases.below_the_gate(None, monkeypatch.setenv, monkeypatch.delenv)
    assert kernels == "nmx_kern_bank", kernels
