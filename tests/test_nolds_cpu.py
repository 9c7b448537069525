"""The nolds feature (sample entropy; features/nolds.py) without a GPU: settings, key layout and construction errors
(dry_run plans), the float64 restatement (tests/nolds_oracle.py), and the kernel's item code in the single-thread
emulator (tests/emu/nmx_emu.cpp) on the cases of tests/nolds_probe_cases.py -- the same cases tests/test_nolds_gpu.py
runs on the device."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import nolds_oracle as oracle  # noqa: E402
from tests import nolds_probe_cases as cases  # noqa: E402
from tests.helpers import load_golden, settings_from_json  # noqa: E402

OTHER = ["correlation_dimension", "lyapunov_exponent", "hurst_exponent", "detrended_fluctuation_analysis"]


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


# ---- settings ---------------------------------------------------------------------------------------------------------
def test_settings_defaults_are_the_model_s():
    from py_neuromodulation_amd import NMSettings

    ns = NMSettings.get_default().nolds_settings
    assert ns.raw is True and ns.frequency_bands == ["low_beta"]
    assert list(ns.features) == ["sample_entropy"] + OTHER
    assert ns.features.get_enabled() == ["lyapunov_exponent"]


def test_settings_accept_plain_dicts_and_validate():
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.nolds_settings.features = {"sample_entropy": True}
    s.nolds_settings.frequency_bands = ["low beta", "theta"]
    assert s.nolds_settings.features.get_enabled() == ["sample_entropy"]
    assert s.nolds_settings.frequency_bands == ["low_beta", "theta"]
    v = s.validate().nolds_settings
    assert v.features.get_enabled() == ["sample_entropy"] and v.frequency_bands == ["low_beta", "theta"] and v.raw is True
    assert NMSettings(nolds_settings={"frequency_bands": ["high beta"]}).nolds_settings.frequency_bands == ["high_beta"]


# ---- surface: keys, errors (no device) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_pipeline_keys_in_reference_order(tag):
    import json

    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("nolds")
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    dp = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True)
    assert dp.keys == [str(c) for c in g[f"{tag}_columns"] if str(c) != "time"]


@pytest.mark.parametrize("measure", OTHER)
def test_other_measures_raise_by_name(measure):
    s = cases.nolds_settings()
    s.nolds_settings.features = {"sample_entropy": True, measure: True}
    from py_neuromodulation_amd.engine import HotPathEngine

    with pytest.raises(NotImplementedError, match=measure) as e:
        HotPathEngine(s, ["a"], 1000.0, dry_run=True)
    assert "RANSAC" in str(e.value)


def test_default_nolds_settings_raise_naming_lyapunov():
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    s = NMSettings.get_default()
    s.features.nolds = True
    with pytest.raises(NotImplementedError, match="lyapunov_exponent"):
        HotPathEngine(s, ["a"], 1000.0, dry_run=True)


def test_missing_segment_length_is_a_key_error():
    s = cases.nolds_settings(bands=["theta"])
    del s.bandpass_filter_settings.segment_lengths_ms["alpha"]
    from py_neuromodulation_amd.engine import HotPathEngine

    with pytest.raises(KeyError, match="alpha"):
        HotPathEngine(s, ["a"], 1000.0, features=["nolds"], dry_run=True)
    s.nolds_settings.frequency_bands = []   # (raw only: the reference builds no BandPower then)
    assert HotPathEngine(s, ["a"], 1000.0, features=["nolds"], dry_run=True).keys == ["a_nolds_sample_entropy_raw"]


def test_undefined_band_asserts():
    from py_neuromodulation_amd.engine import HotPathEngine

    with pytest.raises(AssertionError, match="nope selected in nolds_features"):
        HotPathEngine(cases.nolds_settings(bands=["nope"]), ["a"], 1000.0, features=["nolds"], dry_run=True)


def test_plan_description_carries_factor_and_ddof():
    eng = cases.engine(None, names=["a", "b"], bands=["low_beta", "theta"], dry_run=True)
    d = eng.desc
    assert d.nolds_raw == 1 and d.nolds_n_bands == 2
    assert d.nolds_ddof == 1 and abs(d.nolds_tol_factor - 0.1164 * (0.5627 * np.log(2) + 1.3334)) < 1e-15
    assert d.nolds_n_taps[0] == 999 and d.nolds_measures == 1
    assert d.n_filters == 0   # (bandpass_filter and bursts are off: the band series are nolds' own)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------
def test_restatements_agree_and_match_the_definition():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(40)
    tol = oracle.tolerance(x)
    T = len(x) - 2
    a = b = 0
    for i in range(T):
        for j in range(i + 1, T):
            d2 = max(abs(x[i] - x[j]), abs(x[i + 1] - x[j + 1]))
            b += d2 < tol
            a += max(d2, abs(x[i + 2] - x[j + 2])) < tol
    assert oracle.counts(x) == (a, b)
    y = cases.integer_series(300, 1)
    assert oracle.counts(y) == oracle.counts_small_integers(y)


# ---- the kernel's item code in the emulator ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.LENGTHS)
def test_exact_counts(emu_lib, n):
    cases.check_exact_counts(emu_lib, n)


def test_edge_values(emu_lib):
    cases.check_edge_values(emu_lib)


def test_series_limit_is_stated(emu_lib):
    cases.check_limit(emu_lib)


@pytest.mark.parametrize("seed", [0, 1])
def test_noise_raw(emu_lib, seed):
    cases.check_noise_raw(emu_lib, seed)


@pytest.mark.parametrize("W", [200, 1000])
def test_band_index_quirk(emu_lib, W):
    cases.check_band_index_quirk(emu_lib, W)


def test_long_window_bands(emu_lib):
    cases.check_long_window_bands(emu_lib)


def test_band_default_taps(emu_lib):
    cases.check_band_default_taps(emu_lib)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_pipeline(emu_lib, tag):
    cases.check_fixture_pipeline(emu_lib, tag)


@pytest.mark.parametrize("tag", ["a", "c"])
def test_fixture_direct_and_fused(emu_lib, tag):
    cases.check_fixture_direct(emu_lib, tag)


def test_plan_without_nolds_launches_what_it_launched_before(emu_lib):
    """The committed schedule traces (tests/golden/chunk_schedule*.json) pin every plan without nolds; here: switching nolds
    on inserts its own two launches (band filters, sample entropy) behind the time / oscillatory stage and changes nothing
    else of the sequence."""
    import ctypes as C

    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    end = emu_lib.lib.nmx_emu_trace_end
    end.restype, end.argtypes = C.c_longlong, [C.c_char_p, C.c_longlong]

    def trace(s):
        eng = HotPathEngine(s, ["a", "b"], 1000.0, lib=emu_lib)
        x = cases.noise(3, 2, 1200).astype(np.float32)
        buf = C.create_string_buffer(1 << 16)
        emu_lib.lib.nmx_emu_trace_begin()
        eng.process_batch(x, np.array([0, 100, 200]))
        n = end(buf, 1 << 16)
        # (streams and events are numbered over the library's life: the operations and their order are what is compared)
        return [" ".join(ln.split()[:2]) if ln.startswith("op") else ln.split()[0] for ln in buf.raw[:n].decode().splitlines()]

    s = NMSettings.get_default()
    s.reset()
    s.features.fft = True
    s.features.bandpass_filter = True
    base = trace(s)
    assert not any("nolds" in ln for ln in base)
    s.features.nolds = True
    s.nolds_settings.features = {"sample_entropy": True}
    with_nolds = trace(s)
    at = with_nolds.index("op be_launch_nolds")
    assert with_nolds[at - 1] == "op be_launch_bank_w64" and with_nolds[at - 2].startswith("op be_launch_timeosc")
    assert with_nolds[:at - 1] + with_nolds[at + 1:] == base


def test_channel_shards_cover_the_global_keys():
    """The series are per channel: the parts of a multi-device stream hold disjoint key sets whose union is the global list."""
    import json

    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("nolds")
    s = settings_from_json(g["c_settings_json"])
    ch = json.loads(str(g["c_channels_json"]))
    whole = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True).keys
    parts = [DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, channel_subset=sub).keys
             for sub in (range(0, 2), range(2, 3))]
    assert not set(parts[0]) & set(parts[1]) and set(parts[0]) | set(parts[1]) == set(whole)
    assert [k for k in whole if k in set(parts[0])] == parts[0]
