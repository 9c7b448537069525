"""Coherence (features/coherence.py) without a GPU: settings, key layout and construction errors (dry_run plans), the
float64 restatement against the reference's values, and the kernel's item code in the single-thread emulator
(tests/emu/nmx_emu.cpp) against the reference-generated fixtures (tests/golden/make_golden_coherence.py)."""

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import coherence_oracle as oracle  # noqa: E402
from tests.helpers import load_golden, settings_from_json  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def _direct_settings(g, tag):
    return settings_from_json(g[f"{tag}_settings_json"])


def _ranges(s):
    return {k: (float(v[0]), float(v[1])) for k, v in s.frequency_ranges_hz.items()}


def _cs_dict(s):
    return s.coherence_settings.to_dict()


# ---- settings -------------------------------------------------------------------------------------------------------
def test_settings_defaults_are_the_yaml_values():
    from py_neuromodulation_amd import NMSettings

    cs = NMSettings.get_default().coherence_settings
    assert cs.channels == [] and cs.frequency_bands == ["high_beta"] and cs.nperseg == 128
    assert cs.features.get_enabled() == ["mean_fband", "max_fband", "max_allfbands"]
    assert cs.method.get_enabled() == ["coh", "icoh"]


def test_settings_accept_plain_dicts_and_validate():
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.settings import SettingsError

    s = NMSettings.get_default()
    s.coherence_settings.features = {"mean_fband": True, "max_fband": False, "max_allfbands": False}
    s.coherence_settings.method = {"coh": True, "icoh": False}
    s.coherence_settings.frequency_bands = ["high beta"]
    assert s.coherence_settings.features.get_enabled() == ["mean_fband"]
    assert s.coherence_settings.method.get_enabled() == ["coh"]
    assert s.coherence_settings.frequency_bands == ["high_beta"]
    assert s.validate().coherence_settings.features.get_enabled() == ["mean_fband"]
    for bad in ({"channels": [["a"]]}, {"channels": [["a", "b", "c"]]}, {"channels": [["a", 1]]}, {"nperseg": 0}):
        with pytest.raises(SettingsError):
            NMSettings(coherence_settings=bad)


# ---- key layout and construction errors (no device) -------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_pipeline_keys_in_reference_order(tag):
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("coherence_pipeline")
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    dp = DataProcessor(float(g["sfreq"]), s, ch, line_noise=50, verbose=False, dry_run=True)
    want = [str(c) for c in g[f"{tag}_columns"] if str(c) != "time"]
    assert dp.keys == want


def _engine(s, names, sfreq=1000.0, W=1000):
    from py_neuromodulation_amd.engine import HotPathEngine

    return HotPathEngine(s, names, sfreq, features=["coherence"], window=W, dry_run=True)


def _coh_settings(**cs):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.features.coherence = True
    for k, v in cs.items():
        setattr(s.coherence_settings, k, v)
    return s


def test_construction_errors_are_the_reference_s():
    names = ["ECOG_1", "ECOG_10", "LFP_1"]
    with pytest.raises(RuntimeError, match="does not match any"):
        _engine(_coh_settings(channels=[["ECOG_10", "STN"]]), names)
    with pytest.raises(RuntimeError, match="ambigous"):
        _engine(_coh_settings(channels=[["ECOG_1", "LFP"]]), names)
    with pytest.raises(AssertionError):
        _engine(_coh_settings(channels=[["ECOG_10", "LFP"]], frequency_bands=["nope"]), names)
    s = _coh_settings(channels=[["ECOG_10", "LFP"]], frequency_bands=["hf"])
    s.frequency_ranges_hz["hf"] = [400, 500]
    with pytest.raises(AssertionError, match="Nyquist"):
        _engine(s, names)
    with pytest.raises(ValueError, match="cannot run"):
        _engine(_coh_settings(channels=[["ECOG_10", "LFP"]], method={"coh": False, "icoh": True}), names)
    s = _coh_settings(channels=[["ECOG_10", "LFP"]], frequency_bands=["narrow"])
    s.frequency_ranges_hz["narrow"] = [10.2, 10.4]
    with pytest.raises(ValueError, match="zero-size"):
        _engine(s, names)
    s.coherence_settings.features = {"mean_fband": True, "max_fband": False, "max_allfbands": True}
    assert _engine(s, names).keys == ["coh_ECOG_10_to_LFP_mean_fband_narrow", "coh_ECOG_10_to_LFP_max_allfbands_narrow",
                                      "icoh_ECOG_10_to_LFP_mean_fband_narrow", "icoh_ECOG_10_to_LFP_max_allfbands_narrow"]


def test_repeated_pair_and_icoh_off_keys():
    s = _coh_settings(channels=[["A", "B"], ["B", "A"], ["A", "B"]], method={"coh": True, "icoh": False})
    e = _engine(s, ["A", "B"])
    assert e.keys == [f"coh_{a}_to_{b}_{f}_high_beta" for a, b in (("A", "B"), ("B", "A"))
                      for f in ("mean_fband", "max_fband", "max_allfbands")]
    assert e.coh_pairs == [(0, 1), (1, 0)]


def test_multi_shard_layout_raises():
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("coherence_pipeline")
    s = settings_from_json(g["a_settings_json"])
    ch = json.loads(str(g["a_channels_json"]))
    DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, channel_subset=range(8))
    with pytest.raises(NotImplementedError, match="coherence"):
        DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, channel_subset=range(4))


# ---- float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [str(t) for t in load_golden("coherence_direct")["cases"]])
def test_float64_restatement_matches_reference(tag):
    g = load_golden("coherence_direct")
    s = _direct_settings(g, tag)
    W = int(g[f"{tag}_window"])
    got, _, alts = oracle.features(g["data"][:, :W], [str(c) for c in g["ch_names"]], float(g["sfreq"]), _cs_dict(s),
                                   _ranges(s), with_bound=True)
    keys = [str(k) for k in g[f"{tag}_keys"]]
    assert list(got) == keys
    want = dict(zip(keys, g[f"{tag}_values"]))
    # one segment (nperseg >= window) makes coh 1 up to rounding in every bin: its argmax is a tie of rounding noise (and
    # icoh's may be one within 1e-5); the reference's pick is one of the tied bins
    ties = [k for k in keys if len(alts.get(k, ())) > 1]
    assert all(want[k] in alts[k] for k in ties)
    assert tag in ("n500_w500", "n2000") or not ties
    rest = [k for k in keys if k not in ties]
    np.testing.assert_allclose([got[k] for k in rest], [want[k] for k in rest], rtol=0, atol=1e-9)


# ---- the kernel's item code in the emulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [str(t) for t in load_golden("coherence_direct")["cases"]])
def test_emulator_direct_cases(emu_lib, tag):
    from py_neuromodulation_amd.features import Coherence

    g = load_golden("coherence_direct")
    s = _direct_settings(g, tag)
    W = int(g[f"{tag}_window"])
    x = g["data"][:, :W]
    names = [str(c) for c in g["ch_names"]]
    got = Coherence(s, names, float(g["sfreq"]), lib=emu_lib).calc_feature(x)
    want = dict(zip([str(k) for k in g[f"{tag}_keys"]], g[f"{tag}_values"]))
    assert list(got) == list(want)
    _, bounds, alts = oracle.features(x, names, float(g["sfreq"]), _cs_dict(s), _ranges(s), with_bound=True)
    misses, _ = oracle.compare(got, want, bounds, alts)
    assert not misses, misses[:8]
    if tag == "constant":
        assert all(np.isnan(v) for k, v in got.items() if "max_allfbands" not in k)
        assert all(v == 0.0 for k, v in got.items() if "max_allfbands" in k)


def _pipeline_check(lib, g, tag, sfreq, cols_of_interest=None):
    from py_neuromodulation_amd.stream import Stream

    s = settings_from_json(g[f"{tag}_settings_json"] if f"{tag}_settings_json" in g else g["settings_json"])
    chj = g[f"{tag}_channels_json"] if f"{tag}_channels_json" in g else g["channels_json"]
    cols_k = f"{tag}_columns" if f"{tag}_columns" in g else "columns"
    vals_k = f"{tag}_values" if f"{tag}_values" in g else "values"
    st = Stream(sfreq=sfreq, channels=json.loads(str(chj)), settings=s, line_noise=50, lib=lib)
    df = st.run(g["data"], save_csv=False)
    cols = [str(c) for c in g[cols_k]]
    assert list(df.columns) == cols
    return df, cols, g[vals_k]


def test_emulator_pipeline_case_a(emu_lib):
    g = load_golden("coherence_pipeline")
    df, cols, want = _pipeline_check(emu_lib, g, "a", 1000.0)
    got = df.to_numpy(dtype=np.float64)
    for j, c in enumerate(cols):
        if c == "time":
            continue
        if "max_allfbands" in c:
            # ties / near-ties of the float64 maxima are judged by the GPU tier with the conditioning bound
            assert np.mean(np.float32(got[:, j]) == np.float32(want[:, j])) > 0.9, c
        else:
            assert np.nanmax(np.abs(got[:, j] - want[:, j])) < 2e-4, c


def test_emulator_reference_test_case(emu_lib):
    g = load_golden("coherence_reftest")
    df, cols, want = _pipeline_check(emu_lib, g, "", 500.0)
    got = df.to_numpy(dtype=np.float64)
    # (noise_high, labelled 24 - 249 Hz, reads true 48 - 498 Hz of windows resampled from 500 to 1000 Hz: above the
    # resampler's cut-off the spectra are rounding noise and so are their ratios -- the GPU tier judges them with the
    # float64 conditioning bound)
    sel = [j for j, c in enumerate(cols) if c != "time" and "noise_high" not in c]
    assert np.nanmax(np.abs(got[:, sel] - want[:, sel])) < 2e-4
    res = {c: np.abs(df[c].values).mean() for c in cols if c != "time"}
    node = "icoh_seed_to_target_mean_fband_"
    assert res[node + "signal"] > res[node + "noise_low"] and res[node + "signal"] > res[node + "noise_high"]


# ---- C ABI: the appended fields default to off -----------------------------------------------------------------------
def test_zeroed_coherence_fields_mean_off(emu_lib):
    from py_neuromodulation_amd import _lib

    d = _lib.PlanDesc()
    C.memset(C.byref(d), 0, C.sizeof(d))
    d.abi_version = _lib.NMX_ABI_VERSION
    d.n_channels, d.window, d.sfreq, d.feat_hz = 2, 100, 1000.0, 10.0
    d.features = _lib.F_RAW
    d.raw_cols = _lib.Cols(0, 1, 0, 0)
    d.n_outputs = 2
    d.n_channels_in = 2
    plan = C.c_void_p()
    emu_lib.check(emu_lib.lib.nmx_plan_create(C.byref(d), C.byref(plan)))
    x = np.arange(200, dtype=np.float64).reshape(2, 100)
    out = np.zeros(2, np.float32)
    emu_lib.check(emu_lib.lib.nmx_process_window(plan, x.ctypes.data, 100, out.ctypes.data, None))
    assert out.tolist() == [99.0, 199.0]
    emu_lib.lib.nmx_plan_destroy(plan)
