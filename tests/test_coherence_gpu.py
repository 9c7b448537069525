"""Coherence (features/coherence.py) on the MI355X against the reference-generated fixtures
(tests/golden/make_golden_coherence.py), judged with the float64 restatement's per-entry conditioning
(tests/coherence_oracle.py): 1e-5 absolute, plus a bound for bins whose power is far below the segment energy, and
max_allfbands exact unless the float64 maximum is a tie within that bound.  Accepted entries are counted per test here;
none is booked into parity.STATS (coherence has no entry in accepted_miss_budget.json)."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import coherence_oracle as oracle  # noqa: E402
from tests.helpers import load_golden, settings_from_json  # noqa: E402

pytestmark = pytest.mark.gpu

DIRECT = [str(t) for t in load_golden("coherence_direct")["cases"]]


def _ranges(s):
    return {k: (float(v[0]), float(v[1])) for k, v in s.frequency_ranges_hz.items()}


def _cs(s):
    return s.coherence_settings.to_dict()


def _plain_channels(names):
    n = len(names)
    return {"name": list(names), "rereference": ["None"] * n, "used": [1] * n, "target": [0] * n, "type": ["ecog"] * n,
            "status": ["good"] * n, "new_name": list(names)}


def _judge(got: dict, want: dict, bounds: dict, alts: dict, max_accepted: int, what: str):
    misses, accepted = oracle.compare(got, want, bounds, alts)
    assert not misses, f"{what}: {len(misses)} misses, e.g. {misses[:6]}"
    assert len(accepted) <= max_accepted, f"{what}: {len(accepted)} accepted entries > {max_accepted}: {accepted[:6]}"
    return accepted


def _pipeline(tag, fixture="coherence_pipeline", sfreq=1000.0):
    g = load_golden(fixture)
    pre = f"{tag}_" if tag else ""
    s = settings_from_json(g[pre + "settings_json"])
    ch = json.loads(str(g[pre + "channels_json"]))
    return g, s, ch, [str(c) for c in g[pre + "columns"]], g[pre + "values"]


def _windows_and_bounds(s, ch, data, sfreq, keys):
    """Per-row float64 conditioning from the engine's own pre-processed windows (nmx_process_batch_tap), with the
    feature normaliser off (the bound belongs to the raw coherence values)."""
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.settings import NMSettings

    s2 = NMSettings(**s.to_dict())
    s2.postprocessing.feature_normalization = False
    dp = DataProcessor(sfreq, s2, ch, line_noise=50, verbose=False)
    eng = dp.engine
    from oracle import nm_oracle as orc

    st, en, _ = orc.window_schedule(data.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    starts = np.asarray(st, dtype=np.int64)[: len(st)]
    _, pre = eng.process_batch(np.ascontiguousarray(data), starts, tap=True)
    names = eng.ch_names
    rows = []
    for r in range(pre.shape[0]):
        vals, bnd, alts = oracle.features(pre[r].astype(np.float64), names, eng.sfreq, _cs(s2), _ranges(s2),
                                          with_bound=True)
        rows.append((vals, bnd, alts))
    eng.close()
    return rows


def _check_table(df_vals, cols, want, rows, max_accepted, what):
    coh_cols = [j for j, c in enumerate(cols) if c.startswith(("coh_", "icoh_"))]
    assert coh_cols
    n_acc = 0
    for r in range(want.shape[0]):
        got = {cols[j]: df_vals[r, j] for j in coh_cols}
        wnt = {cols[j]: want[r, j] for j in coh_cols}
        n_acc += len(_judge(got, wnt, rows[r][1], rows[r][2], max_accepted, f"{what} row {r}"))
    assert n_acc <= max_accepted
    return n_acc


# ---- A, B: Stream.run and DataProcessor.process ------------------------------------------------------------------------
def test_case_a_stream_run():
    from py_neuromodulation_amd.stream import Stream

    g, s, ch, cols, want = _pipeline("a")
    df = Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50).run(g["data"], save_csv=False)
    assert list(df.columns) == cols
    rows = _windows_and_bounds(s, ch, g["data"], 1000.0, cols)
    n_acc = _check_table(df.to_numpy(dtype=np.float64), cols, want, rows, max_accepted=600, what="A Stream.run")
    print("A accepted entries:", n_acc)


def test_case_b_stream_run_coherence_columns():
    """fft / welch / bursts on, z-score normaliser on: only the coherence columns are compared (the other families are
    judged by the existing parity tier and its budget)."""
    from py_neuromodulation_amd.stream import Stream

    g, s, ch, cols, want = _pipeline("b")
    df = Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50).run(g["data"], save_csv=False)
    assert list(df.columns) == cols
    got = df.to_numpy(dtype=np.float64)
    j = [i for i, c in enumerate(cols) if c.startswith(("coh_", "icoh_"))]
    # z-scored values: a difference relative to the history's spread; the normaliser's first rows are exact copies
    err = np.abs(got[:, j] - want[:, j])
    assert np.nanmax(err[:1]) < 1e-4
    bad = np.mean(err > 2e-3)
    assert bad < 0.02, f"{bad:.3%} of the normalised coherence entries beyond 2e-3"


def test_case_a_data_processor_process():
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.data_processor import DataProcessor

    g, s, ch, cols, want = _pipeline("a")
    dp = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False)
    st, en, _ = orc.window_schedule(g["data"].shape[1], 1000.0, s.sampling_rate_features_hz, s.segment_length_features_ms)
    rows = _windows_and_bounds(s, ch, g["data"], 1000.0, cols)
    idx = {c: i for i, c in enumerate(cols)}
    n_acc = 0
    for r in range(0, len(st), 10):
        res = dp.process(g["data"][:, st[r]:en[r]])
        got = {k: v for k, v in res.items() if k.startswith(("coh_", "icoh_"))}
        wnt = {k: want[r, idx[k]] for k in got}
        n_acc += len(_judge(got, wnt, rows[r][1], rows[r][2], 10, f"A process row {r}"))
    assert n_acc <= 10


# ---- C: drop-in class and process_window -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", DIRECT)
def test_case_c_dropin_calc_feature(tag):
    from py_neuromodulation_amd.features import Coherence

    g = load_golden("coherence_direct")
    s = settings_from_json(g[f"{tag}_settings_json"])
    W = int(g[f"{tag}_window"])
    x = g["data"][:, :W]
    names = [str(c) for c in g["ch_names"]]
    got = Coherence(s, names, float(g["sfreq"])).calc_feature(x)
    want = dict(zip([str(k) for k in g[f"{tag}_keys"]], g[f"{tag}_values"]))
    assert list(got) == list(want)
    _, bounds, alts = oracle.features(x, names, float(g["sfreq"]), _cs(s), _ranges(s), with_bound=True)
    _judge(got, want, bounds, alts, max_accepted=12, what=f"C {tag}")


def test_case_c_process_window_and_batch_agree():
    """process_window (the reference's call shape) == one row of process_batch, bit for bit."""
    from py_neuromodulation_amd.engine import HotPathEngine

    g = load_golden("coherence_direct")
    s = settings_from_json(g["n128_settings_json"])
    names = [str(c) for c in g["ch_names"]]
    e = HotPathEngine(s, names, 1000.0, features=["coherence"], window=1000)
    one = e.process_window(g["data"])
    batch = e.process_batch(g["data"], np.array([0]))
    np.testing.assert_array_equal(one, batch[0])
    assert "nmx_kern_coh" in e.kernels(7)
    e.close()


# ---- D: the reference's own test_coherence setting ---------------------------------------------------------------------
def test_case_d_reference_test_setting():
    from py_neuromodulation_amd.stream import Stream

    g, s, ch, cols, want = _pipeline("", fixture="coherence_reftest", sfreq=500.0)
    df = Stream(sfreq=500.0, channels=ch, settings=s, line_noise=50).run(g["data"], save_csv=False)
    assert list(df.columns) == cols
    rows = _windows_and_bounds(s, ch, g["data"], 500.0, cols)
    n_acc = _check_table(df.to_numpy(dtype=np.float64), cols, want, rows, max_accepted=400, what="D")
    print("D accepted entries:", n_acc)
    res = {c: np.abs(df[c].values).mean() for c in cols if c != "time"}
    node = "icoh_seed_to_target_mean_fband_"
    assert res[node + "signal"] > res[node + "noise_low"] and res[node + "signal"] > res[node + "noise_high"]


# ---- batching, ragged runs, NaN channels, devices ----------------------------------------------------------------------
def test_batch_equals_window_by_window_ragged_run():
    """A float sampling rate cuts windows of two lengths (ragged run): the table of Stream.run == the windows one by one
    through DataProcessor.process, bit for bit on the coherence columns."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.stream import Stream
    from oracle import nm_oracle as orc

    rng = np.random.default_rng(5)
    sfreq = 999.5
    data = rng.standard_normal((4, 6000))
    data[1] += 0.5 * data[0]
    s = NMSettings.get_default()
    s.reset()
    s.features.coherence = True
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.coherence_settings.channels = [["ch0", "ch1"], ["ch2", "ch3"]]
    s.coherence_settings.frequency_bands = ["theta", "high_beta"]
    ch = [f"ch{i}" for i in range(4)]
    chans = _plain_channels(ch)
    df = Stream(sfreq=sfreq, channels=chans, settings=s).run(data, save_csv=False)
    cols = [c for c in df.columns if c.startswith(("coh_", "icoh_"))]
    assert cols
    st, en, _ = orc.window_schedule(data.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    assert len({b - a for a, b in zip(st, en)}) == 2
    dp = DataProcessor(sfreq, s, chans, verbose=False)
    for r, (a, b) in enumerate(zip(st, en)):
        res = dp.process(data[:, a:b])
        np.testing.assert_array_equal(np.array([res[c] for c in cols], np.float32),
                                      df[cols].to_numpy()[r].astype(np.float32))


def test_nan_channel_rule_on_coherence_keys():
    """A channel that is NaN in a window: every key naming it (the reference's substring rule) is NaN in that row."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.data_processor import DataProcessor

    s = NMSettings.get_default()
    s.reset()
    s.features.coherence = True
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.coherence_settings.channels = [["ca", "cb"], ["cc", "cd"]]
    chans = _plain_channels(["ca", "cb", "cc", "cd"])
    dp = DataProcessor(1000.0, s, chans, verbose=False)
    x = np.random.default_rng(1).standard_normal((4, 1000))
    x[0, 10] = np.nan
    res = dp.process(x)
    for k, v in res.items():
        if "_ca_" in k:
            assert np.isnan(v), k
        elif "_cc_" in k and "max_allfbands" not in k:
            assert np.isfinite(v), k


def test_devices_one_works_two_shards_raise():
    from py_neuromodulation_amd.stream import Stream

    g, s, ch, cols, want = _pipeline("a")
    df = Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50, devices=[0]).run(g["data"], save_csv=False)
    assert list(df.columns) == cols
    base = Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50).run(g["data"], save_csv=False)
    np.testing.assert_array_equal(df.to_numpy(), base.to_numpy())
    with pytest.raises(NotImplementedError, match="coherence"):
        Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50, devices=[0, 0]).run(g["data"], save_csv=False)
