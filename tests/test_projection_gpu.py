"""Grid projection (processing/projection.py) on the MI355X against the reference-generated fixtures
(tests/golden/make_golden_projection.py), through ``Stream.run`` and through ``DataProcessor.process`` hop by hop:
  (i)   every column but the grid columns is bit-identical to the same run with the projection off;
  (ii)  the key list is the reference's;
  (iii) every grid entry is within  sum_k w_gk |x^_k - x_k| + 1e-6 sum_k w_gk |x_k|  of the reference's, x^ the engine's
        inputs BEFORE the NaN policy and x the reference's: the projection adds no error beyond what its inputs carry;
  (iv)  NaN channels: their own keys are NaN, the grid keys are the reference's (the NaN pattern of its final table);
  (v)   the sidecar JSON is the reference's;
  (vi)  several devices raise.
No entry goes through tests/parity.py's accepted-miss path."""

import json
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests.helpers import load_golden, settings_from_json  # noqa: E402
from tests.test_projection_cpu import case_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


def _data(g):
    if "data" in g.files:
        return g["data"]
    r = load_golden("real_recording")
    data = (r["stored"].T.astype(np.float64) * r["scale"][:, None])[g["rows"], :int(g["n_samples"])].copy()
    if "nan_span" in g.files:
        c, a, b = (int(v) for v in g["nan_span"])
        data[c, a:b] = np.nan
    return data


@pytest.fixture
def pre_policy(monkeypatch):
    """The float64 tables handed to the NaN policy (the engine's values before it), in call order."""
    from py_neuromodulation_amd import data_processor as dpm

    seen = []
    real = dpm._LazyNanCols.apply

    def apply(self, table, mask):
        seen.append(np.array(table, dtype=np.float64, copy=True))
        return real(self, table, mask)

    monkeypatch.setattr(dpm._LazyNanCols, "apply", apply)
    return seen


@pytest.fixture
def plugins(request):
    """Case C registers both plugins of tests/user_plugins.py, as the fixture's reference run did."""
    import py_neuromodulation_amd as nmx
    from tests import user_plugins as up

    on = request.param
    if on:
        nmx.add_custom_feature("channel_mean", up.ChannelMean)
        nmx.add_custom_feature("hop_stats", up.HopStats)
    yield on
    if on:
        for name in ("channel_mean", "hop_stats"):
            if name in nmx.user_features:
                nmx.remove_custom_feature(name)


def _layout(g, tmp_path):
    from py_neuromodulation_amd.projection import GridProjection

    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    keys = json.loads(str(g["keys_json"]))
    return GridProjection(s, ch, names, coords, grids).layout([k for k in keys if not k.startswith("grid")])


def _check_grid(lay, got_grid, got_pre, ref_pre, what):
    """(iii): |got - ref| <= sum_k w |x^ - x| + 1e-6 sum_k w |x| per grid entry (NaN / infinities: the same)."""
    x_hat, x = got_pre[:, :lay.n_keys], ref_pre[:, :lay.n_keys]
    ref = ref_pre[:, lay.n_keys:]
    d = np.abs(x_hat - x)
    d = np.where(np.isnan(d) & (np.isnan(x_hat) == np.isnan(x)), 0.0, d)          # (NaN inputs on both sides)
    d = np.where(np.isinf(x_hat) & (x_hat == x), 0.0, d)                              # (the same infinity)
    ax = np.abs(x)
    bound = lay.project(np.nan_to_num(d, nan=np.inf, posinf=np.inf)) + 1e-6 * lay.project(np.where(np.isfinite(ax), ax, 0))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got_grid), np.isnan(ref)), f"{what}: NaN pattern of the grid columns"
    assert np.array_equal(got_grid[np.isinf(ref)], ref[np.isinf(ref)]), f"{what}: infinite grid entries"
    err = np.abs(got_grid[fin] - ref[fin])
    ok = err <= bound[fin]
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} grid entries beyond the bound, worst excess {np.max(err - bound[fin])}"


def _stream(g, tmp_path, project=True):
    from py_neuromodulation_amd.stream import Stream

    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    if not project:
        s.postprocessing.project_cortex = s.postprocessing.project_subcortex = False
    return Stream(float(g["sfreq"]), ch, settings=s, line_noise=50, verbose=False, coord_names=names, coord_list=coords,
                  path_grids=grids)


@pytest.mark.parametrize("case,plugins", [("a", False), ("b", False), ("c", True)], indirect=["plugins"])
def test_stream_run(case, plugins, tmp_path, pre_policy):
    g = load_golden(f"projection_{case}")
    data = _data(g)
    lay = _layout(g, tmp_path)
    st = _stream(g, tmp_path)
    df = st.run(data, out_dir=tmp_path / "out", experiment_name="p", save_csv=False)
    got_pre = pre_policy[-1]
    keys = json.loads(str(g["keys_json"]))
    # (ii) the reference's columns: its keys, then time (case B and C carry no target)
    assert list(df.columns) == json.loads(str(g["columns_json"]))
    assert list(st.data_processor.keys) == keys
    got = df.to_numpy(dtype=np.float64)
    # (iii) grid columns against the reference, bounded by what their inputs carry
    _check_grid(lay, got[:, lay.n_keys:len(keys)], got_pre, g["pre"], f"Stream.run {case}")
    # (iv) the NaN pattern of the reference's final table (NaN channels' own keys NaN, grid keys not)
    assert np.array_equal(np.isnan(got), g["final_nan"])
    # (v) the sidecar
    side = json.loads((tmp_path / "out" / "p" / "p_SIDECAR.json").read_text())
    assert side == json.loads(str(g["sidecar_json"]))
    # (i) every other column bit-identical to the run without the projection
    off = _stream(g, tmp_path, project=False).run(data, out_dir=tmp_path / "off", experiment_name="p", save_csv=False)
    other = [c for c in df.columns if not str(c).startswith("grid")]
    assert list(off.columns) == other
    np.testing.assert_array_equal(df[other].to_numpy(dtype=np.float64), off.to_numpy(dtype=np.float64))


@pytest.mark.parametrize("case,plugins", [("a", False), ("b", False), ("c", True)], indirect=["plugins"])
def test_process_hop_by_hop(case, plugins, tmp_path, pre_policy):
    """DataProcessor.process, the reference's call shape: one window per call (case C: two window lengths)."""
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.generator import window_schedule

    g = load_golden(f"projection_{case}")
    data = _data(g)
    lay = _layout(g, tmp_path)
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    sfreq = float(g["sfreq"])
    starts, lens, _ = window_schedule(data.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    dp = DataProcessor(sfreq, s, ch, coord_names=names, coord_list=coords, path_grids=grids, line_noise=50, verbose=False)
    rows = []
    for a, n in zip(starts, lens):
        d = dp.process(data[:, int(a):int(a) + int(n)])
        rows.append(list(d.values()))
        assert list(d.keys()) == json.loads(str(g["keys_json"]))
    got = np.array(rows)
    got_pre = np.concatenate(pre_policy)
    _check_grid(lay, got[:, lay.n_keys:], got_pre, g["pre"], f"process {case}")
    assert np.array_equal(np.isnan(got), g["final_nan"][:, :got.shape[1]])
    # (i) the other columns: those of a processor without the projection
    s_off = settings_from_json(g["settings_json"])
    s_off.postprocessing.project_cortex = s_off.postprocessing.project_subcortex = False
    dp_off = DataProcessor(sfreq, s_off, ch, line_noise=50, verbose=False)
    off = np.array([list(dp_off.process(data[:, int(a):int(a) + int(n)]).values()) for a, n in zip(starts, lens)])
    keep = [i for i, k in enumerate(d) if not k.startswith("grid")]
    np.testing.assert_array_equal(got[:, keep], off)


def test_kernel_on_device_rows(tmp_path):
    """nmx_proj_process on host and on device rows (torch): within 1e-6 sum_k w |x_k| of the float64 product, NaN and
    infinities as the reference's dense product; the stage-8 kernel is named."""
    import torch

    from py_neuromodulation_amd.projection import DeviceProjection
    from tests.test_projection_cpu import _random_layout

    rng = np.random.default_rng(11)
    lay = _random_layout(rng, tmp_path=tmp_path)
    n = 700
    rows = np.full((n, lay.n_keys + lay.n_grid), 7.0, np.float32)
    rows[:, :lay.n_keys] = rng.standard_normal((n, lay.n_keys)) * 10 ** rng.uniform(-3, 3, (n, lay.n_keys))
    rows[3, lay.gather[0, 2]] = np.nan
    rows[5, lay.gather[-1, 4]] = np.inf
    want = lay.project(rows.astype(np.float64))
    absx = np.abs(rows.astype(np.float64))
    bound = 1e-6 * lay.project(np.where(np.isfinite(absx), absx, 0.0))
    dev = DeviceProjection(lay)
    host = dev.process(rows.copy())[:, lay.n_keys:].astype(np.float64)
    t = torch.from_numpy(rows.copy()).cuda()
    dev.process_device(t.data_ptr(), t.shape[1], n)
    torch.cuda.synchronize()
    on_dev = t.cpu().numpy()[:, lay.n_keys:].astype(np.float64)
    for got in (host, on_dev):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
        assert np.all(np.abs(got[fin] - want[fin]) <= bound[fin])
    np.testing.assert_array_equal(host, on_dev)


def test_stage_8_timer_and_kernel(tmp_path):
    """The attached projection runs as stage 8 of the launch sequence (nmx_last_timing_ms / nmx_last_kernels)."""
    g = load_golden("projection_a")
    data = _data(g)
    st = _stream(g, tmp_path)
    st.run(data, out_dir=tmp_path / "out", experiment_name="p", save_csv=False)
    eng = st.data_processor.engine
    assert "nmx_kern_proj" in eng.kernels(8)
    assert eng.timing_ms(8) > 0.0


def test_several_devices_raise(tmp_path):
    from py_neuromodulation_amd.stream import Stream

    g = load_golden("projection_a")
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    with pytest.raises(NotImplementedError, match="projection"):
        Stream(1000.0, ch, settings=s, coord_names=names, coord_list=coords, path_grids=grids, devices=[0, 1])
