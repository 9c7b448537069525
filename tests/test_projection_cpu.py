"""Grid projection (processing/projection.py) without a GPU: settings, the host plan (coordinates, matrices, active points,
key names) against the reference-generated fixtures (tests/golden/make_golden_projection.py), construction errors (dry_run
plans), and the kernel's item code in the single-thread emulator (tests/emu/nmx_emu.cpp) against a float64 projection of
the same rows."""

import json
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests.helpers import load_golden, settings_from_json  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def write_grids(g, path: Path) -> Path:
    """The fixture's grid tables as the reference's TSV files (the GPU machine has no reference checkout)."""
    path.mkdir(parents=True, exist_ok=True)
    for name in ("cortex", "subcortex"):
        pd.DataFrame(g[f"grid_{name}"], columns=["x", "y", "z"]).to_csv(path / f"grid_{name}.tsv", sep="\t", index=False)
    return path


def case_inputs(g, tmp_path):
    """-> (settings, channel table, coord_names, coord_list, path_grids) of a fixture."""
    return (settings_from_json(g["settings_json"]), pd.DataFrame(json.loads(str(g["channels_json"]))),
            json.loads(str(g["coord_names_json"])), g["coord_list"].tolist(), write_grids(g, tmp_path / "grids"))


def test_settings_defaults_and_validation():
    from py_neuromodulation_amd.settings import NMSettings, SettingsError

    s = NMSettings.get_default()
    assert s.project_cortex_settings.max_dist_mm == 20 and s.project_subcortex_settings.max_dist_mm == 5
    assert not s.postprocessing.project_cortex and not s.postprocessing.project_subcortex
    d = s.to_dict()
    assert d["project_cortex_settings"] == {"max_dist_mm": 20} and d["project_subcortex_settings"] == {"max_dist_mm": 5}
    for bad in (0, -1.5, "20", None, True):
        with pytest.raises(SettingsError, match="max_dist_mm"):
            NMSettings(project_subcortex_settings={"max_dist_mm": bad})
    assert NMSettings(project_cortex_settings={"max_dist_mm": 2.5}).project_cortex_settings.max_dist_mm == 2.5


@pytest.mark.parametrize("case", ["a", "b"])
def test_host_plan_matches_reference(case, tmp_path):
    """Matrices, active points, key names and order of the reference (the built-in keys, then the grid keys)."""
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden(f"projection_{case}")
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    dp = DataProcessor(float(g["sfreq"]), s, ch, coord_names=names, coord_list=coords, path_grids=grids, line_noise=50,
                       verbose=False, dry_run=True)
    assert dp.keys == json.loads(str(g["keys_json"]))
    p = dp.projection
    assert p.sess_right == bool(g["sess_right"])
    for grid in ("cortex", "subcortex"):
        if f"proj_matrix_{grid}" in g.files:
            np.testing.assert_allclose(getattr(p, f"proj_matrix_{grid}"), g[f"proj_matrix_{grid}"], rtol=1e-12, atol=0)
            np.testing.assert_array_equal(getattr(p, f"active_{grid}_gridpoints"), g[f"active_{grid}"])
    side = json.loads(str(g["sidecar_json"]))
    got = json.loads(json.dumps(dp.projection_sidecar(), default=_json_default))
    assert got["coords"] == side["coords"]
    for k in ("grid_cortex", "grid_subcortex", "proj_matrix_cortex", "proj_matrix_subcortex"):
        assert (k in got) == (k in side)
        if k in side:
            assert got[k] == side[k], k


def _json_default(obj):
    from py_neuromodulation_amd.file_writer import _json_default as jd

    return jd(obj)


def test_host_plan_user_keys_and_bad_channel(tmp_path):
    """Case C: the plugin keys that start with a channel's name are projected (HopStats' ``{ch}_rms``), ChannelMean's
    ``channel_mean_{ch}`` are not; the bad ECoG channel leaves the coordinates (and the one behind it is skipped, as the
    reference's deletion while iterating does)."""
    from py_neuromodulation_amd.projection import GridProjection

    g = load_golden("projection_c")
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    p = GridProjection(s, ch, names, coords, grids)
    keys = json.loads(str(g["keys_json"]))
    base = [k for k in keys if not k.startswith("grid")]
    lay = p.layout(base)
    assert base + lay.grid_keys == keys
    assert "rms" in lay.feature_names and "ptp_psd_like" in lay.feature_names
    assert not any(f.startswith("channel_mean") for f in lay.feature_names)
    np.testing.assert_allclose(p.proj_matrix_cortex, g["proj_matrix_cortex"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(p.proj_matrix_subcortex, g["proj_matrix_subcortex"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(p.active_cortex_gridpoints, g["active_cortex"])
    np.testing.assert_array_equal(p.active_subcortex_gridpoints, g["active_subcortex"])
    assert json.loads(json.dumps(p.coords, default=_json_default)) == json.loads(str(g["sidecar_json"]))["coords"]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_float64_projection_reproduces_reference(case, tmp_path):
    """The layout's float64 products on the reference's own (pre-policy) inputs are the reference's grid values."""
    from py_neuromodulation_amd.projection import GridProjection

    g = load_golden(f"projection_{case}")
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    keys = json.loads(str(g["keys_json"]))
    base = [k for k in keys if not k.startswith("grid")]
    lay = GridProjection(s, ch, names, coords, grids).layout(base)
    pre = g["pre"]
    got, want = lay.project(pre), pre[:, len(base):]
    absx = np.abs(pre)
    scale = lay.project(np.where(np.isfinite(absx), absx, 0.0))   # sum_k w |x_k|: the rounding of a product
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * scale[fin])


def _random_layout(rng, n_keys=300, tmp_path=None):
    """A host plan over a synthetic left montage, its layout on made-up keys."""
    from py_neuromodulation_amd.projection import GridProjection
    from py_neuromodulation_amd.settings import NMSettings

    g = load_golden("projection_d")
    grids = write_grids(g, tmp_path / "grids")
    cg, sg = g["grid_cortex"], g["grid_subcortex"]
    ecog = cg[rng.choice(len(cg), 12, replace=False)] + rng.uniform(-3, 3, (12, 3))
    lfp = sg[rng.choice(np.flatnonzero(sg[:, 0] < -8), 6, replace=False)] + rng.uniform(-1, 1, (6, 3))
    names = [f"ECOG_{i:02d}" for i in range(12)] + [f"LFP_{i}" for i in range(6)]
    n = len(names)
    ch = pd.DataFrame({"name": names, "rereference": ["None"] * n, "used": [1] * n, "target": [0] * n,
                       "type": ["ecog"] * 12 + ["dbs"] * 6, "status": ["good"] * n, "new_name": names})
    s = NMSettings.get_default()
    s.postprocessing.project_cortex = True
    s.postprocessing.project_subcortex = True
    s.project_subcortex_settings.max_dist_mm = 8
    p = GridProjection(s, ch, names, (np.concatenate([ecog, lfp]) / 1000).tolist(), grids)
    feats = [f"f{j}" for j in range(7)]
    keys = [f"{c}_{f}" for f in feats for c in names] + [f"other_{j}" for j in range(5)]
    return p.layout(keys)


def test_kernel_emulated_against_float64(emu_lib, tmp_path):
    """nmx_k_proj.h in the emulator: every grid entry within 1e-6 * sum_k w |x_k| of the float64 product of the same rows;
    a non-finite input of a channel out of a point's reach makes the point NaN (0 x NaN of the dense product), within
    its group only."""
    from py_neuromodulation_amd.projection import DeviceProjection

    rng = np.random.default_rng(5)
    lay = _random_layout(rng, tmp_path=tmp_path)
    assert lay.n_grid > 0 and len(lay.groups) == 2
    n = 9
    rows = np.full((n, lay.n_keys + lay.n_grid), 7.0, np.float32)
    rows[:, :lay.n_keys] = (rng.standard_normal((n, lay.n_keys)) * 10 ** rng.uniform(-3, 3, (n, lay.n_keys)))
    rows[3, lay.gather[0, 2]] = np.nan                  # an ECoG input
    rows[5, lay.gather[-1, 4]] = np.inf                 # an LFP input
    rows[6, lay.gather[1, 1]] = -np.inf
    want = lay.project(rows.astype(np.float64))
    dev = DeviceProjection(lay, lib=emu_lib)
    got = dev.process(rows.copy())[:, lay.n_keys:].astype(np.float64)
    # bound: 1e-6 * sum_k w |x_k|
    absx = np.abs(rows.astype(np.float64))
    bound = lay.project(np.where(np.isfinite(absx), absx, 0.0)) * 1e-6
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.all(got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)])
    assert np.all(np.abs(got[fin] - want[fin]) <= bound[fin]), np.max(np.abs(got[fin] - want[fin]) - bound[fin])
    # the NaN of row 3 stays in the cortex grid, the infinity of row 5 in the subcortex grid
    nc = len(lay.groups[0][2]) * lay.n_feat
    assert np.isnan(want[3, :nc]).any() and not np.isnan(want[3, nc:]).any()
    assert not np.isnan(want[5, :nc]).any() and (~np.isfinite(want[5, nc:])).any()
    # the table form (user features, ragged runs) writes the same grid columns
    tab = dev.process_table(rows[:, :lay.n_keys].astype(np.float64))
    np.testing.assert_array_equal(tab[:, lay.n_keys:], got)


def test_kernel_rejects_bad_layouts(emu_lib, tmp_path):
    """nmx_proj_create / _process check what the kernel relies on: columns, groups, row length."""
    import ctypes as C

    from py_neuromodulation_amd.projection import DeviceProjection

    lay = _random_layout(np.random.default_rng(8), tmp_path=tmp_path)
    dev = DeviceProjection(lay, lib=emu_lib)
    with pytest.raises(ValueError, match="row layout"):
        emu_lib.check(emu_lib.lib.nmx_proj_process(dev._h, np.zeros((2, lay.n_keys), np.float32).ctypes.data,
                                                   lay.n_keys, 2, 0, None))
    lay.out_col = lay.out_col - lay.n_keys          # outputs over the inputs
    with pytest.raises(ValueError, match="behind every gathered column"):
        DeviceProjection(lay, lib=emu_lib)
    lay.out_col = lay.out_col + lay.n_keys
    lay.point_group = np.zeros_like(lay.point_group)   # subcortex weights addressed to the cortex group
    with pytest.raises(ValueError, match="group"):
        DeviceProjection(lay, lib=emu_lib)
    assert C.sizeof(C.c_void_p) == 8


def test_errors_as_reference(tmp_path):
    """Case D: the reference's exception type, raised no later than the first hop (here: when the processor is built)."""
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("projection_d")
    want = json.loads(str(g["cases_json"]))
    grids = write_grids(g, tmp_path / "grids")
    names = json.loads(str(g["coord_names_json"]))
    ch = pd.DataFrame(json.loads(str(g["channels_json"])))
    s, s_sub = settings_from_json(g["settings_json"]), settings_from_json(g["settings_sub_json"])
    errors = {"AttributeError": AttributeError, "ValueError": ValueError}

    def build(settings, channels, coord_names, coord_list):
        DataProcessor(1000.0, settings, channels, coord_names=coord_names, coord_list=coord_list, path_grids=grids,
                      line_noise=50, verbose=False, dry_run=True)

    with pytest.raises(errors[want["no_coords"]], match="coords"):
        build(s, ch, None, None)
    with pytest.raises(errors[want["both_hemispheres"]], match="sess_right"):
        build(s, ch, names, g["coord_list_both"].tolist())
    with pytest.raises(errors[want["no_lfp_on_side"]], match="lfp_elec_names"):
        build(s_sub, ch, names, g["coord_list_no_lfp"].tolist())
    with pytest.raises(errors[want["prefix_ragged"]]):
        build(s, pd.DataFrame(json.loads(str(g["channels_prefix_json"]))), names, g["coord_list"].tolist())
    # the same settings with the regular channel table build
    build(s, ch, names, g["coord_list"].tolist())


def test_grid_files_need_a_directory(tmp_path, monkeypatch):
    """path_grids=None takes the grids of an installed reference package; without one the error names path_grids."""
    import importlib.util

    from py_neuromodulation_amd import projection

    real = importlib.util.find_spec
    monkeypatch.setattr(importlib.util, "find_spec",
                        lambda name, *a: None if name == "py_neuromodulation" else real(name, *a))
    with pytest.raises(FileNotFoundError, match="path_grids"):
        projection.grid_dir(None)
    assert projection.grid_dir(tmp_path) == tmp_path


def test_several_devices_raise(tmp_path):
    """Multi-device projection is out of scope: MultiDeviceProcessor, ShardedStream and channel_subset say so."""
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.sharding import MultiDeviceProcessor, ShardedStream
    from py_neuromodulation_amd.stream import Stream

    g = load_golden("projection_a")
    s, ch, names, coords, grids = case_inputs(g, tmp_path)
    with pytest.raises(NotImplementedError, match="projection"):
        MultiDeviceProcessor(1000.0, s, ch, line_noise=50, devices=[0, 1])
    with pytest.raises(NotImplementedError, match="projection"):
        ShardedStream(1000.0, ch, s, rank=0, world_size=2)
    with pytest.raises(NotImplementedError, match="projection"):
        DataProcessor(1000.0, s, ch, coord_names=names, coord_list=coords, path_grids=grids, line_noise=50,
                      verbose=False, dry_run=True, channel_subset=[0, 1])
    with pytest.raises(NotImplementedError, match="projection"):
        Stream(1000.0, ch, settings=s, coord_names=names, coord_list=coords, path_grids=grids, devices=[0, 1])
