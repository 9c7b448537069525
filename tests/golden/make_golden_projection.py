"""Generate tests/golden/projection_*.npz from the reference's own grid projection (processing/projection.py run by its
DataProcessor / Stream).

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden.py); the tests read the
.npz files it writes.  Every case stores the settings, the channel table, the coordinates, BOTH grid tables as arrays (the
tests write them to TSV files: the GPU machine has no reference checkout), the data (case A / B: the rows of
real_recording.npz to take), the reference's key list, its values per hop BEFORE the NaN policy (``Projection.project_features``
patched to record the dict it completes), the NaN pattern of its final table, its matrices, active points and sidecar.
Cases:
  A  sub-testsub's iEEG run with its electrodes (right hemisphere), fast compute, cortex only, z-score
  B  the same recording with cortex AND subcortex, the default feature set with fft return_spectrum (psd keys are projected
     without being normalised), one channel NaN for part of the run, the unused MOV_RIGHT row dropped (the reference's NaN
     policy indexes the used names with a mask over ALL rows); a few hops
  C  a synthetic left-hemisphere montage (16 ECoG + 8 LFP contacts, one ECoG channel bad but listed in the coordinates), both
     plugins of tests/user_plugins.py registered, a ragged sampling rate (1111.111 Hz: two window lengths)
  D  the error cases: projection without coordinates, ECoG on both hemispheres, project_subcortex without LFP contacts on
     the session's side, a new_name that is a prefix of another channel's keys (ragged rows at the first hop)
"""

from __future__ import annotations

import json
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import ref_shim  # noqa: E402

nm = ref_shim.load_reference()
import pandas as pd  # noqa: E402
from py_neuromodulation.processing import projection as ref_projection  # noqa: E402

warnings.filterwarnings("ignore")

REF = Path(ref_shim.REFERENCE_ROOT) / "py_neuromodulation"
ELECTRODES = REF / "data/sub-testsub/ses-EphysMedOff/ieeg/sub-testsub_ses-EphysMedOff_space-mni_electrodes.tsv"
GRID_CORTEX = pd.read_csv(REF / "grid_cortex.tsv", sep="\t")
GRID_SUBCORTEX = pd.read_csv(REF / "grid_subcortex.tsv", sep="\t")

_RECORD: list = []
_orig_project = ref_projection.Projection.project_features


def _recording_project(self, feature_dict):
    _orig_project(self, feature_dict)
    _RECORD.append((list(feature_dict.keys()), np.fromiter(feature_dict.values(), dtype=np.float64)))


ref_projection.Projection.project_features = _recording_project


def dump(settings):
    return json.dumps(settings.model_dump())


def recording():
    g = np.load(HERE / "real_recording.npz", allow_pickle=False)
    data = g["stored"].T.astype(np.float64) * g["scale"][:, None]
    return data, json.loads(str(g["channels_json"])), float(g["sfreq"])


def electrodes():
    e = pd.read_csv(ELECTRODES, sep="\t")
    e = e[e["x"] != "n/a"] if e["x"].dtype == object else e.dropna(subset=["x"])
    return list(e["name"]), e[["x", "y", "z"]].astype(float).to_numpy().tolist()


def run_stream(settings, channels, data, sfreq, coord_names, coord_list, name="proj"):
    """-> dict of the reference's Stream.run: final table, pre-policy rows, key list, sidecar text, projection."""
    _RECORD.clear()
    st = nm.Stream(sfreq=sfreq, channels=pd.DataFrame(channels), settings=settings, line_noise=50, verbose=False,
                   coord_names=coord_names, coord_list=coord_list, path_grids=None)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data, out_dir=td, experiment_name=name, save_csv=False)
        sidecar = (Path(td) / name / f"{name}_SIDECAR.json").read_text()
    keys = _RECORD[0][0]
    assert all(k == keys for k, _ in _RECORD)
    pre = np.stack([v for _, v in _RECORD])
    proj = st.data_processor.projection
    out = {
        "settings_json": dump(st.settings), "channels_json": json.dumps(st.channels.to_dict("list")),
        "coord_names_json": json.dumps(coord_names), "coord_list": np.asarray(coord_list, dtype=np.float64),
        "grid_cortex": GRID_CORTEX.to_numpy(), "grid_subcortex": GRID_SUBCORTEX.to_numpy(),
        "sfreq": sfreq, "keys_json": json.dumps(keys), "columns_json": json.dumps([str(c) for c in df.columns]),
        "pre": pre, "final_nan": np.isnan(df.to_numpy(dtype=np.float64)), "sidecar_json": sidecar,
        "sess_right": bool(proj.sess_right),
    }
    if proj.project_cortex:
        out["proj_matrix_cortex"] = proj.proj_matrix_cortex
        out["active_cortex"] = np.asarray(proj.active_cortex_gridpoints)
    if proj.project_subcortex:
        out["proj_matrix_subcortex"] = proj.proj_matrix_subcortex
        out["active_subcortex"] = np.asarray(proj.active_subcortex_gridpoints)
    print(name, df.shape, "pre", pre.shape, "grid keys", sum(k.startswith("grid") for k in keys))
    return out


def case_a():
    data, ch, sfreq = recording()
    names, coords = electrodes()
    s = nm.NMSettings.get_fast_compute()
    s.postprocessing.project_cortex = True
    out = run_stream(s, ch, data, sfreq, names, coords, "a")
    out["rows"] = np.arange(data.shape[0])
    out["n_samples"] = data.shape[1]
    np.savez_compressed(HERE / "projection_a.npz", **out)


def case_b():
    data, ch, sfreq = recording()
    names, coords = electrodes()
    keep = [i for i, n in enumerate(ch["name"]) if n != "MOV_RIGHT"]
    ch = {k: [v[i] for i in keep] for k, v in ch.items()}
    n_samples = 1000 + 100 * 7   # eight hops
    data = data[keep, :n_samples].copy()
    data[4, 1230:1390] = np.nan   # ECOG_RIGHT_1: hops 3 .. 7 see it
    s = nm.NMSettings.get_default()
    s.postprocessing.project_cortex = True
    s.postprocessing.project_subcortex = True
    s.fft_settings.return_spectrum = True
    s.feature_normalization_settings.normalization_time_s = 1
    out = run_stream(s, ch, data, sfreq, names, coords, "b")
    out["rows"] = np.array(keep)
    out["n_samples"] = n_samples
    out["nan_span"] = np.array([4, 1230, 1390])
    np.savez_compressed(HERE / "projection_b.npz", **out)


def montage_c(rng):
    """16 ECoG contacts on left cortex grid points (jittered by a few mm), 8 LFP contacts near left subcortex points; metres."""
    cg = GRID_CORTEX.to_numpy()
    sg = GRID_SUBCORTEX.to_numpy()
    ci = rng.choice(len(cg), 16, replace=False)
    si = rng.choice(np.flatnonzero((sg[:, 0] < -8) & (np.abs(sg[:, 1]) < 20) & (np.abs(sg[:, 2]) < 15)), 8, replace=False)
    ecog = cg[ci] + rng.uniform(-4, 4, (16, 3))
    lfp = sg[si] + rng.uniform(-1.5, 1.5, (8, 3))
    names = [f"ECOG_L_{i:02d}" for i in range(16)] + [f"LFP_L_{i}" for i in range(8)]   # (no name prefixes another)
    return names, (np.concatenate([ecog, lfp]) / 1000).tolist()


def case_c():
    import user_plugins as up

    rng = np.random.default_rng(31)
    names, coords = montage_c(rng)
    n = len(names)
    ch = {"name": names, "rereference": ["None"] * n, "used": [1] * n, "target": [0] * n,
          "type": ["ecog"] * 16 + ["dbs"] * 8, "status": ["good"] * n, "new_name": list(names)}
    ch["status"][5] = "bad"   # listed in the coordinates, removed from them (remove_not_used_ch_from_coords)
    sfreq = 1111.111
    T = int(2.2 * sfreq)
    t = np.arange(T) / sfreq
    data = rng.standard_normal((n, T)) + 2.0 * np.sin(2 * np.pi * 17 * t)[None, :] * rng.uniform(0.5, 2, (n, 1))
    s = nm.NMSettings.get_default()
    s.reset()
    s.features.fft = True
    s.features.raw_hjorth = True
    s.preprocessing = ["re_referencing"]
    s.postprocessing.feature_normalization = True
    s.feature_normalization_settings.normalization_time_s = 1
    s.postprocessing.project_cortex = True
    s.postprocessing.project_subcortex = True
    s.project_subcortex_settings.max_dist_mm = 6
    nm.add_custom_feature("channel_mean", up.ChannelMean)
    nm.add_custom_feature("hop_stats", up.HopStats)
    try:
        out = run_stream(s, ch, data, sfreq, names, coords, "c")
    finally:
        for name in ("channel_mean", "hop_stats"):
            if name in nm.user_features:
                nm.remove_custom_feature(name)
    out["data"] = data
    np.savez_compressed(HERE / "projection_c.npz", **out)


def case_d():
    """The reference's exception type (class name) per case, with the inputs."""
    data, ch, sfreq = recording()
    names, coords = electrodes()
    cases = {}

    def attempt(tag, s, ch_, names_, coords_, data_=None):
        try:
            st = nm.Stream(sfreq=sfreq, channels=pd.DataFrame(ch_), settings=s, line_noise=50, verbose=False,
                           coord_names=names_, coord_list=coords_)
            if data_ is not None:
                with tempfile.TemporaryDirectory() as td:
                    st.run(data_, out_dir=td, experiment_name="d", save_csv=False)
            cases[tag] = "none"
        except Exception as e:   # noqa: BLE001 -- the type is the fixture
            cases[tag] = type(e).__name__
        print("D", tag, cases[tag])

    s = nm.NMSettings.get_fast_compute()
    s.postprocessing.project_cortex = True
    attempt("no_coords", s, ch, None, None)
    both = [list(c) for c in coords]
    both[names.index("ECOG_RIGHT_0")][0] *= -1   # one ECoG contact on the left
    attempt("both_hemispheres", s, ch, names, both)
    s2 = nm.NMSettings.get_fast_compute()
    s2.postprocessing.project_cortex = True
    s2.postprocessing.project_subcortex = True
    no_lfp = [list(c) for c in coords]
    for i, nme in enumerate(names):
        if nme.startswith("LFP"):
            no_lfp[i][0] *= -1   # LFP contacts on the other side
    attempt("no_lfp_on_side", s2, ch, names, no_lfp)
    # a new_name that prefixes another channel's keys: "ECOG_RIGHT_1" takes the keys of "ECOG_RIGHT_1X" as well
    ch_p = {k: list(v) for k, v in ch.items()}
    ch_p["rereference"] = ["None"] * len(ch_p["name"])
    ch_p["new_name"] = list(ch_p["name"])
    ch_p["new_name"][names.index("ECOG_RIGHT_2")] = "ECOG_RIGHT_1X"
    attempt("prefix_ragged", s, ch_p, names, coords, data[:, :1500])
    out = {"cases_json": json.dumps(cases), "settings_json": dump(s), "settings_sub_json": dump(s2),
           "channels_json": json.dumps(ch), "channels_prefix_json": json.dumps(ch_p), "coord_names_json": json.dumps(names),
           "coord_list": np.asarray(coords), "coord_list_both": np.asarray(both), "coord_list_no_lfp": np.asarray(no_lfp),
           "grid_cortex": GRID_CORTEX.to_numpy(), "grid_subcortex": GRID_SUBCORTEX.to_numpy()}
    np.savez_compressed(HERE / "projection_d.npz", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c", "d"]
    for w in which:
        globals()[f"case_{w}"]()
