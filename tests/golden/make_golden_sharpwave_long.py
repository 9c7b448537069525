"""Generate tests/golden/sharpwave_long.npz: the reference's sharpwave_analysis on windows beyond 14 500 samples.

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden.py: case_long_windows);
the tests read the .npz it writes.  Every case is the reference's own Stream.run on 2 channels and 5 hops with
sampling_rate_features_hz = 10, only sharpwave_analysis enabled, no pre-processing and no normaliser:
  d30k    30 kHz, 30 000-sample windows, default filter ranges and estimators (about 60 extrema of a kind per window)
  d16k    16 kHz, 16 000-sample windows, default filter ranges and estimators
  wide30k 30 kHz, filter_ranges_hz = [[5, 5000]] on white noise: thousands of extrema of each kind per window, most of
          them closer than `distance` to a neighbour
  all30k  30 kHz, all 13 features x 5 estimators, the estimator applied per polarity (the sw_all settings of
          long_windows.npz), on the "fast" recording (tests/sharpwave_long_recording.py: why)
The recordings are NOT stored: the file holds each case's seed and generator parameters (tests regenerate them with
`recording` of tests/sharpwave_long_recording.py), the settings JSON, the columns, the reference's feature
table, and the first half (centre tap included) of every distinct FIR the reference used: the taps are symmetric up
to the rounding of their design (`taps_asym_max`, about 1e-18 against taps of 1e-3; asserted below 1e-15 here), and
whole they would make the file larger than any other fixture.

    python tests/golden/make_golden_sharpwave_long.py
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
import ref_shim  # noqa: E402

nm = ref_shim.load_reference()
import py_neuromodulation.features  # noqa: E402

# the recording generator the tests regenerate the inputs with (loaded by path: numpy only at import time, and the
# reference has a `tests` package of its own)
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("sharpwave_long_recording", HERE.parent / "sharpwave_long_recording.py")
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
HOPS, recording = _rec.HOPS, _rec.recording

warnings.filterwarnings("ignore")

# tag -> generator parameters (everything `recording` needs)
CASES = {
    "d30k": {"seed": 3001, "sfreq": 30000, "kind": "walk"},
    "d16k": {"seed": 1601, "sfreq": 16000, "kind": "walk"},
    "wide30k": {"seed": 3002, "sfreq": 30000, "kind": "white"},
    "all30k": {"seed": 3004, "sfreq": 30000, "kind": "fast"},
}


def sharpwave_all(s):
    sw = s.sharpwave_analysis_settings
    sw.sharpwave_features.enable_all()
    feats = list(type(sw.sharpwave_features).model_fields.keys())
    sw.estimator.mean = list(feats)
    sw.estimator.median = ["prominence", "interval"]
    sw.estimator.max = ["prominence", "sharpness", "rise_steepness"]
    sw.estimator.min = ["decay_time", "sharpness"]
    sw.estimator.var = ["interval", "width"]


def settings_of(tag):
    s = nm.NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.sharpwave_analysis = True
    if tag == "wide30k":
        s.sharpwave_analysis_settings.filter_ranges_hz = [{"frequency_low_hz": 5, "frequency_high_hz": 5000}]
    if tag == "all30k":
        sharpwave_all(s)
        s.sharpwave_analysis_settings.apply_estimator_between_peaks_and_troughs = False
    return s


def main():
    out = {"cases": np.array(list(CASES)), "params_json": json.dumps(CASES), "hops": HOPS}
    taps_seen = {}
    for tag, p in CASES.items():
        data = recording(**p)
        s = settings_of(tag)
        st = nm.Stream(sfreq=p["sfreq"], data=data, settings=s, line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        assert len(df) == HOPS, (tag, df.shape)
        sw = nm.features.SharpwaveAnalyzer(st.settings, ["ch0", "ch1"], p["sfreq"])
        names = []
        for (fname, taps) in sw.list_filter:
            taps = np.asarray(taps, np.float64)
            asym = float(np.abs(taps - taps[::-1]).max())
            assert asym < 1e-15 and len(taps) % 2 == 1, "taps are not symmetric"
            out["taps_asym_max"] = max(out.get("taps_asym_max", 0.0), asym)
            key = f"taps_half_{p['sfreq']}_{fname}"
            taps_seen[key] = taps[: len(taps) // 2 + 1]
            names.append(key)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list")),
                    f"{tag}_taps": np.array(names)})
        print(tag, df.shape, names)
    out.update(taps_seen)
    np.savez_compressed(HERE / "sharpwave_long.npz", **out)
    print("bytes", (HERE / "sharpwave_long.npz").stat().st_size)


if __name__ == "__main__":
    main()
