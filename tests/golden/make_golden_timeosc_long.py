"""Generate tests/golden/timeosc_long.npz: the reference's raw_hjorth / return_raw / linelength / fft / welch (and, in the
headline case, sharpwave_analysis) on windows of 20 000 to 40 000 samples.

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_sharpwave_long.py); the
tests read the .npz it writes.  Every case is the reference's own Stream.run on 2 channels and 5 hops with
sampling_rate_features_hz = 10, no pre-processing and no normaliser:
  d30k    30 kHz, 30 000-sample windows: the default features minus bursts, "walk"
  e40k    40 kHz, 40 000-sample windows: fft + welch with mean / median / std / max, fft without log_transform, the
          time-domain features, "white" with offsets +300 / -100
  t24414  24 414 Hz, 24 414-sample windows: fft + welch, "fast"
  seg20k  20 kHz, 2 s segments (40 000 samples): fft over the last second, welch with three 20 000-sample segments
  wide20k 20 kHz, 20 000-sample windows: fft + welch with an extra band broad = [4, 9000] Hz
The recordings are NOT stored: the file holds each case's generator parameters (tests/timeosc_long_recording.py), the
settings JSON, the channels, the columns and the reference's feature table.

    python tests/golden/make_golden_timeosc_long.py
"""

from __future__ import annotations

import importlib.util
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

_spec = importlib.util.spec_from_file_location("timeosc_long_recording", HERE.parent / "timeosc_long_recording.py")
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
HOPS, case_recording = _rec.HOPS, _rec.case_recording

warnings.filterwarnings("ignore")

# tag -> generator parameters (`window` = samples per window; the stream's rate is `sfreq`)
CASES = {
    "d30k": {"seed": 3101, "sfreq": 30000, "window": 30000, "kind": "walk"},
    "e40k": {"seed": 4101, "sfreq": 40000, "window": 40000, "kind": "white", "offsets": [300.0, -100.0]},
    "t24414": {"seed": 2441, "sfreq": 24414, "window": 24414, "kind": "fast"},
    "seg20k": {"seed": 2001, "sfreq": 20000, "window": 40000, "kind": "walk"},
    "wide20k": {"seed": 2002, "sfreq": 20000, "window": 20000, "kind": "walk"},
}


def settings_of(tag):
    s = nm.NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.fft = True
    s.features.welch = True
    if tag in ("d30k", "e40k"):
        s.features.raw_hjorth = True
        s.features.return_raw = True
        s.features.linelength = True
    if tag == "d30k":
        s.features.sharpwave_analysis = True
    if tag == "e40k":
        for o in (s.fft_settings, s.welch_settings):
            o.features.mean = o.features.median = o.features.std = o.features.max = True
        s.fft_settings.log_transform = False
    if tag == "seg20k":
        s.segment_length_features_ms = 2000
        s.fft_settings.windowlength_ms = 1000
    if tag == "wide20k":
        s.frequency_ranges_hz["broad"] = {"frequency_low_hz": 4, "frequency_high_hz": 9000}
    return s


def main():
    out = {"cases": np.array(list(CASES)), "params_json": json.dumps(CASES), "hops": HOPS}
    for tag, p in CASES.items():
        data = case_recording(p)
        s = settings_of(tag)
        st = nm.Stream(sfreq=p["sfreq"], data=data, settings=s, line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        assert len(df) == HOPS, (tag, df.shape)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list"))})
        print(tag, df.shape)
    np.savez_compressed(HERE / "timeosc_long.npz", **out)
    print("bytes", (HERE / "timeosc_long.npz").stat().st_size)


if __name__ == "__main__":
    main()
