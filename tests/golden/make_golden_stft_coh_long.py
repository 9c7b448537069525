"""Generate tests/golden/stft_coh_long.npz: the reference's stft (features/oscillatory.py) and coherence
(features/coherence.py) on windows of 16 400 to 40 000 samples.

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_timeosc_long.py); the tests
read the .npz it writes.  Every case is the reference's own Stream.run with sampling_rate_features_hz = 10, no
pre-processing and no normaliser; the STFT cases on 2 channels x 5 hops (tests/timeosc_long_recording.py), the coherence
case on 3 channels x 4 hops (tests/stft_coh_long_recording.py: coh_recording):
  s16400    16.4 kHz, 16 400-sample windows, nperseg 500: the last segment is zero-padded (100 samples), "walk"
  s30k      30 kHz, 30 000 samples, nperseg 500, default bands (theta .. low beta hold no bin: NaN), with fft, welch and the
            time-domain features in the same plan, "walk"
  s40k_mid  40 kHz, 40 000 samples, nperseg 1000, mean / median / std / max, "white" with offsets +1000 / -1000
  s2k_20s   2 kHz, 20 s segments (40 000 samples), nperseg 20 000: five segments, "white"
  s_odd     20 kHz, 20 000 samples, nperseg 501, "white"
  s_short   20 kHz, 20 000 samples, nperseg 17 (about 2 350 segments of nine bins), an extra band broad = [1000, 9000] Hz
  s_psd     20 kHz, 20 000 samples, nperseg 500, return_spectrum
  c30k      30 kHz, 30 000 samples, coherence nperseg 256, two pairs, coh + icoh, the three features
Most default bands hold no bin of these grids (NaN in the reference too): the cases add bands that do (`bands`).
The recordings are NOT stored: the file holds each case's generator parameters, the settings JSON, the channels, the
columns and the reference's feature table.

    python tests/golden/make_golden_stft_coh_long.py
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

_spec = importlib.util.spec_from_file_location("stft_coh_long_recording", HERE.parent / "stft_coh_long_recording.py")
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
HOPS, case_recording, coh_recording = _rec.HOPS, _rec.case_recording, _rec.coh_recording

warnings.filterwarnings("ignore")

# tag -> generator parameters (`window` = samples per window; the stream's rate is `sfreq`)
CASES = {
    "s16400": {"seed": 1641, "sfreq": 16400, "window": 16400, "kind": "walk", "nperseg": 500, "bands": {"g1": [60, 200], "g2": [200, 400], "broad": [500, 6000]}},
    "s30k": {"seed": 3011, "sfreq": 30000, "window": 30000, "kind": "walk", "nperseg": 500, "bands": {"g1": [60, 200], "g2": [200, 400], "broad": [500, 6000]}},
    "s40k_mid": {"seed": 4011, "sfreq": 40000, "window": 40000, "kind": "white", "offsets": [1000.0, -1000.0], "nperseg": 1000,
                 "only_bands": {"b1": [30, 90], "b2": [100, 400], "b3": [1000, 3000]}},
    "s2k_20s": {"seed": 2021, "sfreq": 2000, "window": 40000, "kind": "white", "nperseg": 20000},
    "s_odd": {"seed": 5011, "sfreq": 20000, "window": 20000, "kind": "white", "nperseg": 501, "bands": {"g1": [60, 200], "g2": [200, 400], "broad": [500, 6000]}},
    "s_short": {"seed": 1711, "sfreq": 20000, "window": 20000, "kind": "white", "nperseg": 17, "bands": {"broad": [1000, 9000]}},
    "s_psd": {"seed": 5021, "sfreq": 20000, "window": 20000, "kind": "white", "nperseg": 500, "bands": {"g1": [60, 200], "g2": [200, 400], "broad": [500, 6000]}},
    "c30k": {"seed": 3021, "sfreq": 30000, "window": 30000, "n_ch": 3, "hops": 4, "mix": [0.8, 0.6, 0.4], "nperseg": 256},
}


def settings_of(tag):
    p = CASES[tag]
    s = nm.NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    if tag == "c30k":
        s.features.coherence = True
        s.frequency_ranges_hz["mid"] = {"frequency_low_hz": 200, "frequency_high_hz": 400}   # (bins 2, 3 of the 117 Hz grid)
        s.frequency_ranges_hz["wide"] = {"frequency_low_hz": 100, "frequency_high_hz": 5000}
        s.coherence_settings.channels = [["ch0", "ch1"], ["ch1", "ch2"]]
        s.coherence_settings.nperseg = p["nperseg"]
        s.coherence_settings.frequency_bands = ["mid", "wide"]
        s.coherence_settings.method = {"coh": True, "icoh": True}
        s.coherence_settings.features = {"mean_fband": True, "max_fband": True, "max_allfbands": True}
        return s
    s.features.stft = True
    for name, (lo, hi) in p.get("bands", {}).items():   # (beside the default bands: most of those hold no bin of these grids)
        s.frequency_ranges_hz[name] = {"frequency_low_hz": lo, "frequency_high_hz": hi}
    s.stft_settings.windowlength_ms = p["nperseg"]   # (taken as samples: oscillatory.py:199)
    if tag == "s30k":
        for f in ("fft", "welch", "raw_hjorth", "return_raw", "linelength"):
            setattr(s.features, f, True)
    if tag == "s40k_mid":   # (np.max of an empty band raises in the reference: bands that all hold bins of the 40 Hz grid)
        s.frequency_ranges_hz = {n: {"frequency_low_hz": lo, "frequency_high_hz": hi} for n, (lo, hi) in p["only_bands"].items()}
        o = s.stft_settings.features
        o.mean = o.median = o.std = o.max = True
    if tag == "s2k_20s":
        s.segment_length_features_ms = 20000
    if tag == "s_psd":
        s.stft_settings.return_spectrum = True
    return s


def main():
    out = {"cases": np.array(list(CASES)), "params_json": json.dumps(CASES), "hops": HOPS}
    for tag, p in CASES.items():
        data = coh_recording(p) if tag == "c30k" else case_recording(p)
        s = settings_of(tag)
        st = nm.Stream(sfreq=p["sfreq"], data=data, settings=s, line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        assert len(df) == p.get("hops", HOPS), (tag, df.shape)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list"))})
        print(tag, df.shape, "NaN", int(np.isnan(df.to_numpy(dtype=np.float64)).sum()))
    np.savez_compressed(HERE / "stft_coh_long.npz", **out)
    print("bytes", (HERE / "stft_coh_long.npz").stat().st_size)


if __name__ == "__main__":
    main()
