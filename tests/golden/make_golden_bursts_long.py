"""Generate tests/golden/bursts_long.npz: the reference's `bursts` features on windows of 9 000 to 40 000 samples (the cases
of tests/bursts_long_cases.py, which holds the parameters and the settings; tests/bursts_long_recording.py the generator).

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_timeosc_long.py); the tests read
the .npz it writes.  Every case is the reference's own Stream.run.  The recordings are NOT stored: the file holds each case's
generator parameters, the settings JSON, the channels, the columns, the reference's feature table (for defaults30k also the table
of the same run without the z-score), and the first half (centre
tap included) of every distinct band-pass FIR the reference's Bursts object used: the taps are symmetric up to the rounding
of their design (`taps_asym_max`; asserted below 1e-15 here), and the engine's design matches the mirrored half to 1e-12
(test_bursts_long_cpu.py).

    python tests/golden/make_golden_bursts_long.py
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

_spec = importlib.util.spec_from_file_location("bursts_long_cases", HERE.parent / "bursts_long_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)
recording = cases.recording

warnings.filterwarnings("ignore")


def main():
    out = {"cases": np.array(list(cases.CASES)), "params_json": json.dumps(cases.CASES)}
    taps_seen = {}
    for tag, p in cases.CASES.items():
        data = recording(p)
        st = nm.Stream(sfreq=p["sfreq"], data=data, settings=cases.settings_of(nm, p), line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        assert len(df) == p["hops"], (tag, df.shape)
        bands = list(st.settings.bursts_settings.frequency_bands)
        bu = nm.features.Bursts(st.settings, [f"ch{i}" for i in range(p["n_ch"])], p["sfreq"])
        names = []
        for band, taps in zip(bands, np.asarray(bu.bandpass_filter.filter_bank, np.float64)):
            asym = float(np.abs(taps - taps[::-1]).max())
            assert asym < 1e-15 and len(taps) % 2 == 1, "taps are not symmetric"
            out["taps_asym_max"] = max(out.get("taps_asym_max", 0.0), asym)
            key = f"taps_half_{p['sfreq']}_{band}"
            taps_seen[key] = taps[: len(taps) // 2 + 1]
            names.append(key)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list")),
                    f"{tag}_taps": np.array(names)})
        if p.get("defaults"):   # ... and the same run without the z-score (the composition is checked stage by stage)
            s_raw = cases.settings_of(nm, p)
            s_raw.postprocessing.feature_normalization = False
            st_raw = nm.Stream(sfreq=p["sfreq"], data=data, settings=s_raw, line_noise=50, verbose=False)
            with tempfile.TemporaryDirectory() as td:
                df_raw = st_raw.run(data=data, out_dir=td, save_csv=False)
            assert list(df_raw.columns) == list(df.columns)
            out.update({f"{tag}_raw_settings_json": json.dumps(st_raw.settings.model_dump()),
                        f"{tag}_raw_values": df_raw.to_numpy(dtype=np.float64)})
        print(tag, df.shape, names, flush=True)
    out.update(taps_seen)
    np.savez_compressed(HERE / "bursts_long.npz", **out)
    print("bytes", (HERE / "bursts_long.npz").stat().st_size)


if __name__ == "__main__":
    main()
