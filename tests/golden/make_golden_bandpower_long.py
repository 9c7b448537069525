"""Generate tests/golden/bandpower_long.npz: the reference's `bandpass_filter` features on windows of 16 385 to 40 000 samples
(the cases of tests/bandpower_long_cases.py, which holds the parameters, the settings and the recordings' generator).

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_bursts_long.py); the tests read
the .npz it writes.  Every case is the reference's own Stream.run.  The recordings are NOT stored: the file holds each case's
parameters, the settings JSON, the channels, the columns, the reference's feature table (for defaults30k also the table of the
same run without the z-score), and the first half (centre tap included) of two of the band-pass FIRs of the reference's
BandPower object at 20 kHz: the taps are symmetric up to the rounding of their design (`taps_asym_max`; asserted below 1e-15
here), and the engine's design matches the mirrored half to 1e-12 (test_bandpower_long_cpu.py).

    python tests/golden/make_golden_bandpower_long.py
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

_spec = importlib.util.spec_from_file_location("bandpower_long_cases", HERE.parent / "bandpower_long_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

warnings.filterwarnings("ignore")


def _run(p, s):
    data = cases.recording(p)
    st = nm.Stream(sfreq=p["sfreq"], data=data, settings=s, line_noise=50, verbose=False)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data=data, out_dir=td, save_csv=False)
    return st, df


def main():
    out = {"cases": np.array(list(cases.CASES)), "params_json": json.dumps(cases.CASES)}
    for tag, p in cases.CASES.items():
        st, df = _run(p, cases.settings_of(nm, p))
        assert len(df) == p["hops"], (tag, df.shape)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list"))})
        if p.get("defaults"):   # ... and the same run without the z-score (the composition is checked stage by stage)
            s_raw = cases.settings_of(nm, p)
            s_raw.postprocessing.feature_normalization = False
            st_raw, df_raw = _run(p, s_raw)
            assert list(df_raw.columns) == list(df.columns)
            out.update({f"{tag}_raw_settings_json": json.dumps(st_raw.settings.model_dump()),
                        f"{tag}_raw_values": df_raw.to_numpy(dtype=np.float64)})
        if tag == cases.TAPS_OF[0]:
            bp = nm.features.BandPower(st.settings, [f"ch{i}" for i in range(p["n_ch"])], p["sfreq"])
            bank = dict(zip(st.settings.frequency_ranges_hz, np.asarray(bp.bandpass_filter.filter_bank, np.float64)))
            for band in cases.TAPS_OF[1]:
                taps = bank[band]
                asym = float(np.abs(taps - taps[::-1]).max())
                assert asym < 1e-15 and len(taps) % 2 == 1, "taps are not symmetric"
                out["taps_asym_max"] = max(out.get("taps_asym_max", 0.0), asym)
                out[f"taps_half_{band}"] = taps[: len(taps) // 2 + 1]
        print(tag, df.shape, flush=True)
    np.savez_compressed(HERE / "bandpower_long.npz", **out)
    print("bytes", (HERE / "bandpower_long.npz").stat().st_size)


if __name__ == "__main__":
    main()
