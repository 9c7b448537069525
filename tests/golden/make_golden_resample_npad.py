"""tests/golden/resample_npad.npz: the reference's OWN Stream.run on recordings that are not sampled at 1 kHz, with
``mne.filter.resample`` restated WITH THE FUNCTION'S OWN DEFAULTS (npad=100: tests/resample_npad_oracle.py) -- what the
reference's call, which passes no npad, gets.  Build-container only, like make_golden.py: it imports the reference through
tests/golden/ref_shim.py, replaces ``mne.filter.resample`` in the stub, and stores data (arrays and JSON) only.

    python tests/golden/make_golden_resample_npad.py

Three recordings of 3 channels x 2.6 s at 2 kHz, 250 Hz and 1375 Hz (an odd padded length: 1375 + 200); default
pre-processing (raw_resampling, notch_filter, re_referencing); features raw_hjorth, return_raw, linelength, fft,
bandpass_filter; feature normalisation off.  Before it writes, the script runs the same float64 pipeline on the
fp32-ROUNDED recording (what the engine is handed) and requires tests/parity.compare WITHOUT a verifier to pass on every
row: a fixture that the rounding of the input alone could miss is not written (change the seed instead).
"""

from __future__ import annotations

import json
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT))
import ref_shim  # noqa: E402

nm = ref_shim.load_reference()
import mne.filter as mf  # noqa: E402  (the stub)



def _load_tests_package() -> None:
    """The reference has a regular `tests` package of its own, which wins over this repository's namespace package
    whatever the path order: name this repository's `tests` directory as the package."""
    import types

    pkg = types.ModuleType("tests")
    pkg.__path__ = [str(ROOT / "tests")]
    sys.modules["tests"] = pkg


_load_tests_package()
from tests import resample_npad_oracle  # noqa: E402

mf.resample = resample_npad_oracle.resample
warnings.filterwarnings("ignore")

FEATURES = ["raw_hjorth", "return_raw", "linelength", "fft", "bandpass_filter"]
RECORDINGS = (("down_2k", 2000.0, 52), ("up_250", 250.0, 53), ("odd_1375", 1375.0, 54))   # tag, rate, seed


def recording(sf: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    T = int(2.6 * sf)
    t = np.arange(T) / sf
    return (rng.standard_normal((3, T)) * 20 + 30 * np.sin(2 * np.pi * 50 * t) + 25 * np.sin(2 * np.pi * 17 * t)
            + rng.uniform(-100, 100, (3, 1)))


def settings():
    s = nm.NMSettings.get_default()
    for f in s.features.get_enabled():
        setattr(s.features, f, False)
    for f in FEATURES:
        setattr(s.features, f, True)
    s.postprocessing.feature_normalization = False
    return s


def main() -> None:
    out = {}
    for tag, sf, seed in RECORDINGS:
        data = recording(sf, seed)
        s = settings()
        assert list(s.preprocessing) == ["raw_resampling", "notch_filter", "re_referencing"], s.preprocessing
        st = nm.Stream(sfreq=sf, data=data, settings=s, line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        # the float64 pipeline fed the fp32-rounded recording must pass the test's policy (no verifier)
        from tests import parity
        from tests.helpers import settings_from_json

        data32 = data.astype(np.float32).astype(np.float64)
        st32 = nm.Stream(sfreq=sf, data=data32, settings=settings(), line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df32 = st32.run(data=data32, out_dir=td, save_csv=False)
        assert list(df32.columns) == list(df.columns)
        es = settings_from_json(json.dumps(st.settings.model_dump()))
        cols, want, got = [str(c) for c in df.columns], df.to_numpy(dtype=np.float64), df32.to_numpy(dtype=np.float64)
        W_new = int(round(1000.0 / sf * int(sf)))
        for r in range(len(want)):
            n_bad, rep, _ = parity.compare(cols[:-1], got[r, :-1], want[r, :-1], es, sf, float(np.abs(data).max()), W_new)
            assert n_bad == 0, f"{tag} row {r}: the fp32-rounded input alone misses the policy -- change the seed\n{rep}"
        out[f"{tag}_sfreq"] = sf
        out[f"{tag}_data"] = data
        out[f"{tag}_settings_json"] = json.dumps(st.settings.model_dump())
        out[f"{tag}_columns"] = np.array(list(df.columns))
        out[f"{tag}_values"] = df.to_numpy(dtype=np.float64)
        out[f"{tag}_channels_json"] = json.dumps(st.channels.to_dict("list"))
        print("resample_npad", tag, df.shape)
    np.savez_compressed(HERE / "resample_npad.npz", **out)
    print(HERE / "resample_npad.npz", (HERE / "resample_npad.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
