"""Generate tests/golden/nolds.npz from the reference's own nolds feature (features/nolds.py) and DataProcessor.

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden.py); the tests read the
.npz file it writes.  The `nolds` package itself is not installed there: a stub module `nolds` is installed whose
``sampen`` is the float64 restatement of tests/nolds_oracle.py.  Keys, their order, the band-index quirk (nolds.py:59-65),
nan_to_num and the sum rule are therefore pinned by the reference's code; only ``sampen`` itself is restated.  Cases:
  a  three ECoG channels at 1 kHz, 1000-sample windows, 6 hops, default band table and pre-processing, sample_entropy of
     raw plus frequency_bands = ["low_beta", "theta"], normalisation off: the reference's Stream.run table
  b  the same, raw only
  c  the same as a with an all-zero channel and a channel holding NaNs
  d  direct Nolds(settings, ch_names, sfreq).calc_feature calls on the first window of a and of c
"""

from __future__ import annotations

import json
import sys
import tempfile
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import ref_shim  # noqa: E402

nm = ref_shim.load_reference()
import importlib.util  # noqa: E402

# (by path: the reference has a `tests` package of its own)
_spec = importlib.util.spec_from_file_location("nolds_oracle", HERE.parent / "nolds_oracle.py")
nolds_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(nolds_oracle)

stub = types.ModuleType("nolds")
stub.sampen = nolds_oracle.sampen
sys.modules["nolds"] = stub
from py_neuromodulation.features.nolds import Nolds, NoldsFeatures, NoldsSettings  # noqa: E402

warnings.filterwarnings("ignore")

# The reference's NMSettings declares the model as `nolds_features` while its Nolds class reads `settings.nolds_settings`:
# that attribute is an undeclared extra, which every validate() (a copy through model_dump) turns back into a plain dict,
# and Nolds then fails on `.frequency_bands`.  The generator puts the model back on every validated copy; nothing else of
# the reference is touched.
_validate = nm.NMSettings.validate


def _validate_keeping_nolds(self, *args, **kwargs):
    out = _validate(self, *args, **kwargs)
    ns = getattr(out, "nolds_settings", None)
    if isinstance(ns, dict) and "frequency_bands" in ns:
        out.nolds_settings = NoldsSettings(**ns)
    return out


nm.NMSettings.validate = _validate_keeping_nolds

CH_NAMES = ["ECOG_R_0", "ECOG_R_1", "ECOG_R_2"]
CH_TYPES = ["ecog"] * 3
SFREQ = 1000.0


def recording(seed, zero_ch=None, nan_ch=None):
    rng = np.random.default_rng(seed)
    T = 1500   # 6 hops of a 1000-sample window at 10 Hz
    t = np.arange(T) / SFREQ
    x = rng.standard_normal((3, T)) * 50 + 10 * np.sin(2 * np.pi * 20 * t) + rng.uniform(-200, 200, (3, 1))
    if zero_ch is not None:
        x[zero_ch] = 0.0
    if nan_ch is not None:
        x[nan_ch, 300:320] = np.nan
        x[nan_ch, 1210] = np.nan
    return x


def settings(bands):
    s = nm.NMSettings.get_default()
    s.reset()
    s.features.nolds = True
    # (the reference's Nolds reads settings.nolds_settings, its NMSettings declares the model as `nolds_features` and its
    # YAML's nolds_settings block has another shape: the model is assigned under the name the class reads)
    s.nolds_settings = NoldsSettings(raw=True, frequency_bands=list(bands),
                                     features=NoldsFeatures(sample_entropy=True, lyapunov_exponent=False))
    s.postprocessing.feature_normalization = False
    return s


def stream_case(s, data, reference):
    channels = nm.utils.set_channels(ch_names=CH_NAMES, ch_types=CH_TYPES, reference=reference, bads=None,
                                     new_names="default", used_types=("ecog",), target_keywords=None)
    st = nm.Stream(settings=s, channels=channels, sfreq=SFREQ, line_noise=50, verbose=False)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data, out_dir=td, experiment_name="nolds", save_csv=False)
    return st, df


def main():
    out = {"sfreq": SFREQ}
    cases = {
        "a": (settings(["low_beta", "theta"]), recording(11), "default"),
        "b": (settings([]), recording(12), "default"),
        # (no re-reference: the all-zero channel stays all zero)
        "c": (settings(["low_beta", "theta"]), recording(13, zero_ch=1, nan_ch=2), None),
    }
    for tag, (s, data, reference) in cases.items():
        st, df = stream_case(s, data, reference)
        out[f"{tag}_data"] = data
        out[f"{tag}_settings_json"] = json.dumps(st.settings.model_dump())
        out[f"{tag}_columns"] = np.array(list(df.columns))
        out[f"{tag}_values"] = df.to_numpy(dtype=np.float64)
        out[f"{tag}_channels_json"] = json.dumps(st.channels.to_dict("list"))
        print("pipeline", tag, df.shape, list(df.columns)[:4])
    for tag in ("a", "c"):
        s, data, _ = cases[tag]
        res = Nolds(s, CH_NAMES, SFREQ).calc_feature(data[:, :1000])
        out[f"d{tag}_keys"] = np.array(list(res))
        out[f"d{tag}_values"] = np.array([float(v) for v in res.values()])
        print("direct", tag, len(res))
    out["ch_names"] = np.array(CH_NAMES)
    np.savez_compressed(HERE / "nolds.npz", **out)
    print((HERE / "nolds.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
