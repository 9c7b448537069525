"""Generate tests/golden/nolds_hurst.npz from the reference's own nolds feature (features/nolds.py), DataProcessor and
Stream.run, with the Hurst exponent enabled.

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_nolds_dfa.py); the tests read
the .npz file it writes.  The `nolds` package itself is not installed there: a stub module `nolds` is installed whose
``hurst_rs`` is the float64 restatement of tests/nolds_hurst_oracle.py (nolds.hurst_rs with fit="poly"), whose ``dfa`` is
that of tests/nolds_dfa_oracle.py and whose ``sampen`` is that of tests/nolds_oracle.py.  Keys, their order
(sample_entropy, hurst_exponent, detrended_fluctuation_analysis inside a series and a channel), the band-index quirk,
nan_to_num and the sum rule are therefore pinned by the reference's code; only the measures themselves are restated.
Cases (three ECoG channels at 1 kHz, 1000-sample windows, 6 hops, default band table and pre-processing, normalisation
off):
  a  Hurst alone, raw plus frequency_bands = ["low_beta", "theta"]: the reference's Stream.run table
  b  sample entropy, Hurst and DFA, the same recording and series
  c  as a with an all-zero channel and a channel holding NaNs (no re-reference)
  e  Hurst plus sample entropy with raw off, frequency_bands = ["theta"], the recording of a
  d  direct Nolds(settings, ch_names, sfreq).calc_feature calls on the first window of a, b and c
"""

from __future__ import annotations

import importlib.util
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


def _by_path(name):   # (by path: the reference has a `tests` package of its own)
    spec = importlib.util.spec_from_file_location(name, HERE.parent / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


stub = types.ModuleType("nolds")
stub.sampen = _by_path("nolds_oracle").sampen
stub.dfa = _by_path("nolds_dfa_oracle").dfa
stub.hurst_rs = _by_path("nolds_hurst_oracle").hurst
sys.modules["nolds"] = stub
from py_neuromodulation.features.nolds import Nolds, NoldsFeatures, NoldsSettings  # noqa: E402

warnings.filterwarnings("ignore")

# (the reference's NMSettings declares the model as `nolds_features` while its Nolds class reads `settings.nolds_settings`:
# see make_golden_nolds.py -- the model is put back on every validated copy, nothing else of the reference is touched)
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
    x[0] = np.cumsum(x[0] - x[0].mean())   # (one channel with long-range correlations: H near 1)
    if zero_ch is not None:
        x[zero_ch] = 0.0
    if nan_ch is not None:
        x[nan_ch, 300:320] = np.nan
        x[nan_ch, 1210] = np.nan
    return x


def settings(bands, sampen, raw=True, dfa=False):
    s = nm.NMSettings.get_default()
    s.reset()
    s.features.nolds = True
    s.nolds_settings = NoldsSettings(raw=raw, frequency_bands=list(bands),
                                     features=NoldsFeatures(sample_entropy=sampen, lyapunov_exponent=False,
                                                            hurst_exponent=True,
                                                            detrended_fluctuation_analysis=dfa))
    s.postprocessing.feature_normalization = False
    return s


def stream_case(s, data, reference):
    channels = nm.utils.set_channels(ch_names=CH_NAMES, ch_types=CH_TYPES, reference=reference, bads=None,
                                     new_names="default", used_types=("ecog",), target_keywords=None)
    st = nm.Stream(settings=s, channels=channels, sfreq=SFREQ, line_noise=50, verbose=False)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data, out_dir=td, experiment_name="nolds_hurst", save_csv=False)
    return st, df


def main():
    out = {"sfreq": SFREQ}
    recs = {"r1": recording(31), "r2": recording(33, zero_ch=1, nan_ch=2)}
    cases = {
        "a": (settings(["low_beta", "theta"], sampen=False), "r1", "default"),
        "b": (settings(["low_beta", "theta"], sampen=True, dfa=True), "r1", "default"),
        # (no re-reference: the all-zero channel stays all zero)
        "c": (settings(["low_beta", "theta"], sampen=False), "r2", None),
        "e": (settings(["theta"], sampen=True, raw=False), "r1", "default"),
    }
    for name, data in recs.items():
        out[f"{name}_data"] = data
    for tag, (s, rec, reference) in cases.items():
        st, df = stream_case(s, recs[rec], reference)
        out[f"{tag}_recording"] = rec
        out[f"{tag}_settings_json"] = json.dumps(st.settings.model_dump())
        out[f"{tag}_columns"] = np.array(list(df.columns))
        out[f"{tag}_values"] = df.to_numpy(dtype=np.float64)
        out[f"{tag}_channels_json"] = json.dumps(st.channels.to_dict("list"))
        print("pipeline", tag, df.shape, list(df.columns)[:4])
    for tag in ("a", "b", "c"):
        s, rec, _ = cases[tag]
        res = Nolds(s, CH_NAMES, SFREQ).calc_feature(recs[rec][:, :1000])
        out[f"d{tag}_keys"] = np.array(list(res))
        out[f"d{tag}_values"] = np.array([float(v) for v in res.values()])
        print("direct", tag, len(res))
    out["ch_names"] = np.array(CH_NAMES)
    np.savez_compressed(HERE / "nolds_hurst.npz", **out)
    print((HERE / "nolds_hurst.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
