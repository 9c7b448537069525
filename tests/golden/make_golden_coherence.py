"""Generate tests/golden/coherence*.npz from the reference's own coherence feature (features/coherence.py).

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden.py); the tests read the
.npz files it writes.  Cases:
  A  eight named ECoG + LFP channels, default notch + re-reference, coherence only (three pairs: one reversed, one resolved
     by prefix, one repeated; theta, high_beta and a custom band), normalisation off: the reference's Stream.run table
  B  case A with fft, welch and bursts on, z-score on, max_allfbands off: key interleaving and the normaliser
  C  direct Coherence.calc_feature calls on stored windows (nperseg 128, 125, 256, 500 on a 500-sample window, 2000;
     icoh off, an empty mean band, a constant channel)
  D  the setting of the reference's tests/test_coherence.py with a NumPy-built coupled signal
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
from py_neuromodulation.features.coherence import Coherence  # noqa: E402
from py_neuromodulation.utils.types import FrequencyRange  # noqa: E402

warnings.filterwarnings("ignore")

CH_NAMES = ["ECOG_R_0", "ECOG_R_1", "ECOG_R_2", "ECOG_R_3", "LFP_R_0", "LFP_R_1", "LFP_R_2", "LFP_R_3"]
CH_TYPES = ["ecog"] * 4 + ["dbs"] * 4


def bandlimited(rng, n, sfreq, lo, hi):
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / sfreq)
    spec[(f < lo) | (f > hi)] = 0
    x = np.fft.irfft(spec, n)
    return x / x.std()


def data_a(seed=7, sfreq=1000.0, seconds=12.0):
    rng = np.random.default_rng(seed)
    T = int(seconds * sfreq)
    t = np.arange(T) / sfreq
    shared = bandlimited(rng, T + 25, sfreq, 15, 20)
    x = rng.standard_normal((8, T)) * 2.0 + 3.0 * np.sin(2 * np.pi * 50 * t)
    for c in range(8):
        lag = 25 if c % 2 else 0
        x[c] += 4.0 * shared[lag:lag + T]
    x[5] += 1e3 * x[5].std()   # one channel far off zero
    return x


def dump(settings):
    return json.dumps(settings.model_dump())


def stream_case(s, data, sfreq):
    channels = nm.utils.set_channels(ch_names=CH_NAMES, ch_types=CH_TYPES, reference="default", bads=None,
                                     new_names="default", used_types=("ecog", "dbs"), target_keywords=None)
    st = nm.Stream(settings=s, channels=channels, sfreq=sfreq, line_noise=50, verbose=False)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data, out_dir=td, experiment_name="coh", save_csv=False)
    return st, df


def settings_a():
    s = nm.NMSettings.get_default()
    s.reset()
    s.features.coherence = True
    s.frequency_ranges_hz["custom"] = {"frequency_low_hz": 14, "frequency_high_hz": 22}
    s.coherence_settings.frequency_bands = ["theta", "high_beta", "custom"]
    return s


def case_pipeline():
    sfreq = 1000.0
    data = data_a()
    out = {"sfreq": sfreq, "data": data}
    s = settings_a()
    s.postprocessing.feature_normalization = False
    probe = nm.utils.set_channels(ch_names=CH_NAMES, ch_types=CH_TYPES, reference="default", bads=None,
                                  new_names="default", used_types=("ecog", "dbs"), target_keywords=None)
    names = list(probe[probe["used"] == 1]["new_name"])
    # reversed pair, a pair resolved by prefix (the first LFP bipolar name), a repeated pair
    lfp = next(n for n in names if n.startswith("LFP_R_0"))
    pairs = [[names[1], names[0]], ["LFP_R_0", names[2]], [names[1], names[0]]]
    print("pairs", pairs, "of", names, "(", lfp, ")")
    s.coherence_settings.channels = pairs
    for tag, mutate in {
        "a": lambda s: None,
        "b": lambda s: (setattr(s.features, "fft", True), setattr(s.features, "welch", True),
                        setattr(s.features, "bursts", True),
                        setattr(s.postprocessing, "feature_normalization", True),
                        setattr(s.coherence_settings.features, "max_allfbands", False)),
    }.items():
        sc = s.model_copy(deep=True)
        mutate(sc)
        st, df = stream_case(sc, data, sfreq)
        out[f"{tag}_settings_json"] = dump(st.settings)
        out[f"{tag}_columns"] = np.array(list(df.columns))
        out[f"{tag}_values"] = df.to_numpy(dtype=np.float64)
        out[f"{tag}_channels_json"] = json.dumps(st.channels.to_dict("list"))
        print("pipeline", tag, df.shape)
    np.savez_compressed(HERE / "coherence_pipeline.npz", **out)


def case_direct():
    """C: Coherence(settings, ch_names, sfreq).calc_feature on windows."""
    rng = np.random.default_rng(3)
    sfreq = 1000.0
    W = 1000
    t = np.arange(W) / sfreq
    base = np.sin(2 * np.pi * 18 * t)
    x = np.stack([base + 0.5 * rng.standard_normal(W),
                  np.roll(base, 9) * 1e-3 + 0.7e-3 * rng.standard_normal(W),   # quiet and delayed
                  rng.standard_normal(W) * 30 + 500.0,
                  np.full(W, 2.0)])                                          # constant
    names = ["A1", "B1", "C1", "K1"]
    out = {"sfreq": sfreq, "data": x, "ch_names": np.array(names)}
    cases = {
        "n128": dict(nperseg=128),
        "n125": dict(nperseg=125, bands=["low_beta", "high_beta"]),   # (8 Hz bins: theta holds none)
        "n256": dict(nperseg=256),
        "n500_w500": dict(nperseg=500, window=500),
        "n2000": dict(nperseg=2000),
        "icoh_off": dict(nperseg=128, method={"coh": True, "icoh": False}),
        "empty_mean": dict(nperseg=128, bands=["narrow", "high_beta"],
                           features={"mean_fband": True, "max_fband": False, "max_allfbands": True}),
        "constant": dict(nperseg=128, channels=[["A1", "K1"], ["K1", "C1"]]),
    }
    out["cases"] = np.array(list(cases))
    for tag, c in cases.items():
        s = nm.NMSettings.get_default()
        s.reset()
        s.features.coherence = True
        s.frequency_ranges_hz["narrow"] = FrequencyRange(10.2, 10.4)   # (no bin of any grid here strictly inside)
        s.coherence_settings.channels = c.get("channels", [["A1", "B1"], ["B1", "C1"], ["C1", "A1"]])
        s.coherence_settings.nperseg = c["nperseg"]
        s.coherence_settings.frequency_bands = c.get("bands", ["theta", "low_beta", "high_beta"])
        for k, v in c.get("method", {}).items():
            setattr(s.coherence_settings.method, k, v)
        for k, v in c.get("features", {}).items():
            setattr(s.coherence_settings.features, k, v)
        w = c.get("window", W)
        win = x[:, :w]
        res = Coherence(s, names, sfreq).calc_feature(win)
        out[f"{tag}_settings_json"] = dump(s)
        out[f"{tag}_window"] = np.int64(w)
        out[f"{tag}_keys"] = np.array(list(res.keys()))
        out[f"{tag}_values"] = np.array([float(v) for v in res.values()], dtype=np.float64)
        print("direct", tag, len(res))
    np.savez_compressed(HERE / "coherence_direct.npz", **out)


def case_reference_test():
    """D: tests/test_coherence.py's setting (sfreq 500, nperseg 500, signal / noise bands, mean_fband only) on a NumPy
    signal with a 5-sample coupling delay (in place of mne_connectivity.make_signals_in_freq_bands; the band MEAN of icoh
    is tested, so the delay keeps the cross-spectrum's phase on one side across the band).  The default
    pre-processing resamples the 500 Hz recording to 1000 Hz while the features stay designed for 500 Hz (the reference's
    raw-resampling quirk, stream/data_processor.py): the labelled frequency axis is half the true one, so the coupled
    component is put at true 30 - 40 Hz, where the "signal" band (15 - 20 Hz) reads it.  The re-reference is off: of two
    channels, a common average or a bipolar pair leaves mirror images (icoh = 0 everywhere)."""
    sfreq = 500.0
    T = 5000
    rng = np.random.default_rng(44)
    shared = bandlimited(rng, T + 5, sfreq, 30, 40)
    seed = 0.9 * shared[5:] + 0.2 * bandlimited(rng, T, sfreq, 1, 249)
    target = 0.9 * shared[:T] + 0.2 * bandlimited(rng, T, sfreq, 1, 249)
    data = np.stack([seed, target])
    # (no re-reference: of two channels, a common average or a bipolar pair leaves mirror images, icoh = 0)
    channels = nm.utils.set_channels(ch_names=["seed", "target"], ch_types=["eeg", "eeg"], reference=None,
                                     bads=None, new_names="default", used_types=("eeg",), target_keywords=None)
    s = nm.NMSettings.get_default()
    s.reset()
    s.features.coherence = True
    s.frequency_ranges_hz = {
        "signal": {"frequency_low_hz": 15, "frequency_high_hz": 20},
        "noise_low": {"frequency_low_hz": 1, "frequency_high_hz": 11},
        "noise_high": {"frequency_low_hz": 24, "frequency_high_hz": 249},
    }
    s.coherence_settings.frequency_bands = ["signal", "noise_low", "noise_high"]
    s.coherence_settings.nperseg = 500
    s.coherence_settings.features = {"mean_fband": True, "max_fband": False, "max_allfbands": False}
    s.coherence_settings.channels = [["seed", "target"]]
    s.postprocessing.feature_normalization = False
    st = nm.Stream(settings=s, channels=channels, sfreq=sfreq, verbose=False)
    with tempfile.TemporaryDirectory() as td:
        df = st.run(data, out_dir=td, experiment_name="test_coherence", save_csv=False)
    res = {k: np.abs(df[k].values).mean() for k in df.columns if k != "time"}
    node = "icoh_seed_to_target_mean_fband_"
    assert res[node + "signal"] > res[node + "noise_low"] and res[node + "signal"] > res[node + "noise_high"]
    out = {"sfreq": sfreq, "data": data, "settings_json": dump(st.settings),
           "channels_json": json.dumps(st.channels.to_dict("list")), "columns": np.array(list(df.columns)),
           "values": df.to_numpy(dtype=np.float64)}
    np.savez_compressed(HERE / "coherence_reftest.npz", **out)
    print("reference test", df.shape)


if __name__ == "__main__":
    case_pipeline()
    case_direct()
    case_reference_test()
