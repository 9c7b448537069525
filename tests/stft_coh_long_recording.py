"""Recordings of the long-window STFT / coherence cases: tests/golden/make_golden_stft_coh_long.py feeds the reference with
them, the tests regenerate the same inputs from the parameters in tests/golden/stft_coh_long.npz.  NumPy only.

STFT cases: tests/timeosc_long_recording.py's case_recording (two channels, five hops).  Coherence cases: coh_recording."""

import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("_timeosc_long_recording", Path(__file__).with_name("timeosc_long_recording.py"))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
HOPS, case_recording = _rec.HOPS, _rec.case_recording


def coh_recording(p: dict) -> np.ndarray:
    """(p["n_ch"], window + (hops - 1) sfreq / 10) float64, exactly representable in float32: unit white noise per channel
    plus a white component SHARED by all channels, delayed by 3 i samples in channel i and weighted p["mix"][i] -- so that
    coherence is neither 0 nor 1 and its imaginary part is not 0.  (White throughout: every bin then sits at the level of
    the segment energy, where tests/coherence_oracle.py's conditioning bound is below 1e-5.)  `const`: (channel, hop) whose
    window -- and every sample behind it -- holds one value."""
    rng = np.random.default_rng(p["seed"])
    T = p["window"] + int(np.ceil((p["hops"] - 1) * p["sfreq"] / 10))
    shared = rng.standard_normal(T + 64)
    x = rng.standard_normal((p["n_ch"], T))
    for i, g in enumerate(p["mix"]):
        x[i] += g * shared[3 * i:3 * i + T]
    x = x + np.asarray(p.get("offsets", [0.0] * p["n_ch"]), np.float64)[:, None]
    if "const" in p:
        c, hop = p["const"]
        x[c, int(hop * p["sfreq"] / 10):] = 0.25
    return x.astype(np.float32).astype(np.float64)
