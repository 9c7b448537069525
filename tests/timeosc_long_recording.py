"""Recordings of the long-window time / oscillatory cases: tests/golden/make_golden_timeosc_long.py feeds the reference
with them, the tests regenerate the same inputs from the parameters in tests/golden/timeosc_long.npz.  NumPy only."""

import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("_sharpwave_long_recording", Path(__file__).with_name("sharpwave_long_recording.py"))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
HOPS, recording = _rec.HOPS, _rec.recording


def case_recording(p: dict) -> np.ndarray:
    """(2, window + 4 hops of sfreq / 10 samples) float64, exactly representable in float32: `recording` of
    sharpwave_long_recording.py for p["window"] samples per window (its kinds "walk", "white", "fast"; the tones keep their place relative to the window),
    plus a constant per channel (p["offsets"])."""
    T = p["window"] + int(np.ceil((HOPS - 1) * p["sfreq"] / 10))   # five rows at 10 Hz, whatever the rate
    x = recording(p["seed"], p["window"], p["kind"], hops=HOPS + 1)[:, :T]
    x = x + np.asarray(p.get("offsets", [0.0, 0.0]), np.float64)[:, None]
    return x.astype(np.float32).astype(np.float64)
