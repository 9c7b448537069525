"""Recording generator of the long-window sharp-wave cases: tests/golden/make_golden_sharpwave_long.py feeds the
reference with it, the tests regenerate the same inputs from the seeds in tests/golden/sharpwave_long.npz."""

import numpy as np

HOPS = 5


def recording(seed: int, sfreq: int, kind: str, hops: int = HOPS) -> np.ndarray:
    """(2, W + (hops - 1) W / 10) float64, exactly representable in float32.  "walk": a slow random walk + white noise +
    11 Hz and 47 Hz tones (the same spectrum at every rate: the walk's step shrinks with the root of the rate);
    "white": unit white noise; "fast": see below."""
    rng = np.random.default_rng(seed)
    T = sfreq + (hops - 1) * (sfreq // 10)
    t = np.arange(T) / sfreq
    if kind == "white":
        x = rng.standard_normal((2, T))
    elif kind == "fast":
        # tones near the upper edge of each default pass band (25 Hz, 70 Hz) + white noise, no drift: at 30 kHz the two
        # samples around an extremum differ by A (w dt)^2 |1/2 - d| (d: where the true extremum falls between them) --
        # with slow in-band activity that is within fp32 rounding of the FIR output for several extrema per window, and
        # order / variance estimators of the time-like features move by far more than 1e-5 with each of them
        x = rng.standard_normal((2, T)) * 0.5 + 6 * np.sin(2 * np.pi * 25 * t + 0.3) + 3 * np.sin(2 * np.pi * 70 * t + 1.0)
    else:
        x = np.cumsum(rng.standard_normal((2, T)), axis=1) * (0.05 * np.sqrt(7000.0 / sfreq)) + rng.standard_normal((2, T)) * 0.5
        x += 6 * np.sin(2 * np.pi * 11 * t) + 3 * np.sin(2 * np.pi * 47 * t + 1.0)
    return x.astype(np.float32).astype(np.float64)
