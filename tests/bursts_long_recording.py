"""Recordings of the long-window `bursts` cases: tests/golden/make_golden_bursts_long.py feeds the reference with them, the
tests regenerate the same inputs from the parameters in tests/golden/bursts_long.npz.  NumPy only.

A burst feature counts the samples at or above a percentile of the envelope's own history, and the cases want every such
decision further from its threshold than fp32 moves it (tests/bursts_long_cases.py: MARGIN).  The expected number of
samples within d of the threshold is window x d x (density of the envelope's values at the threshold): any envelope with a
smooth distribution -- noise, a modulated tone -- has dozens of them per case at d = 1e-5 of the amplitude, whatever the
seed.  So the envelopes here are TWO-LEVEL: one carrier per burst band, gated on for a quarter of the time, over a little
white noise.  The 75th percentile of such a history falls between the levels, on the gate's edges, which are as steep as the
band allows; the seed moves the carriers' phases and the noise, i.e. where the samples fall on those edges."""

import numpy as np


def n_samples(p: dict) -> int:
    """One window and p["hops"] - 1 hops of sfreq / feat_hz samples behind it."""
    return int(p["window"] + np.ceil((p["hops"] - 1) * p["sfreq"] / p.get("feat_hz", 10)))


def gate(p: dict, t: np.ndarray, rng) -> np.ndarray:
    """1 where the carriers are on: p["gate_width"] seconds in the middle of every p["gate_period"] seconds (the windows end on
    multiples of the period: their ends, where the filter and the length-W Hilbert transform see a cut, lie in the gaps),
    every pulse moved by up to p["gate_jitter"] seconds either way: its edges then fall differently between the samples, and
    the history's order statistics around the threshold are spread over the edge instead of repeating one pulse's values."""
    k = np.floor(t / p["gate_period"]).astype(np.int64)
    jit = rng.uniform(-1.0, 1.0, int(k[-1]) + 1) * p.get("gate_jitter", 0.0)
    lo = k * p["gate_period"] + 0.5 * (p["gate_period"] - p["gate_width"]) + jit[k]
    return ((t >= lo) & (t < lo + p["gate_width"])).astype(np.float64)


def recording(p: dict) -> np.ndarray:
    """(p["n_ch"], n_samples(p)) float64, exactly representable in float32: per channel c, p["amps"][c] x 100 x gate x the sum
    of unit carriers at p["carriers"] Hz (one per burst band; the same phases and the same gate in every channel, so that a common
    average reference leaves every channel a two-level envelope), growing to (1 + p["growth"]) times the first amplitude, + white
    noise of p["noise"] x 100 + a constant per channel."""
    rng = np.random.default_rng(int(p["seed"]))
    sfreq, T, C = float(p["sfreq"]), n_samples(p), int(p["n_ch"])
    t = np.arange(T) / sfreq
    tone = np.zeros(T)
    for f0 in p["carriers"]:
        tone += np.sin(2 * np.pi * f0 * t + rng.uniform(0, 2 * np.pi))
    tone *= gate(p, t, rng) * (1 + p.get("growth", 0.0) * t / t[-1])
    x = 100.0 * np.asarray(p["amps"], np.float64)[:, None] * tone + 100.0 * p["noise"] * rng.standard_normal((C, T))
    x += rng.uniform(-20, 20, (C, 1))
    return x.astype(np.float32).astype(np.float64)
