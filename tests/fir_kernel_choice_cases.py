"""The plans of tests/golden/fir_kernel_choice.json: the smallest shapes that reach every kernel of the one-wave FIR family
(nmx_w64.hip) and every batch-size threshold of its launch geometry.  tests/golden/make_fir_kernel_choice.py records, and
tests/test_fir_kernel_choice_gpu.py compares, the kernels a batch launched (stages 1, 3 and 6) and the SHA-256 of the
table it returned.  The hashes pin BYTES (a regression check); tests/fir_sample_probe_cases.py pins the VALUES of the same
kernels, sample by sample against float64.

Recordings: fixed-seed noise + a 20 Hz sine + per-channel offsets.  The 1 kHz cases run notch (50 Hz) + common average
reference in front of the default features with bandpass_filter on; the other rates run the band-pass features alone.
Environment selectors are read when a plan is built: `setenv` / `delenv` (monkeypatch's, or os.environ's in the generator)
bracket the engine's construction."""

from __future__ import annotations

import hashlib

import numpy as np

STAGES = (1, 3, 6)

# name -> env, sfreq, window, channels, hops, settings kind, notch
CASES = {
    "default": ({}, 1000.0, 1000, 4, 8, "default", True),
    "default_wide": ({}, 1000.0, 1000, 64, 66, "default", True),
    "nofuse": ({"NMX_NOTCH_SW_FUSE": "0"}, 1000.0, 1000, 4, 8, "default", True),
    "odd_channels": ({}, 1000.0, 1000, 33, 40, "default", True),
    "rate500": ({}, 500.0, 500, 33, 40, "bandpass", False),
    "rate600": ({}, 600.0, 600, 33, 40, "bandpass", False),
    "rate750": ({}, 750.0, 750, 33, 40, "bandpass", False),
    "no_pair_e_small": ({"NMX_BANK_W64E": "0"}, 1000.0, 1000, 4, 8, "default", True),
    "no_pair_e_mid": ({"NMX_BANK_W64E": "0"}, 1000.0, 1000, 64, 66, "default", True),
    "no_pair_e_large": ({"NMX_BANK_W64E": "0"}, 1000.0, 1000, 256, 96, "default", True),
    "no_pair_c": ({"NMX_BANK_W64C": "0"}, 1000.0, 1000, 64, 66, "default", True),
    "bp_hjorth": ({}, 1000.0, 1000, 64, 66, "hjorth", True),
    "w901": ({"NMX_BANK_W64E": "0"}, 1000.0, 901, 64, 66, "w901", True),
    "notch_generic": ({}, 800.0, 800, 8, 16, "low_bands", True),
    "x2_half": ({}, 2000.0, 2000, 8, 8, "bandpass", False),
    "x2_full": ({}, 2500.0, 2500, 8, 8, "bandpass", False),
    "filter_window": ({}, 1000.0, 1000, 4, 1, "default", True),
}


def _settings(kind, window):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    if kind in ("bandpass", "w901"):
        s.features.disable_all()
    s.features.bandpass_filter = True
    if kind == "hjorth":
        s.bandpass_filter_settings.bandpower_features.mobility = True
    if kind == "w901":   # (an odd window: the band-pass segments may not be longer than it)
        s.features.sharpwave_analysis = True
        s.segment_length_features_ms = window
        s.bandpass_filter_settings.segment_lengths_ms = {"theta": window, "alpha": 500, "low_beta": 333, "high_beta": 333}
    if kind == "low_bands":   # (800 Hz: the bands that end below its Nyquist frequency)
        s.frequency_ranges_hz = {k: v for k, v in s.frequency_ranges_hz.items() if v[1] < 100}
    return s.validate()


def recording(name):
    _, sfreq, W, C, n_hops, _, _ = CASES[name]
    hop = int(sfreq / 10)
    T = W + (n_hops - 1) * hop
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    t = np.arange(T) / sfreq
    x = rng.standard_normal((C, T)) * 50 + 10 * np.sin(2 * np.pi * 20 * t) + rng.uniform(-300, 300, (C, 1))
    return x.astype(np.float32), np.arange(n_hops) * hop


def run_case(lib, name, setenv, delenv):
    """{"kernels_1", "kernels_3", "kernels_6", "sha256"} of case `name` on library `lib`."""
    from py_neuromodulation_amd import fir_design
    from py_neuromodulation_amd.engine import HotPathEngine

    env, sfreq, W, C, _, kind, notch = CASES[name]
    x, starts = recording(name)
    R = np.full((C, C), -1.0 / (C - 1))
    np.fill_diagonal(R, 1.0)
    for k, v in env.items():
        setenv(k, v)
    try:
        eng = HotPathEngine(_settings(kind, W), [f"ch{i}_avgref" for i in range(C)], sfreq, lib=lib,
                            ref_matrix=R if notch else None, notch_taps=fir_design.notch_bank(sfreq, 50) if notch else None)
    finally:
        for k in env:
            delenv(k)
    try:
        if name == "filter_window":
            got = eng.filter_window(x.astype(np.float64))
        else:
            got = eng.process_batch(x, starts)
            assert got.dtype == np.float32
        out = {f"kernels_{i}": eng.kernels(i) for i in STAGES}
    finally:
        eng.close()
    out["sha256"] = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()
    return out
