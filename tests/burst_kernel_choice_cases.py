"""The plans of tests/golden/burst_kernel_choice.json: the smallest streams that reach every branch of the bursts chain's and
the sharp-wave stage's plan-time choices (BurstStage / SharpStage, nmx_engine_plan_bursts.inc) -- the walk's schedule (fill
phase, workgroup kernel, one-wave walk with its list in LDS or in L2), the Hilbert and run-statistics kinds, and each
selector.  tests/golden/make_fir_kernel_choice.py records (given this module's name), and
tests/test_burst_kernel_choice_gpu.py compares, after every batch of a stream the kernels of stages 4 and 5 (any
`env_tail_rows=` note stripped: the floor a Hilbert launch reads depends on timing) and the SHA-256 of the returned table.

A case is a sequence of process_batch calls on ONE engine.  Recordings: fixed-seed noise + 17 / 27 Hz lines + per-channel
offsets (as in tests/test_burst_env_sparse.py).  Every batch of the small cases has at most 128 hops, so the batch's first
chunk -- the one whose kernels are recorded -- is the whole batch.  Environment selectors are read when a plan is built:
`setenv` / `delenv` (monkeypatch's, or os.environ's in the generator) bracket the engine's construction."""

from __future__ import annotations

import hashlib

import numpy as np

STAGES = (4, 5)

# 1 kHz, 1000-sample windows, 100-sample hops, a 5 s history at the 75th percentile: K = 1251 list entries, and the ring is
# full -- the one-wave walk may start -- at the hop that finds 41 hops absorbed (1000 + 40 x 100 samples)
_RING5 = dict(env={}, sfreq=1000.0, window=1000, channels=2, duration_s=5, kind="bursts_sharp", batches=(30, 30, 30))


def _ring5(**kw):
    return dict(_RING5, **kw)


# batches: hops per process_batch call; a tuple inside stands for that many one-hop calls hashed together
CASES = {
    # fill phase (30 hops); workgroup kernel 11 hops + one-wave walk 19 hops in one chunk; one-wave walk
    "ring5": _ring5(),
    # one hop per call: nw < 2, never a fill launch; the walk changes kernel at call 42
    "ring5_single": _ring5(batches=(1, 1, 1, (45,))),
    # one selector each
    "ring5_no_fill": _ring5(env={"NMX_THR_FILL": "0"}),
    "ring5_no_wave": _ring5(env={"NMX_THR_WAVE": "0"}),
    "ring5_fill_one_launch": _ring5(env={"NMX_FILL_SPLIT": "0"}),
    "ring5_list_l2": _ring5(env={"NMX_THR_LIST_LDS": "0"}),
    "ring5_list_global": _ring5(env={"NMX_THR_LIST_GLOBAL": "1"}),
    "ring5_env_dense": _ring5(env={"NMX_BURST_ENV_SPARSE": "0"}),
    "ring5_sw_list_only": _ring5(env={"NMX_SW_DENSE": "0"}),
    "ring5_overlap0": _ring5(env={"NMX_OVERLAP": "0"}),
    "ring5_overlap1": _ring5(env={"NMX_OVERLAP": "1"}),
    "ring5_overlap2": _ring5(env={"NMX_OVERLAP": "2"}),
    "ring5_chunk9": _ring5(env={"NMX_CHUNK_WINDOWS": "9"}),   # (the ring fills inside the second batch's second chunk: workgroup 2 + one-wave 7 hops)
    # K = 501 <= 1024: the one-wave walk never runs
    "ring2": _ring5(duration_s=2, batches=(30, 30)),
    # the default 30 s history: the fill phase stops at hop 291 and the one-wave walk takes the 9 behind it -- the stream is
    # young: its list in LDS
    "ring30": _ring5(duration_s=30, batches=(300, 8)),
    # an old stream: <2, true> for the launches that start at 4090 and 4094 absorbed hops, <2, false> at 4098
    "old": _ring5(batches=(4090, 4, 4, 4)),
    # more sequences than two rounds of walks with the list in LDS hold (2 x 768 at the default history): the list stays in L2
    # although the stream is young.  (520 channels reach that with three burst bands, 1560 sequences; the default two
    # bands would need 769 channels)
    "wide": _ring5(duration_s=30, channels=520, kind="bursts_3bands", batches=(300, 8)),
    # 2 kHz, 2000-sample windows, 200-sample hops, 5 s history (K = 2501, full at 41 absorbed hops): four registers per lane
    # in the walk, nmx_kern_hilbert_w1000(_sparse), the 32-chunk run statistics
    "rate2000": _ring5(sfreq=2000.0, window=2000),
    # 901-sample windows (the w901 settings of tests/fir_kernel_choice_cases.py, bursts on): the 128-thread Hilbert kernel and the
    # LDS run statistics
    "w901": _ring5(window=901, kind="w901", batches=(30, 30)),
}


def _settings(kind, window, sfreq, duration_s):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bursts = True
    s.features.sharpwave_analysis = kind != "bursts_3bands"
    s.bursts_settings.time_duration_s = duration_s
    if kind == "bursts_3bands":
        s.bursts_settings.frequency_bands = ["alpha", "low_beta", "high_beta"]
    if kind == "w901":   # (an odd window: the band-pass segments may not be longer than it)
        s.features.bandpass_filter = True
        s.segment_length_features_ms = window
        s.bandpass_filter_settings.segment_lengths_ms = {"theta": window, "alpha": 500, "low_beta": 333, "high_beta": 333}
    return s.validate()


def n_hops(name):
    return sum(sum(b) if isinstance(b, tuple) else b for b in CASES[name]["batches"])


def recording(name):
    c = CASES[name]
    sfreq, W, C = c["sfreq"], c["window"], c["channels"]
    hop = int(sfreq / 10)
    T = W + (n_hops(name) - 1) * hop
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    t = np.arange(T) / sfreq
    osc = np.sin(2 * np.pi * 17 * t) + np.sin(2 * np.pi * 27 * t + 0.7)
    x = rng.standard_normal((C, T), dtype=np.float32) * 30 + (3 * osc).astype(np.float32) + rng.uniform(-20, 20, (C, 1)).astype(np.float32)
    return x, hop


def _kernels(eng, stage):
    return ",".join(p for p in eng.kernels(stage).split(",") if not p.startswith("env_tail_rows="))


def run_case(lib, name, setenv, delenv):
    """One entry per batch of case `name` on library `lib`: {"kernels_4", "kernels_5", "sha256"}."""
    from py_neuromodulation_amd.engine import HotPathEngine

    c = CASES[name]
    x, hop = recording(name)
    W = c["window"]
    for k, v in c["env"].items():
        setenv(k, v)
    try:
        eng = HotPathEngine(_settings(c["kind"], W, c["sfreq"], c["duration_s"]), [f"ch{i}" for i in range(c["channels"])],
                            c["sfreq"], lib=lib)
    finally:
        for k in c["env"]:
            delenv(k)
    out, at = [], 0
    try:
        for b in c["batches"]:
            calls = [1] * b[0] if isinstance(b, tuple) else [b]
            h = hashlib.sha256()
            for n in calls:   # (each call gets its own samples, starts from 0: the stream's state lives in the engine)
                seg = np.ascontiguousarray(x[:, at * hop:(at + n - 1) * hop + W])
                got = eng.process_batch(seg, np.arange(n) * hop)
                assert got.dtype == np.float32 and got.shape[0] == n
                h.update(np.ascontiguousarray(got).tobytes())
                at += n
            out.append({**{f"kernels_{i}": _kernels(eng, i) for i in STAGES}, "sha256": h.hexdigest()})
    finally:
        eng.close()
    return out
