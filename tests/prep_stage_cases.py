"""The plans of tests/golden/prep_stage.json (GPU) and tests/golden/prep_stage_emu.json (the logic emulator): the smallest
streams that reach every branch of a chunk's front end (re-reference or offset shift: FrontStage, launch_front), of the
pre-processing chain behind it (run_prep_stages: preprocessing_filter, notch, resampler, raw normaliser), of the tap, of the
copy with the offset added back (dc_windows) and of the time / oscillatory, coherence, bank and Kalman launches
(nmx_engine_run.inc: run_chunk; nmx_preprocess_window).  tests/golden/make_fir_kernel_choice.py records (given this module's
name; `--emu` for the emulator's file), tests/test_prep_stage_gpu.py / tests/test_prep_stage_cpu.py compare with equality:

    kernels_1, _2, _3, _7   what the batch launched in the stages pre-processing, time / oscillatory, bank and coherence
    sha256                  one SHA-256 over, in this order: the process_batch table and its NaN mask (and the tapped windows
                            where the case taps), one process_window row on the last window, preprocess_window of the first

Each case: 6 channels, 12 hops, 1 kHz, 1000-sample windows, 100-sample hops unless it says otherwise; fixed-seed noise of
sigma 30 + a 20 Hz sine; per-channel offsets within +-20, or +-5000 (`big`: the learned split engages); float64 input rides
on 1e5 (the host split engages).  A case with `big` and the split on asserts that the plan does carry offsets; a case with
`kernel_2` asserts that the device launched that time / oscillatory kernel."""

from __future__ import annotations

import hashlib

import numpy as np

STAGES = (1, 2, 3, 7)
SFREQ, W, HOP, C, HOPS = 1000.0, 1000, 100, 6, 12
RAGGED = np.array([0, 0, 3, 3, 3, 3, 7, 7, 7, 7, 7, 7])   # starts that are no arithmetic progression: the `starts` path
EMU_KERNELS = "host emulator (tests only)"

TIME = ("raw_hjorth", "return_raw", "linelength")
FE = TIME + ("fft",)
BANDS_35 = {"theta": [4, 8], "alpha": [8, 12], "low beta": [13, 20], "high beta": [20, 35]}   # bins 4 .. 35: the matrix pipe's 32 rows
BANDS_80 = dict(BANDS_35, **{"low gamma": [60, 80]})                                              # ... 4 .. 80: too many for it, all below bin 100


def _car(c):
    R = np.full((c, c), -1.0 / (c - 1))
    np.fill_diagonal(R, 1.0)
    return R


def _struct(c):
    """The reference's "average" rows over two type groups; the last channel is left out of both and passes through."""
    R = np.zeros((c, c))
    for grp in (list(range(0, c // 2)), list(range(c // 2, c - 1))):
        for i in grp:
            for j in grp:
                R[i, j] = 1.0 if i == j else -1.0 / (len(grp) - 1)
    R[c - 1, c - 1] = 1.0
    return R


def _dense(c):
    return np.random.default_rng(5).standard_normal((c, c))


def _pick(c):
    return np.eye(c)[:c - 2]   # a channel pick: C_in != C


def _case(feats, **kw):
    return dict(dict(feats=tuple(feats), ref=None, notch=False, env={}, big=False, f64=False, bad=(), ragged=False, tap=False,
                     kw={}, pre=False, kalman=False, bands=None, window=W, sfreq=SFREQ, channels=C, hops=HOPS, stft_ms=None,
                     kernel_2=None), **kw)


CASES = {
    # 1. front end: the column-sum kernel, the structured kernel, the dense product (twice: C_in != C, and a CAR matrix with
    #    both searches off)
    "car": _case(FE + ("welch", "stft"), ref=_car, notch=True),
    "struct": _case(FE, ref=_struct, notch=True),
    "dense": _case(FE, ref=_dense),
    "pick": _case(FE, ref=_pick, notch=True),
    "car_dense_kernel": _case(FE, ref=_car, env={"NMX_CAR_FAST": "0", "NMX_REREF_STRUCT": "0"}),
    # 2. no re-reference: the features read the caller's samples (hop path, `starts` path); host offsets and the shift with
    #    nanv; learned offsets and the shift in front of the notch
    "raw": _case(FE),
    "raw_ragged": _case(FE, ragged=True),
    "raw_f64_nan_inf": _case(FE + ("stft",), f64=True, bad=((1, 500, np.nan), (2, 1299, np.inf))),
    "notch_learned": _case(FE + ("welch",), notch=True, big=True),
    # 3. offsets through a re-reference
    "car_notch_learned_ragged": _case(FE, ref=_car, notch=True, big=True, ragged=True),
    "car_notch_no_split": _case(FE, ref=_car, notch=True, big=True, ragged=True, env={"NMX_DC_SPLIT": "0"}),
    # 4. consumers that cannot take the offset on load: they read x_dc
    "stft500_offsets": _case(("stft",), ref=_car, big=True, window=600, stft_ms=500, kernel_2="nmx_kern_timeosc_stft500"),
    "w510_offsets": _case(("stft",), ref=_car, big=True, window=1020, stft_ms=510, kernel_2="nmx_kern_timeosc_w510"),
    # 5. time / oscillatory kinds
    "scan": _case(TIME, kernel_2="nmx_kern_scan"),
    "specmm_redo": _case(FE, bands=BANDS_35, bad=((3, 777, np.nan),), kernel_2="nmx_kern_specmm_w1000"),
    "w1000_low": _case(("fft",), bands=BANDS_80, kernel_2="nmx_kern_timeosc_w1000_low"),
    "long": _case(("fft", "raw_hjorth"), ref=_car, window=17000, sfreq=17000.0, channels=2, hops=3, kernel_2="nmx_kern_timeosc_long"),
    # 6. tap
    "tap": _case(FE, ref=_car, notch=True, big=True, tap=True),
    # 7. stages that stop the split
    "resample": _case(FE, ref=_car, kw=dict(resample_from=2000.0)),
    "rawnorm": _case(("return_raw", "raw_hjorth"), ref=_car, notch=True, kw=dict(raw_norm=("zscore", 3, 700, HOP))),
    "prefilter": _case(FE, notch=True, pre=True),
    # 8. coherence: two pairs, with fft
    "coh": _case(("coherence", "fft"), ref=_car, notch=True),
    # 9. bank and Kalman
    "bank_kalman": _case(("bandpass_filter", "fft"), ref=_car, notch=True, big=True, kalman=True),
}


def _settings(c):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    if c["bands"] is not None:
        base = s.to_dict()
        base["frequency_ranges_hz"] = {k: [float(a), float(b)] for k, (a, b) in c["bands"].items()}
        s = NMSettings(**base)
    s.features.disable_all()
    for f in c["feats"]:
        s.features[f] = True
    s.segment_length_features_ms = c["window"] / c["sfreq"] * 1000
    if c["stft_ms"] is not None:
        s.stft_settings.windowlength_ms = c["stft_ms"]
    if "coherence" in c["feats"]:
        s.coherence_settings.channels = [["ch0", "ch1"], ["ch2", "ch3"]]
    if c["kalman"]:
        s.bandpass_filter_settings.kalman_filter = True
    return s.validate()


def recording(name):
    """-> (x[C_in, T], starts, samples per incoming window)"""
    c = CASES[name]
    sf_in = c["kw"].get("resample_from", c["sfreq"])
    wi, hop = int(c["window"] * sf_in / c["sfreq"]), int(sf_in / 10)
    n, ch = c["hops"], c["channels"]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    T = wi + (n - 1) * hop + 7
    x = rng.standard_normal((ch, T)) * 30 + 8 * np.sin(2 * np.pi * 20 * np.arange(T) / sf_in)
    x += rng.uniform(-5e3, 5e3, (ch, 1)) if c["big"] else rng.uniform(-20, 20, (ch, 1))
    if c["f64"]:
        x += 1e5
    for row, t, v in c["bad"]:
        x[row, t] = v
    starts = np.arange(n) * hop
    if c["ragged"]:
        starts = starts + RAGGED
    return (x if c["f64"] else x.astype(np.float32)), starts, wi


def run_case(lib, name, setenv, delenv):
    """{"kernels_1", "kernels_2", "kernels_3", "kernels_7", "sha256"} of case `name` on library `lib`."""
    from py_neuromodulation_amd import fir_design
    from py_neuromodulation_amd.engine import HotPathEngine

    c = CASES[name]
    x, starts, wi = recording(name)
    sf_in = c["kw"].get("resample_from", c["sfreq"])
    R = c["ref"](c["channels"]) if c["ref"] else None
    kw = dict(c["kw"])
    if c["pre"]:
        kw["pre_taps"] = [fir_design.notch_bank(c["sfreq"], 100)]
    for k, v in c["env"].items():
        setenv(k, v)
    try:
        eng = HotPathEngine(_settings(c), [f"ch{i}" for i in range(R.shape[0] if R is not None else c["channels"])], c["sfreq"],
                            lib=lib, ref_matrix=R, notch_taps=fir_design.notch_bank(sf_in, 50) if c["notch"] else None, **kw)
    finally:
        for k in c["env"]:
            delenv(k)
    h = hashlib.sha256()
    try:
        got = eng.process_batch(x, starts, want_nan_mask=True, tap=c["tap"])
        assert len(got) == (3 if c["tap"] else 2) and got[0].shape[0] == c["hops"]
        for a in got:
            h.update(np.ascontiguousarray(a).tobytes())
        kernels = {f"kernels_{i}": eng.kernels(i) for i in STAGES}
        split = c["big"] and c["env"].get("NMX_DC_SPLIT") != "0"
        assert bool(np.any(eng.offsets()[1] != 0.0)) == (split or c["f64"]), f"{name}: offsets carried {eng.offsets()}"
        if c["kernel_2"] and kernels["kernels_2"] != EMU_KERNELS:
            assert kernels["kernels_2"].split("<")[0] == c["kernel_2"], f"{name}: stage 2 ran {kernels['kernels_2']}"
        last = int(starts[-1])
        h.update(eng.process_window(np.asarray(x[:, last:last + wi], dtype=np.float64)).tobytes())
        h.update(np.ascontiguousarray(eng.preprocess_window(np.asarray(x[:, :wi], dtype=np.float64))).tobytes())
    finally:
        eng.close()
    return {**kernels, "sha256": h.hexdigest()}
