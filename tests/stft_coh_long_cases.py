"""STFT and coherence on windows above 16 384 samples (opt-in: NMX_LONG_STFT=1, NMX_LONG_COHERENCE=1, read when the plan is
built): the cases of tests/golden/stft_coh_long.npz and the checks around them, shared by the emulator tier
(test_stft_coh_long_cpu.py) and the MI355X tier (test_stft_coh_long_gpu.py).  The recordings come from
tests/stft_coh_long_recording.py (the fixture stores generator parameters, not recordings).

STFT cases: Stream.run on 2 channels x 5 hops, sampling_rate_features_hz = 10, no normaliser; the table is compared with the
reference's (the fixture) AND with oracle.run_stream under tests/parity.compare -- the 1e-5 policy, a miss accepted only on
the conditioning report of the float64 restatement (a PipelineVerifiers row), as timeosc_long_cases.run_case does.  Per-bin
probes: spectral_probe_cases.probe on white noise, one single-bin band per probe; they accept nothing.

Coherence cases: judged with tests/coherence_oracle.py on the engine's own pre-processed windows (process_batch(...,
tap=True)), as tests/test_coherence_gpu.py does: 1e-5 absolute plus the per-entry bound, max_allfbands exact unless the
float64 maximum is a tie.

Caps on accepted misses -- conditions of this change, not measurements: per case at most STFT_CAP (1 %) of the case's stft
entries and COH_CAP (2 %) of its coherence entries; the probes none.  `stft_ill_conditioned` / the `ill` count of `coh_case`
are the float64 oracle's OWN counts of entries that could be forgiven (an STFT entry with a bin below FP32_BIN_EPS of the
segment's white-noise level; a coherence entry whose bound exceeds 1e-5): the emulator tier asserts that they stay within
the same caps, so that the device tier cannot pass by forgiving."""

from __future__ import annotations

import json
import os

import numpy as np

from tests import coherence_oracle as coh_oracle
from tests import parity
from tests import spectral_probe_cases as sp
from tests.stft_coh_long_recording import HOPS, case_recording, coh_recording  # noqa: F401

STFT_TAGS = ["s16400", "s30k", "s40k_mid", "s2k_20s", "s_odd", "s_short", "s_psd"]
STFT_CAP, COH_CAP = 0.01, 0.02
ENV_STFT = {"NMX_LONG_STFT": "1"}
ALL_SWITCHES = ("NMX_LONG_BURSTS", "NMX_LONG_BANDPOWER", "NMX_LONG_STFT", "NMX_LONG_COHERENCE")

# the kernel of each segment class (nmx_timeosc_long.hip)
K_WAVE500 = "nmx_kern_timeosc_long_stft<NMX_TOL_STFT_WAVE500>"
K_DIRECT = "nmx_kern_timeosc_long_stft<NMX_TOL_STFT_DIRECT>"
K_LDS = "nmx_kern_timeosc_long_stft<NMX_TOL_STFT_LDS>"
K_SPLIT = "nmx_kern_timeosc_long_stft<NMX_TOL_STFT_SPLIT>"
KERNEL_OF = {"s16400": K_WAVE500, "s30k": K_WAVE500, "s40k_mid": K_LDS, "s2k_20s": K_SPLIT, "s_odd": K_LDS, "s_short": K_DIRECT,
             "s_psd": K_WAVE500}


def load_case(tag):
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("stft_coh_long")
    p = json.loads(str(g["params_json"]))[tag]
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def _accepted_since(before):
    after = parity.STATS["forgiven"]
    return {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}


def _against(tag, name, cols, got, ref, s, sfreq, x, W, pv):
    amp = float(np.nanmax(np.abs(x)))
    for i in range(got.shape[0]):
        n_bad, rep, worst = parity.compare(cols[:-1], got[i, :-1], ref[i, :-1], s, sfreq, amp, W, verifier=pv.row(i))
        print(f"{tag} vs {name} hop {i}: {n_bad} bad, worst relative error {worst}")
        assert n_bad == 0, f"{tag} vs {name} hop {i}\n{rep}"


def _oracle_table(x, sfreq, s, ch, cols):
    from oracle import nm_oracle as orc

    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    assert [list(r) for r in rows] == [cols] * len(rows)
    tab = np.array([[r[c] for c in cols] for r in rows])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    return tab, starts, ends


def n_stft(cols, rows):
    return rows * sum("_stft_" in c for c in cols)


def check_stft_cap(tag, acc, cols, rows, only_stft=True):
    cap = int(STFT_CAP * n_stft(cols, rows))
    print(f"{tag}: stft misses accepted {acc.get('stft', 0)} of {n_stft(cols, rows)} entries, cap {cap}")
    if only_stft:
        assert set(acc) <= {"stft"}, (tag, acc)
    assert acc.get("stft", 0) <= cap, (tag, acc, cap)


def run_stft(lib, tag, s, ch, cols, sfreq, x, W, want=None, kernel=None):
    """Stream.run against the fixture table `want` (when given) and oracle.run_stream.  -> (accepted per family, rows, oracle
    table, the PipelineVerifiers)."""
    from py_neuromodulation_amd.stream import Stream

    st = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib))
    df = st.run(x, save_csv=False)
    if kernel is not None and lib is None:   # (the emulator names no kernels)
        names = st.data_processor.engine.kernels(2)
        assert kernel in names.split(" + "), f"{tag}: wanted {kernel}, ran {names}"
    if cols is None:
        cols = list(df.columns)
    assert list(df.columns) == cols, tag
    got = df.to_numpy(float)
    tab, starts, ends = _oracle_table(x, sfreq, s, ch, cols)
    assert got.shape == tab.shape, tag
    np.testing.assert_array_equal(got[:, -1], tab[:, -1])
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = dict(parity.STATS["forgiven"])
    if want is not None:
        assert got.shape == want.shape, tag
        _against(tag, "fixture", cols, got, want, s, sfreq, x, W, pv)
    _against(tag, "oracle", cols, got, tab, s, sfreq, x, W, pv)
    acc = _accepted_since(before)
    return acc, got, tab, pv, cols


def run_case(lib, tag):
    """A fixture case.  -> (accepted misses per family, the rows)."""
    p, s, ch, cols, want = load_case(tag)
    sfreq = float(p["sfreq"])
    x = case_recording(p)
    W = int(sfreq * s.segment_length_features_ms / 1000)
    assert W == p["window"] >= 16400 and int(s.stft_settings.windowlength_ms) == p["nperseg"]
    acc, got, _, _, _ = run_stft(lib, tag, s, ch, cols, sfreq, x, W, want=want, kernel=KERNEL_OF[tag])
    # (s30k: fft, welch and the time-domain families ride along; theirs is tests/timeosc_long_cases.py's policy: none accepted
    # in the emulator, fft + welch on a conditioning report on the device)
    check_stft_cap(tag, acc, cols, got.shape[0], only_stft=False)
    assert set(acc) <= {"stft", "fft", "welch"}, (tag, acc)
    return acc, got


def stft_ill_conditioned(tag):
    """The float64 oracle's own count for a fixture case: stft entries (band estimators and psd keys) that hold a bin below
    FP32_BIN_EPS of the white-noise level of its segment's samples -- the entries parity.Verifier.spectral could forgive
    outright.  -> (count, entries)."""
    from oracle import nm_oracle as orc

    p, s, ch, cols, _ = load_case(tag)
    sfreq = float(p["sfreq"])
    x = case_recording(p)
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, p["window"], line_noise=50, ends=ends)
    keys = [c for c in cols if "_stft_" in c]
    ill = 0
    for i in range(len(starts)):
        v = pv.row(i)
        for ci in range(x.shape[0]):
            mag, idx_range, freqs, gain = orc.spectral_magnitudes("stft", s, sfreq, v.x[ci])
            floor = gain * v._rms(ci) * parity.FP32_BIN_EPS
            low = np.abs(np.asarray(mag, np.float64)) < floor          # [bin, segment]
            bad_bins = low.any(axis=-1) if low.ndim == 2 else low
            for k in keys:
                kc, rest = parity._split_key(k, v.ch)
                if kc != ci:
                    continue
                rest = rest[len("stft") + 1:]
                if rest.startswith("psd_"):
                    idx = [b for b, fr in enumerate(freqs) if int(fr) == int(rest[4:])]
                else:
                    idx = dict(idx_range)[rest.rsplit("_", 1)[0]]
                ill += bool(np.any(bad_bins[np.asarray(idx, dtype=int)])) if len(idx) else 0
    return ill, n_stft(cols, len(starts))


def nan_case(lib):
    """s30k with NaN samples in channel 0 of two hops: the NaN pattern equals the oracle's, and the other channel's values are
    the ones of the clean run."""
    p, s, ch, cols, _ = load_case("s30k")
    sfreq, W = float(p["sfreq"]), p["window"]
    x = case_recording(p)
    hop = W // 10
    xn = x.copy()
    xn[0, W + hop + 100:W + hop + 140] = np.nan
    xn[0, W + 50:W + 60] = np.nan
    acc, got, tab, _, _ = run_stft(lib, "s30k nan", s, ch, cols, sfreq, xn, W)
    assert np.array_equal(np.isnan(got), np.isnan(tab)), "NaN pattern differs from the oracle's"
    ch1 = [j for j, c in enumerate(cols) if c.startswith("ch1")]
    assert np.isnan(got[:, [j for j, c in enumerate(cols) if c.startswith("ch0")]]).any()
    return acc, got[:, ch1], ch1, cols


def notch_reref_case(lib):
    """s30k's recording behind notch_filter + re_referencing (the default channels' common average)."""
    p, s, ch, _, _ = load_case("s30k")
    from py_neuromodulation_amd import NMSettings

    s = NMSettings(**s.to_dict())
    s.preprocessing = ["notch_filter", "re_referencing"]
    sfreq, W = float(p["sfreq"]), p["window"]
    x = case_recording(p)
    x = np.concatenate([x, case_recording(dict(p, seed=p["seed"] + 1))[:1]])   # (of two channels the average leaves mirror images)
    from py_neuromodulation_amd import channels as chmod

    ch3 = chmod.get_default_channels_from_data(x)
    acc, got, _, _, cols = run_stft(lib, "s30k notch + reref", s, ch3, None, sfreq, x, W, kernel=K_WAVE500)
    check_stft_cap("s30k notch + reref", acc, cols, got.shape[0], only_stft=False)
    return acc


def process_equals_run(lib, run_rows):
    """DataProcessor.process window by window gives the Stream.run rows of s30k (1e-6 relative: the tolerance between call
    shapes used throughout tests/parity_cases.py)."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.data_processor import DataProcessor

    p, s, ch, cols, _ = load_case("s30k")
    sfreq = float(p["sfreq"])
    x = case_recording(p)
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    dp = DataProcessor(sfreq=sfreq, settings=s, channels=ch, line_noise=50, **_kw(lib))
    feat = [c for c in cols if c != "time"]
    for i, (a, b) in enumerate(zip(starts, ends)):
        row = dp.process(x[:, a:b])
        assert list(row) == feat
        np.testing.assert_allclose(np.array(list(row.values()), float), run_rows[i, :len(feat)], rtol=1e-6, atol=0,
                                   err_msg=f"hop {i}")


# ---- per-bin probes ---------------------------------------------------------------------------------------------------------
def probe_500(lib, sfreq):
    """Bins 1, 2, 124, 125, 126, 248, 249 of the 500-sample segments on a window of `sfreq` samples."""
    acc, worst = sp.probe(lib, float(sfreq), 1000, ["stft"], sp.STFT_BINS, grid="stft", stft_ms=500, seed=sfreq + 500, env=ENV_STFT,
                          kernel=K_WAVE500.split("<")[0], tag=f"long stft 500 at {sfreq}")
    assert acc == {}, acc
    return worst


def probe_split(lib):
    """spread_bins(20 000) of one 20 000-sample segment class (D = 2): 2 kHz, 20 s windows."""
    assert sp.long_split(20000) == 2
    acc, worst = sp.probe(lib, 2000.0, 20000, ["stft"], sp.spread_bins(20000), grid="stft", stft_ms=20000, seed=22000, env=ENV_STFT,
                          kernel=K_SPLIT.split("<")[0], tag="long stft split 20000")
    assert acc == {}, acc
    return worst


# ---- coherence ----------------------------------------------------------------------------------------------------------------
COH_CASES = {
    "c16400": {"seed": 1642, "sfreq": 16400, "window": 16400, "n_ch": 2, "hops": 4, "mix": [0.8, 0.6], "nperseg": 256,
               "pairs": [["ch0", "ch1"]], "bands": {"mid": [200, 400], "wide": [100, 5000]}},
    "c40k": {"seed": 4021, "sfreq": 40000, "window": 40000, "n_ch": 2, "hops": 3, "mix": [0.7, 0.9], "nperseg": 4096,
             "pairs": [["ch0", "ch1"]], "bands": {"mid": [200, 400], "wide": [100, 5000]}, "feats": ["mean_fband", "max_allfbands"]},
    "c20k_pre": {"seed": 2031, "sfreq": 20000, "window": 20000, "n_ch": 3, "hops": 4, "mix": [0.8, 0.6, 0.4], "nperseg": 300,
                 "pairs": [["ch0", "ch1"], ["ch2", "ch0"]], "bands": {"mid": [200, 400], "wide": [100, 5000]},
                 "pre": ["notch_filter", "re_referencing"]},
    "c_const": {"seed": 2041, "sfreq": 20000, "window": 20000, "n_ch": 2, "hops": 3, "mix": [0.8, 0.6], "nperseg": 256,
                "pairs": [["ch0", "ch1"]], "bands": {"mid": [200, 400], "wide": [100, 5000]}, "const": [1, 2]},
}


def coh_settings(p):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = list(p.get("pre", []))
    s.postprocessing.feature_normalization = False
    s.features.coherence = True
    for name, (lo, hi) in p["bands"].items():
        s.frequency_ranges_hz[name] = [lo, hi]
    s.coherence_settings.channels = p["pairs"]
    s.coherence_settings.nperseg = p["nperseg"]
    s.coherence_settings.frequency_bands = list(p["bands"])
    s.coherence_settings.method = {"coh": True, "icoh": True}
    feats = p.get("feats", ["mean_fband", "max_fband", "max_allfbands"])
    s.coherence_settings.features = {f: f in feats for f in ("mean_fband", "max_fband", "max_allfbands")}
    return s


def plain_channels(n):
    names = [f"ch{i}" for i in range(n)]
    return {"name": names, "rereference": ["None"] * n, "used": [1] * n, "target": [0] * n, "type": ["ecog"] * n,
            "status": ["good"] * n, "new_name": list(names)}


def coh_case(lib, tag, p=None, s=None, ch=None, cols=None, want=None):
    """Stream.run of a coherence plan; every coh_ / icoh_ entry against the float64 restatement on the engine's own
    pre-processed windows (and against the fixture table `want` when given).
    -> {"accepted", "ill" (entries whose float64 bound exceeds 1e-5), "entries", "nan" (NaN entries), "rows"}."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.stream import Stream

    p = COH_CASES[tag] if p is None else p
    s = coh_settings(p) if s is None else s
    x = coh_recording(p)
    sfreq = float(p["sfreq"])
    if ch is None:
        ch = chmod.get_default_channels_from_data(x) if "re_referencing" in s.preprocessing else plain_channels(p["n_ch"])
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    if cols is not None:
        assert list(df.columns) == cols, tag
    cols = list(df.columns)
    got = df.to_numpy(float)
    assert got.shape[0] == p["hops"], (tag, got.shape)
    st, _, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    dp = DataProcessor(sfreq, s, ch, line_noise=50, verbose=False, **_kw(lib))
    eng = dp.engine
    try:
        _, pre = eng.process_batch(np.ascontiguousarray(x), np.asarray(st, dtype=np.int64), tap=True)
        names, esf = list(eng.ch_names), eng.sfreq
        pre = np.array(pre, np.float64)
    finally:
        eng.close()
    assert pre.shape[-1] == p["window"], pre.shape
    cs = s.coherence_settings.to_dict()
    ranges = {k: (float(v[0]), float(v[1])) for k, v in s.frequency_ranges_hz.items()}
    coh_cols = [j for j, c in enumerate(cols) if c.startswith(("coh_", "icoh_"))]
    assert coh_cols, cols
    out = {"accepted": 0, "ill": 0, "entries": len(coh_cols) * got.shape[0], "nan": 0, "rows": got, "cols": cols}
    for r in range(got.shape[0]):
        vals, bounds, alts = coh_oracle.features(pre[r], names, esf, cs, ranges, with_bound=True)
        g = {cols[j]: got[r, j] for j in coh_cols}
        assert set(g) == set(vals), (tag, sorted(set(g) ^ set(vals)))
        for name, w in (("restatement", vals),) + ((("fixture", {cols[j]: want[r, j] for j in coh_cols}),) if want is not None else ()):
            misses, accepted = coh_oracle.compare(g, w, bounds, alts)
            assert not misses, f"{tag} row {r} vs {name}: {len(misses)} misses, e.g. {misses[:6]}"
            out["accepted"] += len(accepted) if name == "restatement" else 0
        ill = [k for k in g if "max_allfbands" not in k and not np.isnan(vals[k]) and bounds[k] > 1e-5]
        ill += [k for k in g if "max_allfbands" in k and len(alts.get(k, ())) > 1]
        if ill:
            print(f"{tag} row {r}: ill-conditioned in float64: " + ", ".join(f"{k} (bound {bounds[k]:.2e})" for k in ill))
        out["ill"] += len(ill)
        out["nan"] += sum(1 for k in g if np.isnan(g[k]))
    cap = int(COH_CAP * out["entries"])
    print(f"{tag}: coherence entries {out['entries']}, accepted {out['accepted']}, ill-conditioned in float64 {out['ill']}, cap {cap}, "
          f"NaN {out['nan']}")
    assert out["accepted"] <= cap, (tag, out["accepted"], cap)
    return out


def coh_fixture_case(lib):
    p, s, ch, cols, want = load_case("c30k")
    return coh_case(lib, "c30k", p=p, s=s, ch=ch, cols=cols, want=want)


# ---- the gate -------------------------------------------------------------------------------------------------------------------
# nmx_plan_create's refusal at the parent commit (nmx_engine_abi.inc), for the four settings of the two older switches: (bursts,
# bandpower) -> text
_HEAD = "window must be in [4, 16 384] samples for a plan with "
_MID = " run up to 40 000 samples, behind re-referencing and FIR pre-processing"
PARENT_MESSAGES = {
    (False, False): _HEAD + "stft, bandpass_filter, bursts, coherence, raw_normalization or raw_resampling; only raw_hjorth, return_raw, "
    "linelength, fft, welch and sharpwave_analysis" + _MID +
    " (bursts too with NMX_LONG_BURSTS=1 in the environment, bandpass_filter with NMX_LONG_BANDPOWER=1)",
    (True, False): _HEAD + "stft, bandpass_filter, coherence, raw_normalization or raw_resampling; only raw_hjorth, return_raw, "
    "linelength, fft, welch, sharpwave_analysis and bursts" + _MID + " (bandpass_filter too with NMX_LONG_BANDPOWER=1 in the environment)",
    (False, True): _HEAD + "stft, bursts, coherence, raw_normalization or raw_resampling; only raw_hjorth, return_raw, "
    "linelength, fft, welch, sharpwave_analysis and bandpass_filter" + _MID + " (bursts too with NMX_LONG_BURSTS=1 in the environment)",
    (True, True): _HEAD + "stft, coherence, raw_normalization or raw_resampling; only raw_hjorth, return_raw, "
    "linelength, fft, welch, sharpwave_analysis, bursts and bandpass_filter" + _MID,
}


def _plain(*features):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    for f in features:
        setattr(s.features, f, True)
    if "coherence" in features:
        s.coherence_settings.channels = [["ch0", "ch1"]]
        s.frequency_ranges_hz["wide"] = [100, 400]
        s.coherence_settings.frequency_bands = ["wide"]
    return s


def _run(lib, sfreq, s):
    from py_neuromodulation_amd.stream import Stream

    n = int(sfreq)
    x = np.random.default_rng(1).standard_normal((2, n + n // 10)).astype(np.float32).astype(np.float64)
    return Stream(float(sfreq), data=x, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)


def _message(lib, sfreq, s):
    import pytest

    with pytest.raises(ValueError) as e:
        _run(lib, sfreq, s)
    return str(e.value)


def gate_closed(lib, setenv, delenv, feature, var):
    """With `var` unset a 20 000-sample plan with `feature` is refused, naming 16 384 and the variable; with it set -- and a
    feature that stays limited beside it -- `feature` sits behind the ';'."""
    for v in ALL_SWITCHES:
        delenv(v, raising=False)
    msg = _message(lib, 20000, _plain("fft", feature))
    assert "16 384" in msg and var + "=1" in msg and feature in msg.split(";")[0], msg
    setenv(var, "1")
    s = _plain("fft", feature)
    s.preprocessing = ["raw_normalization"]
    msg = _message(lib, 20000, s)
    assert feature not in msg.split(";")[0] and feature in msg.split(";")[1] and var not in msg, msg
    assert "raw_normalization or raw_resampling" in msg.split(";")[0], msg


def parent_messages(lib, setenv, delenv):
    """Neither new variable set, a plan without stft and coherence: the text of each setting of the two older switches is the
    parent commit's, byte for byte."""
    for v in ALL_SWITCHES:
        delenv(v, raising=False)
    s = _plain("fft")
    s.preprocessing = ["raw_normalization"]
    for (bursts, bandpower), text in PARENT_MESSAGES.items():
        for var, on in (("NMX_LONG_BURSTS", bursts), ("NMX_LONG_BANDPOWER", bandpower)):
            setenv(var, "1") if on else delenv(var, raising=False)
        assert _message(lib, 20000, s) == "nmx: " + text, (bursts, bandpower)   # (the prefix of the Python wrapper)
    for var in ("NMX_LONG_BURSTS", "NMX_LONG_BANDPOWER"):
        delenv(var, raising=False)


def over_limit_raises(lib):
    import pytest

    for f in ("stft", "coherence"):
        with pytest.raises(ValueError, match="40 000 samples"):
            _run(lib, 40001, _plain(f))


def long_segment_raises(lib):
    """Coherence segments stay at most 4096 samples (after the clamp to the window), with the message plans always got."""
    import pytest

    s = _plain("coherence")
    s.coherence_settings.nperseg = 5000
    with pytest.raises(ValueError, match=r"coherence: nperseg .* must lie in \[2, 4096\]"):
        _run(lib, 20000, s)


def no_split_raises(lib):
    """2 x 9973 samples per segment: no divisor leaves a transform the LDS machinery takes; the refusal names the family."""
    import pytest

    from py_neuromodulation_amd.stream import Stream

    s = _plain("stft")
    s.segment_length_features_ms = 20000   # (2 kHz: 40 000-sample windows; windowlength_ms is taken as samples)
    s.stft_settings.windowlength_ms = 19946
    x = sp.white(3, 2, 40400)
    with pytest.raises(ValueError, match="stft: no supported split of a 19 946-point transform"):
        Stream(2000.0, data=x, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)


def fft_return_spectrum_still_raises(lib):
    import pytest

    s = _plain("fft", "stft")
    s.fft_settings.return_spectrum = True
    with pytest.raises(NotImplementedError, match="fft: return_spectrum"):
        _run(lib, 20000, s)


def _trace_of(lib, s, sfreq, n_ch=2):
    import ctypes

    from py_neuromodulation_amd.engine import HotPathEngine

    W = int(sfreq)
    x = sp.white(77, n_ch, W + 2 * (W // 10)).astype(np.float32)
    eng = HotPathEngine(s, [f"ch{i}" for i in range(n_ch)], float(sfreq), window=W, **_kw(lib))
    try:
        lib.lib.nmx_emu_trace_begin()
        rows = eng.process_batch(x, np.arange(3, dtype=np.int64) * (W // 10)).copy()
        n_text = lib.lib.nmx_emu_trace_end(None, 0)
        buf = ctypes.create_string_buffer(n_text)
        lib.lib.nmx_emu_trace_end(buf, n_text)
    finally:
        lib.lib.nmx_emu_trace_end(None, 0)
        eng.close()
    # (stream and event handles are numbered per process: the operations and their order are the trace)
    ops = [" ".join(ln.split()[:2 if ln.startswith("op ") else 1]) for ln in buf.raw.decode().splitlines()]
    return ops, rows


def below_the_gate_emu(lib, setenv, delenv):
    """Plans of at most 16 384 samples (stft + fft, and coherence; 8000 and 16 000 samples): the emulator's launch trace and
    the rows are the same with the four variables set and unset."""
    out = []
    for sfreq, feats in ((8000, ("fft", "stft")), (16000, ("stft",)), (16000, ("coherence", "raw_hjorth"))):
        res = []
        for on in (False, True):
            for v in ("NMX_LONG_STFT", "NMX_LONG_COHERENCE"):
                setenv(v, "1") if on else delenv(v, raising=False)
            res.append(_trace_of(lib, _plain(*feats), sfreq))
        assert res[0][0] == res[1][0], (sfreq, feats)
        assert res[0][1].tobytes() == res[1][1].tobytes(), (sfreq, feats)
        assert "op be_launch_timeosc" in res[0][0], res[0][0]
        out.append(res[0][0])
    return out


def below_the_gate_kernels(setenv, delenv):
    """The device tier's form: kernel names of stages 2 and 7 and the rows, with and without the variables."""
    from py_neuromodulation_amd.engine import HotPathEngine

    for sfreq, feats in ((8000, ("fft", "stft")), (16000, ("stft",)), (16000, ("coherence", "raw_hjorth"))):
        res = []
        for on in (False, True):
            for v in ("NMX_LONG_STFT", "NMX_LONG_COHERENCE"):
                setenv(v, "1") if on else delenv(v, raising=False)
            W = int(sfreq)
            eng = HotPathEngine(_plain(*feats), ["ch0", "ch1"], float(sfreq), window=W)
            try:
                rows = eng.process_batch(sp.white(77, 2, W + 2 * (W // 10)).astype(np.float32), np.arange(3, dtype=np.int64) * (W // 10)).copy()
                res.append((eng.kernels(2), eng.kernels(7), rows.tobytes()))
            finally:
                eng.close()
        assert res[0] == res[1], (sfreq, feats, res[0][:2], res[1][:2])
        assert "long" not in res[0][0], res[0][0]


def stft_16000_goes_long(lib, setenv, delenv):
    """A 16 000-sample plan whose generic layout does not fit LDS (2 kHz, 8 s windows, 8000-sample segments, a band of 3957
    bins x 5 segments beside the window and the two buffers): "needs more than 160 KiB LDS" without the variable, the
    long-window kernel with it, against the oracle."""
    import pytest

    s = _plain("stft")
    s.segment_length_features_ms = 8000
    s.stft_settings.windowlength_ms = 8000
    s.frequency_ranges_hz["broad"] = [1, 990]
    assert not sp.generic_layout_fits(16000, 8000, 3957, 5) and sp.generic_layout_fits(16000, 8000, 1600, 5)
    x = sp.white(160, 2, sp.samples_for(3, 2000.0, 10, 8000))
    delenv("NMX_LONG_STFT", raising=False)
    with pytest.raises(ValueError, match="needs more than 160 KiB LDS"):
        sp.run_and_compare(lib, "stft 16000", 2000.0, s, x)
    setenv("NMX_LONG_STFT", "1")
    acc, _ = sp.run_and_compare(lib, "stft 16000", 2000.0, s, x, kernel=K_LDS.split("<")[0])
    assert acc == {}, acc


# ---- everything in one plan -------------------------------------------------------------------------------------------------------
def all_in_one_plan(lib=None):
    """A 30 kHz stream with 1 s segments -- the reference's default features plus stft and one coherence pair,
    behind notch and re-referencing -- in one plan with the four switches set, against oracle.run_stream under the policy
    (the coherence columns with tests/coherence_oracle.py on the engine's windows)."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd import channels as chmod

    p = {"seed": 3031, "sfreq": 30000, "window": 30000, "n_ch": 3, "hops": 3, "mix": [0.8, 0.6, 0.4]}
    s = NMSettings.get_default()
    s.postprocessing.feature_normalization = False
    s.preprocessing = ["notch_filter", "re_referencing"]
    s.features.stft = True
    s.features.coherence = True
    s.frequency_ranges_hz["mid"] = [200, 400]
    s.frequency_ranges_hz["wide"] = [100, 5000]
    s.coherence_settings.channels = [["ch0", "ch1"]]
    s.coherence_settings.nperseg = 256
    # (no max_fband: bin 3 of the 117 Hz grid lies 1.6 Hz beside the notch's stop band at 350 Hz, its bound is 1.06e-5, and a
    # band maximum carries the largest bound of its bins)
    s.coherence_settings.features = {"mean_fband": True, "max_fband": False, "max_allfbands": True}
    s.coherence_settings.frequency_bands = ["mid", "wide"]
    old = {k: os.environ.get(k) for k in ALL_SWITCHES}
    os.environ.update({k: "1" for k in ALL_SWITCHES})
    try:
        x = coh_recording(p)
        ch = chmod.get_default_channels_from_data(x)
        out = coh_case(lib, "all in one", p=p, s=s, ch=ch)
        cols, got = out["cols"], out["rows"]
        keep = [j for j, c in enumerate(cols) if not c.startswith(("coh_", "icoh_"))]
        kc = [cols[j] for j in keep]
        so = NMSettings(**s.to_dict())   # (the float64 restatement of the stream has no coherence: its columns were judged above)
        so.features.coherence = False
        tab, starts, ends = _oracle_table(x, 30000.0, so, ch, kc)
        pv = parity.PipelineVerifiers(so, ch, 30000.0, x, starts, 30000, line_noise=50, ends=ends)
        before = dict(parity.STATS["forgiven"])
        _against("all in one", "oracle", kc, got[:, keep], tab, so, 30000.0, x, 30000, pv)
        acc = _accepted_since(before)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    check_stft_cap("all in one", acc, cols, got.shape[0], only_stft=False)
    return acc, out
