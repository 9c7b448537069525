"""`bandpass_filter` on windows above 16 384 samples (NMX_LONG_BANDPOWER=1: the partitioned bank with the band-pass power
epilogue from DIFFERENCED TAPS, nmx_kern_bank_diff): the cases of tests/golden/bandpower_long.npz, shared by the emulator tier
(test_bandpower_long_cpu.py) and the MI355X tier (test_bandpower_long_gpu.py).  The recordings are regenerated from seeds
(`recording`; defaults30k: tests/bursts_long_recording.py with the parameters of bursts_long_cases' case of that name, whose
seed keeps the burst decisions clear); the fixture holds settings, channels, columns, the reference's tables and the first
halves of two of its band-pass FIRs.

  tag          window  what it crosses
  odd16385     16 385  odd; the first length behind the gate.  Default bands, three features.  2 ch x 3 hops
  w20k         20 000  20 kHz: default bands, three features, log10, Kalman on theta and low_beta.  2 ch x 4 hops
  w20k_nolog   20 000  ... without log10 and Kalman
  w32704       32 704  the last window with blocks of 2048 samples beside it in LDS.  2 ch x 2 hops
  w32708       32 708  the first with blocks of 1024
  w40k         40 000  the maximum, blocks of 128; two bands: low_beta with a tail of the whole window (1000 ms), and 1 - 3 kHz
                       with the shortest tail the settings hold (1 ms: 40 samples, one to three periods.  Of a default band
                       1 ms is 3 % of a period at most: var(y) of such a tail is what the mean's removal leaves of fp32
                       samples, ill-conditioned in any arithmetic that stores y in fp32 -- below the gate too -- and
                       nothing the policy without a verifier can hold).  2 ch x 2 hops
  defaults30k  30 000  the reference's defaults with raw_resampling off and bandpass_filter on, both opt-ins set: band-pass and
                       burst filters in one bank.  3 ch x 2 hops

Policy.  Every table case is a Stream.run compared with the reference's table (the fixture) AND with oracle.run_stream under
tests/parity.compare WITHOUT a verifier: no miss of the `bandpass` family can be accepted.  A log10 activity near 0 has no
relative precision; the amplitude (sigma 200) keeps the float64 oracle's |log10 activity| above LOG_MARGIN in every case,
asserted from the oracle alone (`log_margin`).  defaults30k follows bursts_long_cases.run_case for the other families
(PipelineVerifiers; the z-score checked stage by stage) and accepts nothing in `bandpass` either.  The offsets case
(oracle only, no reference table) is read with the suite's conditioning verifier, as its other offsets cases are; the device
tier accepts nothing there, the emulator tier one entry at the most.

The emulator sums a variance in ONE float32 accumulator.  Where that alone -- restated in float64 on the exact series
(`_single_accumulator`) -- takes half of tests/parity.tolerances, the entry is left to the device tier, which leaves nothing
out: the long tails of the identity probe, and theta of the constant channel of the special rows (3.4e-5 of its activity in
the emulator, 6e-7 on the MI355X: profiles/bandpower_long.md).  `filter_window_series`: the series outlet of a long plan, the
launch without an output row, sample by sample."""

from __future__ import annotations

import importlib.util
import json
import os
from pathlib import Path

import numpy as np

# (by path: the fixture's generator loads this module next to the reference, whose own `tests` package shadows this one)
_spec = importlib.util.spec_from_file_location("_bursts_long_recording", Path(__file__).with_name("bursts_long_recording.py"))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)

LOG_MARGIN = 0.1
SIGMA = 200.0
FEATS = ("activity", "mobility", "complexity")

CASES = {
    "odd16385": {"seed": 16001, "sfreq": 16385, "window": 16385, "n_ch": 2, "hops": 3},
    "w20k": {"seed": 20001, "sfreq": 20000, "window": 20000, "n_ch": 2, "hops": 4, "kalman": ["theta", "low_beta"]},
    "w20k_nolog": {"seed": 20001, "sfreq": 20000, "window": 20000, "n_ch": 2, "hops": 4, "log": False},
    "w32704": {"seed": 32001, "sfreq": 32704, "window": 32704, "n_ch": 2, "hops": 2},
    "w32708": {"seed": 32002, "sfreq": 32708, "window": 32708, "n_ch": 2, "hops": 2},
    "w40k": {"seed": 40001, "sfreq": 40000, "window": 40000, "n_ch": 2, "hops": 2,
             "bands": {"low_beta": None, "fast": [1000, 3000]}, "seglens_ms": {"low_beta": 1000, "fast": 1}},
    # (bursts_long_cases.CASES["defaults30k"], restated: that module needs this project's package, the generator has none.
    # Its amplitudes of 1 leave log10 activities at 0.04: the recording is scaled by 8)
    "defaults30k": {"seed": 30422, "sfreq": 30000, "window": 30000, "n_ch": 3, "hops": 2, "defaults": True, "amps": [1.0, -1.0, 1.0],
                    "carriers": [17.0, 27.0], "noise": 0.03, "gate_period": 1.0, "gate_width": 0.27, "scale": 8.0},
}
TABLE_CASES = list(CASES)
TAPS_OF = ("w20k", ("theta", "high_beta"))   # the FIRs whose first halves the fixture holds


def recording(p, sigma=SIGMA) -> np.ndarray:
    """float64 [n_ch, T] of exact float32 values: white noise of `sigma`, window + (hops - 1) hops at 10 Hz."""
    if p.get("defaults"):
        return _rec.recording(p) * p["scale"]   # (a power of two: every burst decision of the seed stays what it is)
    T = p["window"] + -(-(p["hops"] - 1) * p["sfreq"] // 10)   # (the hop is sfreq / 10 samples, whole or not)
    return (np.random.default_rng(p["seed"]).standard_normal((p["n_ch"], T)) * sigma).astype(np.float32).astype(np.float64)


def settings_of(nm, p, feats=FEATS):
    """The case's settings on package `nm` (this project's, or the reference's in the fixture's generator)."""
    s = nm.NMSettings.get_default()
    if p.get("defaults"):
        s.preprocessing = [q for q in s.preprocessing if q != "raw_resampling"]
        s.features.bandpass_filter = True
        return s
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.bandpass_filter = True
    s.sampling_rate_features_hz = 10
    s.segment_length_features_ms = 1000
    bp = s.bandpass_filter_settings
    for f in FEATS:
        setattr(bp.bandpower_features, f, f in feats)
    bp.log_transform = bool(p.get("log", True))
    if "bands" in p:
        for k, v in p["bands"].items():   # (None: the default band of that name)
            if v is not None:
                s.frequency_ranges_hz[k] = {"frequency_low_hz": v[0], "frequency_high_hz": v[1]}
        s.frequency_ranges_hz = {k: v for k, v in s.frequency_ranges_hz.items() if k in p["bands"]}
        bp.segment_lengths_ms = {**dict(bp.segment_lengths_ms), **p["seglens_ms"]}
    if "kalman" in p:
        bp.kalman_filter = True
        s.kalman_filter_settings.frequency_bands = list(p["kalman"])
    return s


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def load_case(tag):
    """-> (fixture, parameters, settings, channels, columns, the reference's table)."""
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("bandpower_long")
    p = json.loads(str(g["params_json"]))[tag]
    assert p == CASES[tag], "the fixture was generated from other parameters"
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return g, p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


_ORACLE = {}


def oracle_of(tag):
    """The float64 restatement of a case -- without the z-score where the case has one --, computed once per process and left
    unchanged: (recording, un-normalised settings, columns, table)."""
    if tag not in _ORACLE:
        from oracle import nm_oracle as orc
        from tests.helpers import settings_from_json

        g, p, s, ch, cols, _ = load_case(tag)
        if p.get("defaults"):
            s = settings_from_json(g[f"{tag}_raw_settings_json"])
        x = recording(p)
        x.setflags(write=False)
        rows = orc.run_stream(x, float(p["sfreq"]), s, ch, line_noise=50)
        assert [list(r) for r in rows] == [cols] * p["hops"], tag
        tab = np.array([[r[c] for c in cols] for r in rows])
        tab.setflags(write=False)
        _ORACLE[tag] = (x, s, cols, tab)
    return _ORACLE[tag]


def log_margin(tag) -> float:
    """min |log10 activity| over every hop, channel and band of the float64 oracle's table (inf without log10)."""
    _, s, cols, tab = oracle_of(tag)
    if not s.bandpass_filter_settings.log_transform:
        return float("inf")
    idx = [i for i, c in enumerate(cols) if "_bandpass_activity_" in c]
    assert idx
    return float(np.abs(tab[:, idx]).min())


WORST: dict = {}   # tag -> {family: worst err / tolerance against the oracle} (printed; profiles/bandpower_long.md)


def _against(tag, name, cols, got, ref, s, sfreq, x, W, pv=None, only=None):
    """`only`: the families compared (all of them when None)."""
    from tests import parity

    amp = float(np.nanmax(np.abs(x)))
    ratio = 0.0
    skip = None if only is None else (lambda k: parity.family_of(k) not in only)
    for i in range(got.shape[0]):
        n_bad, rep, _ = parity.compare(cols[:-1], got[i, :-1], ref[i, :-1], s, sfreq, amp, W, skip=skip,
                                       verifier=pv.row(i) if pv else None)
        assert n_bad == 0, f"{tag} vs {name} hop {i}\n{rep}"
        for k, g_, w_ in zip(cols[:-1], got[i, :-1], ref[i, :-1]):
            if parity.family_of(k) == "bandpass" and np.isfinite(w_):
                rtol, atol = parity.tolerances(k, s, sfreq, amp, W)
                ratio = max(ratio, abs(g_ - w_) / (rtol * abs(w_) + atol))
    print(f"{tag} vs {name}: {got.shape[0]} rows, worst bandpass err / tolerance {ratio:.3f}")
    WORST.setdefault(tag, {})[name] = ratio


def run_case(lib, tag):
    """Stream.run of case `tag` on library `lib` against the fixture and the oracle.  -> the engine's (un-normalised) rows."""
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    g, p, s, ch, cols, want = load_case(tag)
    sfreq, W = float(p["sfreq"]), p["window"]
    assert W == int(sfreq * s.segment_length_features_ms / 1000) and W > 16384
    assert "bandpass_filter" in list(s.features.get_enabled())
    x, s_raw, ocols, tab = oracle_of(tag)
    pv, got = None, None
    if p.get("defaults"):   # (the other families' policy: bursts_long_cases.run_case)
        from oracle import nm_oracle as orc

        assert "bursts" in list(s.features.get_enabled())
        starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
        pv = parity.PipelineVerifiers(s_raw, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
        df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
        assert list(df.columns) == cols, tag
        got = df.to_numpy(float)
        want_norm, want = want, g[f"{tag}_raw_values"]
    df = Stream(sfreq, channels=ch, settings=s_raw, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
    assert list(df.columns) == cols == ocols, tag
    raw = df.to_numpy(float)
    assert raw.shape == want.shape == tab.shape == (p["hops"], len(cols)), (tag, raw.shape, want.shape)
    np.testing.assert_array_equal(raw[:, -1], want[:, -1])
    before = dict(parity.STATS["forgiven"])
    _against(tag, "fixture", cols, raw, want, s_raw, sfreq, x, W, pv)
    # (defaults30k: the families that are not this case's subject are read once, against the reference's table -- the two
    # tables agree far below the policy, and every miss accepted on a conditioning report counts towards the tier's budget)
    _against(tag, "oracle", cols, raw, tab, s_raw, sfreq, x, W, pv, only=("bandpass", "bursts") if p.get("defaults") else None)
    after = parity.STATS["forgiven"]
    acc = {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}
    print(f"{tag}: accepted misses {acc}")
    assert acc.get("bandpass", 0) == 0 and acc.get("bursts", 0) == 0, acc
    if not p.get("defaults"):
        assert acc == {}, acc
    if got is not None:
        from oracle import nm_oracle as orc

        norm = orc.FeatureNormalizer(s)
        want_n = np.stack([norm.process(r.copy()) for r in raw[:, :-1]])
        np.testing.assert_array_equal(got[:, -1], want_norm[:, -1])
        np.testing.assert_array_equal(got[0, :-1], raw[0, :-1])
        np.testing.assert_allclose(got[:, :-1], want_n, rtol=1e-5, atol=2e-6, err_msg=tag)
        assert np.nanmedian(np.abs(got[1:, :-1] - want_norm[1:, :-1])) < 1e-4, tag
    return raw


def fixture_taps(g):
    """The reference's band-pass FIRs of TAPS_OF, rebuilt from their stored first halves (centre included)."""
    out = []
    for band in TAPS_OF[1]:
        h = np.asarray(g[f"taps_half_{band}"], np.float64)
        out.append(np.concatenate([h, h[-2::-1]]))
    return out


# ---- the cancellation itself ---------------------------------------------------------------------------------------------------
def cancellation_case(lib):
    """-> (worst relative error per feature, share of entries beyond 1e-5 per feature) of the 20 kHz white-noise plan:
    W = 20 000, sigma 50, the default bands, three features, 4 hops, 2 channels, against oracle.run_stream."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream

    p = CASES["w20k_nolog"]
    s = settings_of(nm, dict(p, log=True)).validate()
    x = recording(p, sigma=50.0)
    ch = chmod.get_default_channels_from_data(x)
    df = Stream(float(p["sfreq"]), channels=ch, settings=s, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
    rows = orc.run_stream(x, float(p["sfreq"]), s, ch, line_noise=50)
    cols = list(rows[0])
    assert list(df.columns) == cols and len(rows) == len(df) == p["hops"]
    tab, got = np.array([[r[c] for c in cols] for r in rows]), df.to_numpy(float)
    worst, share = {}, {}
    for f in FEATS:
        idx = [i for i, c in enumerate(cols) if f"_bandpass_{f}_" in c]
        assert len(idx) == p["n_ch"] * len(s.frequency_ranges_hz)
        rel = np.abs(got[:, idx] - tab[:, idx]) / np.abs(tab[:, idx])
        worst[f], share[f] = float(rel.max()), float((rel > 1e-5).mean())
        print(f"cancellation {f}: worst relative error {worst[f]:.3g}, share beyond 1e-5 {share[f]:.3g}")
    return worst, share


# ---- identity taps: the index shifts of g1 / g2 and the tail bounds ----------------------------------------------------------------
ID_W = 16400   # (any window behind the gate; the tails are what is probed)
ID_TAILS = (3, 64, 65, ID_W - 1, ID_W)


def _single_accumulator(t) -> dict:
    """The three features of the float64 tail `t` with every variance summed as the emulator sums it: two passes in float32,
    ONE accumulator (bandpower_probe_cases.var32_lanes with one lane) -- the series themselves exact."""
    from tests import bandpower_probe_cases as probe

    v = [probe.var32_lanes(np.diff(t, d), 1) if t.size > d else np.nan for d in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        mob = np.sqrt(np.float64(v[1]) / v[0])
        comp = np.sqrt(np.float64(v[2]) / v[1]) / mob
    return dict(zip(FEATS, (float(np.nan_to_num(v[0])), float(np.nan_to_num(mob)), float(np.nan_to_num(comp)))))


def identity_probe(lib, feats=FEATS, W=ID_W, tails=ID_TAILS) -> int:
    """Integer-valued series (|x| <= 1000) through the one-tap filter h = [1] handed in as bank_taps: g1 = [-1, 1] and
    g2 = [1, -2, 1], the three series are exact in float32, and activity, mobility and complexity are the float64 statistics
    of x, diff(x), diff(x, 2) over the tail -- within the limit tests/bandpower_probe_cases.py holds its identity-tap cases to
    (`judge`: tests/parity.tolerances, nothing forgiven).  Two windows one sample apart, so that a shifted series shows."""
    from tests import bandpower_probe_cases as probe
    from tests import parity
    from tests.fir_sample_probe_cases import build_engine

    sfreq, C = 1000.0, 3  # (the settings hold whole milliseconds: every tail length exists at 1 kHz; the kernel reads W)
    s = probe.identity_settings(sfreq, W, tails, feats=feats)
    eng = build_engine(lib, {}, s, probe.channels(C), sfreq, features=["bandpass_filter"], bank_taps=np.ones((len(tails), 1)), window=W)
    try:
        assert eng.W == W and probe.tails_of(eng, s, sfreq) == list(tails)
        rng = np.random.default_rng(7)
        # (noise only: a ramp or a constant has var(diff) = 0 in float64 and what an fp32 transform leaves of it here)
        x = np.stack([rng.integers(-a, a + 1, W + 1) for a in (1000, 37, 5)]).astype(np.float32)
        out = probe.columns(eng, eng.process_batch(x, np.array([0, 1], np.int64)))
        if lib is None:
            assert eng.kernels(3) == "nmx_kern_bank_diff", eng.kernels(3)
        win = np.stack([x[:, :W], x[:, 1:W + 1]]).astype(np.float64)
        cnt = left_out = 0
        for b, n_tail in enumerate(tails):
            t = win[:, :, W - n_tail:]
            want = dict(zip(FEATS, probe.hjorth64(t, False)))
            for c in range(C):
                for f in feats:
                    key = probe.key_of(f"ch{c}", f, f"b{b}")
                    k = np.ones(2, bool)
                    if lib is not None:
                        # (the emulator's ONE accumulator rounds the sum of 16 400 quantised squares the same way every time:
                        # the stand-in's own error.  As class a of bandpower_probe_cases leaves it out (_identity_rows): the
                        # entry restated with the three variances summed that way -- var32_lanes of the exact series -- and
                        # left out where that alone is half the policy's tolerance from the float64 value.  Entry by entry:
                        # a feature that does not read the variance in question stays.  The device tier leaves nothing out)
                        rtol, atol = parity.tolerances(key, s, sfreq, 1.0, W)
                        for r in range(2):
                            k[r] = abs(_single_accumulator(t[r, c])[f] - want[f][r, c]) <= 0.5 * (atol + rtol * abs(want[f][r, c]))
                    probe.judge("long_identity", "+".join(feats), key, out[key][k], want[f][k, c], s, sfreq, W)
                    cnt += int(k.sum())
                    left_out += int((~k).sum())
        print(f"identity probe {feats}: {cnt} entries, {left_out} left to the device tier")
        assert left_out == 0 or lib is not None
        assert cnt >= 2 * C * 3 * len(feats), "the short tails are all there"
    finally:
        eng.close()
    return cnt


# ---- special rows -------------------------------------------------------------------------------------------------------------------
def special_rows(lib):
    """W = 20 000: a constant channel, a zero channel and a channel with one NaN sample in hop 1, against oracle.run_stream:
    the same NaN pattern (the NaN-channel policy), the nan_to_num outcomes of a dead series, every live entry by the policy."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    p = dict(CASES["w20k_nolog"], n_ch=4, hops=3)
    W, hop = p["window"], p["sfreq"] // 10
    s = settings_of(nm, p).validate()
    x = recording(p).copy()
    x[1] = 300.0
    x[2] = 0.0
    x[3, W + 50] = np.nan   # (a new sample of hop 1; hop 2 holds it too)
    ch = chmod.get_default_channels_from_data(x)
    sfreq = float(p["sfreq"])
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    cols = list(rows[0])
    assert list(df.columns) == cols
    tab, got = np.array([[r[c] for c in cols] for r in rows]), df.to_numpy(float)
    assert np.array_equal(np.isnan(got), np.isnan(tab)), "NaN pattern differs from the oracle's"
    assert np.isnan(got[1:]).any() and not np.isnan(got[0]).any()
    zero = [i for i, c in enumerate(cols) if c.startswith("ch2") and "_bandpass_" in c]
    assert zero and (tab[:, zero] == 0).all() and (got[:, zero] == 0).all(), "a zero channel: nan_to_num leaves 0"
    # the constant channel: its band series is the taps' edge transient times 300 (zero padding), a live signal of its own,
    # and the one whose level sits inside the reach of the zero-padded g1 / g2: compared by the policy like the noise channels
    const = [i for i, c in enumerate(cols) if c.startswith("ch1") and "_bandpass_" in c]
    assert len(const) == len(FEATS) * len(s.frequency_ranges_hz) and np.all(tab[:, const] > 0)
    left_out = set()
    if lib is not None:
        # (the emulator's ONE accumulator again -- identity_probe: a smooth transient of 20 000 samples is summed with every
        # rounding the same way, 3.4e-5 of theta's variance.  The entries of this channel restated that way from the float64
        # series, and left out where that alone takes half the tolerance; the device tier leaves nothing out)
        from py_neuromodulation_amd import fir_design
        from scipy.signal import fftconvolve

        for band, fr in s.frequency_ranges_hz.items():
            h = np.asarray(fir_design.band_pass_bank([(fr[0], fr[1])], sfreq)[0], np.float64)
            half = (len(h) - 1) // 2
            y = fftconvolve(np.full(W, 300.0), h)[half:half + W]
            seg = int(round(s.bandpass_filter_settings.segment_lengths_ms[band] * sfreq / 1000))
            emu = _single_accumulator(y[W - seg:])
            for f in FEATS:
                j = cols.index(f"ch1_avgref_bandpass_{f}_{band}")
                assert j in const
                rtol, atol = parity.tolerances(cols[j], s, sfreq, 300.0, W)
                if abs(emu[f] - tab[0, j]) > 0.5 * (atol + rtol * abs(tab[0, j])):
                    left_out.add(j)
        print(f"special rows, constant channel: {sorted(cols[j] for j in left_out)} left to the device tier")
        assert len(left_out) <= len(const) // 2, "most of the constant channel is compared in the emulator too"
    live = [i for i, c in enumerate(cols[:-1]) if not c.startswith("ch2") and i not in left_out]
    assert set(const) - left_out <= set(live)
    for i in range(got.shape[0]):
        n_bad, rep, _ = parity.compare([cols[j] for j in live], got[i, live], tab[i, live], s, sfreq, float(np.nanmax(np.abs(x))), W)
        assert n_bad == 0, f"special rows hop {i}\n{rep}"
    rel = np.abs(got[:, const] - tab[:, const]) / np.abs(tab[:, const])
    print(f"special rows, constant channel: worst relative error {rel.max():.3g} ({cols[const[int(rel.max(0).argmax())]]})")
    return len(left_out)


def offsets_case(lib):
    """Offsets of +1000 / -1000 on the w20k_nolog recording, through the offset split: oracle only, by the policy.
    -> {family: misses accepted on a conditioning report}."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    p = CASES["w20k_nolog"]
    s = settings_of(nm, dict(p, log=True)).validate()
    x = (recording(p) + np.array([[1000.0], [-1000.0]])).astype(np.float32).astype(np.float64)
    ch = chmod.get_default_channels_from_data(x)
    sfreq, W = float(p["sfreq"]), p["window"]
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    cols = list(rows[0])
    assert list(df.columns) == cols
    tab = np.array([[r[c] for c in cols] for r in rows])
    # (the rows' conditioning with the level in: tests/parity.PipelineVerifiers, as every offsets case of the suite --
    # timeosc_long_cases.n16k_case.  The frame transforms hold the level of 5 sigma in the bin next to theta's)
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = dict(parity.STATS["forgiven"])
    _against("offsets1000", "oracle", cols, df.to_numpy(float), tab, s, sfreq, x, W, pv)
    after = parity.STATS["forgiven"]
    return {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}


# ---- the series outlet of a long plan ------------------------------------------------------------------------------------------------
def filter_window_series(lib):
    """HotPathEngine.filter_window on a 20 000-sample band-pass plan (three features: every filter is one of the differenced-taps
    form): the launch has no output row and no tail, and every filter leaves its whole series -- each sample against the
    float64 direct convolution, by the limit and the single-precision yardstick of tests/fir_sample_probe_cases.py (check_rows;
    its partitioned cases).  Noise, noise on a level of 300 and a constant window; theta and high_beta.  -> worst ratio."""
    import py_neuromodulation_amd as nm
    from tests import fir_sample_probe_cases as fir

    p = dict(CASES["w20k_nolog"], bands={b: None for b in fir.TWO_BANDS}, seglens_ms={})
    W, C = p["window"], 3
    s = settings_of(nm, p).validate()
    eng = fir.build_engine(lib, {}, s, [f"ch{i}" for i in range(C)], float(p["sfreq"]))
    try:
        assert eng.W == W
        taps = eng.filter_taps
        assert len(taps) == 2
        x = np.random.default_rng(p["seed"]).standard_normal((C, W)) * fir.SIGMA
        x[1] += 300.0
        x[2] = 300.0
        x = x.astype(np.float32).astype(np.float64)
        got = eng.filter_window(x)
        if lib is None:
            assert eng.kernels(3) == "nmx_kern_bank_diff", eng.kernels(3)
        assert got.shape == (C, len(taps), W)
        y64, y32 = fir._bank_reference(x, taps, 0)
        n = C * len(taps)
        worst = fir.check_rows("long_filter_window", "series", got.reshape(n, W), y64.reshape(n, W), y32.reshape(n, W),
                               np.repeat(x, len(taps), axis=0))
        print(f"filter_window at {W} samples: worst error {worst:.3f} yardsticks")
        # ... and the batch after it still runs the epilogue (the call patched a copy of the plan's arguments)
        rows = eng.process_batch(x.astype(np.float32), np.array([0], np.int64))
        assert np.isfinite(rows).all() and np.all(rows[:, :len(eng.keys)] != 0)
    finally:
        eng.close()
    return worst


# ---- call shapes -------------------------------------------------------------------------------------------------------------------
def process_equals_run(lib, run_rows, tag="w20k"):
    """DataProcessor.process window by window gives the Stream.run rows (1e-6 relative: the tolerance between call shapes
    used throughout tests/parity_cases.py) -- the Kalman state of w20k carried from call to call."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.data_processor import DataProcessor

    _, p, s, ch, cols, _ = load_case(tag)
    sfreq = float(p["sfreq"])
    x = oracle_of(tag)[0]
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    dp = DataProcessor(sfreq=sfreq, settings=s, channels=ch, line_noise=50, **_kw(lib))
    feat = [c for c in cols if c != "time"]
    for i, (a, b) in enumerate(zip(starts, ends)):
        row = dp.process(np.array(x[:, a:b]))
        assert list(row) == feat
        np.testing.assert_allclose(np.array(list(row.values()), float), run_rows[i, :len(feat)], rtol=1e-6, atol=0, err_msg=f"hop {i}")


def dropin_equals_row(lib, run_rows, tag="w20k_nolog"):
    """features.BandPower.calc_feature on the first 20 000-sample window equals the row."""
    from py_neuromodulation_amd import features

    _, p, s, ch, cols, _ = load_case(tag)
    x = oracle_of(tag)[0]
    names = [n for n, u in zip(ch["new_name"], ch["used"]) if u]
    bp = features.BandPower(s, names, float(p["sfreq"]), **_kw(lib))
    got = bp.calc_feature(np.array(x[:, :p["window"]]))
    assert list(got) == [c for c in cols if c != "time"]
    np.testing.assert_allclose(np.array(list(got.values()), float), run_rows[0, :-1], rtol=1e-6, atol=0)


def ragged_pair(lib):
    """20 000.7 Hz with 1 s segments: windows of 20 000 and 20 001 samples, one plan per length, the Kalman state handed from
    plan to plan (data_processor.LengthTable) -- Stream.run against oracle.run_stream by the policy."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream

    p = dict(CASES["w20k"], sfreq=20000.7, window=20001, hops=8)
    sfreq = p["sfreq"]
    s = settings_of(nm, p).validate()
    T = 20001 + 7 * 2001
    x = (np.random.default_rng(p["seed"]).standard_normal((2, T)) * SIGMA).astype(np.float32).astype(np.float64)
    ch = chmod.get_default_channels_from_data(x)
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    cols = list(rows[0])
    assert list(df.columns) == cols and len(rows) == len(df) >= 4
    tab = np.array([[r[c] for c in cols] for r in rows])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    lengths = sorted({int(b - a) for a, b in zip(starts, ends)})
    assert lengths == [20000, 20001], lengths
    kal = [i for i, c in enumerate(cols) if "_bandpass_activity_theta" in c]
    unf = orc.run_stream(x, sfreq, settings_of(nm, dict(p, kalman=[])).validate(), ch, line_noise=50)
    assert any(abs(unf[-1][cols[i]] - tab[-1, i]) > 1e-3 for i in kal), "the Kalman filter does not move the last row: no state to carry"
    _against("ragged20k", "oracle", cols, df.to_numpy(float), tab, s, sfreq, x, 20001)
    return lengths


# ---- gates, all at plan construction --------------------------------------------------------------------------------------------------
def _run(lib, sfreq, s):
    from py_neuromodulation_amd.stream import Stream

    n = int(sfreq)
    x = np.random.default_rng(1).standard_normal((2, n + n // 10)).astype(np.float32).astype(np.float64)
    Stream(float(sfreq), data=x, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)


def _plain(*features):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    for f in features:
        setattr(s.features, f, True)
    return s


def gate_is_closed_without_the_opt_in(lib, delenv):
    import pytest

    delenv("NMX_LONG_BANDPOWER")
    with pytest.raises(ValueError) as e:
        _run(lib, 20000, _plain("bandpass_filter"))
    msg = str(e.value)
    assert "16 384" in msg and "NMX_LONG_BANDPOWER=1" in msg and "bandpass_filter" in msg.split(";")[0], msg
    # (the bursts opt-in, set or not by the caller: its name on the side of the ';' it belongs to, its variable named while unset)
    front, behind = msg.split(";")
    bursts_on = os.environ.get("NMX_LONG_BURSTS", "0") not in ("", "0")
    assert ("bursts" in front) != bursts_on and ("bursts run up to" in behind) == bursts_on, msg
    assert ("NMX_LONG_BURSTS=1" in msg) != bursts_on, msg


def limited_features_raise(lib):
    import pytest

    with pytest.raises(ValueError) as e:
        _run(lib, 20000, _plain("fft", "bandpass_filter", "stft"))
    msg = str(e.value)
    assert "16 384" in msg and "40 000" in msg, msg
    assert "stft" in msg.split(";")[0] and "bandpass_filter" not in msg.split(";")[0] and "bandpass_filter" in msg.split(";")[1], msg


def over_limit_raises(lib):
    import pytest

    with pytest.raises(ValueError, match="40 000 samples"):
        _run(lib, 40001, _plain("bandpass_filter"))


# ---- nothing below the gate moved -----------------------------------------------------------------------------------------------------
PARENT_SEED, PARENT_HOPS = 8002, 3


def rows_8k(lib):
    """(rows, stage-3 kernels) of an 8 kHz / 8000-sample band-pass plan (the partitioned bank, three features): 2 ch x 3 hops."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    p = {"seed": PARENT_SEED, "sfreq": 8000, "window": 8000, "n_ch": 2, "hops": PARENT_HOPS}
    s = settings_of(nm, p).validate()
    eng = HotPathEngine(s, ["ch0", "ch1"], 8000.0, **_kw(lib))
    try:
        rows = eng.process_batch(recording(p).astype(np.float32), np.arange(PARENT_HOPS, dtype=np.int64) * 800).copy()
        return rows, eng.kernels(3)
    finally:
        eng.close()


def below_the_gate(lib, setenv, delenv):
    setenv("NMX_LONG_BANDPOWER", "1")
    on, k_on = rows_8k(lib)
    delenv("NMX_LONG_BANDPOWER")
    off, k_off = rows_8k(lib)
    assert k_on == k_off, (k_on, k_off)
    assert np.isfinite(on).all() and on.tobytes() == off.tobytes()
    return on, k_on
