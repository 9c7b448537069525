"""`bursts` on windows up to 40 000 samples (the partitioned band-pass bank, nmx_kern_hilbert_long, the threshold walk with
bounded staging, nmx_kern_burst_stat_scan, the chunk cap of the hand-off buffers): the cases of
tests/golden/bursts_long.npz, shared by the emulator tier (test_bursts_long_cpu.py) and the MI355X tier
(test_bursts_long_gpu.py).  The recordings come from tests/bursts_long_recording.py (the fixture stores generator parameters,
settings, channels, columns, the reference's table and the first halves of its band-pass taps -- not recordings).

  tag          window  what it crosses
  k9k          9 000   time_duration_s = 1.38: K = 3 106 <= 65 536, ring (12 420) full at the fifth hop.  First shape past
                       the power-of-two staging arrays (8 188): register merge in tiles.  2 ch x 5 hops
  w14k         14 000  default 30 s history: K = 105 001, the tiled merge.  Past the walk's (12 900) and the Hilbert kernel's
                       (13 650) layouts, below the old gate.  2 ch x 5 hops
  odd16385     16 385  odd: 5 x 3277 = 5 x 29 x 113 points.  First length past the old gate.  2 ch x 5 hops.  Threshold 73: at
                       the 75th percentile the rank 0.75 (m - 1) is whole at hops 0, 2 and 4 (m - 1 = 16 384 + 1638 k), the
                       threshold then IS a sample of the window and no seed keeps a margin (its gate is on for 27 % of the time)
  w20k_f100    20 000  100 Hz features (200 samples per hop), time_duration_s = 1.05: ring (21 000) full after five hops, seven
                       steady hops behind them -- the steady regime and the one-wave walk on a long window.  1 ch, 1 band, 12 hops
  w40k         40 000  the maximum; past the statistics item's LDS series; K = 300 001.  2 ch x 5 hops
  defaults30k  30 000  the reference's default settings with only raw_resampling off: notch, re-referencing, the seven default
                       features, z-score.  3 ch x 3 hops

Every case is a Stream.run compared with the reference's table (the fixture) AND with oracle.run_stream under
tests/parity.compare with a PipelineVerifiers row, the amplitude scale from the recording's own max |x|.

Seeds.  A burst feature counts samples at or above the threshold; a sample nearer to it than fp32 resolves is decided by
rounding.  Each seed is the first of seed0 = 1000 x (window // 1000) + 1, seed0 + 1, ... for which, in the float64 oracle alone, min |env[n] - thr| over
every sample, hop, channel and band is at least MARGIN = 1e-5 x max |input row| -- ten times parity.DECISION_RTOL, the size of
the amplitude tolerance itself (`python tests/bursts_long_cases.py scan <tag> <seed> ...` prints the margins; the emulator tier
asserts them from the oracle, independently of the engine).  With such inputs no `bursts` miss is accepted in either tier."""

from __future__ import annotations

import ctypes
import importlib.util
import json
from pathlib import Path

import numpy as np

# (by path: the fixture's generator loads this module next to the reference, whose own `tests` package shadows this one)
_spec = importlib.util.spec_from_file_location("_bursts_long_recording", Path(__file__).with_name("bursts_long_recording.py"))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)
recording = _rec.recording

MARGIN = 1e-5

# tag -> generator parameters (tests/bursts_long_recording.py) and the settings that differ from settings_of's base.
# FAST: two burst bands wide enough that the gate's edges take half a millisecond (25 samples at 40 kHz); the default beta
# bands need a tenth of a second, 3000 samples at 30 kHz, and hold a dozen times as many samples near any threshold.
FAST = {"bands": {"fast_a": [400, 1200], "fast_b": [1500, 3000]}, "carriers": [800.0, 2200.0], "noise": 0.02, "gate_jitter": 0.0003}
CASES = {
    "k9k": dict(FAST, seed=9007, sfreq=9000, window=9000, n_ch=2, hops=5, amps=[1.0, 0.7], time_duration_s=1.38,
                gate_period=0.01, gate_width=0.0025),
    "w14k": dict(FAST, seed=14003, sfreq=14000, window=14000, n_ch=2, hops=5, amps=[1.0, 0.7], gate_period=0.1, gate_width=0.025),
    "odd16385": dict(FAST, seed=16003, sfreq=16385, window=16385, n_ch=2, hops=5, amps=[1.0, 0.7], gate_period=0.1,
                     gate_width=0.027, threshold=73),
    "w20k_f100": dict(FAST, seed=20004, sfreq=20000, window=20000, n_ch=1, hops=12, amps=[1.0], feat_hz=100, time_duration_s=1.05,
                      bands={"fast_a": [400, 1200]}, carriers=[800.0], growth=0.2, gate_period=0.01, gate_width=0.0025),
    "w40k": dict(FAST, seed=40001, sfreq=40000, window=40000, n_ch=2, hops=5, amps=[1.0, 0.7], gate_period=0.1, gate_width=0.025),
    # the default bands (low beta, high beta); one gate of 0.27 s (0.365 s to 0.635 s) that every window holds; the same gate in every channel, so that
    # the common average reference (each channel minus the mean of the others: 1, -2, 1) leaves two-level envelopes
    "defaults30k": {"seed": 30422, "sfreq": 30000, "window": 30000, "n_ch": 3, "hops": 3, "defaults": True, "amps": [1.0, -1.0, 1.0],
                    "carriers": [17.0, 27.0], "noise": 0.03, "gate_period": 1.0, "gate_width": 0.27},
}
# (k9k: int(9000 x 1.38) = 12 420 ring entries, K = 3 106; full at the last hop, 12 600 samples)


def settings_of(nm, p):
    """The case's settings on package `nm` (this project's, or the reference's in the fixture's generator)."""
    s = nm.NMSettings.get_default()
    if p.get("defaults"):
        s.preprocessing = [q for q in s.preprocessing if q != "raw_resampling"]
        return s
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.bursts = True
    s.sampling_rate_features_hz = p.get("feat_hz", 10)
    s.segment_length_features_ms = 1000
    if "threshold" in p:
        s.bursts_settings.threshold = p["threshold"]
    if "time_duration_s" in p:
        s.bursts_settings.time_duration_s = p["time_duration_s"]
    if "bands" in p:
        for name, (lo, hi) in p["bands"].items():
            s.frequency_ranges_hz[name] = {"frequency_low_hz": lo, "frequency_high_hz": hi}
        s.bursts_settings.frequency_bands = list(p["bands"])
    return s


def list_entries(p, s) -> int:
    q = s.bursts_settings.threshold / 100
    n_ring = int(p["sfreq"] * s.bursts_settings.time_duration_s)
    return min(int(np.floor((1 - q) * (n_ring - 1))) + 2, n_ring)


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def load_case(tag):
    """-> (fixture, parameters, settings, channels, columns, the reference's table)."""
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("bursts_long")
    p = json.loads(str(g["params_json"]))[tag]
    assert p == CASES[tag], "the fixture was generated from other parameters"
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return g, p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


def fixture_taps(g, tag):
    """The reference's burst band-pass FIRs of a case, rebuilt from their stored first halves (centre included)."""
    out = []
    for name in g[f"{tag}_taps"]:
        h = np.asarray(g[str(name)], np.float64)
        out.append(np.concatenate([h, h[-2::-1]]))
    return out


_ORACLE = {}


def oracle_of(tag):
    """The float64 restatement of a case -- without the z-score where the case has one --, computed once per process and left
    unchanged: (recording, un-normalised settings, columns, table, verifiers)."""
    if tag not in _ORACLE:
        from oracle import nm_oracle as orc
        from tests import parity
        from tests.helpers import settings_from_json

        g, p, s, ch, cols, _ = load_case(tag)
        if p.get("defaults"):
            s = settings_from_json(g[f"{tag}_raw_settings_json"])
        sfreq = float(p["sfreq"])
        x = recording(p)
        x.setflags(write=False)
        rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
        assert [list(r) for r in rows] == [cols] * p["hops"], tag
        tab = np.array([[r[c] for c in cols] for r in rows])
        tab.setflags(write=False)
        starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
        pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, p["window"], line_noise=50, ends=ends)
        _ORACLE[tag] = (x, s, cols, tab, pv)
    return _ORACLE[tag]


def oracle_margin(tag, p=None, s=None, ch=None):
    """min |env[n] - thr| / max |input row| over every sample, hop, channel and band, in the float64 oracle alone (behind
    re-referencing a channel holds a mix of rows: the largest row is the scale)."""
    from oracle import nm_oracle as orc
    from tests import parity

    if p is None:
        _, p, _, ch, _, _ = load_case(tag)
        x, s, _, _, _ = oracle_of(tag)
    else:
        x = recording(p)
    starts, ends, _ = orc.window_schedule(x.shape[1], float(p["sfreq"]), s.sampling_rate_features_hz, s.segment_length_features_ms)
    pv = parity.PipelineVerifiers(s, ch, float(p["sfreq"]), x, starts, p["window"], line_noise=50, ends=ends)
    amp_row = np.abs(x).max(axis=1)
    worst = np.inf
    for i in range(p["hops"]):
        tr = pv._burst_trace(i)
        env, thr = np.asarray(tr.last_env), np.asarray(tr.last_thr)
        assert env.shape[0] == x.shape[0] and env.shape[-1] == p["window"], env.shape
        for c in range(env.shape[0]):
            amp = amp_row.max() if p.get("defaults") else amp_row[c]
            for b in range(env.shape[1]):
                worst = min(worst, orc.burst_decision_margin(env[c, b], thr[c, b]) / amp)
        pv._cache.pop(i, None)
    return float(worst)


def _against(tag, name, cols, got, ref, s, sfreq, x, W, pv):
    from tests import parity

    amp = float(np.nanmax(np.abs(x)))
    worst_all = {}
    for i in range(got.shape[0]):
        n_bad, rep, worst = parity.compare(cols[:-1], got[i, :-1], ref[i, :-1], s, sfreq, amp, W, verifier=pv.row(i))
        for f, v in worst.items():
            worst_all[f] = max(worst_all.get(f, 0.0), v)
        assert n_bad == 0, f"{tag} vs {name} hop {i}\n{rep}"
    print(f"{tag} vs {name}: {got.shape[0]} rows, worst relative error {worst_all}")


def run_case(lib, tag):
    """Stream.run of case `tag` on library `lib` against the fixture and the oracle.
    -> {family: misses accepted on a conditioning report}.

    defaults30k ends in a z-score, which divides by the spread of three rows and amplifies the fp32 rounding of a feature
    by value / spread: the composition is checked stage by stage, as tests/parity_cases.py checks the default pipeline --
    (1) the same run without the normaliser against the reference's and the oracle's un-normalised tables, 1e-5 policy;
    (2) the normalised rows against the float64 oracle normaliser applied to the ENGINE'S OWN un-normalised rows, 1e-5
    relative + 2e-6; (3) the first row un-normalised, the time column exact, and the reference's normalised table within a
    median error of 1e-4."""
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    g, p, s, ch, cols, want = load_case(tag)
    sfreq, W = float(p["sfreq"]), p["window"]
    assert W == int(sfreq * s.segment_length_features_ms / 1000)
    assert "bursts" in list(s.features.get_enabled())
    x, s_raw, ocols, tab, pv = oracle_of(tag)
    got = None
    if p.get("defaults"):
        df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
        assert list(df.columns) == cols, tag
        got = df.to_numpy(float)
        want_norm, want = want, g[f"{tag}_raw_values"]
    df = Stream(sfreq, channels=ch, settings=s_raw, line_noise=50, **_kw(lib)).run(np.array(x), save_csv=False)
    assert list(df.columns) == cols == ocols, tag
    raw = df.to_numpy(float)
    assert raw.shape == want.shape == tab.shape == (p["hops"], len(cols)), (tag, raw.shape, want.shape)
    np.testing.assert_array_equal(raw[:, -1], want[:, -1])
    dm = [c for c in cols if c.endswith("_duration_mean")]
    assert dm and all((tab[:, cols.index(c)] != 0).any() for c in dm), f"{tag}: a (channel, band) without a burst in any row"
    before = dict(parity.STATS["forgiven"])
    _against(tag, "fixture", cols, raw, want, s_raw, sfreq, x, W, pv)
    _against(tag, "oracle", cols, raw, tab, s_raw, sfreq, x, W, pv)
    after = parity.STATS["forgiven"]
    acc = {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}
    print(f"{tag}: accepted misses {acc}")
    if got is not None:
        from oracle import nm_oracle as orc

        norm = orc.FeatureNormalizer(s)
        want_n = np.stack([norm.process(r.copy()) for r in raw[:, :-1]])
        np.testing.assert_array_equal(got[:, -1], want_norm[:, -1])
        np.testing.assert_array_equal(got[0, :-1], raw[0, :-1])
        np.testing.assert_allclose(got[:, :-1], want_n, rtol=1e-5, atol=2e-6, err_msg=tag)
        assert np.nanmedian(np.abs(got[1:, :-1] - want_norm[1:, :-1])) < 1e-4, tag
    return acc


# ---- one engine, several process_batch calls ------------------------------------------------------------------------------
def engine_of(lib, tag=None, sfreq=None, s=None, n_ch=2):
    """A bursts-only engine: of case `tag`, or of the plain settings at `sfreq` samples per second and window."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    if tag is not None:
        p = CASES[tag]
        s, sfreq, n_ch = settings_of(nm, p).validate(), p["sfreq"], p["n_ch"]
    elif s is None:
        s = settings_of(nm, {}).validate()
    return HotPathEngine(s, [f"ch{i}" for i in range(n_ch)], float(sfreq), **_kw(lib))


def feed(eng, x32, at, calls, W, hop):
    """`calls` process_batch calls from hop `at` on -> (their rows, kernels of stage 4 after each call)."""
    rows, kernels = [], []
    for n in calls:
        seg = np.ascontiguousarray(x32[:, at * hop:(at + n - 1) * hop + W])
        rows.append(eng.process_batch(seg, np.arange(n, dtype=np.int64) * hop).copy())
        kernels.append(eng.kernels(4))
        at += n
    return np.concatenate(rows), kernels


_F100 = {}


def f100_rows(lib, calls):
    """w20k_f100 through process_batch in `calls` batches, once per (library, calls): (rows, kernels per call)."""
    key = (id(lib), calls)
    if key not in _F100:
        p = CASES["w20k_f100"]
        assert sum(calls) == p["hops"]
        eng = engine_of(lib, "w20k_f100")
        try:
            rows, kernels = feed(eng, recording(p).astype(np.float32), 0, calls, p["window"], p["sfreq"] // p["feat_hz"])
        finally:
            eng.close()
        rows.setflags(write=False)
        _F100[key] = (rows, kernels)
    return _F100[key]


F100_ONE, F100_THREE = (12,), (3, 5, 4)   # (the ring is full behind hop 5: the last batch of three starts on a full ring)


def batching_gives_same_bytes(lib):
    a, _ = f100_rows(lib, F100_ONE)
    b, _ = f100_rows(lib, F100_THREE)
    assert a.shape == b.shape and np.isfinite(a).all()
    assert (a[6:] != a[5]).any(), "the steady rows do not move: the walk is not exercised"
    assert a.tobytes() == b.tobytes(), f"rows that differ: {np.flatnonzero((a != b).any(axis=1))[:10]}"


def state_travels(lib, at=7):
    """Export behind hop `at` of w20k_f100 (the ring is full), import into a fresh plan, continue: the rows from there on are
    the uninterrupted run's, bit for bit."""
    p = CASES["w20k_f100"]
    want, _ = f100_rows(lib, F100_ONE)
    x32 = recording(p).astype(np.float32)
    W, hop = p["window"], p["sfreq"] // p["feat_hz"]
    e1 = engine_of(lib, "w20k_f100")
    try:
        head, _ = feed(e1, x32, 0, (at,), W, hop)
        blob = e1.export_state()
    finally:
        e1.close()
    assert head.tobytes() == want[:at].tobytes()
    e2 = engine_of(lib, "w20k_f100")
    try:
        e2.import_state(blob)
        tail, _ = feed(e2, x32, at, (p["hops"] - at,), W, hop)
        assert tail.tobytes() == want[at:].tobytes(), f"rows that differ: {at + np.flatnonzero((tail != want[at:]).any(axis=1))[:10]}"
    finally:
        e2.close()


def kernels_of(lib, tag, calls=None):
    """Stage-4 (bursts chain) kernels of each process_batch call of a case's bursts-only engine."""
    p = CASES[tag]
    eng = engine_of(lib, tag)
    try:
        return feed(eng, recording(p).astype(np.float32), 0, calls or (p["hops"],), p["window"], p["sfreq"] // p.get("feat_hz", 10))[1]
    finally:
        eng.close()


# ---- plans that build today keep their kernels and their bytes ------------------------------------------------------------------
PARENT_SEED, PARENT_HOPS = 8001, 5
def plain_rows(lib, sfreq, hops=PARENT_HOPS):
    """(rows, stage-4 kernels) of a bursts-only plan with `sfreq`-sample windows: 2 ch x `hops` hops, one batch."""
    p = {"seed": PARENT_SEED, "sfreq": sfreq, "window": sfreq, "n_ch": 2, "hops": hops, "amps": [1.0, 0.7], "carriers": [17.0, 27.0],
         "noise": 0.3, "gate_period": 0.5, "gate_width": 0.125}
    eng = engine_of(lib, sfreq=sfreq)
    try:
        rows, kernels = feed(eng, recording(p).astype(np.float32), 0, (hops,), sfreq, sfreq // 10)
    finally:
        eng.close()
    return rows, kernels[0]


# ---- ragged window lengths ---------------------------------------------------------------------------------------------------
def ragged_pair(lib):
    """14 000.7 Hz with 1 s segments: windows of 14 000 and 14 001 samples (3 x 4667 = 3 x 13 x 359 points), one plan per
    length, the burst history handed from plan to plan (data_processor.LengthTable) -- Stream.run against oracle.run_stream
    under the parity policy (w14k's recording at that rate; the seed is not chosen for it)."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    p = dict(CASES["w14k"], sfreq=14000.7, window=14001, hops=8)
    sfreq = p["sfreq"]
    s = settings_of(nm, p).validate()
    x = recording(p)
    ch = chmod.get_default_channels_from_data(x)
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    cols = list(rows[0])
    assert list(df.columns) == cols and len(rows) == len(df)
    tab = np.array([[r[c] for c in cols] for r in rows])
    got = df.to_numpy(float)
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    lengths = sorted({int(b - a) for a, b in zip(starts, ends)})
    assert lengths == [14000, 14001], lengths
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, 14001, line_noise=50, ends=ends)
    _against("ragged14k", "oracle", cols, got, tab, s, sfreq, x, 14001, pv)
    return lengths


# ---- the chunk cap ----------------------------------------------------------------------------------------------------------
def chunk_cap(lib, setenv, delenv):
    """A 6-hop host batch of odd16385's plan: 3 buffers x 2 channels x 2 bands x 16 385 floats = 786 480 bytes per hop.
    NMX_BURST_HANDOFF_MB=2 holds two hops: three chunks, each with one Hilbert launch; unset (2 GiB) one chunk.  Same bytes."""
    p = dict(CASES["odd16385"], hops=6)
    x32 = recording(p).astype(np.float32)
    W, hop = p["window"], p["sfreq"] // 10
    out = {}
    for mb in (None, "2"):
        if mb:
            setenv("NMX_BURST_HANDOFF_MB", mb)
        try:
            eng = engine_of(lib, "odd16385")
        finally:
            if mb:
                delenv("NMX_BURST_HANDOFF_MB")
        try:
            lib.lib.nmx_emu_trace_begin()
            rows, _ = feed(eng, x32, 0, (6,), W, hop)
            n_text = lib.lib.nmx_emu_trace_end(None, 0)
            buf = ctypes.create_string_buffer(n_text)
            lib.lib.nmx_emu_trace_end(buf, n_text)
        finally:
            lib.lib.nmx_emu_trace_end(None, 0)
            eng.close()
        ops = [ln.split()[1] for ln in buf.raw.decode().splitlines() if ln.startswith("op ")]
        out[mb] = (rows, {k: ops.count(k) for k in ("be_launch_bank", "be_launch_hilbert", "be_launch_burst_thr", "be_launch_burst_stat")})
    (rows0, n0), (rows1, n1) = out[None], out["2"]
    per_hop = 3 * 2 * 2 * W * 4
    want = -(-6 // max(1, (2 << 20) // per_hop))
    assert want == 3
    assert n0["be_launch_hilbert"] == 1 and n0["be_launch_burst_stat"] == 1, n0
    assert n1["be_launch_hilbert"] == want and n1["be_launch_burst_stat"] == want and n1["be_launch_bank"] == want, n1
    assert np.isfinite(rows0).all() and rows0.tobytes() == rows1.tobytes()


# ---- errors, all at plan construction -----------------------------------------------------------------------------------------
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


def over_limit_raises(lib):
    import pytest

    with pytest.raises(ValueError, match="40 000 samples"):
        _run(lib, 40001, _plain("bursts"))


def limited_features_raise(lib):
    """A 20 000-sample plan with bursts and a feature that stays limited: the message names what remains limited."""
    import pytest

    def expect(s):
        with pytest.raises(ValueError) as e:
            _run(lib, 20000, s)
        msg = str(e.value)
        assert "16 384" in msg and "40 000" in msg, msg
        for f in ("stft", "bandpass_filter", "coherence", "raw_normalization", "raw_resampling"):
            assert f in msg.split(";")[0], msg   # (the limited ones, in front of the list of what runs up to 40 000)
        assert "bursts" in msg.split(";")[1], msg

    for f in ("stft", "bandpass_filter"):
        expect(_plain("bursts", f))
    s = _plain("bursts", "coherence")
    s.coherence_settings.channels = [["ch0", "ch1"]]
    s.frequency_ranges_hz["wide"] = [100, 400]
    s.coherence_settings.frequency_bands = ["wide"]
    expect(s)


# lengths above 13 650 samples without a divisor D <= 64 that leaves a transform of at most 8192 points: a prime below and one
# above the gate, and 2 x 9973 (D = 2 leaves 9973 points, the next divisor is 9973)
NO_SPLIT = {13669: "13 669", 16411: "16 411", 19946: "19 946"}


def no_split_raises(lib):
    import pytest

    for n, text in NO_SPLIT.items():
        assert not [d for d in range(2, 65) if n % d == 0 and n // d <= 8192], n
        with pytest.raises(ValueError, match=text):
            _run(lib, n, _plain("bursts"))


def gate_is_closed_without_the_opt_in(lib, delenv):
    """Without NMX_LONG_BURSTS a 20 000-sample bursts plan is refused as before; the message now names the variable."""
    import pytest

    delenv("NMX_LONG_BURSTS")
    with pytest.raises(ValueError) as e:
        _run(lib, 20000, _plain("bursts"))
    assert "16 384" in str(e.value) and "NMX_LONG_BURSTS=1" in str(e.value), str(e.value)


def fill_only_where_it_fits(lib):
    """The sort-once fill holds NMX_FILL_MAX = 32 768 samples.  A fresh 3-hop batch at 20 000 samples (24 000 in all) is the
    fill's; at 30 000 the first hop leaves room for no second one, at 40 000 not for itself: no fill launch, the workgroup walk
    absorbs the first hop in tiles (emulator trace: launches of each kind)."""
    import ctypes

    out = {}
    for sfreq in (20000, 30000, 40000):
        p = {"seed": PARENT_SEED, "sfreq": sfreq, "window": sfreq, "n_ch": 1, "hops": 3, "amps": [1.0], "carriers": [17.0, 27.0],
             "noise": 0.3, "gate_period": 0.5, "gate_width": 0.125}
        eng = engine_of(lib, sfreq=sfreq, n_ch=1)
        try:
            lib.lib.nmx_emu_trace_begin()
            rows, _ = feed(eng, recording(p).astype(np.float32), 0, (3,), sfreq, sfreq // 10)
            n_text = lib.lib.nmx_emu_trace_end(None, 0)
            buf = ctypes.create_string_buffer(n_text)
            lib.lib.nmx_emu_trace_end(buf, n_text)
        finally:
            lib.lib.nmx_emu_trace_end(None, 0)
            eng.close()
        ops = [ln.split()[1] for ln in buf.raw.decode().splitlines() if ln.startswith("op ")]
        assert np.isfinite(rows).all()
        out[sfreq] = (ops.count("be_launch_burst_fill"), ops.count("be_launch_burst_thr"))
    assert out == {20000: (1, 0), 30000: (0, 1), 40000: (0, 1)}, out


def history_limit_fails_first(lib):
    """K above 1 048 576 on a long window: the list's own message, as on a short one (40 kHz x 60 s at the 10th percentile:
    2 159 999 entries)."""
    import pytest

    s = _plain("bursts")
    s.bursts_settings.threshold = 10
    s.bursts_settings.time_duration_s = 60
    with pytest.raises(ValueError) as e:
        _run(lib, 40000, s)
    assert "1 048 576" in str(e.value) and "top-K" in str(e.value), str(e.value)


if __name__ == "__main__":
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    if len(sys.argv) >= 4 and sys.argv[1] == "scan":
        import py_neuromodulation_amd as nm
        from py_neuromodulation_amd import channels as chmod

        for seed in sys.argv[3:]:
            p = dict(CASES[sys.argv[2]], seed=int(seed))
            s = settings_of(nm, p).validate()
            ch = chmod.get_default_channels_from_data(np.zeros((p["n_ch"], 4)))
            print(sys.argv[2], seed, f"margin {oracle_margin(sys.argv[2], p, s, ch):.2e}", flush=True)
