"""Burst threshold histories beyond 65 536 top-K entries (nmx_merge_into_tiled / nmx_kern_burst_thr_tiled, nmx_k_bursts.h): the
cases shared by the emulator tier (test_burst_long_history_cpu.py) and the MI355X tier (test_burst_long_history_gpu.py).

Every case: two channels, no pre-processing, no normaliser, only `bursts` on [low_beta, high_beta] at the 50th percentile,
10 Hz features, 1 s windows; K = floor(0.5 (int(sfreq x time_duration_s) - 1)) + 2 = 70 001 list entries in all of them.

  tag        sfreq  time_duration_s  hops  ring full from hop  growth  compared with
  h2k        2000   70               800   691                 1       fixture + oracle
  h4k        4000   35               400   341                 1       fixture + oracle
  h4k_steep  4000   35               400   341                 20      oracle
  h1k        1000   140              1500  1391                1       oracle
  r12k       12000  30 (75th perc.)  25    -                   1       oracle   (K = 90 001: the default history)

  h2k        fill launch -> tiled workgroup kernel (fill regime) -> one-wave walk, four registers per lane (the emulator: the
             workgroup item's fringe / pending scheme on top of the tiled merge)
  h4k        400 samples per hop > 256: the tiled kernel on every hop, with truncation at K once the ring is full
  h4k_steep  nearly every new sample sorts to the head: the largest shift through every tile
  h1k        one-wave walk with two registers per lane

The recording's amplitude GROWS: once the ring is full the reference's threshold only rises, on a stationary signal every
burst feature soon is 0 and such a table passes with any threshold.  Each case therefore asserts, on the oracle's table, that
at least half of the ring-full rows have a non-zero duration_mean, for every (channel, band).

Comparison: tests/parity.compare with PipelineVerifiers, row by row (the 1e-5 policy; a `bursts` miss accepted only on the
conditioning report of the float64 restatement), as tests/timeosc_long_cases.py.

Seeds.  A burst feature is a count of samples at or above the threshold: a sample nearer to its threshold than fp32 resolves
is decided by rounding, whatever the code.  Every recording of this generator has such samples -- in the float64 restatement
alone, some 100 of a case's (hop, channel, band) triples have min |envelope - threshold| below 1e-6 of the window's amplitude
(the bound up to which tests/parity accepts a miss), 5 - 15 below 1e-7 and up to 9 below 3e-8, half an fp32 ulp of a value of
that amplitude.  The seed of a case is, among seed0 + 10 k (k = 0 .. 7; seed0 = 7001 .. 7005 in the order of the table), the
one with the FEWEST triples below 3e-8, ties to the larger minimum: a rule on the restatement's numbers only
(`python tests/burst_long_history_cases.py scan h2k 7001 7011 ...` prints them), taken before any kernel ran on them.  It
lowers the number of coin tosses; it cannot bring it to zero.  The fixture
(tests/golden/make_golden_burst_long_history.py) stores generator parameters, settings, channels, columns and the reference's
table -- not the recordings."""

from __future__ import annotations

import json

import numpy as np

CASES = {
    "h2k": {"seed": 7041, "sfreq": 2000, "time_duration_s": 70, "hops": 800, "full_from": 691, "growth": 1.0},
    "h4k": {"seed": 7032, "sfreq": 4000, "time_duration_s": 35, "hops": 400, "full_from": 341, "growth": 1.0},
    "h4k_steep": {"seed": 7063, "sfreq": 4000, "time_duration_s": 35, "hops": 400, "full_from": 341, "growth": 20.0},
    "h1k": {"seed": 7044, "sfreq": 1000, "time_duration_s": 140, "hops": 1500, "full_from": 1391, "growth": 1.0},
    # the default history (30 s at the 75th percentile) on 1 s windows at 12 kHz: K = 90 001, 1200 samples per hop.  The fill launch
    # takes 18 hops, the tiled kernel the rest; its pc / ps / ins arrays are 12 004 long (a power of two would not fit LDS)
    "r12k": {"seed": 7065, "sfreq": 12000, "time_duration_s": 30, "threshold": 75, "hops": 25, "full_from": None, "growth": 1.0,
             "K": 90001},
}
FIXTURE_TAGS = ["h2k", "h4k"]
K = 70001
BANDS = ["low_beta", "high_beta"]


def recording(p) -> np.ndarray:
    """[2, T] float64 holding float32 values: noise + a 17 Hz line with a slow amplitude modulation, all of it growing
    linearly to (1 + growth) times its first amplitude, + a per-channel offset."""
    sfreq = int(p["sfreq"])
    W, hop = sfreq, sfreq // 10
    T = W + (int(p["hops"]) - 1) * hop
    rng = np.random.default_rng(int(p["seed"]))
    t = np.arange(T) / sfreq
    x = ((rng.standard_normal((2, T)) * 30 + 20 * np.sin(2 * np.pi * 17 * t) * (1 + 0.8 * np.sin(2 * np.pi * 0.37 * t)))
         * (1 + p["growth"] * t / t[-1]) + rng.uniform(-20, 20, (2, 1)))
    return x.astype(np.float32).astype(np.float64)


def settings_of(nm, p):
    """The case's settings on package `nm` (this project's, or the reference's in the fixture's generator)."""
    s = nm.NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.bursts = True
    s.bursts_settings.threshold = p.get("threshold", 50)
    s.bursts_settings.time_duration_s = p["time_duration_s"]
    s.bursts_settings.frequency_bands = list(BANDS)
    s.sampling_rate_features_hz = 10
    s.segment_length_features_ms = 1000
    return s


def list_entries(p) -> int:
    return int(np.floor((1 - p.get("threshold", 50) / 100) * (int(p["sfreq"] * p["time_duration_s"]) - 1))) + 2


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def load_case(tag):
    """-> (parameters, settings, channels, columns, the reference's table or None)."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd import channels as chmod

    p = CASES[tag]
    assert list_entries(p) == p.get("K", K)
    if tag not in FIXTURE_TAGS:
        s = settings_of(nm, p).validate()
        return p, s, chmod.get_default_channels_from_data(np.zeros((2, 4))), None, None
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("burst_long_history")
    assert json.loads(str(g["params_json"]))[tag] == p, "the fixture was generated from other parameters"
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


_ORACLE = {}


def oracle_table(tag, x, s, ch):
    """The float64 restatement's table of a case, computed once per process, with the hops' sample ranges."""
    if tag not in _ORACLE:
        from oracle import nm_oracle as orc

        sfreq = float(CASES[tag]["sfreq"])
        rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
        cols = list(rows[0])
        assert all(list(r) == cols for r in rows)
        tab = np.array([[r[c] for c in cols] for r in rows])
        tab.setflags(write=False)
        starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
        _ORACLE[tag] = (cols, tab, starts, ends)
    return _ORACLE[tag]


def _assert_input_exercises_threshold(tag, p, cols, tab):
    """A condition on the INPUT: with the ring full, at least half of the rows have a burst, per (channel, band)."""
    if p["full_from"] is None:   # (the ring does not fill in this case: every hop's rank moves)
        return
    full = tab[p["full_from"]:]
    dm = [c for c in cols if c.endswith("_duration_mean")]
    assert len(dm) == 2 * len(BANDS), dm
    for c in dm:
        share = float(np.mean(full[:, cols.index(c)] != 0))
        print(f"{tag}: ring-full rows with a non-zero {c}: {share:.2f}")
        assert share >= 0.5, f"{tag}: {c} is non-zero in {share:.2f} of the ring-full rows: the table would pass with any threshold"


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
    """Stream.run of case `tag` on library `lib` against the fixture (where the case has one) and the oracle.
    -> {family: misses accepted on a conditioning report}."""
    from py_neuromodulation_amd.stream import Stream
    from tests import parity

    p, s, ch, cols, want = load_case(tag)
    sfreq = float(p["sfreq"])
    W = int(sfreq)
    x = recording(p)
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    got = df.to_numpy(float)
    ocols, tab, starts, ends = oracle_table(tag, x, s, ch)
    assert list(df.columns) == ocols, tag
    assert got.shape == tab.shape == (p["hops"], len(ocols)), (tag, got.shape, tab.shape)
    _assert_input_exercises_threshold(tag, p, ocols, tab)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = dict(parity.STATS["forgiven"])
    if want is not None:
        assert cols == ocols and want.shape == got.shape, tag
        np.testing.assert_array_equal(got[:, -1], want[:, -1])
        _against(tag, "fixture", ocols, got, want, s, sfreq, x, W, pv)
    _against(tag, "oracle", ocols, got, tab, s, sfreq, x, W, pv)
    after = parity.STATS["forgiven"]
    acc = {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}
    print(f"{tag}: accepted misses {acc}")
    return acc


# ---- one engine, several process_batch calls ------------------------------------------------------------------------------
def _engine(lib, tag):
    from py_neuromodulation_amd.engine import HotPathEngine

    p, s, _, _, _ = load_case(tag)
    return HotPathEngine(s, ["ch0", "ch1"], float(p["sfreq"]), **_kw(lib))


def _feed(eng, x32, at, calls, sfreq):
    """`calls` process_batch calls from hop `at` on -> (their rows, kernels of stage 4 after each call)."""
    W, hop = sfreq, sfreq // 10
    rows, kernels = [], []
    for n in calls:
        seg = np.ascontiguousarray(x32[:, at * hop:(at + n - 1) * hop + W])
        rows.append(eng.process_batch(seg, np.arange(n, dtype=np.int64) * hop).copy())
        kernels.append(eng.kernels(4))
        at += n
    return np.concatenate(rows), kernels


def run_batches(lib, tag, calls):
    p = CASES[tag]
    assert sum(calls) == p["hops"]
    x32 = recording(p).astype(np.float32)
    eng = _engine(lib, tag)
    try:
        return _feed(eng, x32, 0, calls, int(p["sfreq"]))
    finally:
        eng.close()


H2K_BATCHES_A = (128, 512) + (1,) * 60 + (100,)   # one-hop calls across hop 691, where the ring fills
H2K_BATCHES_B = (300, 300, 200)
_H2K = {}


def h2k_rows(lib, which):
    """The h2k table through process_batch in batches A or B, once per (library, batches): (rows, kernels per call)."""
    key = (id(lib), which)
    if key not in _H2K:
        rows, kernels = run_batches(lib, "h2k", H2K_BATCHES_A if which == "A" else H2K_BATCHES_B)
        rows.setflags(write=False)
        _H2K[key] = (rows, kernels)
    return _H2K[key]


def batching_gives_same_bytes(lib):
    a, _ = h2k_rows(lib, "A")
    b, _ = h2k_rows(lib, "B")
    assert a.shape == b.shape and np.isfinite(a).all()
    assert a.tobytes() == b.tobytes(), f"rows that differ: {np.flatnonzero((a != b).any(axis=1))[:10]}"


def state_travels(lib, at=720):
    """Export at hop `at` of h2k (the ring is full: 70 001 entries x 4 sequences), import into a fresh engine, continue: the
    rows from there on are the uninterrupted run's, bit for bit."""
    p = CASES["h2k"]
    want, _ = h2k_rows(lib, "B")
    x32 = recording(p).astype(np.float32)
    sfreq = int(p["sfreq"])
    e1 = _engine(lib, "h2k")
    try:
        head, _ = _feed(e1, x32, 0, (at,), sfreq)
        blob = e1.export_state()
    finally:
        e1.close()
    assert len(blob) >= 4 * K * 4
    assert head.tobytes() == want[:at].tobytes()
    e2 = _engine(lib, "h2k")
    try:
        e2.import_state(blob)
        tail, _ = _feed(e2, x32, at, (p["hops"] - at,), sfreq)
        assert tail.tobytes() == want[at:].tobytes(), f"rows that differ: {at + np.flatnonzero((tail != want[at:]).any(axis=1))[:10]}"
        e2.reset_state()   # ... and a reset stream starts over: the first rows again
        again, _ = _feed(e2, x32, 0, (40,), sfreq)
        assert again.tobytes() == want[:40].tobytes()
    finally:
        e2.close()


def wave_walk_beyond_64k_lds(setenv, delenv):
    """The one-wave walk keeps K / 64 + 2 block counters of its flush in LDS: beyond ~639 000 entries its launch asks for more
    than 64 KiB.  1 kHz, 720 s at the 10th percentile: K = 648 001 (65.7 KiB), ring full from hop 7191.  Device only: 7300
    hops in two calls, the second -- behind hop 7191 -- on nmx_kern_burst_thr_wave<2, false>, against the same stream with
    NMX_THR_WAVE=0 (the tiled workgroup kernel throughout), bit for bit; the growing recording keeps samples entering."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    p = {"seed": 7005, "sfreq": 1000, "time_duration_s": 720, "hops": 7300, "growth": 1.0}
    s = settings_of(nm, p)
    s.bursts_settings.threshold = 10
    s = s.validate()
    x32 = recording(p).astype(np.float32)
    out = {}
    for wave in ("1", "0"):
        setenv("NMX_THR_WAVE", wave)
        try:
            eng = HotPathEngine(s, ["ch0", "ch1"], 1000.0)
        finally:
            delenv("NMX_THR_WAVE")
        try:
            out[wave] = _feed(eng, x32, 0, (7200, 100), 1000)
        finally:
            eng.close()
    (rows, kernels), (rows0, kernels0) = out["1"], out["0"]
    assert "nmx_kern_burst_thr_wave<2, false>" in kernels[1] and "tiled" not in kernels[1], kernels[1]
    assert "nmx_kern_burst_thr_tiled" in kernels0[1] and "wave" not in kernels0[1], kernels0[1]
    assert np.isfinite(rows).all()
    tail = rows[7200:]
    assert (tail != tail[0]).any(), "the rows behind hop 7200 do not move: the walk is not exercised"
    assert rows.tobytes() == rows0.tobytes(), f"rows that differ: {np.flatnonzero((rows != rows0).any(axis=1))[:10]}"


def over_limit_raises(lib):
    """K = 1 100 000 > 1 048 576: refused when the plan is built, before the state (8.8 MB here, any size in general) is
    allocated; the message names the limit and the three settings."""
    import pytest

    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    p = {"sfreq": 1000, "time_duration_s": 1100}
    s = settings_of(nm, p)
    s.bursts_settings.threshold = 0
    with pytest.raises(ValueError) as e:
        HotPathEngine(s.validate(), ["ch0", "ch1"], 1000.0, **_kw(lib)).close()
    msg = str(e.value)
    assert "1 048 576" in msg and "1100000" in msg, msg
    for word in ("threshold", "time_duration_s", "sampling rate"):
        assert word in msg, msg


def at_limit_builds(lib):
    """K = 1 048 576 exactly (1 048 576 Hz-seconds at threshold 0: K = min(n_ring + 1, n_ring)) builds: 2 x 2 x 4 MB of state."""
    import py_neuromodulation_amd as nm
    from py_neuromodulation_amd.engine import HotPathEngine

    s = settings_of(nm, {"sfreq": 1024, "time_duration_s": 1024})
    s.bursts_settings.threshold = 0
    HotPathEngine(s.validate(), ["ch0", "ch1"], 1024.0, **_kw(lib)).close()


# ---- the seeds' rule (module docstring): the float64 restatement alone ---------------------------------------------------------
def oracle_margins(tag, seed):
    """min |envelope - threshold| / max |window| of every (hop, channel, band) of case `tag` with `seed`, ascending."""
    import py_neuromodulation_amd as nm
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from tests import parity

    p = dict(CASES[tag], seed=seed)
    s = settings_of(nm, p).validate()
    x = recording(p)
    sfreq = float(p["sfreq"])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, 10, 1000)
    pv = parity.PipelineVerifiers(s, chmod.get_default_channels_from_data(np.zeros((2, 4))), sfreq, x, starts, int(sfreq), line_noise=50,
                                  ends=ends)
    m = []
    for i in range(p["hops"]):
        tr = pv._burst_trace(i)
        amp = np.abs(pv.window(i)).max(axis=1)
        m += [orc.burst_decision_margin(tr.last_env[c, b], tr.last_thr[c, b]) / amp[c] for c in range(2) for b in range(len(BANDS))]
        pv._cache.pop(i, None)
    return np.sort(np.array(m))


if __name__ == "__main__":
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    if len(sys.argv) >= 4 and sys.argv[1] == "scan":
        for seed in sys.argv[3:]:
            m = oracle_margins(sys.argv[2], int(seed))
            print(sys.argv[2], seed, "below 3e-8:", int((m < 3e-8).sum()), "below 1e-7:", int((m < 1e-7).sum()), "below 1e-6:",
                  int((m < 1e-6).sum()), "smallest:", f"{m[0]:.1e}")
