"""Cases of the nolds detrended-fluctuation-analysis tests, shared by the emulator tier (tests/test_nolds_dfa_cpu.py) and the
GPU tier (tests/test_nolds_dfa_gpu.py): every function takes the library to run on (the logic emulator, or None: libnmx.so).

What is judged and against what.  Every entry goes through nmx_nolds_dfa_probe, which runs a batch and hands back per
(window, series, channel) the kernel's F(n) of every scale, its slope, sum flag and number of kept scales AND the float32
series it read:
  * F(n) -- the float64 restatement (tests/nolds_dfa_oracle.py: np.polyfit per chunk, no closed form) on THAT series, to
    1e-5 relative (tests/parity.py's policy); a scale the oracle has at exactly 0 must be exactly 0;
  * alpha -- the oracle's final np.polyfit over its own F, to 1e-5 max(1, sum |w_k|) absolute, w_k the exact sensitivity of
    the slope to ln F(n_k) over the kept scales (oracle.alpha_limit); NaN where the oracle has NaN; the row holds the
    float32 of that slope, or 0 under the reference's sum rule;
  * the series -- the raw series against the float64 windows, the band series against the float64 convolution with the taps
    the reference's index quirk picks, sample by sample (tests/nolds_probe_cases.py: check_series / fir_limit).
No entry is excused.
"""

from __future__ import annotations

import json
import math

import numpy as np

from tests import nolds_dfa_oracle as oracle
from tests import nolds_probe_cases as base
from tests.helpers import load_golden, settings_from_json

DFA = "detrended_fluctuation_analysis"
# 10: the table [8, 9]; 11, 70: the fixed table; 71: three scales; 200: one wave; 260: 128 chunks at n = 4, two full rounds of a wave; 333: 165
# chunks, a ragged last round; 1000: the default window (498 chunks at n = 4, 17 scales over four waves)
LENGTHS = [10, 11, 70, 71, 200, 260, 333, 1000]
TABLE_LENGTHS = [4, 10, 11, 70, 71, 200, 1000, 16400, 40000]
KINDS = ["noise", "cumsum", "am_sine", "offset_1e5", "tiny", "huge", "constant", "zero", "zigzag", "nan"]
# (the constant series has a plan of its own: a row whose level dwarfs its spread makes the engine carry every row's mean
# next to the float32 samples, and the float64 sum of a zigzag minus a rounded mean is no longer exactly 0)
GROUPS = {"a": ["noise", "cumsum", "am_sine"], "b": ["offset_1e5", "tiny", "huge"], "c": ["zero", "zigzag"],
          "d": ["nan"], "e": ["constant"]}


def dfa_settings(bands=(), raw=True, sampen=False):
    s = base.nolds_settings(bands, raw)
    s.nolds_settings.features = {"sample_entropy": bool(sampen), DFA: True}
    return s


def engine(lib, names=("a",), W=1000, bands=(), raw=True, sampen=False, nolds_fit="poly", **kw):
    from py_neuromodulation_amd.engine import HotPathEngine

    return HotPathEngine(dfa_settings(bands, raw, sampen), list(names), 1000.0, features=["nolds"], window=W, lib=lib,
                         nolds_fit=nolds_fit, **kw)


def series_of(kind: str, T: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(T) / 1000.0
    if kind == "noise":
        return rng.standard_normal(T) * 50 + 120.0
    if kind == "cumsum":
        return np.cumsum(rng.standard_normal(T) * 50)
    if kind == "am_sine":   # smooth: the residual of a four-sample chunk is a hundredth of its walk
        return (1.0 + 0.5 * np.sin(2 * np.pi * 0.7 * t)) * (30 * np.sin(2 * np.pi * 6 * t) + 12 * np.sin(2 * np.pi * 16 * t + 0.4))
    if kind == "offset_1e5":
        return rng.standard_normal(T) + 1e5
    if kind == "tiny":
        return rng.standard_normal(T) * 1e-12
    if kind == "huge":
        return rng.standard_normal(T) * 1e12
    if kind == "constant":
        return np.full(T, 3.5)
    if kind == "zero":
        return np.zeros(T)
    if kind == "zigzag":    # not constant, float64 sum exactly 0 over an even number of samples
        return np.tile([1.0, -1.0], T // 2 + 1)[:T]
    if kind == "nan":
        x = rng.standard_normal(T) * 50 + 20.0
        x[T // 3:T // 3 + max(1, T // 50)] = np.nan
        x[(2 * T) // 3] = np.nan
        return x
    raise ValueError(kind)


def judge_probe(p: dict, col_of, d_pre, what: str) -> dict:
    """Every (window, series, channel) entry of a probe against the oracle on the series the kernel read.  col_of(series,
    channel) -> column of the entry in p["out"]; d_pre[C]: the constants the plan carries next to its raw series."""
    n_w, n_s, n_c = p["alpha"].shape
    nv = [int(n) for n in p["scales"]]
    worst = {"F": 0.0, "alpha": 0.0, "alpha_limit_share": 0.0, "n": 0}
    for w in range(n_w):
        for s in range(n_s):
            for c in range(n_c):
                xs = p["series"][w, s, c].astype(np.float64)
                F = oracle.fluctuations(xs, nv)
                got_f, got_a, row = p["F"][w, s, c], float(p["alpha"][w, s, c]), float(p["out"][w, col_of(s, c)])
                where = f"{what}: window {w} series {s} channel {c}"
                worst["n"] += 1
                live = F != 0
                assert np.all(got_f[~live] == 0.0), (where, got_f, F)
                rel = np.abs(got_f[live] - F[live]) / F[live]
                if rel.size:
                    worst["F"] = max(worst["F"], float(rel.max()))
                    assert float(rel.max()) <= 1e-5, (where, float(rel.max()), got_f, F)
                assert int(p["n_kept"][w, s, c]) == int(np.count_nonzero(live)), where
                want = oracle.slope(nv, F)
                if math.isnan(want):
                    assert math.isnan(got_a), (where, got_a)
                else:
                    lim = oracle.alpha_limit(np.asarray(nv)[live])
                    err = abs(got_a - want)
                    worst["alpha"] = max(worst["alpha"], err)
                    worst["alpha_limit_share"] = max(worst["alpha_limit_share"], err / lim)
                    assert err <= lim, (where, got_a, want, lim)
                # the sum rule: the float64 sum of the series (with the constant the plan carries next to a raw series)
                dc = float(d_pre[c]) if (d_pre is not None and s == 0 and len(d_pre)) else 0.0
                zero = bool(xs.sum() + xs.size * dc == 0.0)
                assert bool(p["sum_zero"][w, s, c]) == zero, where
                if zero:
                    assert row == 0.0, (where, row)
                elif math.isnan(got_a):
                    assert math.isnan(row), (where, row)
                else:
                    assert row == float(np.float32(got_a)), (where, row, got_a)
    print(f"{what}: {worst['n']} entries, largest F error {worst['F']:.3e} (limit 1e-5), largest alpha error "
          f"{worst['alpha']:.3e} ({worst['alpha_limit_share']:.3f} of its limit)")
    return worst


def check_kinds(lib, W: int, group: str, hops: int = 3, bands=()) -> dict:
    """One group of series kinds as the channels of one plan, `hops` windows a tenth of a window apart."""
    kinds = GROUPS[group]
    step = max(1, W // 10)
    T = W + step * (hops - 1)
    x = np.stack([series_of(k, T, seed=W + i) for i, k in enumerate(kinds)])
    eng = engine(lib, names=kinds, W=W, bands=bands, raw=True)
    starts = np.arange(hops) * step
    p = eng.nolds_dfa_probe(x, starts)
    assert p["scales"].tolist() == oracle.scales(W)
    d_pre = eng.offsets()[1]
    taps = base.default_taps()[:len(bands)]
    C = len(kinds)
    for w, a in enumerate(starts):
        base.check_series({"A": p["alpha"], "series": p["series"]}, w, np.nan_to_num(x[:, a:a + W]), d_pre, taps, f"W = {W} group {group}")
    worst = judge_probe(p, lambda s, c: s * C + c, d_pre, f"W = {W} group {group}")
    # what the kinds are there for
    if group == "e":
        assert np.all(np.isnan(p["out"][:, 0])) and not p["sum_zero"].any() and np.all(p["n_kept"] == 0)
    if W % 2 == 0 and group == "c":
        assert np.all(p["out"] == 0.0) and p["sum_zero"].all()
        assert np.all(p["n_kept"][:, 0, 1] > 0)   # (the zigzag has fluctuations: 0 is the sum rule, not the fit)
    assert np.array_equal(p["out"], eng.process_batch(x, starts), equal_nan=True)   # (the plain batch computes the same)
    return worst


def check_orientation(lib) -> None:
    """The issue's orientation values in float64 at 1000 samples: noise about 0.58, its cumulative sum about 1.51, a 6 Hz
    sinusoid about 2.01 -- of the oracle and of the kernel.  (The sinusoid stands on an offset, which DFA does not see: over
    whole periods the FLOAT32 samples cancel half a period apart and sum to exactly 0 -- the sum rule's 0 -- while the float64
    ones do not.)"""
    rng = np.random.default_rng(0)
    n = rng.standard_normal(1000)
    x = np.stack([n, np.cumsum(n), np.sin(2 * np.pi * 6 * np.arange(1000) / 1000.0) + 0.25])
    p = engine(lib, names=["n", "c", "s"], W=1000).nolds_dfa_probe(x, np.array([0]))
    for c, (lo, hi) in enumerate([(0.4, 0.75), (1.3, 1.7), (1.9, 2.1)]):
        assert lo < oracle.dfa(x[c]) < hi and lo < float(p["out"][0, c]) < hi, (c, oracle.dfa(x[c]), p["out"][0])


def check_long_window_bands(lib, W: int = 16400) -> dict:
    """a window above 16 384 samples with a band series: the long-window FIR path feeds the kernel"""
    kinds = ["noise", "cumsum"]
    hops, step = 2, 500
    x = np.stack([series_of(k, W + step * (hops - 1), seed=W + i) for i, k in enumerate(kinds)])
    eng = engine(lib, names=kinds, W=W, bands=["low_beta"])
    p = eng.nolds_dfa_probe(x, np.arange(hops) * step)
    assert p["scales"].tolist() == oracle.scales(W) and len(p["scales"]) == 32 and p["scales"][-1] == 1367
    taps = base.default_taps()[:1]
    for w in range(hops):
        base.check_series({"A": p["alpha"], "series": p["series"]}, w, x[:, w * step:w * step + W], eng.offsets()[1], taps, f"W = {W}")
    return judge_probe(p, lambda s, c: s * 2 + c, eng.offsets()[1], f"W = {W} with a band")


def check_limit_length(lib, kind: str, W: int = 40000) -> dict:
    """the longest series: one channel, one hop"""
    x = series_of(kind, W, seed=7)[None]
    eng = engine(lib, names=[kind], W=W)
    p = eng.nolds_dfa_probe(x, np.array([0]))
    assert len(p["scales"]) == 37 and p["scales"][-1] == 3402
    base.check_series({"A": p["alpha"], "series": p["series"]}, 0, np.nan_to_num(x), eng.offsets()[1], [], f"W = {W} {kind}")
    return judge_probe(p, lambda s, c: c, eng.offsets()[1], f"W = {W} {kind}")


def check_refusals(lib) -> None:
    """what the library itself refuses of a DFA plan description"""
    import ctypes as C

    import pytest

    from py_neuromodulation_amd import _lib

    L = lib if lib is not None else _lib.get_library()
    plan = C.c_void_p()

    def create(edit, exc, match):
        eng = engine(None, W=200, dry_run=True)
        edit(eng.desc, eng)
        with pytest.raises(exc, match=match):
            L.check(L.lib.nmx_plan_create(C.byref(eng.desc), C.byref(plan)))

    create(lambda d, e: setattr(d, "nolds_dfa_fit", 0), NotImplementedError, "RANSAC")
    create(lambda d, e: setattr(d, "nolds_dfa_fit", 2), ValueError, "nolds_dfa_fit")
    create(lambda d, e: setattr(d, "nolds_dfa_n_scales", 1), ValueError, "2 .. 64 scales")
    create(lambda d, e: setattr(d, "window", 12), ValueError, "ascend within")   # (the table of 200 samples reaches 17)
    with pytest.raises(ValueError, match="no DFA kernel"):
        base.engine(lib, W=50).nolds_dfa_probe(np.ones((1, 50)), np.array([0]))
    with pytest.raises(ValueError, match="sample-entropy"):
        engine(lib, W=50).nolds_probe(np.ones((1, 50)), np.array([0]))


def check_sampen_columns_unchanged(lib, bands=("low_beta",)) -> None:
    """The sample-entropy columns of a plan with both measures are bit-identical to those of the same plan with sample
    entropy alone, and so are the DFA columns to those of a plan with DFA alone; a batch equals the same windows one by one."""
    W, C, hops = 1000, 2, 4
    x = base.noise(4, C, W + 100 * (hops - 1))
    x[1] = np.cumsum(x[1] - x[1].mean())
    starts = np.arange(hops) * 100
    names = ["a", "b"]
    both = engine(lib, names=names, W=W, bands=bands, sampen=True)
    only_s = base.engine(lib, names=names, W=W, bands=bands)
    only_d = engine(lib, names=names, W=W, bands=bands)
    rows = both.process_batch(x, starts)
    se = [i for i, k in enumerate(both.keys) if "_sample_entropy_" in k]
    de = [i for i, k in enumerate(both.keys) if f"_{DFA}_" in k]
    assert len(se) == len(de) == C * (1 + len(bands)) and sorted(se + de) == list(range(len(both.keys)))
    assert [both.keys[i] for i in se] == only_s.keys and [both.keys[i] for i in de] == only_d.keys
    assert np.array_equal(rows[:, se].view(np.uint32), only_s.process_batch(x, starts).view(np.uint32))
    assert np.array_equal(rows[:, de].view(np.uint32), only_d.process_batch(x, starts).view(np.uint32))
    assert np.all(np.isfinite(rows))
    single = engine(lib, names=names, W=W, bands=bands, sampen=True)
    for w, a in enumerate(starts):
        one = single.process_window(x[:, a:a + W])
        assert np.array_equal(np.asarray(one, np.float32).view(np.uint32), rows[w].view(np.uint32)), w


def _fixture(tag):
    g = load_golden("nolds_dfa")
    s = settings_from_json(g[f"{tag}_settings_json"])
    channels = json.loads(str(g[f"{tag}_channels_json"]))
    return g, s, channels, g[f"{str(g[f'{tag}_recording'])}_data"]


def measure_fixture(lib, tag: str) -> dict:
    """The reference's own Stream.run table (tests/golden/make_golden_nolds_dfa.py) against Stream.run here.
    -> the largest relative deviation of a DFA column from the fixture (`engine`), and that of the oracle run on the series
    the kernel itself read (`oracle_on_kernel_series`): what the float32 pre-processing in front of the series moved."""
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.stream import Stream

    g, s, channels, data = _fixture(tag)
    df = Stream(sfreq=1000.0, channels=channels, settings=s, line_noise=50, lib=lib, nolds_fit="poly").run(data, save_csv=False)
    cols = [str(c) for c in g[f"{tag}_columns"]]
    assert list(df.columns) == cols
    got, want = df.to_numpy(dtype=np.float64), g[f"{tag}_values"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0.0, want == 0.0)
    dfa_cols = [j for j, c in enumerate(cols) if f"_{DFA}_" in c]
    ok = ~np.isnan(want[:, dfa_cols]) & (want[:, dfa_cols] != 0.0)
    rel = np.abs(got[:, dfa_cols] - want[:, dfa_cols])[ok] / np.abs(want[:, dfa_cols])[ok]
    # the oracle on the kernel's own series
    dp = DataProcessor(1000.0, s, channels, line_noise=50, verbose=False, lib=lib, nolds_fit="poly")
    feat = [j for j, c in enumerate(cols) if c != "time"]
    assert dp.keys == [cols[j] for j in feat]
    starts = np.arange(0, data.shape[1] - 1000 + 1, 100)
    p = dp.engine.nolds_dfa_probe(data, starts)
    n_w, n_s, n_c = p["alpha"].shape
    nf = len(s.nolds_settings.features.get_enabled())
    own = 0.0
    for w in range(n_w):
        for si in range(n_s):
            for c in range(n_c):
                j = feat[(si * n_c + c) * nf + (nf - 1)]
                assert f"_{DFA}_" in cols[j]
                if not math.isnan(want[w, j]) and want[w, j] != 0.0:
                    own = max(own, abs(oracle.dfa(p["series"][w, si, c].astype(np.float64)) - want[w, j]) / abs(want[w, j]))
    out = {"engine": float(rel.max()), "oracle_on_kernel_series": own, "entries": int(ok.sum())}
    print(f"fixture {tag}: {out}")
    return out


def check_fixture_pipeline(lib, tag: str) -> None:
    """Stream.run here against the reference's table: its columns in its order, NaN where it has NaN, 0 where it has 0 (the
    sum rule), and every DFA value within tests/parity.py's 1e-5 of the reference's."""
    m = measure_fixture(lib, tag)
    assert m["engine"] <= 1e-5, m


def check_fixture_oracle(tag: str) -> None:
    """The float64 pipeline (oracle/nm_oracle.py) rebuilds the series the reference saw: the fixture's DFA values are the
    restatement's on them, to 1e-9 -- the reference side of the comparison is understood.  No device."""
    import copy

    from oracle import nm_oracle

    g, s, channels, data = _fixture(tag)
    cols = [str(c) for c in g[f"{tag}_columns"]]
    want = g[f"{tag}_values"]
    s64 = copy.deepcopy(s)
    s64.features.nolds = False
    s64.features.raw_hjorth = True
    ref = nm_oracle.DataProcessor(1000.0, s64, channels, 50)
    starts, ends, _ = nm_oracle.window_schedule(data.shape[1], 1000.0, s.sampling_rate_features_hz, s.segment_length_features_ms)
    assert len(starts) == want.shape[0]
    bands = list(s.nolds_settings.frequency_bands)
    taps = base.default_taps()[:len(bands)]
    names = ref.ch_names_used
    n = 0
    for r, (a, b) in enumerate(zip(starts, ends)):
        y64 = ref.preprocess(np.nan_to_num(data[:, a:b])[ref.feature_idx, :])
        for j, col in enumerate(cols):
            if f"_nolds_{DFA}_" not in col or math.isnan(want[r, j]):
                continue
            ch, sname = col.split(f"_nolds_{DFA}_")
            y = y64[names.index(ch)]
            if sname != "raw":
                y = np.convolve(y, taps[bands.index(sname)], "same")
            assert abs(float(oracle.series_value(y)) - want[r, j]) <= 1e-9, (col, r)
            n += 1
    assert n > 0


def check_fixture_direct(lib, tag: str) -> None:
    """Stand-alone Nolds(settings, ch_names, sfreq, nolds_fit="poly").calc_feature: the reference's keys in its order, the
    fused path's values, 0 where the reference has 0, and the DFA values to 1e-5 of the reference's (the window is only cast
    to float32 here)."""
    from py_neuromodulation_amd.features import HotPathFeatures, Nolds

    g, s, _, data = _fixture(tag)
    names = [str(c) for c in g["ch_names"]]
    x = data[:, :1000]
    got = Nolds(s, names, 1000.0, lib=lib, nolds_fit="poly").calc_feature(x)
    keys = [str(k) for k in g[f"d{tag}_keys"]]
    assert list(got) == keys
    want = dict(zip(keys, g[f"d{tag}_values"]))
    fused = HotPathFeatures(s, names, 1000.0, lib=lib, nolds_fit="poly").calc_feature(x)
    assert list(fused) == keys
    assert all((math.isnan(fused[k]) and math.isnan(got[k])) or fused[k] == got[k] for k in keys)
    assert all((want[k] == 0.0) == (got[k] == 0.0) for k in keys)
    for k in keys:
        if f"_{DFA}_" in k and want[k] != 0.0:
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
