"""Cases of the nolds Hurst-exponent tests, shared by the emulator tier (tests/test_nolds_hurst_cpu.py) and the GPU tier
(tests/test_nolds_hurst_gpu.py): every function takes the library to run on (the logic emulator, or None: libnmx.so).

What is judged and against what.  Every entry goes through nmx_nolds_hurst_probe, which runs a batch and hands back per
(window, series, channel) the kernel's (R/S)_n and kept-chunk count of every scale, its H, sum flag and number of kept
scales AND the float32 series it read:
  * (R/S)_n -- the float64 restatement (tests/nolds_hurst_oracle.py) on THAT series, to 1e-5 relative (tests/parity.py's
    policy); NaN exactly where the oracle keeps no chunk;
  * kept chunks per scale, kept scales and the sum flag -- exact;
  * H -- the oracle's final np.polyfit over its own (R/S)_n, to 1e-5 max(1, sum |w_k|) absolute, w_k the exact sensitivity of
    the slope to ln (R/S)_{n_k} over the kept scales (oracle.h_limit); NaN where the oracle has NaN; the row holds the
    float32 of that H, or 0 under the reference's sum rule;
  * the series -- as tests/nolds_dfa_cases.py has it (tests/nolds_probe_cases.py: check_series / fir_limit).
No entry is excused: the only decision in the measure, r == 0, is exact for constant chunks and far from rounding otherwise.
The series kinds and their groups are those of tests/nolds_dfa_cases.py.
"""

from __future__ import annotations

import json
import math

import numpy as np

from tests import nolds_dfa_cases as dfa_cases
from tests import nolds_hurst_oracle as oracle
from tests import nolds_probe_cases as base
from tests.helpers import load_golden, settings_from_json

HURST = "hurst_exponent"
DFA = dfa_cases.DFA
FIT = {HURST: "poly", DFA: "poly"}
# 5, 8: the tables [2, 3], [2, 3, 4] (the scale rule's lower end); 16, 50, 100: 3, 8 and 11 scales; 256 | 257: one wave of 16
# teams of 4 lanes | four waves, teams of 16; 333: ragged rounds; 1000: the default window; 1500: band series longer than the
# filters; 8192 | 8193: teams of 16 | of 64 lanes (a wave per scale)
LENGTHS = [5, 8, 16, 50, 100, 256, 257, 333, 1000, 1500, 8192, 8193]
TABLE_FACTS = {5: [2, 3], 8: [2, 3, 4], 16: [3, 4, 5], 50: list(range(4, 12)), 100: list(range(6, 17)),
               1000: [13, 15, 17, 19, 21, 24, 27, 30, 33, 38, 42, 47, 53, 60, 67], 16400: (15, 38, 312, 366),
               40000: (15, 53, None, 630)}
KINDS, GROUPS, series_of = dfa_cases.KINDS, dfa_cases.GROUPS, dfa_cases.series_of
WORST = {"RS": 0.0, "H": 0.0, "H_share": 0.0}   # largest deviations seen by this process (printed by judge_probe)


def hurst_settings(bands=(), raw=True, sampen=False, dfa=False):
    s = base.nolds_settings(bands, raw)
    s.nolds_settings.features = {"sample_entropy": bool(sampen), HURST: True, DFA: bool(dfa)}
    return s


def engine(lib, names=("a",), W=1000, bands=(), raw=True, sampen=False, dfa=False, nolds_fit=FIT, **kw):
    from py_neuromodulation_amd.engine import HotPathEngine

    return HotPathEngine(hurst_settings(bands, raw, sampen, dfa), list(names), 1000.0, features=["nolds"], window=W, lib=lib,
                         nolds_fit=nolds_fit, **kw)


def table(d):
    return [d.nolds_hurst_scales[k] for k in range(d.nolds_hurst_n_scales)]


def judge_probe(p: dict, col_of, d_pre, what: str) -> dict:
    """Every (window, series, channel) entry of a probe against the oracle on the series the kernel read.  col_of(series,
    channel) -> column of the entry in p["out"]; d_pre[C]: the constants the plan carries next to its raw series."""
    n_w, n_s, n_c = p["hurst"].shape
    nv = [int(n) for n in p["scales"]]
    assert np.allclose(p["log_expected"], np.log([oracle.expected_rs(n) for n in nv]), rtol=0, atol=1e-14)
    worst = {"RS": 0.0, "H": 0.0, "H_share": 0.0, "n": 0}
    for w in range(n_w):
        for s in range(n_s):
            for c in range(n_c):
                xs = p["series"][w, s, c].astype(np.float64)
                rs, kept = oracle.rs_values(xs, nv)
                got_rs, got_h, row = p["RS"][w, s, c], float(p["hurst"][w, s, c]), float(p["out"][w, col_of(s, c)])
                where = f"{what}: window {w} series {s} channel {c}"
                worst["n"] += 1
                assert np.array_equal(p["kept"][w, s, c], kept), (where, p["kept"][w, s, c], kept)
                live = ~np.isnan(rs)
                assert np.all(np.isnan(got_rs[~live])), (where, got_rs, rs)
                rel = np.abs(got_rs[live] - rs[live]) / rs[live]
                if rel.size:
                    worst["RS"] = max(worst["RS"], float(rel.max()))
                    assert float(rel.max()) <= 1e-5, (where, float(rel.max()), got_rs, rs)
                assert int(p["n_kept"][w, s, c]) == int(np.count_nonzero(live)), where
                want = oracle.slope(nv, rs)
                if math.isnan(want):
                    assert math.isnan(got_h), (where, got_h)
                else:
                    lim = oracle.h_limit(np.asarray(nv)[live])
                    err = abs(got_h - want)
                    worst["H"] = max(worst["H"], err)
                    worst["H_share"] = max(worst["H_share"], err / lim)
                    assert err <= lim, (where, got_h, want, lim)
                # the sum rule: the float64 sum of the series (with the constant the plan carries next to a raw series)
                dc = float(d_pre[c]) if (d_pre is not None and s == 0 and len(d_pre)) else 0.0
                zero = bool(xs.sum() + xs.size * dc == 0.0)
                assert bool(p["sum_zero"][w, s, c]) == zero, where
                if zero:
                    assert row == 0.0, (where, row)
                elif math.isnan(got_h):
                    assert math.isnan(row), (where, row)
                else:
                    assert row == float(np.float32(got_h)), (where, row, got_h)
    for k in WORST:
        WORST[k] = max(WORST[k], worst[k])
    print(f"{what}: {worst['n']} entries, largest (R/S) error {worst['RS']:.3e} (limit 1e-5), largest H error "
          f"{worst['H']:.3e} ({worst['H_share']:.2e} of its limit); this process so far {WORST}")
    return worst


def _series_check(p, w, raw64, d_pre, taps, what):
    base.check_series({"A": p["hurst"], "series": p["series"]}, w, raw64, d_pre, taps, what)


def check_kinds(lib, W: int, group: str, hops: int = 3, bands=()) -> dict:
    """One group of series kinds as the channels of one plan, `hops` windows a tenth of a window apart."""
    kinds = GROUPS[group]
    step = max(1, W // 10)
    T = W + step * (hops - 1)
    x = np.stack([series_of(k, T, seed=W + i) for i, k in enumerate(kinds)])
    eng = engine(lib, names=kinds, W=W, bands=bands, raw=True)
    starts = np.arange(hops) * step
    p = eng.nolds_hurst_probe(x, starts)
    assert p["scales"].tolist() == oracle.scales(W)
    d_pre = eng.offsets()[1]
    taps = base.default_taps()[:len(bands)]
    C = len(kinds)
    for w, a in enumerate(starts):
        _series_check(p, w, np.nan_to_num(x[:, a:a + W]), d_pre, taps, f"W = {W} group {group}")
    worst = judge_probe(p, lambda s, c: s * C + c, d_pre, f"W = {W} group {group}")
    # what the kinds are there for
    if group == "e":   # constant: every chunk has r == 0, no scale is left
        assert np.all(np.isnan(p["out"][:, 0])) and not p["sum_zero"].any() and np.all(p["n_kept"] == 0) and not p["kept"].any()
    if group == "c":
        assert np.all(p["out"][:, 0] == 0.0) and p["sum_zero"][:, 0, 0].all() and not p["kept"][:, 0, 0].any()   # all zero
        if W % 2 == 0:   # (the zigzag has ranges: 0 is the sum rule, not the fit)
            assert np.all(p["out"][:, 1] == 0.0) and p["sum_zero"][:, 0, 1].all() and np.all(p["n_kept"][:, 0, 1] >= 2)
    if group == "d":   # NaN samples read as 0
        assert np.all(np.isfinite(p["series"])) and np.all(np.isfinite(p["out"]))
    if group == "b" and W >= 100:   # the offset is carried next to the window, not inside the float32 samples
        assert abs(float(d_pre[0]) - 1e5) < 10.0 and float(np.max(np.abs(p["series"][:, 0, 0]))) < 100.0
    assert np.array_equal(p["out"], eng.process_batch(x, starts), equal_nan=True)   # (the plain batch computes the same)
    return worst


def check_long_window_bands(lib, W: int = 16400) -> dict:
    """a window above 16 384 samples with a band series: the long-window FIR path feeds the kernel; E's switch from the gamma
    quotient to the asymptote lies inside the table (312 | 366)"""
    kinds = ["noise", "cumsum"]
    hops, step = 2, 500
    x = np.stack([series_of(k, W + step * (hops - 1), seed=W + i) for i, k in enumerate(kinds)])
    eng = engine(lib, names=kinds, W=W, bands=["low_beta"])
    p = eng.nolds_hurst_probe(x, np.arange(hops) * step)
    assert p["scales"].tolist() == oracle.scales(W) and len(p["scales"]) == 15 and p["scales"][-2:].tolist() == [312, 366]
    taps = base.default_taps()[:1]
    for w in range(hops):
        _series_check(p, w, x[:, w * step:w * step + W], eng.offsets()[1], taps, f"W = {W}")
    return judge_probe(p, lambda s, c: s * 2 + c, eng.offsets()[1], f"W = {W} with a band")


def check_limit_length(lib, kind: str, W: int = 40000) -> dict:
    """the longest series: one channel, one hop"""
    x = series_of(kind, W, seed=7)[None]
    eng = engine(lib, names=[kind], W=W)
    p = eng.nolds_hurst_probe(x, np.array([0]))
    assert len(p["scales"]) == 15 and (p["scales"][0], p["scales"][-1]) == (53, 630)
    _series_check(p, 0, np.nan_to_num(x), eng.offsets()[1], [], f"W = {W} {kind}")
    return judge_probe(p, lambda s, c: c, eng.offsets()[1], f"W = {W} {kind}")


# ---- constructed series ------------------------------------------------------------------------------------------------------
KEPT_HELD = [62, 53, 47, 42, 39, 34, 31, 27, 25, 21, 20, 18, 15, 13, 12]
CHUNKS_1000 = [76, 66, 58, 52, 47, 41, 37, 33, 30, 26, 23, 21, 18, 16, 14]


def constructed_series() -> dict:
    """The constructed series at N = 1000, in float32 values like every series the kernel reads: n equal float32 samples sum
    exactly in float64, so the mean of a constant chunk is the sample and r == 0 holds exactly (of n equal arbitrary float64
    values it does not: their sum rounds)."""
    rng = np.random.default_rng(77)
    noise = (rng.standard_normal(1000) * 20 + 3.0).astype(np.float32).astype(np.float64)
    outlier = noise.copy()
    outlier[-1] = 1e6
    held = noise.copy()
    held[300:500] = held[300]
    spike = np.zeros(1000)
    spike[417] = 5.0
    return {"noise": noise, "outlier": outlier, "held": held, "spike": spike, "constant": np.full(1000, -7.25),
            "zigzag": np.tile([1.0, -1.0], 500)}


def check_constructed_oracle() -> None:
    """What the constructed series are built to show, on the oracle alone (no library)."""
    x = constructed_series()
    nv = oracle.scales(1000)
    assert all(1000 % n >= 1 for n in nv) and [1000 // n for n in nv] == CHUNKS_1000
    rs0, k0 = oracle.rs_values(x["noise"])
    rs1, k1 = oracle.rs_values(x["outlier"])
    assert np.array_equal(rs0, rs1) and np.array_equal(k0, k1) and k0.tolist() == CHUNKS_1000   # (the tail is dropped)
    assert oracle.rs_values(x["held"])[1].tolist() == KEPT_HELD
    rs, k = oracle.rs_values(x["spike"])
    assert k.tolist() == [1] * 15 and np.all(np.isfinite(rs)) and math.isfinite(oracle.hurst(x["spike"]))
    rs, k = oracle.rs_values(x["constant"])
    assert np.all(np.isnan(rs)) and not k.any() and math.isnan(oracle.hurst(x["constant"]))
    assert oracle.series_value(x["zigzag"]) == 0 and math.isfinite(oracle.hurst(x["zigzag"]))


def check_constructed(lib) -> dict:
    """The constructed series through the kernel: an outlier in the dropped tail, a held stretch (kept-chunk counts), a single
    spike (one chunk per scale), a constant (NaN), alternating +-1 (0 by the sum rule)."""
    x = constructed_series()
    names = ["noise", "outlier", "held", "spike", "zigzag"]
    data = np.stack([x[k] for k in names])
    eng = engine(lib, names=names, W=1000)
    p = eng.nolds_hurst_probe(data, np.array([0]))
    d_pre = eng.offsets()[1]
    worst = judge_probe(p, lambda s, c: c, d_pre, "constructed")
    assert p["series"][0, 0, 1, -1] > 1e5   # (the outlier is in the series the kernel read, and in no chunk)
    assert np.array_equal(p["RS"][0, 0, 0], p["RS"][0, 0, 1]) and p["hurst"][0, 0, 0] == p["hurst"][0, 0, 1]
    assert p["out"][0, 0] == p["out"][0, 1]
    assert p["kept"][0, 0, 0].tolist() == CHUNKS_1000 and p["kept"][0, 0, 2].tolist() == KEPT_HELD
    assert p["kept"][0, 0, 3].tolist() == [1] * 15 and p["n_kept"][0, 0, 3] == 15 and math.isfinite(p["out"][0, 3])
    assert p["out"][0, 4] == 0.0 and p["sum_zero"][0, 0, 4] and math.isfinite(p["hurst"][0, 0, 4]) and p["n_kept"][0, 0, 4] == 15
    # a constant series (a plan of its own: its level is carried next to the float32 samples)
    eng = engine(lib, names=["constant"], W=1000)
    p = eng.nolds_hurst_probe(x["constant"][None], np.array([0]))
    judge_probe(p, lambda s, c: c, eng.offsets()[1], "constant")
    assert np.all(np.isnan(p["RS"])) and not p["kept"].any() and math.isnan(p["out"][0, 0]) and not p["sum_zero"].any()
    return worst


def check_two_sample_chunks(lib) -> None:
    """N = 5 .. 8: every chunk of the scale n = 2 that is not constant has r / s = 1 / sqrt(2)"""
    a = np.array([1.0, 3.0, 2.0, 7.0, 4.0, 9.0, 5.0, 8.0])
    b = np.array([1.0, 3.0, 4.0, 4.0, 2.0, 9.0, 5.0, 8.0])   # (samples 2, 3: a constant chunk at n = 2, left out)
    for W in (5, 6, 7, 8):
        eng = engine(lib, names=["a", "b"], W=W)
        p = eng.nolds_hurst_probe(np.stack([a[:W], b[:W]]), np.array([0]))
        assert p["scales"][0] == 2
        judge_probe(p, lambda s, c: c, eng.offsets()[1], f"W = {W}")
        assert p["kept"][0, 0, :, 0].tolist() == [W // 2, W // 2 - 1]
        assert np.all(np.abs(p["RS"][0, 0, :, 0] - 1.0 / math.sqrt(2.0)) < 1e-15)


def check_amplitudes(lib) -> None:
    """H does not see the amplitude: one noise series scaled by powers of ten from 1e-16 to 1e16 (exactly representable
    scalings of the float32 samples they are not -- every series is judged against the oracle on what the kernel read, and
    all of them against the unscaled H within the limit)."""
    noise = np.random.default_rng(5).standard_normal(1000).astype(np.float32).astype(np.float64)
    amps = [1e-16, 1e-8, 1.0, 1e8, 1e16]
    nv = oracle.scales(1000)
    h1 = oracle.hurst(noise)
    for a in amps:   # (one plan each: the engine carries a common scale-dependent constant per plan)
        eng = engine(lib, names=["x"], W=1000)
        p = eng.nolds_hurst_probe((noise * a)[None], np.array([0]))
        judge_probe(p, lambda s, c: c, eng.offsets()[1], f"amplitude {a:g}")
        # float32 rounding of the scaled samples moves every (R/S)_n by about 2^-24 relative: far inside the limit
        assert abs(float(p["hurst"][0, 0, 0]) - h1) <= oracle.h_limit(nv), (a, p["hurst"], h1)


def check_refusals(lib) -> None:
    """what the library itself refuses of a Hurst plan description"""
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

    create(lambda d, e: setattr(d, "nolds_hurst_fit", 0), NotImplementedError, "RANSAC")
    create(lambda d, e: setattr(d, "nolds_hurst_fit", 2), ValueError, "nolds_hurst_fit")
    create(lambda d, e: setattr(d, "nolds_hurst_n_scales", 1), ValueError, "2 .. 15 scales")
    create(lambda d, e: setattr(d, "nolds_hurst_n_scales", 16), ValueError, "2 .. 15 scales")
    create(lambda d, e: setattr(d, "window", 12), ValueError, "ascend within")   # (the table of 200 samples reaches 25)
    with pytest.raises(ValueError, match="no Hurst kernel"):
        dfa_cases.engine(lib, W=50).nolds_hurst_probe(np.ones((1, 50)), np.array([0]))
    with pytest.raises(ValueError, match="no DFA kernel"):
        engine(lib, W=50).nolds_dfa_probe(np.ones((1, 50)), np.array([0]))
    with pytest.raises(ValueError, match="sample-entropy"):
        engine(lib, W=50).nolds_probe(np.ones((1, 50)), np.array([0]))


def check_other_columns_unchanged(lib, bands=("low_beta",)) -> None:
    """The sample-entropy and DFA columns of a plan with all three measures are bit-identical to those of the plans without
    Hurst, and the Hurst columns to those of a plan with Hurst alone; a batch equals the same windows one by one."""
    W, C, hops = 1000, 2, 4
    x = base.noise(4, C, W + 100 * (hops - 1))
    x[1] = np.cumsum(x[1] - x[1].mean())
    starts = np.arange(hops) * 100
    names = ["a", "b"]
    three = engine(lib, names=names, W=W, bands=bands, sampen=True, dfa=True)
    only_s = base.engine(lib, names=names, W=W, bands=bands)
    only_d = dfa_cases.engine(lib, names=names, W=W, bands=bands)
    two = dfa_cases.engine(lib, names=names, W=W, bands=bands, sampen=True)
    only_h = engine(lib, names=names, W=W, bands=bands)
    rows = three.process_batch(x, starts)
    se = [i for i, k in enumerate(three.keys) if "_sample_entropy_" in k]
    he = [i for i, k in enumerate(three.keys) if f"_{HURST}_" in k]
    de = [i for i, k in enumerate(three.keys) if f"_{DFA}_" in k]
    n = C * (1 + len(bands))
    assert len(se) == len(he) == len(de) == n and sorted(se + he + de) == list(range(len(three.keys)))
    assert all(se[i] + 1 == he[i] and he[i] + 1 == de[i] for i in range(n))   # (get_enabled() order inside a series and a channel)
    assert [three.keys[i] for i in se] == only_s.keys and [three.keys[i] for i in de] == only_d.keys
    assert [three.keys[i] for i in he] == only_h.keys and [three.keys[i] for i in sorted(se + de)] == two.keys
    assert np.array_equal(rows[:, se].view(np.uint32), only_s.process_batch(x, starts).view(np.uint32))
    assert np.array_equal(rows[:, de].view(np.uint32), only_d.process_batch(x, starts).view(np.uint32))
    assert np.array_equal(rows[:, sorted(se + de)].view(np.uint32), two.process_batch(x, starts).view(np.uint32))
    assert np.array_equal(rows[:, he].view(np.uint32), only_h.process_batch(x, starts).view(np.uint32))
    assert np.all(np.isfinite(rows))
    single = engine(lib, names=names, W=W, bands=bands, sampen=True, dfa=True)
    for w, a in enumerate(starts):
        one = single.process_window(x[:, a:a + W])
        assert np.array_equal(np.asarray(one, np.float32).view(np.uint32), rows[w].view(np.uint32)), w


# ---- the reference-generated fixture (tests/golden/make_golden_nolds_hurst.py) ----------------------------------------------
def _fixture(tag):
    g = load_golden("nolds_hurst")
    s = settings_from_json(g[f"{tag}_settings_json"])
    channels = json.loads(str(g[f"{tag}_channels_json"]))
    return g, s, channels, g[f"{str(g[f'{tag}_recording'])}_data"]


def measure_fixture(lib, tag: str) -> dict:
    """The reference's own Stream.run table against Stream.run here.  -> the largest relative deviation of a Hurst column
    from the fixture."""
    from py_neuromodulation_amd.stream import Stream

    g, s, channels, data = _fixture(tag)
    df = Stream(sfreq=1000.0, channels=channels, settings=s, line_noise=50, lib=lib, nolds_fit=FIT).run(data, save_csv=False)
    cols = [str(c) for c in g[f"{tag}_columns"]]
    assert list(df.columns) == cols
    got, want = df.to_numpy(dtype=np.float64), g[f"{tag}_values"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0.0, want == 0.0)
    h_cols = [j for j, c in enumerate(cols) if f"_{HURST}_" in c]
    assert h_cols
    ok = ~np.isnan(want[:, h_cols]) & (want[:, h_cols] != 0.0)
    rel = np.abs(got[:, h_cols] - want[:, h_cols])[ok] / np.abs(want[:, h_cols])[ok]
    out = {"engine": float(rel.max()), "entries": int(ok.sum())}
    print(f"fixture {tag}: {out}")
    return out


def check_fixture_pipeline(lib, tag: str) -> None:
    """Stream.run here against the reference's table: its columns in its order, NaN where it has NaN, 0 where it has 0 (the
    sum rule), and every Hurst value within tests/parity.py's 1e-5 of the reference's."""
    m = measure_fixture(lib, tag)
    assert m["engine"] <= 1e-5, m


def check_fixture_oracle(tag: str) -> None:
    """The float64 pipeline (oracle/nm_oracle.py) rebuilds the series the reference saw: the fixture's Hurst values are the
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
            if f"_nolds_{HURST}_" not in col or math.isnan(want[r, j]):
                continue
            ch, sname = col.split(f"_nolds_{HURST}_")
            y = y64[names.index(ch)]
            if sname != "raw":
                y = np.convolve(y, taps[bands.index(sname)], "same")
            assert abs(float(oracle.series_value(y)) - want[r, j]) <= 1e-9, (col, r)
            n += 1
    assert n > 0


def check_fixture_direct(lib, tag: str) -> None:
    """Stand-alone Nolds(settings, ch_names, sfreq, nolds_fit={...}).calc_feature: the reference's keys in its order, the
    fused path's values, 0 where the reference has 0, and the Hurst values to 1e-5 of the reference's (the window is only
    cast to float32 here)."""
    from py_neuromodulation_amd.features import HotPathFeatures, Nolds

    g, s, _, data = _fixture(tag)
    names = [str(c) for c in g["ch_names"]]
    x = data[:, :1000]
    got = Nolds(s, names, 1000.0, lib=lib, nolds_fit=FIT).calc_feature(x)
    keys = [str(k) for k in g[f"d{tag}_keys"]]
    assert list(got) == keys
    want = dict(zip(keys, g[f"d{tag}_values"]))
    fused = HotPathFeatures(s, names, 1000.0, lib=lib, nolds_fit=FIT).calc_feature(x)
    assert list(fused) == keys
    assert all((math.isnan(fused[k]) and math.isnan(got[k])) or fused[k] == got[k] for k in keys)
    assert all((want[k] == 0.0) == (got[k] == 0.0) for k in keys)
    n = 0
    for k in keys:
        if f"_{HURST}_" in k and want[k] != 0.0:
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
            n += 1
    assert n > 0
