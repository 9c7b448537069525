"""Cases of the nolds (sample entropy) tests, shared by the emulator tier (tests/test_nolds_cpu.py) and the GPU tier
(tests/test_nolds_gpu.py): every function takes the library to run on (the logic emulator, or None: libnmx.so).

What is judged and against what:
Every entry is judged in two separate steps, both through nmx_nolds_probe, which runs a batch and hands back per (window,
series, channel) the kernel's A, B, tol and sum flag AND the float32 series the walk read:
  * the counting -- the oracle's conditioning report (tests/nolds_oracle.py) on THAT series, with delta = 2^-23 (|d| + tol),
    the float32 rounding of a difference and of tol, and nothing else.  An entry without an undecided pair must have the
    oracle's A and B exactly and its value to 1e-5; one with undecided pairs must have counts inside [A-, A+] x [B-, B+]
    and a value inside its interval widened by 1e-5.  The share of entries with an undecided pair comes from the oracle
    alone and is asserted to be at most 10 % in every test (`judge_probe`);
  * the series -- the raw series against the float64 pipeline's windows, the band series against the float64 convolution
    of the raw series with the taps of the bank position the reference's quirk picks, sample by sample within the FIR
    kernels' documented limit (profiles/fir_sample_probes.md: 64 eps32 max(rms(x), max|y64|)) (`check_series`).
On integer-valued series (integer taps for the bands) every difference is exact and tol is irrational: no pair is
undecided anywhere and the counts are the oracle's, at every length where the kernel's shape changes.
The reference-generated fixture (tests/golden/make_golden_nolds.py) pins keys, order, quirk, nan_to_num, sum rule and NaN
rows by the reference's own Nolds class and DataProcessor; only `sampen` is restated.
"""

from __future__ import annotations

import json
import math

import numpy as np

from tests import nolds_oracle as oracle
from tests.helpers import load_golden, settings_from_json

# 3 .. 6: the first lengths with 0, 1, 2, 3 diagonals; 63 .. 66, 127 .. 132: a wave's worth of diagonal pairs (T / 2 = 64 at
# N = 130, 131) and around it; 255 .. 258: one wave -> four (N <= 256 runs 64 threads); 514 .. 516: T / 2 = 256 diagonal pairs,
# one round of four waves -> two; 1000: the default window; 8191 .. 8194: four waves -> sixteen (N <= 8192 runs 256 threads);
# 16 319 .. 16 321: the longest series whose LDS layout (series + 64 floats) stays within 64 KiB, and the first that needs the
# launch helper's opt-in; 40 000: the limit
LENGTHS = [3, 4, 5, 6, 63, 64, 65, 66, 127, 128, 129, 130, 131, 132, 255, 256, 257, 258, 514, 515, 516, 1000,
           8191, 8192, 8193, 8194, 16319, 16320, 16321, 40000]
MAX_N = 40000
PLUS_INF_SERIES = [0, 5, 9, -9, -7, 6, 9, -5, -4, 7, -1]   # B = 1, A = 0 (found by search; the oracle confirms it in the test)


def nolds_settings(bands=(), raw=True):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.features.nolds = True
    s.nolds_settings.raw = raw
    s.nolds_settings.frequency_bands = list(bands)
    s.nolds_settings.features = {"sample_entropy": True}
    s.postprocessing.feature_normalization = False
    return s


def engine(lib, names=("a",), W=1000, bands=(), raw=True, **kw):
    from py_neuromodulation_amd.engine import HotPathEngine

    return HotPathEngine(nolds_settings(bands, raw), list(names), 1000.0, features=["nolds"], window=W, lib=lib, **kw)


def integer_series(n: int, seed: int) -> np.ndarray:
    """Small integers with rare large steps: eight values, so tol (about 0.2 std) spans a few of the unit steps."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4, n) + 30 * (rng.random(n) < 0.2)).astype(np.float64)


def integer_margin(x) -> float:
    """distance of tol from the nearest integer (every difference of an integer series is one)"""
    tol = oracle.tolerance(x)
    return abs(tol - round(tol)) if tol == tol else math.inf


def probe_one(lib, x, **kw) -> dict:
    """one window of len(x[0]) samples through a plan of that window length"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    eng = engine(lib, names=[f"c{i}" for i in range(x.shape[0])], W=x.shape[1], **kw)
    return eng.nolds_probe(x, np.array([0]))


def judge_probe(p: dict, col_of, what: str, max_share: float = 0.1) -> dict:
    """Every (window, series, channel) entry of a probe against the conditioning report on the series the kernel read.
    col_of(series, channel) -> column of the entry in p["out"]."""
    n_w, n_s, n_c = p["A"].shape
    stats = {"n": 0, "ambiguous": 0}
    for w in range(n_w):
        for s in range(n_s):
            for c in range(n_c):
                cond = oracle.conditioning(p["series"][w, s, c])
                A, B, got = int(p["A"][w, s, c]), int(p["B"][w, s, c]), float(p["out"][w, col_of(s, c)])
                where = f"{what}: window {w} series {s} channel {c}: A, B = {A}, {B}, value {got!r}; report {cond}"
                stats["n"] += 1
                t = float(p["tol"][w, s, c])
                assert (math.isnan(t) and math.isnan(cond["tol"])) or abs(t - cond["tol"]) <= 2.0 ** -23 * cond["tol"], where
                if bool(p["sum_zero"][w, s, c]) or cond["zero"]:
                    assert got == 0.0 and not p["series"][w, s, c].any(), where
                    continue
                if cond["ambiguous"] == 0:
                    v = cond["value"]
                    assert (A, B) == (cond["A"], cond["B"]), where
                    assert (math.isnan(got) and math.isnan(v)) or got == v or abs(got - v) <= 1e-5, where
                else:
                    stats["ambiguous"] += 1
                    assert cond["A_lo"] <= A <= cond["A_hi"] and cond["B_lo"] <= B <= cond["B_hi"], where
                    assert cond["lo"] - 1e-5 <= got <= cond["hi"] + 1e-5, where
    print(f"{what}: {stats['n']} entries, {stats['ambiguous']} with an undecided pair")
    assert stats["ambiguous"] <= max_share * stats["n"], (what, stats)
    return stats


def fir_limit(x, y) -> float:
    """per-sample limit of the FIR kernels (profiles/fir_sample_probes.md)"""
    return 64.0 * 2.0 ** -24 * max(float(np.sqrt(np.mean(np.square(x)))), float(np.max(np.abs(y))), 1e-30)


def check_series(p: dict, w: int, raw64: np.ndarray, d_pre, taps, what: str, raw_limit=None) -> None:
    """The series the walk read in window w: series 0 (when the plan has raw) against raw64[C, W] -- the float64 windows,
    d_pre[C] the constants the plan carries next to them --, band series j against raw64 filtered with taps[j]."""
    n_s, n_c = p["A"].shape[1:]
    first_band = n_s - len(taps)
    for c in range(n_c):
        if first_band:
            lim = raw_limit[c] if raw_limit is not None else 2.0 ** -24 * float(np.max(np.abs(raw64[c])))
            err = float(np.max(np.abs(p["series"][w, 0, c].astype(np.float64) + d_pre[c] - raw64[c])))
            assert err <= lim, f"{what}: window {w} raw channel {c}: {err!r} > {lim!r}"
        for j, h in enumerate(taps):
            y = np.convolve(raw64[c], h, "same")
            lim = fir_limit(raw64[c], y) + (raw_limit[c] * float(np.sum(np.abs(h))) if raw_limit is not None else 0.0)
            err = float(np.max(np.abs(p["series"][w, first_band + j, c].astype(np.float64) - y)))
            assert err <= lim, f"{what}: window {w} band {j} channel {c}: {err!r} > {lim!r}"


def check_exact_counts(lib, n: int) -> None:
    x = integer_series(n, seed=n)
    assert integer_margin(x) > 1e-3 or n < 4
    want = oracle.counts(x) if n <= 2000 else oracle.counts_small_integers(x)
    if 100 <= n <= 2000:
        assert want == oracle.counts_small_integers(x)   # (the two restatements agree where both are affordable)
    p = probe_one(lib, x)
    got = (int(p["A"][0, 0, 0]), int(p["B"][0, 0, 0]))
    tol = oracle.tolerance(x)
    print(f"N = {n}: A, B = {got} (oracle {want}), tol = {float(p['tol'][0, 0, 0])!r} (oracle {tol!r})")
    assert np.array_equal(p["series"][0, 0, 0], x.astype(np.float32))
    assert got == want
    if tol == tol:
        assert abs(float(p["tol"][0, 0, 0]) - tol) <= 2.0 ** -23 * tol
    else:
        assert math.isnan(float(p["tol"][0, 0, 0]))
    v, w = float(p["out"][0, 0]), oracle.series_value(x)
    assert (math.isnan(v) and math.isnan(w)) or v == np.float32(w) or abs(v - w) <= 1e-6 * abs(w)


def check_edge_values(lib) -> None:
    def run(x):
        p = probe_one(lib, x)
        return float(p["out"][0, 0]), int(p["A"][0, 0, 0]), int(p["B"][0, 0, 0]), bool(p["sum_zero"][0, 0, 0])

    v, a, b, z = run(np.full(50, 3.5))            # constant, non-zero: tol = 0, no pair
    assert math.isnan(v) and (a, b, z) == (0, 0, False)
    v, a, b, z = run(np.zeros(50))                 # all zero: the sum rule
    assert v == 0.0 and z
    zig = np.tile([1.0, -1.0], 32)                 # sum exactly 0: the reference returns 0 here as well
    v, a, b, z = run(zig)
    assert v == 0.0 and z and oracle.series_value(zig) == 0
    for short in ([2.0], [1.0, 2.0], [1.0, 2.0, 4.0]):   # N < 4: no pair of templates
        v, a, b, z = run(short)
        assert math.isnan(v) and (a, b, z) == (0, 0, False) and math.isnan(oracle.series_value(short))
    assert oracle.counts(PLUS_INF_SERIES) == (0, 1)
    v, a, b, z = run(PLUS_INF_SERIES)
    assert v == math.inf and (a, b, z) == (0, 1, False)
    # cleaned like any window: NaN -> 0, infinities -> the largest float32
    p = probe_one(lib, [np.nan, 1.0, np.inf, 2.0, 1.0, 2.0, -np.inf, 1.0])
    f = float(np.finfo(np.float32).max)
    assert p["series"][0, 0, 0].tolist() == [0.0, 1.0, f, 2.0, 1.0, 2.0, -f, 1.0]


def check_limit(lib) -> None:
    """a longer series is refused, and the message states the limit: by the plan description and by the library"""
    import ctypes as C

    import pytest

    from py_neuromodulation_amd import _lib

    with pytest.raises(ValueError, match="40000"):
        engine(None, W=MAX_N + 1, dry_run=True)
    d = engine(None, W=MAX_N, dry_run=True).desc
    d.window = MAX_N + 1
    L = lib if lib is not None else _lib.get_library()
    plan = C.c_void_p()
    with pytest.raises(ValueError, match="40 000"):
        L.check(L.lib.nmx_plan_create(C.byref(d), C.byref(plan)))


def noise(seed: int, C: int, T: int, sfreq: float = 1000.0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(T) / sfreq
    return rng.standard_normal((C, T)) * 50 + 10 * np.sin(2 * np.pi * 20 * t) + rng.uniform(-200, 200, (C, 1))


def check_noise_raw(lib, seed: int, W: int = 1000, C: int = 3, hops: int = 6) -> None:
    """raw series of seeded noise through a plan, hop by hop"""
    x = noise(seed, C, W + 100 * (hops - 1))
    eng = engine(lib, names=[f"c{i}" for i in range(C)], W=W)
    p = eng.nolds_probe(x, np.arange(hops) * 100)
    d_pre = eng.offsets()[1]
    for w in range(hops):
        check_series(p, w, x[:, 100 * w:100 * w + W], d_pre, [], f"seed {seed}")
    judge_probe(p, lambda s, c: c, f"noise seed {seed}")
    assert np.array_equal(p["out"], eng.process_batch(x, np.arange(hops) * 100), equal_nan=True)   # (the plain batch computes the same)


INT_TAPS = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 0, 1, 0, 1], [1, 1, 1, 1, 1]], np.float64)   # theta, alpha, low_beta, high_beta


def check_band_index_quirk(lib, W: int) -> None:
    """Integer taps, integer data: the band series are exact integers up to the FIR kernels' rounding.  nolds' bands
    ["low_beta", "high_beta"] read the bank's series 0 and 1 -- theta's and alpha's filters -- under their own names; the
    kernel's counts on them are the oracle's."""
    C = 2
    x = np.stack([integer_series(W, seed=100 + W + c) for c in range(C)])
    eng = engine(lib, names=["a", "b"], W=W, bands=["low_beta", "high_beta"], bank_taps=INT_TAPS)
    assert eng.keys == [f"{ch}_nolds_sample_entropy_{s}" for s in ("raw", "low_beta", "high_beta") for ch in ("a", "b")]
    p = eng.nolds_probe(x, np.array([0]))
    check_series(p, 0, x, eng.offsets()[1], INT_TAPS[:2], f"W = {W}")
    for si, row in enumerate((None, 0, 1)):
        for c in range(C):
            y = x[c] if row is None else np.convolve(x[c], INT_TAPS[row], "same")
            assert integer_margin(y) > 1e-2
            want = oracle.counts(y) if W <= 2000 else oracle.counts_small_integers(y)
            got = (int(p["A"][0, si, c]), int(p["B"][0, si, c]))
            print(f"W = {W} series {si} channel {c}: A, B = {got}, oracle {want}")
            assert got == want and want[0] > 0
            assert abs(float(p["out"][0, si * C + c]) - oracle.value(*want)) <= 2.0 ** -22 * oracle.value(*want)
    # the filters that the names would suggest give other counts
    assert oracle.counts_small_integers(np.convolve(x[0], INT_TAPS[2], "same")) != (int(p["A"][0, 1, 0]), int(p["B"][0, 1, 0]))


def check_long_window_bands(lib, W: int = 16400) -> None:
    """a window above 16 384 samples with band series: the long-window FIR path feeds the stage"""
    check_band_index_quirk(lib, W)


def default_taps():
    from py_neuromodulation_amd import fir_design

    return fir_design.band_pass_bank([tuple(v) for v in nolds_settings().frequency_ranges_hz.values()], 1000.0)


def check_band_default_taps(lib, seed: int = 5) -> None:
    """Default taps, seeded noise, three hops: the band series the stage wrote against the float64 convolution of the raw
    series with the taps of bank positions 0 and 1, and the kernel's counts on the series it read."""
    W, C, hops = 1000, 2, 3
    x = noise(seed, C, W + 100 * (hops - 1))
    eng = engine(lib, names=["a", "b"], W=W, bands=["low_beta", "theta"])
    p = eng.nolds_probe(x, np.arange(hops) * 100)
    taps = default_taps()[:2]   # (series i of the bank for nolds band i: the quirk)
    for w in range(hops):
        check_series(p, w, x[:, 100 * w:100 * w + W], eng.offsets()[1], taps, "default taps")
    judge_probe(p, lambda s, c: s * C + c, "default taps")


def check_fixture_pipeline(lib, tag: str) -> None:
    """The reference's own Stream.run table (tests/golden/make_golden_nolds.py).
    1. Stream.run here gives the reference's columns in its order, NaN where it has NaN (a window that held a NaN) and 0 where
       it has 0 (the sum rule).
    2. The float64 pipeline (oracle/nm_oracle.py) rebuilds the series the reference saw: the fixture's values are the
       restatement's on them, to 1e-9 -- the reference side of the comparison is understood.
    3. The engine's side: the probe of the same plan on the same recording.  Its rows are Stream.run's; the series its walk
       read are the float64 pipeline's within the pre-processing's limit (check_series); and its counts are judged on those
       series (judge_probe).  A reference value and an engine value differ where the float32 pre-processing moved a pair
       across tol -- one pair is 1 / A of a value -- which is why the values themselves are not compared at 1e-5."""
    import copy

    from oracle import nm_oracle
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.stream import Stream

    g = load_golden("nolds")
    s = settings_from_json(g[f"{tag}_settings_json"])
    channels = json.loads(str(g[f"{tag}_channels_json"]))
    data = g[f"{tag}_data"]
    df = Stream(sfreq=1000.0, channels=channels, settings=s, line_noise=50, lib=lib).run(data, save_csv=False)
    cols = [str(c) for c in g[f"{tag}_columns"]]
    assert list(df.columns) == cols
    got, want = df.to_numpy(dtype=np.float64), g[f"{tag}_values"]
    feat = [j for j, c in enumerate(cols) if c != "time"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0.0, want == 0.0)
    # 2. the reference side
    s64 = copy.deepcopy(s)
    s64.features.nolds = False
    s64.features.raw_hjorth = True
    ref = nm_oracle.DataProcessor(1000.0, s64, channels, 50)
    starts, ends, _ = nm_oracle.window_schedule(data.shape[1], 1000.0, s.sampling_rate_features_hz, s.segment_length_features_ms)
    assert len(starts) == got.shape[0]
    bands = list(s.nolds_settings.frequency_bands)
    taps = default_taps()[:len(bands)]
    names = ref.ch_names_used
    y64 = [ref.preprocess(np.nan_to_num(data[:, a:b])[ref.feature_idx, :]) for a, b in zip(starts, ends)]
    for r in range(len(starts)):
        for j in feat:
            ch, sname = cols[j].split("_nolds_sample_entropy_")
            y = y64[r][names.index(ch)]
            if sname != "raw":
                y = np.convolve(y, taps[bands.index(sname)], "same")
            if not math.isnan(want[r, j]):
                assert abs(float(oracle.series_value(y)) - want[r, j]) <= 1e-9, (cols[j], r)
    # 3. the engine side
    dp = DataProcessor(1000.0, s, channels, line_noise=50, verbose=False, lib=lib)
    assert dp.keys == [cols[j] for j in feat]
    p = dp.engine.nolds_probe(data, np.asarray(starts))
    ok = ~np.isnan(got[:, feat])
    assert np.array_equal(p["out"].astype(np.float64)[ok], got[:, feat][ok])
    d_pre = dp.engine.offsets()[1]
    for r, (a, b) in enumerate(zip(starts, ends)):
        w = np.nan_to_num(data[:, a:b])
        # float32 cast and re-reference, then the notch kernel's per-sample limit
        lim = [8.0 * 2.0 ** -24 * float(np.max(np.abs(w))) + fir_limit(w, y64[r][c]) for c in range(len(names))]
        check_series(p, r, y64[r], d_pre, taps, f"fixture {tag}", raw_limit=lim)
    C = len(names)
    judge_probe(p, lambda si, c: si * C + c, f"fixture {tag}")


def check_fixture_direct(lib, tag: str) -> None:
    """Stand-alone Nolds(settings, ch_names, sfreq).calc_feature: the reference's keys in its order, the fused path's values,
    and -- no pre-processing here, the window is only cast to float32 -- the probe's rows, judged as everywhere."""
    from py_neuromodulation_amd.features import HotPathFeatures, Nolds

    g = load_golden("nolds")
    s = settings_from_json(g[f"{tag}_settings_json"])
    names = [str(c) for c in g["ch_names"]]
    x = g[f"{tag}_data"][:, :1000]
    alone = Nolds(s, names, 1000.0, lib=lib)
    got = alone.calc_feature(x)
    keys = [str(k) for k in g[f"d{tag}_keys"]]
    assert list(got) == keys
    want = dict(zip(keys, g[f"d{tag}_values"]))
    fused = HotPathFeatures(s, names, 1000.0, lib=lib).calc_feature(x)   # (nolds is the only feature enabled)
    assert list(fused) == keys
    assert all((math.isnan(fused[k]) and math.isnan(got[k])) or fused[k] == got[k] for k in keys)
    assert all((want[k] == 0.0) == (got[k] == 0.0) for k in keys)   # the sum rule: the all-zero channel
    # the probe of the same plan, over every hop of the recording (the first is the window above)
    rec = np.nan_to_num(g[f"{tag}_data"])
    starts = np.arange(0, rec.shape[1] - 1000 + 1, 100)
    taps = default_taps()[:len(s.nolds_settings.frequency_bands)]
    p = alone.engine.nolds_probe(rec, starts)
    assert all((math.isnan(got[k]) and math.isnan(v)) or got[k] == v for k, v in zip(keys, p["out"][0].astype(np.float64)))
    for w, a in enumerate(starts):
        check_series(p, w, rec[:, a:a + 1000], alone.engine.offsets()[1], taps, f"direct {tag}")
    C = len(names)
    judge_probe(p, lambda si, c: si * C + c, f"direct {tag}")
