"""Per-trough probes of the sharp-wave detector (nmx_k_sharpwave.h), shared by the emulator tier
(test_sharpwave_probes_cpu.py) and the MI355X tier (test_sharpwave_probes_gpu.py).

The only other comparison of this stage (tests/parity.py) filters in float64 and forgives every entry of a (channel,
filter) whose float64 series holds one near-tie anywhere in the window.  A probe takes the float32 series the detector
itself was given -- read out through filter_window on the same plan, widened exactly -- and runs the float64 restatement
(oracle.nm_oracle.analyze_waveform, both polarities; the estimators and the between-polarity step of SharpwaveAnalyzer on
top) on THAT series.  Comparisons of float32 numbers are exact in float64, so every decision of the reference (extremum or
not, which of two neighbours is higher, which peak flanks a trough) is the decision a correct kernel takes; only the
estimator arithmetic is left to a tolerance.  No verifier, no accepted miss, no row left out of a constructed case.

Inputs
  (a) constructed series behind identity taps [1.0]: piecewise-linear zigzags (`zigzag`) whose extrema sit at chosen
      positions (same-kind gaps of 2 samples and up), heights (H0 + Q level), the levels a seeded permutation (distinct
      within any 128 neighbours of a kind; distinct altogether up to 128 of a kind), the minima mirrored.  Conditions on
      every row (asserted by `check_inputs`, conditions and not measurements): oracle.sharpwave_decision_margin >= 1e-3
      max|x|, four orders of magnitude above the FIR's rounding, and the read-out within YARD_CAP = 16 eps32 max|x| of
      the input.  With these margins a batch kernel and the one-window kernel may round a sample differently.
      A second filter [-1.0] (cases `two_filters*`): its Peak results must equal filter 0's Trough results, which checks the
      (window, channel, filter) item arithmetic without the oracle.  One exactly-zero row per batch case: the one plateau
      the FIR delivers exactly; every output 0.  Plateaus of positive length cannot be delivered through an fp32 FFT
      convolution (equal neighbours do not stay equal), so the device plateau walk is NOT covered here.
  (b) noise: seeded white noise, sigma 50, 64 channels, the two default filters and default settings, one window per
      call; the read-out comes from filter_window on the same plan (stage-3 and stage-6 kernels of the two calls asserted
      equal).  A (channel, filter) whose read-out has a decision margin below 8 eps32 max|y| is left out (a near-tie could
      flip on a 2-ulp difference between two stores); at most 5 % may be, the share is printed and asserted.

Limits (derived; `value_err`, `estimate`, `between`), Y = max|y| of the row, v the per-trough values of the reference:
  num_peaks, width and trough / peak_left / peak_right under max / min   equal
  interval, rise_time, decay_time under max / min   2 eps32 |v|      (one float32 product with the rounded ms)
  prominence, sharpness, steepness under max / min  4 eps32 Y        (at most three roundings of numbers <= 2 Y)
  mean over n values      largest per-value error + (n - 1) eps32 mean|v| + 2 eps32 |result|   (any summation order)
  median                  as max / min, plus one rounding when n is even
  var                     the mean's bound on the squared deviations d, whose own error is 2 |d|max err(d) + eps32 d^2max,
                          err(d) = per-value error + err(mean) + eps32 |d|max; + 4 eps32 var (square root and square)
  between polarities      one more operation of the same kind on the two results and their limits
Sensitivity (`check_sensitivity`): every case estimates num_peaks, which is exact -- one trough more or less fails it
whatever n is; up to SENS_N = 512 troughs the mean interval is asserted too: one trough more or less moves it by 1 / n of
itself, which must be at least ten limits.  (Beyond ~1 000 troughs the summation bound (n - 1) eps32 passes 1 / (10 n):
the W = 8000 cases rest on the exact outputs -- num_peaks, and width under max / min for a pairing one peak off.)

    case            rate   W      C x hops  kind (GPU)   kernels(5)                    what it exercises
    extrema forms (distances 5 / 10, default estimators + num_peaks): extrema at 1 and W - 2, on both sides of every lane
    boundary (k chunk, 1 + k chunk), in the last partly filled lane; a zero row
    x1000 x963 x1026  1000  ..    4 x 2     DENSE_LIST   dense + todo                  chunk 16: the branch-free form
    x962 x1027        1000  ..    4 x 2     DENSE_LIST   dense + todo                  chunk 15 / 17: 64-bit mask form
    x512 x450         1000  ..    4 x 2     DENSE_LIST   dense + todo                  chunk 8 branch-free / chunk 7
    x66 x40           1000  ..    4 x 2     DENSE_LIST   dense + todo                  chunk 1
    x4098 x4099       4000  ..    4 x 1     DENSE_LIST   dense + todo                  chunk 64 (bit 63) / 65: two-pass
    x962_list x4098_list  ..  ..  4 x 2 / 1  LIST        nmx_kern_sharp                NMX_SW_DENSE=0: the mask form feeding full-length lists
    dense boundaries (W = 1000, distances 5 / 10)
    counts          1000   1000   8 x 1     DENSE_LIST   dense + todo                  64/64 64/65 65/64 65/65 128/128 128/129 129/128
    mixed           1000   1000   4 x 4     DENSE_LIST   dense + todo                  overflowing and other items mixed: todo index
    wrap            1000   1000   4 x 1     DENSE_LIST   dense + todo                  gap-2 run over raw elements 56..72; ramps of 100 gap-2 peaks
    pairing edges
    edges           1000   1000   8 x 2     DENSE_LIST   dense + todo                  0 extrema, one peak, one trough, peak-trough, trough-peak,
                                                                                       troughs before the first / behind the last kept peak
    list path: the dense rows again
    list_env        1000   1000   8 x 2     LIST         nmx_kern_sharp                NMX_SW_DENSE=0
    list_dist       1000   1000   8 x 2     LIST         nmx_kern_sharp                distances 25 / 40
    pairs_8k        8000   8000   2 x 1     LIST         nmx_kern_sharp                gap-2 zigzag, distances 1 / 1: ~4 000 pairs, 4 blocks of
                                                                                       the lf[] rewrite, step0 = 2048, sharp_off = 0
    pairs_8k_fv     8000   8000   2 x 1     LIST         nmx_kern_sharp                the same, distances 101 / 1: 50 troughs before the first
                                                                                       kept peak (kept peaks are >= 101 apart: the ~3 900 PAIRS
                                                                                       are troughs between the first and the last of them)
    estimators
    est_fast        1000   1000   8 x 2     DENSE_LIST   dense + todo                  every loop-free feature under mean, max, min: fast_est<1>
                                                                                       and <2> (a trough distance of 10 keeps at most 100 troughs
                                                                                       of 1000 samples: the strided loop beyond 128 runs in pairs_8k*)
    est_vals        1000   1000   8 x 2     LIST         nmx_kern_sharp                + median, var, the three steepness features
    sharp_250       250    250    4 x 2     DENSE_LIST   dense + todo                  sharp_off = 20: troughs at 20, 21, W - 21, W - 20
    sharp_1k        1000   1000   4 x 2     DENSE_LIST   dense + todo                  sharp_off = 5: troughs at 5, 6, W - 6, W - 5
    nobetween       1000   1000   4 x 2     DENSE_LIST   dense + todo                  apply_estimator_between_peaks_and_troughs off
    peaks_only / troughs_only  1000  1000  4 x 2  DENSE_LIST  dense + todo             one polarity
    two_filters     1000   1000   4 x 2     DENSE_LIST   dense + todo                  taps [1.0] and [-1.0]
    two_filters_list  1000  1000  4 x 2     LIST         nmx_kern_sharp                the same, NMX_SW_DENSE=0
    long window (identity taps [1.0] accepted as they are)
    long_dense      16000  16000  2 x 2     DENSE_SLAB   dense + nmx_kern_sharp_slab   sparse extrema; one row beyond 128 of a kind
    long_slab       16000  16000  2 x 2     SLAB         nmx_kern_sharp_slab           distances 25 / 40

(8 kHz cases: sharpness with sharp_off = 0 is identically 0.)  The emulator tier runs every case: its plans are of the LIST
kind with the host extrema walk whatever the settings (nmx_engine_plan_state.inc: dense = false under NMX_HOST_EMU), so it
validates inputs, glue and limits; the dense and slab kinds, the device extrema forms and the fast estimators run on the
MI355X only.  The figures observed are in profiles/sharpwave_probes.md."""

from __future__ import annotations

import math

import numpy as np

from tests.fir_sample_probe_cases import YARD_CAP, build_engine

EPS32 = float(np.finfo(np.float32).eps)
TAIL_SLOPE = 25.0
H0, Q = 1000.0, 8.0      # heights H0 + Q level, level < 556: Q / max|x| >= 1.4e-3
MARGIN = 1e-3            # decision margin of a constructed row, in units of max|x|
NOISE_MARGIN = 8.0       # ... of a noise row, in eps32 max|y|; rows below it are left out
NOISE_LEFT_OUT = 0.05
SENS_N, SENS_RATIO = 512, 10.0
FACTORS: dict = {}       # case -> factor on the limits where it is not 1 (at most 2; profiles/sharpwave_probes.md)
EXACT = ("width", "trough", "peak_left", "peak_right")
TIMES = ("interval", "rise_time", "decay_time")
FAST_FEATURES = ["peak_left", "peak_right", "trough", "width", "prominence", "interval", "decay_time", "rise_time", "sharpness"]
STEEP = ["rise_steepness", "decay_steepness", "slope_ratio"]
KERNELS = {"LIST": {"nmx_kern_sharp"}, "DENSE_LIST": {"nmx_kern_sharp_dense", "nmx_kern_sharp_todo"},
           "DENSE_SLAB": {"nmx_kern_sharp_dense", "nmx_kern_sharp_slab"}, "SLAB": {"nmx_kern_sharp_slab"}}


# ---- the plan's choices, restated (nmx_engine_plan_state.inc: build_sharp; test_sharpwave_probes_cpu.py ties them to the source)
def _al4(n: int) -> int:
    return (n + 3) & ~3


def plan_choice(W: int, sfreq: float, dp: float, dt: float, combos, env_dense: bool = True) -> dict:
    fast = all(e in ("mean", "max", "min") and f not in STEEP for f, e in combos if f != "num_peaks")
    dense_ok = bool(env_dense and fast and math.ceil(dp) <= 10 and math.ceil(dt) <= 10)
    pm = W // 2 + 2
    lw = _al4((pm + 1) // 2)
    tail = max(lw + _al4((2 * pm + 3) // 4), _al4(pm))
    lds_floats = _al4(W) + 5 * lw + tail + _al4(2 * len(combos) + 2) + 64
    slab = lds_floats * 4 > 160 * 1024
    kind = ("DENSE_SLAB" if dense_ok else "SLAB") if slab else ("DENSE_LIST" if dense_ok else "LIST")
    return {"kind": kind, "chunk": -(-(W - 2) // 64) if W > 2 else 0, "dense_ok": dense_ok, "fast_estimators": fast,
            "sharp_off": int(5.0 * (1000.0 / sfreq))}


def chunk_form(chunk: int) -> str:
    """The branch of the device nmx_extrema a window takes."""
    return "branchfree16" if chunk == 16 else "branchfree8" if chunk == 8 else "twopass" if chunk > 64 else "mask64"


# ---- constructed series -------------------------------------------------------------------------------------------------
def levels(n: int, rng) -> np.ndarray:
    """n levels below 256, distinct within any 128 neighbours: blocks of 128, a permutation each, the blocks' parities
    alternating."""
    out = np.empty(n, int)
    for b, a in enumerate(range(0, n, 128)):
        m = min(128, n - a)
        out[a:a + m] = 2 * rng.permutation(128)[:m] + (b & 1)
    return out


def zigzag(W: int, pos, first: str = "max", seed: int = 0, lev_max=None, lev_min=None) -> np.ndarray:
    """float32-exact series of W samples: extrema at `pos` (ascending, within [1, W - 2]) alternating from
    `first`, straight lines between them.  Heights: +(H0 + Q level) for maxima, -(H0 + Q level) for minima."""
    pos = np.asarray(pos, int)
    assert pos.size == 0 or (pos[0] >= 1 and pos[-1] <= W - 2 and np.all(np.diff(pos) >= 1)), pos
    rng = np.random.default_rng(seed)
    is_max = (np.arange(pos.size) % 2 == 0) == (first == "max")
    n_max, n_min = int(is_max.sum()), int((~is_max).sum())
    lev_max = levels(n_max, rng) if lev_max is None else np.asarray(lev_max)
    lev_min = levels(n_min, rng) if lev_min is None else np.asarray(lev_min)
    assert len(lev_max) == n_max and len(lev_min) == n_min
    h = np.empty(pos.size)
    h[is_max] = H0 + Q * lev_max
    h[~is_max] = -(H0 + Q * lev_min)
    if pos.size == 0:   # a monotone ramp
        return np.linspace(-H0, H0, W).astype(np.float32).astype(np.float64)
    # (the two ends: towards 0, or 25 a sample where that is steeper -- a long flat tail would be a near-tie of neighbours)
    ends = [h[0] - np.sign(h[0]) * max(abs(h[0]), TAIL_SLOPE * pos[0]), h[-1] - np.sign(h[-1]) * max(abs(h[-1]), TAIL_SLOPE * (W - 1 - pos[-1]))]
    z = np.interp(np.arange(W), np.concatenate([[0], pos, [W - 1]]), np.concatenate([ends[:1], h, ends[1:]]))
    return z.astype(np.float32).astype(np.float64)


def lane_positions(W: int) -> list[int]:
    """1 and W - 2, both sides of every lane boundary of the extrema pass (k chunk | 1 + k chunk), the last two
    positions of the last partly filled lane."""
    chunk = -(-(W - 2) // 64)
    p = {1, W - 2, W - 3}
    for k in range(1, 64):
        p |= {k * chunk, 1 + k * chunk}
    return sorted(q for q in p if 1 <= q <= W - 2)


def count_positions(W: int, n: int, seed: int, start: int = 1) -> np.ndarray:
    """n positions from `start` on that spread over the window: consecutive gaps drawn from 1 .. 2 (W - 2 - start) / n - 1,
    the largest shortened until the last position fits."""
    room = W - 2 - start
    g = max(2 * room // max(n, 1) - 1, 1)
    gaps = np.random.default_rng(seed).integers(1, g + 1, size=n)
    gaps[0] = 0
    while gaps.sum() > room:
        gaps[np.argmax(gaps)] -= 1
    return start + np.cumsum(gaps)


def gap_positions(gaps, start: int = 1) -> np.ndarray:
    g = np.asarray(gaps, int).copy()
    g[0] = 0
    return start + np.cumsum(g)


def count_row(W, n_max, n_min, seed):
    """Exactly n_max maxima and n_min minima (|n_max - n_min| <= 1)."""
    return zigzag(W, count_positions(W, n_max + n_min, seed), "max" if n_max >= n_min else "min", seed)


def rows_extrema(W: int) -> list[np.ndarray]:
    lp = lane_positions(W)
    fill = sorted(set(count_positions(W, max((W - 3) // 9, 1), W).tolist()) | {1, W - 2})
    return [zigzag(W, lp, "max", W), zigzag(W, lp, "min", W + 1), zigzag(W, fill, "max", W + 2), np.zeros(W),
            zigzag(W, fill, "min", W + 3), zigzag(W, lp[:-2], "min", W + 4), zigzag(W, lp[1:], "max", W + 5),
            zigzag(W, lp[::2], "max", W + 6)]


def rows_counts(W: int = 1000) -> list[np.ndarray]:
    return [count_row(W, a, b, 10 * a + b) for a, b in ((64, 64), (64, 65), (65, 64), (65, 65), (128, 128), (128, 129), (129, 128))] + \
        [np.zeros(W)]


def rows_mixed(W: int = 1000) -> list[np.ndarray]:
    """4 channels x 4 hops: items beyond 128 extrema of a kind at scattered (hop, channel) places."""
    n = [(40, 40), (129, 128), (64, 65), (130, 130), (200, 200), (12, 11), (128, 128), (128, 129),
         (0, 0), (150, 151), (129, 129), (65, 65), (90, 90), (33, 34), (249, 249), (128, 127)]
    return [np.zeros(W) if a == 0 else count_row(W, a, b, 7 * a + b + i) for i, (a, b) in enumerate(n)]


def rows_wrap(W: int = 1000) -> list[np.ndarray]:
    """A run of gap-2 extrema (consecutive gap 1) over raw elements 56..72 of both kinds, gaps of 6 around it; an ascending
    and a descending ramp of 100 gap-2 peaks (the longest fixed-point chain), the troughs ramping the other way."""
    gaps = [6] * 112 + [1] * 34 + [6] * 14
    run = gap_positions(gaps)
    pre, post = list(range(10, 290, 14)), list(range(510, 986, 14))   # (an even number in front: the ramp starts with `first`)
    ramp = pre + list(range(300, 500)) + post
    flat = lambda lv: np.concatenate([150 + np.arange(len(pre) // 2), lv, 170 + np.arange(len(post) // 2)])   # noqa: E731
    up, dn = flat(np.arange(100)), flat(np.arange(100)[::-1])
    return [zigzag(W, run, "max", 1), zigzag(W, run, "min", 2),
            zigzag(W, ramp, "max", 3, lev_max=up, lev_min=dn), zigzag(W, ramp, "min", 4, lev_max=dn, lev_min=up)]


def rows_edges(W: int = 1000) -> list[np.ndarray]:
    mid = list(range(100, 900, 15))
    # (a minimum, a low maximum, a minimum, a high maximum 4 samples behind the low one: under distance 5 the low one goes,
    # and with it every peak between the two troughs)
    before = [2, 9, 12, 13] + list(range(30, 900, 15))
    # (mirrored at the end: a high maximum, a minimum, a low maximum 4 samples behind the high one, a minimum)
    behind = list(range(30, 900, 15)) + [900, 901, 904, 914]
    lv = lambda seed, n: list(levels(n, np.random.default_rng(seed)))   # noqa: E731
    return [zigzag(W, [], "max"), zigzag(W, [500], "max"), zigzag(W, [500], "min"), zigzag(W, [300, 600], "max"),
            zigzag(W, [300, 600], "min"), zigzag(W, mid, "min", 5), zigzag(W, mid, "max", 6), np.zeros(W),
            zigzag(W, before, "min", 7, lev_max=[3, 200] + lv(7, len(before) // 2 - 2)),
            zigzag(W, before, "max", 8, lev_min=[3, 200] + lv(8, len(before) // 2 - 2)),
            zigzag(W, behind, "max", 9, lev_max=lv(9, len(behind) // 2 - 2) + [200, 3]),
            zigzag(W, behind, "min", 10, lev_min=lv(10, len(behind) // 2 - 2) + [200, 3]),
            zigzag(W, [1, 2], "max"), zigzag(W, [W - 3, W - 2], "min"), zigzag(W, [1, W - 2], "max"), zigzag(W, [1, 2, 3], "min")]


def rows_dense_again(W: int = 1000) -> list[np.ndarray]:
    return rows_counts(W)[:7] + rows_wrap(W) + rows_mixed(W)[3:8]


def rows_est(W: int = 1000) -> list[np.ndarray]:
    """Up to 64 and up to 128 raw extrema of a kind, and beyond (fast_est<1> and <2> behind the dense selection and behind the
    list code)."""
    n = [(20, 20), (60, 61), (64, 64), (100, 100), (128, 128), (140, 140), (200, 201), (249, 249),
         (0, 0), (30, 31), (70, 70), (127, 128), (129, 129), (160, 160), (240, 240), (5, 5)]
    return [np.zeros(W) if a == 0 else count_row(W, a, b, 3 * a + b + i) for i, (a, b) in enumerate(n)]


def rows_sharp(W: int, s: int) -> list[np.ndarray]:
    """Troughs (of either polarity) at s, s + 1, W - s - 1, W - s with a peak on either side: the edges of
    `t - s > 0 and t + s < W` (features/sharpwaves.py:393-406)."""
    mid = list(range(s + 18, W - s - 18, 15))
    a = [s - 3, s, s + 3] + mid + [W - s - 4, W - s - 1, W - s + 2]
    b = [s - 2, s + 1, s + 4] + mid + [W - s - 3, W - s, W - s + 3]
    r = [zigzag(W, a, "max", 1), zigzag(W, a[1:-1], "max", 2), zigzag(W, b, "max", 3), zigzag(W, b[1:-1], "max", 4),
         zigzag(W, a, "min", 5), zigzag(W, b, "min", 6), np.zeros(W), zigzag(W, a[1:-1], "min", 7)]
    return r


def rows_8k(W: int = 8000, fv: bool = False) -> list[np.ndarray]:
    """A gap-2 zigzag over the whole window (every sample from 1 to W - 2 an extremum); fv: every 51st maximum from the
    51st on is 300 levels above the others, so that under a peak distance of 101 only those are kept."""
    out = []
    for first, seed in (("max", 1), ("min", 2)):
        pos = np.arange(1, W - 1)
        n_max = (pos.size + (first == "max")) // 2
        lev = levels(n_max, np.random.default_rng(seed))
        if fv:
            lev = lev.copy()
            lev[50::51] += 300
        out.append(zigzag(W, pos, first, seed, lev_max=lev))
    return out


def rows_long(W: int = 16000) -> list[np.ndarray]:
    return [count_row(W, 100, 100, 1), count_row(W, 128, 128, 2), count_row(W, 140, 141, 3), np.zeros(W)]


# ---- cases ----------------------------------------------------------------------------------------------------------------
DEFAULT_COMBOS = [("interval", "mean"), ("prominence", "max"), ("sharpness", "max"), ("num_peaks", "max")]
ALL_FAST = [(f, e) for f in FAST_FEATURES for e in ("mean", "max", "min")] + [("num_peaks", "max")]
ALL_VALS = [(f, e) for f in FAST_FEATURES + STEEP for e in ("mean", "max", "min")] + \
           [(f, e) for f in ("interval", "prominence", "width", "rise_steepness") for e in ("median", "var")] + [("num_peaks", "max")]


def _case(rows, C, hops, sfreq=1000.0, W=1000, dist=(5, 10), combos=DEFAULT_COMBOS, env=None, between=True, pols=(True, True),
          taps=(1.0,)):
    return {"rows": rows, "C": C, "hops": hops, "sfreq": float(sfreq), "W": W, "dist": dist, "combos": combos, "env": env or {},
            "between": between, "pols": pols, "taps": taps}


NO_DENSE = {"NMX_SW_DENSE": "0"}
CASES = {f"x{W}": _case(lambda W=W: rows_extrema(W), 4, 2, W=W) for W in (1000, 963, 1026, 962, 1027, 512, 450, 66, 40)}
CASES.update({
    "x4098": _case(lambda: rows_extrema(4098)[:4], 4, 1, sfreq=4000, W=4098),
    "x4099": _case(lambda: rows_extrema(4099)[:4], 4, 1, sfreq=4000, W=4099),
    "x962_list": _case(lambda: rows_extrema(962), 4, 2, W=962, env=NO_DENSE),
    "x4098_list": _case(lambda: rows_extrema(4098)[:4], 4, 1, sfreq=4000, W=4098, env=NO_DENSE),
    "counts": _case(rows_counts, 8, 1),
    "mixed": _case(rows_mixed, 4, 4),
    "wrap": _case(rows_wrap, 4, 1),
    "edges": _case(rows_edges, 8, 2),
    "list_env": _case(rows_dense_again, 8, 2, env=NO_DENSE),
    "list_dist": _case(rows_dense_again, 8, 2, dist=(25, 40)),
    "pairs_8k": _case(rows_8k, 2, 1, sfreq=8000, W=8000, dist=(1, 1), combos=ALL_FAST, env=NO_DENSE),
    "pairs_8k_fv": _case(lambda: rows_8k(fv=True), 2, 1, sfreq=8000, W=8000, dist=(101, 1), combos=ALL_FAST),
    "est_fast": _case(rows_est, 8, 2, combos=ALL_FAST),
    "est_vals": _case(rows_est, 8, 2, combos=ALL_VALS),
    "sharp_250": _case(lambda: rows_sharp(250, 20), 4, 2, sfreq=250, W=250, combos=ALL_FAST),
    "sharp_1k": _case(lambda: rows_sharp(1000, 5), 4, 2, combos=ALL_FAST),
    "nobetween": _case(lambda: rows_est()[:8], 4, 2, between=False),
    "peaks_only": _case(lambda: rows_est()[:8], 4, 2, between=False, pols=(True, False)),
    "troughs_only": _case(lambda: rows_est()[:8], 4, 2, between=False, pols=(False, True)),
    "two_filters": _case(lambda: rows_est()[4:12], 4, 2, between=False, taps=(1.0, -1.0), combos=ALL_FAST),
    "two_filters_list": _case(lambda: rows_est()[4:12], 4, 2, between=False, taps=(1.0, -1.0), combos=ALL_FAST, env=NO_DENSE),
    "long_dense": _case(rows_long, 2, 2, sfreq=16000, W=16000),
    "long_slab": _case(rows_long, 2, 2, sfreq=16000, W=16000, dist=(25, 40)),
})
FILTER_RANGES = [[5, 80], [5, 30]]


def case_choice(name: str) -> dict:
    c = CASES[name]
    return plan_choice(c["W"], c["sfreq"], *c["dist"], c["combos"], c["env"].get("NMX_SW_DENSE", "1") != "0")


def case_settings(c: dict, n_filters: int | None = None):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.features.sharpwave_analysis = True
    s.segment_length_features_ms = c["W"] * 1000.0 / c["sfreq"]
    sw = s.sharpwave_analysis_settings
    sw.filter_ranges_hz = [list(r) for r in FILTER_RANGES[:n_filters or len(c["taps"])]]
    used = {f for f, _ in c["combos"]}
    for f in sw.sharpwave_features.to_dict():
        setattr(sw.sharpwave_features, f, f in used)
    for e in ("mean", "median", "max", "min", "var"):
        sw.estimator[e] = [f for f, ee in c["combos"] if ee == e]
    sw.detect_troughs.distance_peaks_ms, sw.detect_troughs.distance_troughs_ms = c["dist"]
    sw.detect_peaks.estimate, sw.detect_troughs.estimate = c["pols"]
    sw.apply_estimator_between_peaks_and_troughs = c["between"]
    return s


# ---- the reference and its limits -------------------------------------------------------------------------------------
def value_err(f: str, v: np.ndarray, Y: float) -> float:
    """Largest error of one per-trough float32 value of feature f (module docstring)."""
    if f in EXACT or v.size == 0:
        return 0.0
    if f in TIMES:
        return 2 * EPS32 * float(np.abs(v).max())
    return 4 * EPS32 * Y


def _mean_lim(v, ev, r):
    return ev + (v.size - 1) * EPS32 * float(np.abs(v).mean()) + 2 * EPS32 * abs(r)


def estimate(e: str, v: np.ndarray, ev: float):
    """(value, limit) of estimator e over the reference's values v whose float32 forms carry at most ev each."""
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return 0.0, 0.0
    if e == "max":
        return float(v.max()), ev
    if e == "min":
        return float(v.min()), ev
    if e == "median":
        r = float(np.median(v))
        return r, ev + (EPS32 * abs(r) if v.size % 2 == 0 else 0.0)
    m = float(np.add.reduce(v) / v.size)
    lm = _mean_lim(v, ev, m)
    if e == "mean":
        return m, lm
    d = v - m
    var = float(np.var(v))
    dmax = float(np.abs(d).max())
    e_d = ev + lm + EPS32 * dmax
    e_d2 = 2 * dmax * e_d + e_d * e_d + EPS32 * dmax * dmax
    return var, _mean_lim(d * d, e_d2, var) + 4 * EPS32 * var


def between(e: str, a, b):
    (va, la), (vb, lb) = a, b
    if e in ("mean", "median"):
        r = 0.5 * (va + vb)
        return r, 0.5 * (la + lb) + EPS32 * abs(r)
    if e == "max":
        return max(va, vb), max(la, lb)
    if e == "min":
        return min(va, vb), max(la, lb)
    r = float(np.var([va, vb]))
    return r, 0.5 * abs(va - vb) * (la + lb) + 0.25 * (la + lb) ** 2 + 4 * EPS32 * r


def analyze_row(y: np.ndarray, c: dict) -> dict:
    """Both polarities of the float64 restatement on the float32-exact series y: {polarity: analyze_waveform's dict + counts}."""
    from oracle import nm_oracle as orc

    need = {f for f, _ in c["combos"]}
    out = {}
    for pname, sign in (("Peak", 1.0), ("Trough", -1.0)):
        z = sign * np.asarray(y, np.float64)
        r = orc.analyze_waveform(z, c["sfreq"], c["dist"][0], c["dist"][1], need | {"num_peaks", "interval"})
        r["_nT"], r["_n_pairs"] = len(r["trough"]), len(r["peak_left"])
        r["_n_raw"] = (len(orc.find_peaks_distance(z, None)), len(orc.find_peaks_distance(-z, None)))
        pk, tr = orc.find_peaks_distance(z, c["dist"][0]), orc.find_peaks_distance(-z, c["dist"][1])
        r["_nPk"] = len(pk)
        r["_first_valid"] = int(np.sum(tr < pk[0])) if len(pk) else len(tr)
        r["_behind"] = int(np.sum(tr > pk[-1])) if len(pk) else len(tr)
        out[pname] = r
    return out


def reference_row(y: np.ndarray, c: dict, ch: str, fname: str, an: dict | None = None) -> dict:
    """{key: (value, limit)} of one (channel, filter) in the engine's key names."""
    an = analyze_row(y, c) if an is None else an
    Y = float(np.abs(y).max())
    pols = [p for p, on in zip(("Peak", "Trough"), c["pols"]) if on]
    per: dict = {}
    for p in pols:
        r = an[p]
        for f, e in c["combos"]:
            if f == "num_peaks":
                per.setdefault(f"{ch}_Sharpwave_num_peaks_{fname}", {})[p] = (float(r["num_peaks"][0]), 0.0)
            else:
                v = np.asarray(r[f], np.float64)
                per.setdefault(f"{ch}_Sharpwave_{e.title()}_{f}_{fname}", {})[p] = estimate(e, v, value_err(f, v, Y))
    out = {}
    for (f, e) in c["combos"]:
        k = f"{ch}_Sharpwave_num_peaks_{fname}" if f == "num_peaks" else f"{ch}_Sharpwave_{e.title()}_{f}_{fname}"
        if c["between"]:
            out[k] = between("mean" if f == "num_peaks" else e, per[k]["Peak"], per[k]["Trough"])
            if f == "num_peaks":
                out[k] = (out[k][0], 0.0)   # (half of a sum of two small integers: exact)
        else:
            for p in pols:
                out[f"{k}_analyze_{p}"] = per[k][p]
    return out


def check_inputs(name: str, x: np.ndarray, y: np.ndarray, c: dict) -> None:
    """The two conditions on a constructed row x and its read-out y (module docstring)."""
    from oracle import nm_oracle as orc

    amp = float(np.abs(x).max())
    if amp == 0.0:
        assert not np.any(y), f"{name}: a zero row's read-out is not exactly zero"
        return
    m = orc.sharpwave_decision_margin(x, *c["dist"])
    assert m >= MARGIN * amp, f"{name}: decision margin {m:.3g} below {MARGIN} max|x| = {MARGIN * amp:.3g}"
    d = float(np.abs(y - x).max())
    assert d <= YARD_CAP * EPS32 * amp, f"{name}: read-out {d / (EPS32 * amp):.2f} eps32 max|x| from the input"


def check_sensitivity(name: str, c: dict, an: dict) -> None:
    """A case too insensitive to see a single wrong trough does not pass as a case (module docstring)."""
    assert any(f == "num_peaks" for f, _ in c["combos"]), f"{name}: num_peaks (exact) must be estimated"
    for p in ("Peak", "Trough"):
        v = np.asarray(an[p]["interval"], np.float64)
        if 2 <= v.size <= SENS_N and ("interval", "mean") in c["combos"]:
            r, lim = estimate("mean", v, value_err("interval", v, 0.0))
            assert abs(r) / v.size >= SENS_RATIO * lim, f"{name} {p}: one trough in {v.size} moves the mean interval by " \
                                                        f"{abs(r) / v.size:.3g}, the limit is {lim:.3g}"


class Report:
    """Largest error per family in units of its limit, items compared (profiles/sharpwave_probes.md)."""

    def __init__(self):
        self.worst, self.n = {}, 0

    def add(self, fam, ratio):
        self.worst[fam] = max(self.worst.get(fam, 0.0), ratio)

    def line(self, name, extra=""):
        w = " ".join(f"{k} {v:.3f}" for k, v in sorted(self.worst.items()))
        print(f"SWPROBE {name:18s} items {self.n:4d}  worst error / limit: {w} {extra}")


def family(key: str) -> str:
    if "num_peaks" in key:
        return "num_peaks"
    _, _, rest = key.partition("_Sharpwave_")
    e, _, f = rest.partition("_")
    return f"{e.lower()}:{'exact' if any(f.startswith(x) for x in EXACT) else 'time' if any(f.startswith(x) for x in TIMES) else 'amp'}"


def compare_item(name: str, where: str, got: dict, ref: dict, rep: Report, factor: float = 1.0) -> None:
    bad = []
    for k, (want, lim) in ref.items():
        g = float(got[k])
        err = abs(g - want)
        ok = np.isfinite(g) and err <= factor * lim
        if lim > 0:
            rep.add(family(k), err / lim)
        if not ok:
            bad.append(f"{k}: got {g!r}, reference {want!r}, error {err:.3g}, limit {factor * lim:.3g}")
    rep.n += 1
    assert not bad, f"{name} {where}: {len(bad)} of {len(ref)} outputs beyond their limits\n  " + "\n  ".join(bad[:12])


def case_rows(name: str) -> np.ndarray:
    """[hops, C, W] float32-exact rows of a case (item (h, c) = row h C + c)."""
    c = CASES[name]
    rows = c["rows"]()
    assert len(rows) == c["hops"] * c["C"], (name, len(rows))
    return np.stack(rows).reshape(c["hops"], c["C"], c["W"])


def run_case(lib, name: str) -> Report:
    """Case `name`: one batch of hops x C items, every output of every item against the reference on the read-out series."""
    c = CASES[name]
    C, hops, W, nf = c["C"], c["hops"], c["W"], len(c["taps"])
    ch_names = [f"ch{i}" for i in range(C)]
    fnames = [f"range_{a:.0f}_{b:.0f}" for a, b in FILTER_RANGES[:nf]]
    X = case_rows(name)
    choice = case_choice(name)
    eng = build_engine(lib, c["env"], case_settings(c), ch_names, c["sfreq"], features=["sharpwave_analysis"],
                       sharpwave_taps=[np.array([t]) for t in c["taps"]], window=W)
    rep = Report()
    try:
        assert eng.W == W and eng.desc.n_filters == nf
        rec = np.ascontiguousarray(np.concatenate(list(X), axis=1), dtype=np.float32)   # hop h = samples [h W, (h + 1) W)
        out = eng.process_batch(rec, np.arange(hops, dtype=np.int64) * W).astype(np.float64)
        if lib is None:
            names = set(eng.kernels(5).split(" + "))
            assert names == KERNELS[choice["kind"]], f"{name}: stage 5 ran {sorted(names)}, wanted {sorted(KERNELS[choice['kind']])}"
        assert not np.any(eng.offsets()[0]) and not np.any(eng.offsets()[1])
        assert out.shape == (hops, len(eng.keys))
        col = {k: i for i, k in enumerate(eng.keys)}
        for h in range(hops):
            Y = eng.filter_window(X[h])
            assert Y.shape == (C, nf, W)
            for ci in range(C):
                got0 = None
                for fi in range(nf):
                    y = Y[ci, fi]
                    check_inputs(f"{name} hop {h} ch {ci} filter {fi}", c["taps"][fi] * X[h, ci], y, c)
                    an = analyze_row(y, c)
                    ref = reference_row(y, c, ch_names[ci], fnames[fi], an)
                    check_sensitivity(f"{name} hop {h} ch {ci}", c, an)
                    got = {k: out[h, col[k]] for k in ref}
                    if not y.any():
                        assert not any(got.values()) and all(v == (0.0, 0.0) for v in ref.values()), (name, h, ci, got)
                    compare_item(name, f"hop {h} ch {ci} filter {fi}", got, ref, rep, FACTORS.get(name, 1.0))
                    if fi == 0:
                        got0 = got
                    elif c["taps"][fi] == -c["taps"][0] and not c["between"]:
                        # the mirrored filter: its Peak analysis is filter 0's Trough analysis, bit for bit
                        for k, v in got.items():
                            twin = k.replace(fnames[fi], fnames[0]).replace("_analyze_Peak", "_analyze_Trough") \
                                if k.endswith("_Peak") else k.replace(fnames[fi], fnames[0]).replace("_analyze_Trough", "_analyze_Peak")
                            assert got0[twin] == v, f"{name} hop {h} ch {ci}: {k} = {v!r}, {twin} = {got0[twin]!r}"
        assert len(col) == C * nf * len(ref), (len(col), C, nf, len(ref))   # every column of the row was compared
    finally:
        eng.close()
    rep.line(name, f"kind {choice['kind']} chunk {choice['chunk']}")
    return rep


# ---- noise layer --------------------------------------------------------------------------------------------------------
def run_noise(lib, seeds=(1, 2), C: int = 64) -> float:
    """Default filters and settings (+ num_peaks), white noise sigma 50, one window per call.  -> share of rows left out."""
    from oracle import nm_oracle as orc

    c = _case(None, C, 1, taps=(None, None))
    ch_names = [f"ch{i}" for i in range(C)]
    fnames = [f"range_{a:.0f}_{b:.0f}" for a, b in FILTER_RANGES]
    eng = build_engine(lib, {}, case_settings(c, 2), ch_names, 1000.0, features=["sharpwave_analysis"])
    rep, left, total = Report(), 0, 0
    try:
        col = {k: i for i, k in enumerate(eng.keys)}
        for seed in seeds:
            x = (np.random.default_rng(seed).standard_normal((C, 1000)) * 50.0).astype(np.float32)
            out = eng.process_batch(x, np.zeros(1, np.int64)).astype(np.float64)[0]
            k_batch = (eng.kernels(3), eng.kernels(6), eng.kernels(5)) if lib is None else None
            Y = eng.filter_window(x.astype(np.float64))
            if lib is None:
                assert (eng.kernels(3), eng.kernels(6)) == k_batch[:2], f"noise: the read-out ran {eng.kernels(3)!r} / " \
                    f"{eng.kernels(6)!r}, the batch {k_batch[:2]!r}"
                assert set(k_batch[2].split(" + ")) == KERNELS["DENSE_LIST"], k_batch[2]
            for ci in range(C):
                for fi in range(2):
                    y = Y[ci, fi]
                    total += 1
                    if orc.sharpwave_decision_margin(y, *c["dist"]) < NOISE_MARGIN * EPS32 * float(np.abs(y).max()):
                        left += 1
                        continue
                    ref = reference_row(y, c, ch_names[ci], fnames[fi])
                    compare_item("noise", f"seed {seed} ch {ci} filter {fi}", {k: out[col[k]] for k in ref}, ref, rep)
    finally:
        eng.close()
    share = left / total
    rep.line("noise", f"rows left out {left} of {total} = {100 * share:.2f} %")
    assert share <= NOISE_LEFT_OUT, f"noise layer: {100 * share:.1f} % of the rows left out"
    return share
