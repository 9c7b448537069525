"""Per-sample probes of the FIR kernels (pre-filters, notch, band-pass bank), shared by the emulator tier
(test_fir_sample_probes_cpu.py) and the MI355X tier (test_fir_sample_probes_gpu.py).

Every other test reads the filtered series through reductions (band power: a variance over 333 - 1000 samples) or
decisions (bursts, sharp waves), or pins its bytes (tests/golden/fir_kernel_choice.json); the two per-sample comparisons
that exist (parity_cases: filter_window, preprocessing_notch_and_reref) allow 2e-5 max|y|, about 100 times the error of a
correct fp32 FFT convolution.  A probe compares EVERY sample of EVERY row the kernel stores with a float64 direct
convolution and allows four times the error of the same convolution restated in single precision on the CPU.

Outlets (calls that exist; nothing is exported for the probes):
  filter_window      the bank without the notch, n_items = channels; every filter goes out through the `sw_out` store
                     (the feature epilogue and `yb_out` stay with the feature tests: band power, bursts, sharp waves)
  preprocess_window  front end -> pre-filters -> notch, one window
  process_batch(tap=True)   the pre-processed windows of a whole batch: the notch at batch sizes
The band-pass bank in a batch of MANY windows has no per-sample outlet: the bit-equality tests (a batch against
window-by-window calls, on features) stay its link to the one-window form probed here.

Inputs, per case (`noise_inputs`, `impulse_inputs`, `constant_input`):
  (a) unit impulses, one per channel, at POSITIONS (where the kernels' index arithmetic changes), a few calls of C
      positions each; C = 4099 hits every position in both halves of a channel pair
  (b) fixed-seed white noise, sigma = 50, the channel pairs cycling through PAIR_PATTERNS: a level of 300, amplitudes
      1e4 and 1e-3 apart in both orders,
  (c) ... and a zero channel in either half of a pair: without a re-reference its output is exactly +-0
  (d) a constant window at 300 (zero-padded bank: the edge transient)

Reference: np.convolve in float64 on the explicitly padded window (zeros: bank, pre-filters; the odd reflection of
mne_restated._smart_pad: notch); more than BULK_ROWS rows go through scipy.signal.oaconvolve in float64, tied to the direct
convolution on 64 rows spread over the case.  test_fir_sample_probes_cpu.py ties the direct convolution to
oracle.nm_oracle.fir_bank_apply and mne_restated._overlap_add_filter at 1e-12 max|y| on every tap set.

Limit: max_n |y_kernel - y64| <= FACTOR * max(e32[row], eps32 * rms(x_row)) for every row, FACTOR = 4, where
e32[row] = max_n |y32 - y64| and y32 is the yardstick: the same chain on the same fp32 input in single precision --
scipy.fft on complex64 at the kind's transform length M, the taps' spectrum rounded to complex64, the same padding, every
hand-off rounded to float32.  The yardstick itself must stay within YARD_CAP eps32 of the row's scale from the float64
reference (a wrong reference would otherwise inflate e32 and pass).  No row and no sample is left out, no verifier, no
accepted miss.

    case (outlet)              rate  W     C x hops   kernel asserted                          M      what it exercises
    bank: filter_window
    w64c_c7                    1000  1000  7          nmx_kern_bank_w64c_rd64                  1536   < 2048 pairs: two waves, odd count
    w64c_c4099                 1000  1000  4099       nmx_kern_bank_w64c_rd64                  1536   2050 pairs > 256 x 8: chunk 2, waves with 2 / 1 / 0 items
    w64c_750                   750   750   5          nmx_kern_bank_w64c_rd64                  1536   W + half = 1124 > 1024
    w64d_half                  500   500   5          nmx_kern_bank_w64d_rd64<1>               1024   W <= 512
    w64d_full                  600   600   5          nmx_kern_bank_w64d_rd64<0>               1024
    w64e_sw / w64e_sw_nofuse   1000  1000  5          ..w64c (3) + nmx_kern_bank_w64e_rd64<0> (6)  1536 / 2048   1651 taps: second launch
    w901 / w901_one            1000  901   5          ..w64c + ..w64e<0> / nmx_kern_bank_w64_rd64      1536 / 2048   odd W: dword-wise accesses
    one_small                  1000  1000  4          nmx_kern_bank_w64_rd64                   2048   one channel per transform
    one_pp_half                1000  1000  4099       nmx_kern_bank_w64pp_rd64<1>              2048   >= 4096 items: persistent pipelined
    one_pp_full                1100  1100  4096       nmx_kern_bank_w64pp_rd64<0>              2048   W > 1024: the full inverse
    x2_half / x2_full          2000 / 2500  5         nmx_kern_bank_w64x2_rd64<1> / <0>        4096
    generic                    1000  1000  3          nmx_kern_bank                            1500   NMX_BANK_W64=0 (emulator tier too)
    partitioned                1000  1000  3          nmx_kern_bank                            ola    NMX_BANK_PARTITIONED=1 (emulator tier too)
    partitioned_8k             8000  8000  2          nmx_kern_bank                            ola    case_high_rate_partitioned_fir's shape
    mobility                   1000  1000  4          nmx_kern_bank_w64_rd64                   2048   nmx_w64_pair_shape_ok false
    one_emu                    1000  1000  3          (emulator: the one-channel M = 2048 item) 2048
    notch: preprocess_window
    notch_c2 / notch_c7 (+ _ref)  1000  1000  2 / 7   nmx_kern_bank_w64e_rd64<1, 1000, 499>    2048   compile-time shape, with / without R
    notch_w901                 1000  901   5          nmx_kern_bank_w64e_rd64<1>               2048   run-time shape
    notch_800                  800   800   8          nmx_kern_bank_w64e_rd64<1>               2048   the fixture's notch_generic
    notch_2k                   2000  2000  3          nmx_kern_bank                            4000   W + 2 half > 2048: LDS kernel
    notch_one                  1000  1000  3          nmx_kern_notch_w64_rd64                  2048   NMX_BANK_W64E=0 (emulator tier too)
    pre_bandstop / _lowpass / _highpass  1000  1000  3   nmx_kern_bank_w64_rd64 + the notch    2048   one preprocessing_filter stage, chained
    notch in batches: tap
    tap_4x8 / tap_33x40        1000  1000  4 x 8 / 33 x 40   nmx_kern_bank_w64e_rd64<1, 1000, 499>     pair notch over many windows, odd count
    tap_q                      1000  1000  64 x 66    nmx_kern_notch_w64q_rd64                 2048   >= 1024 items, four per workgroup
    tap_qp                     1000  1000  256 x 96   nmx_kern_notch_w64qp_rd64                2048   >= 24 576 items, persistent
    tap_fused                  1000  1000  64 x 66    nmx_kern_notch_bank_w64e_rd64<1000, 499, 1>     bytes == NMX_NOTCH_SW_FUSE=0
    tap_chunks                 1000  1000  4 x 40     (pair notch) NMX_CHUNK_WINDOWS=16: bytes == one chunk

Further rows: notch_one_ref (the one-channel notch behind a common average), tap_fused2 (NMX_NOTCH_SW_FUSE=2:
nmx_kern_notch_bank_w64e_rd64<1000, 499, 2>), tap_nofuse and tap_4x40 (the plans tap_fused and tap_chunks are compared
with byte for byte).  Every kernel nmx_w64.hip launches and nmx_kern_bank is reached through one of the three
outlets and asserted by name (test_fir_sample_probes_cpu.py checks the tables against the launchers' source); none is
left out.  HotPathEngine.kernels() names what the last filter_window / preprocess_window call launched.

The figures observed are in profiles/fir_sample_probes.md."""

from __future__ import annotations

import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
FACTOR = 4.0            # the limit, in units of the yardstick's error (module docstring)
# The yardstick is judged too, or a wrong reference would only inflate e32 and pass: its error may not exceed YARD_CAP eps32
# times the row's scale max(rms(x_row), max|y64|).  Two M <= 4096-point fp32 transforms round about sqrt(2 log2 M) ~ 4.7 times
# per sample (random-walk growth), the largest of ~1000 samples is ~3.5 sigma: 16.
YARD_CAP = 16.0
FACTORS: dict = {}      # case name -> factor in force where it is not FACTOR (at most 8; profiles/fir_sample_probes.md)
BULK_ROWS = 512         # more (row, filter) convolutions than this: oaconvolve, tied on TIE_ROWS rows
TIE_ROWS = 64
SIGMA = 50.0
# (scale of the even channel, of the odd channel, level of the even channel) of a channel pair
PAIR_PATTERNS = ((1.0, 1.0, 300.0), (1.0, 1e4, 0.0), (1e4, 1.0, 0.0), (1.0, 1e-3, 0.0), (1e-3, 1.0, 0.0),
                 (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))


# ---- the plan's arithmetic, restated ----------------------------------------------------------------------------------
def _smooth5(n: int) -> bool:
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def choose_M(need: int) -> int:
    """nmx_engine_plan_fir.inc: choose_M -- the LDS kernel's transform length."""
    M = need + (need & 1)
    while not _smooth5(M // 2):
        M += 2
    return M


def positions(W: int, pad_half: int = 0) -> list[int]:
    """Impulse positions: the ends, the middle, both sides of the per-lane block boundaries (multiples of 16, 24, 32 for
    M = 1024, 1536, 2048), 63 / 64 / 65, 255 / 256, 511 / 512 (the HALF forms), and for the notch the first and last
    `pad_half` samples' ends, where the odd reflection folds."""
    p = {0, 1, 2, W // 2 - 1, W // 2, W - 3, W - 2, W - 1}
    for b in (16, 24, 32, 48, 64, 96, 256, 512, 768, 1024, 1536, 2048):
        p |= {b - 1, b, b + 1}
    for b in (24, 32):
        k = (W - 1) // b * b
        p |= {k - 1, k, k + 1}
    if pad_half:
        p |= {pad_half - 1, pad_half, pad_half + 1, W - pad_half - 2, W - pad_half - 1, W - pad_half}
    return sorted(q for q in p if 0 <= q < W)


# ---- references -------------------------------------------------------------------------------------------------------
def live_taps(h: np.ndarray, W: int) -> np.ndarray:
    """Only taps within W - 1 of the centre touch a window (build_bank: uh = min(half, W - 1))."""
    half = (len(h) - 1) // 2
    uh = min(half, W - 1)
    return np.asarray(h, np.float64)[half - uh:half + uh + 1]


def pad_zero(x: np.ndarray, half: int) -> np.ndarray:
    return np.concatenate([np.zeros(half, x.dtype), x, np.zeros(half, x.dtype)])


def pad_odd(x: np.ndarray, L: int) -> np.ndarray:
    """The window as the notch sees it, cut to the `half` samples each side that the taps reach: MNE's reflect_limited
    padding (mne_restated._smart_pad with n_edge = min(L, W) - 1; zeros beyond it)."""
    from oracle import mne_restated

    W, half = len(x), (L - 1) // 2
    n_edge = max(min(L, W) - 1, 0)
    xe = mne_restated._smart_pad(x, n_edge)
    extra = max(half - n_edge, 0)
    if extra:
        xe = pad_zero(xe, extra)
    a = n_edge + extra - half
    return xe[a:a + W + 2 * half]


def pad_odd_rows(X: np.ndarray, L: int) -> np.ndarray:
    """pad_odd on every row at once (the same operations element by element; `conv64` ties the bulk reference, which pads
    this way, to the direct one, which pads through mne_restated._smart_pad)."""
    W, half = X.shape[1], (L - 1) // 2
    n_edge = max(min(L, W) - 1, 0)
    xe = np.concatenate([2 * X[:, :1] - X[:, n_edge:0:-1], X, 2 * X[:, -1:] - X[:, -2:-n_edge - 2:-1]], axis=1)
    extra = max(half - n_edge, 0)
    if extra:
        z = np.zeros((len(X), extra), X.dtype)
        xe = np.concatenate([z, xe, z], axis=1)
    a = n_edge + extra - half
    return xe[:, a:a + W + 2 * half]


def _padded(rows: np.ndarray, h: np.ndarray, odd: bool) -> np.ndarray:
    half = (len(h) - 1) // 2
    if not odd:
        z = np.zeros((len(rows), half), rows.dtype)
        return np.concatenate([z, rows, z], axis=1)
    if len(rows) > TIE_ROWS:
        return pad_odd_rows(rows, len(h))
    return np.stack([pad_odd(r, len(h)) for r in rows])


def conv64_direct(rows: np.ndarray, h: np.ndarray, odd: bool = False) -> np.ndarray:
    """y[r, n] = sum_k h[k] x_ext[r, n + half - k]: np.convolve in float64 on the explicitly padded rows, no FFT."""
    rows = np.asarray(rows, np.float64)
    h = np.asarray(h, np.float64)
    return np.stack([np.convolve(r, h, mode="valid") for r in _padded(rows, h, odd)])


def conv64_bulk(rows: np.ndarray, h: np.ndarray, odd: bool = False) -> np.ndarray:
    """The same through scipy.signal.oaconvolve in float64 (the large cases), tied to conv64_direct by `conv64`."""
    from scipy.signal import oaconvolve

    rows = np.asarray(rows, np.float64)
    h = np.asarray(h, np.float64)
    return oaconvolve(_padded(rows, h, odd), h[None, :], mode="valid", axes=-1)


def conv64(rows: np.ndarray, h: np.ndarray, odd: bool = False, budget: int = BULK_ROWS) -> np.ndarray:
    rows = np.asarray(rows, np.float64)
    if len(rows) <= budget:
        return conv64_direct(rows, h, odd)
    y = conv64_bulk(rows, h, odd)
    pick = np.unique(np.linspace(0, len(rows) - 1, TIE_ROWS).astype(int))
    d = conv64_direct(rows[pick], h, odd)
    tol = 1e-12 * max(float(np.abs(d).max()), 1e-300)
    assert float(np.abs(y[pick] - d).max()) <= tol, "oaconvolve reference left the direct convolution"
    return y


def conv32(rows: np.ndarray, h: np.ndarray, M: int, odd: bool = False) -> np.ndarray:
    """The yardstick: the same convolution in single precision -- the fp32 rows (padded the same way) in a complex64
    buffer of M points, scipy.fft forward, times the taps' float64 spectrum rounded to complex64, scipy.fft back.
    M = 0: the next fast length of the full convolution (the partitioned form has no single transform)."""
    import scipy.fft as sf

    rows = np.asarray(rows, np.float32)
    W = rows.shape[1]
    h = live_taps(h, W) if not odd else np.asarray(h, np.float64)
    half = (len(h) - 1) // 2
    u = _padded(rows, h, True) if odd else rows          # zero padding is the buffer's own zeros
    off = 2 * half if odd else half
    if not M:
        M = sf.next_fast_len(u.shape[1] + len(h) - 1)
    assert u.shape[1] <= M and u.shape[1] + len(h) - 1 - M <= off, (u.shape, len(h), M)   # (the wrap stays off the outputs)
    H = sf.fft(np.concatenate([h, np.zeros(M - len(h))])).astype(np.complex64)
    buf = np.zeros((len(rows), M), np.complex64)
    buf[:, :u.shape[1]] = u
    y = sf.ifft(sf.fft(buf, axis=-1) * H[None, :], axis=-1)
    assert y.dtype == np.complex64
    return y.real[:, off:off + W].astype(np.float32)


def rms(rows: np.ndarray) -> np.ndarray:
    return np.sqrt(np.mean(np.asarray(rows, np.float64) ** 2, axis=-1))


class Report:
    """Per (case, input class): rows compared, the worst ratio kernel error / yardstick, and the median ratio that
    2e-5 max|y| would have allowed.  One line per entry when a case ends (profiles/fir_sample_probes.md)."""

    def __init__(self) -> None:
        self.seen: dict = {}

    def add(self, case, cls, ratio, old, rows):
        r, o, n = self.seen.get((case, cls), (0.0, [], 0))
        self.seen[(case, cls)] = (max(r, float(ratio)), o + [float(old)], n + int(rows))

    def flush(self, case):
        for (c, cls), (r, o, n) in list(self.seen.items()):
            if c == case:
                print(f"FIRPROBE {c:16s} {cls:9s} rows {n:7d}  worst ratio {r:6.3f}  2e-5 max|y| allowed {float(np.median(o)):8.1f}")
                del self.seen[(c, cls)]


REPORT = Report()


def check_rows(case: str, cls: str, got: np.ndarray, y64: np.ndarray, y32: np.ndarray, x_rows: np.ndarray,
               zero_rows: np.ndarray | None = None) -> float:
    """Every row of `got` (rows x W) within FACTOR yardsticks of `y64`; rows of `zero_rows` exactly +-0."""
    got = np.asarray(got, np.float64).reshape(y64.shape)
    assert np.isfinite(got).all(), f"{case} {cls}: non-finite samples"
    e32 = np.abs(y32.astype(np.float64) - y64).max(axis=-1)
    floor = np.maximum(e32, EPS32 * rms(x_rows))
    cap = YARD_CAP * EPS32 * np.maximum(rms(x_rows), np.abs(y64).max(axis=-1))
    assert np.all(e32 <= cap), (f"{case} {cls}: the single-precision yardstick is {np.max(e32 / np.maximum(cap, 1e-300)) * YARD_CAP:.1f} "
                                f"eps32 of the row's scale from the float64 reference: one of the two is wrong")
    err = np.abs(got - y64).max(axis=-1)
    if zero_rows is not None and zero_rows.any():
        assert not np.any(got[zero_rows]), f"{case} {cls}: a zero channel's output is not exactly zero " \
                                           f"(max {np.abs(got[zero_rows]).max():.3e})"
    live = floor > 0
    assert np.all(err[~live] == 0), f"{case} {cls}: output on rows without input"
    ratio = np.zeros(len(err))
    ratio[live] = err[live] / floor[live]
    factor = FACTORS.get(case, FACTOR)
    worst = int(np.argmax(ratio))
    old = float(np.median(2e-5 * np.abs(y64[live]).max(axis=-1) / floor[live])) if live.any() else 0.0
    REPORT.add(case, cls, ratio.max(), old, len(err))
    assert ratio.max() <= factor, (f"{case} {cls}: row {worst} of {len(err)}: error {err[worst]:.3e} is {ratio[worst]:.2f} "
                                   f"yardsticks (e32 {e32[worst]:.3e}, eps32 rms {EPS32 * rms(x_rows)[worst]:.3e}); "
                                   f"{int((ratio > factor).sum())} rows beyond {factor:g}")
    return float(ratio.max())


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _f32(x: np.ndarray) -> np.ndarray:
    """Float64 values that float32 holds exactly: what every outlet casts to is what the references read."""
    return np.asarray(x, np.float32).astype(np.float64)


def impulse_inputs(C: int, W: int, pad_half: int = 0) -> list[np.ndarray]:
    """Calls of C unit impulses.  Up to W channels: POSITIONS in chunks of C.  More: channel c at (c + c // W) mod W --
    every position, and from the second block on in the other half of a pair."""
    if C > 64:
        x = np.zeros((C, W))
        c = np.arange(C)
        x[c, (c + c // W) % W] = 1.0
        return [x]
    pos = positions(W, pad_half)
    if W > 4000:   # (long windows: the ends, the middle and the 2048-sample blocks of the partitioned form)
        pos = [q for q in pos if q < 2 or q >= W - 2 or q == W // 2 or abs(q % 2048 - 1024) >= 1023 and q > 2000]
    out = []
    for i in range(0, len(pos), C):
        x = np.zeros((C, W))
        for c in range(C):
            x[c, pos[(i + c) % len(pos)]] = 1.0
        out.append(x)
    return out


def noise_inputs(C: int, W: int, seed: int) -> list[tuple[np.ndarray, np.ndarray]]:
    """Calls of (C x W noise, zero-row mask): the channel pairs cycle through PAIR_PATTERNS until every pattern has run
    (one call when there are at least seven pairs); a lone last channel has scale 1."""
    rng = np.random.default_rng(seed)
    n_pairs = C // 2
    calls = 1 if n_pairs >= len(PAIR_PATTERNS) else -(-len(PAIR_PATTERNS) // max(n_pairs, 1))
    out = []
    for k in range(calls):
        x = rng.standard_normal((C, W)) * SIGMA
        for p in range(n_pairs):
            a, b, lvl = PAIR_PATTERNS[(k * max(n_pairs, 1) + p) % len(PAIR_PATTERNS)]
            x[2 * p] = x[2 * p] * a + lvl
            x[2 * p + 1] *= b
        x = _f32(x)
        out.append((x, ~x.any(axis=1)))
    return out


def constant_input(C: int, W: int) -> np.ndarray:
    return np.full((C, W), 300.0)


# ---- engines ----------------------------------------------------------------------------------------------------------
def _kw(lib):
    return {} if lib is None else {"lib": lib}


def ran(names: str, kernel: str) -> bool:
    """`names`: HotPathEngine.kernels(stage), "a + b<4> + ..."; `kernel`: a full name, template arguments included."""
    return kernel in names.split(" + ")


def build_engine(lib, env: dict, *args, **kw):
    """Environment selectors are read when a plan is built: they are set around the engine's construction only."""
    from py_neuromodulation_amd.engine import HotPathEngine

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return HotPathEngine(*args, **_kw(lib), **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def assert_kernels(lib, case: str, eng, want: dict) -> None:
    """want: {stage: kernel name}.  The emulator (lib given) names no kernels: it runs the items its plan builds."""
    if lib is not None:
        return
    for stage, name in want.items():
        names = eng.kernels(stage)
        if name == "":
            assert names == "", f"{case}: stage {stage} ran {names!r}, wanted nothing"
        else:
            assert ran(names, name), f"{case}: stage {stage} ran {names!r}, wanted {name}"


def bank_settings(kind: str, W: int, bands=None):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bandpass_filter = True
    if bands is not None:
        s.frequency_ranges_hz = {k: v for k, v in s.frequency_ranges_hz.items() if k in bands}
    if kind == "sw":
        s.features.sharpwave_analysis = True
    if kind == "mobility":
        s.bandpass_filter_settings.bandpower_features.mobility = True
    if kind == "w901":   # (tests/fir_kernel_choice_cases.py: an odd window; the band-pass segments may not be longer than it)
        s.features.sharpwave_analysis = True
        s.segment_length_features_ms = W
        s.bandpass_filter_settings.segment_lengths_ms = {"theta": W, "alpha": 500, "low_beta": 333, "high_beta": 333}
    return s.validate()


TWO_BANDS = ("theta", "high_beta")
W64C, W64E0, ONE = "nmx_kern_bank_w64c_rd64", "nmx_kern_bank_w64e_rd64<0>", "nmx_kern_bank_w64_rd64"
NOTCH_WC, NOTCH_RT = "nmx_kern_bank_w64e_rd64<1, 1000, 499>", "nmx_kern_bank_w64e_rd64<1>"
NO_PAIRS = {"NMX_BANK_W64C": "0", "NMX_BANK_W64E": "0"}


def _m_pair(first: int):
    """Filters whose W + half fits the first launch's M run there, the others on M = 2048 (build_bank)."""
    return lambda W, half: first if W + half <= first else 2048


# name -> env, sfreq, W, C, settings kind, bands, {stage: kernel}, M (int, or f(W, half of the live taps)), emulator tier
BANK_CASES = {
    "w64c_c7": ({}, 1000.0, 1000, 7, "bp", None, {3: W64C, 6: ""}, 1536, False),
    "w64c_c4099": ({}, 1000.0, 1000, 4099, "bp", TWO_BANDS, {3: W64C, 6: ""}, 1536, False),
    "w64c_750": ({}, 750.0, 750, 5, "bp", None, {3: W64C}, 1536, False),
    "w64d_half": ({}, 500.0, 500, 5, "bp", None, {3: "nmx_kern_bank_w64d_rd64<1>"}, 1024, False),
    "w64d_full": ({}, 600.0, 600, 5, "bp", None, {3: "nmx_kern_bank_w64d_rd64<0>"}, 1024, False),
    "w64e_sw": ({}, 1000.0, 1000, 5, "sw", None, {3: W64C, 6: W64E0}, _m_pair(1536), False),
    "w64e_sw_nofuse": ({"NMX_NOTCH_SW_FUSE": "0"}, 1000.0, 1000, 5, "sw", None, {3: W64C, 6: W64E0}, _m_pair(1536), False),
    "w901": ({}, 1000.0, 901, 5, "w901", None, {3: W64C, 6: W64E0}, _m_pair(1536), False),
    "w901_one": ({"NMX_BANK_W64E": "0"}, 1000.0, 901, 5, "w901", None, {3: W64C, 6: ONE}, _m_pair(1536), False),
    "one_small": (NO_PAIRS, 1000.0, 1000, 4, "sw", None, {3: ONE, 6: ""}, 2048, False),
    "one_pp_half": (NO_PAIRS, 1000.0, 1000, 4099, "bp", TWO_BANDS, {3: "nmx_kern_bank_w64pp_rd64<1>"}, 2048, False),
    "one_pp_full": ({}, 1100.0, 1100, 4096, "bp", TWO_BANDS, {3: "nmx_kern_bank_w64pp_rd64<0>"}, 2048, False),
    "x2_half": ({}, 2000.0, 2000, 5, "bp", None, {3: "nmx_kern_bank_w64x2_rd64<1>"}, 4096, False),
    "x2_full": ({}, 2500.0, 2500, 5, "bp", None, {3: "nmx_kern_bank_w64x2_rd64<0>"}, 4096, False),
    "generic": ({"NMX_BANK_W64": "0"}, 1000.0, 1000, 3, "bp", None, {3: "nmx_kern_bank"}, lambda W, half: choose_M(W + half), True),
    "partitioned": ({"NMX_BANK_W64": "0", "NMX_BANK_PARTITIONED": "1"}, 1000.0, 1000, 3, "bp", None, {3: "nmx_kern_bank"}, 0, True),
    "partitioned_8k": ({}, 8000.0, 8000, 2, "bp", ("alpha", "high_beta"), {3: "nmx_kern_bank"}, 0, True),
    "mobility": ({}, 1000.0, 1000, 4, "mobility", None, {3: ONE}, 2048, False),
    "one_emu": ({}, 1000.0, 1000, 3, "sw", None, {}, 2048, True),   # (the emulator's plan of the default shape)
}
LARGE_BANK = ("w64c_c4099", "one_pp_half", "one_pp_full")
EMU_BANK = [n for n, c in BANK_CASES.items() if c[8]]
GPU_BANK = [n for n in BANK_CASES if n != "one_emu" and n not in LARGE_BANK]


def _bank_reference(x, taps, M, budget=BULK_ROWS):
    """(y64, y32) [C, n_filters, W] of the zero-padded bank on the fp32-exact rows `x`."""
    C, W = x.shape
    y64 = np.empty((C, len(taps), W))
    y32 = np.empty((C, len(taps), W), np.float32)
    for f, h in enumerate(taps):
        hl = live_taps(h, W)
        y64[:, f] = conv64(x, hl, budget=budget // max(len(taps), 1))
        y32[:, f] = conv32(x, h, M(W, (len(hl) - 1) // 2) if callable(M) else M)
    return y64, y32


def bank_case(lib, name: str, classes=("impulse", "noise", "constant")) -> dict:
    """Every input class of bank case `name` through filter_window.  -> {class: worst ratio}."""
    env, sfreq, W, C, kind, bands, kernels, M, _ = BANK_CASES[name]
    eng = build_engine(lib, env, bank_settings(kind, W, bands), [f"ch{i}" for i in range(C)], sfreq)
    worst: dict = {}
    try:
        assert eng.W == W
        taps = eng.filter_taps
        calls = []
        if "impulse" in classes:
            calls += [("impulse", x, None) for x in impulse_inputs(C, W)]
        if "noise" in classes:
            calls += [("noise", x, z) for x, z in noise_inputs(C, W, seed=len(name) + W + C)]
        if "constant" in classes:
            calls += [("constant", constant_input(C, W), None)]
        for cls, x, zero in calls:
            got = eng.filter_window(x)
            assert_kernels(lib, name, eng, kernels)
            assert got.shape == (C, len(taps), W)
            y64, y32 = _bank_reference(x, taps, M)
            n = C * len(taps)
            r = check_rows(name, cls, got.reshape(n, W), y64.reshape(n, W), y32.reshape(n, W), np.repeat(x, len(taps), axis=0),
                           None if zero is None else np.repeat(zero, len(taps)))
            worst[cls] = max(worst.get(cls, 0.0), r)
    finally:
        eng.close()
        REPORT.flush(name)
    return worst


# ---- notch and pre-filters: preprocess_window ---------------------------------------------------------------------------
def car_matrix(C: int) -> np.ndarray:
    R = np.full((C, C), -1.0 / (C - 1))
    np.fill_diagonal(R, 1.0)
    return R


def pre_taps(kind: str, sfreq: float) -> np.ndarray:
    """One preprocessing_filter stage as processing/filter_preprocessing.py designs it (fir_design.mne_filter_single)."""
    from py_neuromodulation_amd import fir_design

    lo, hi = {"bandstop": (160.0, 100.0), "lowpass": (None, 200.0), "highpass": (3.0, None)}[kind]
    return fir_design.mne_filter_single(sfreq, lo, hi)


# name -> env, sfreq, W, C, re-reference ("car", "mix", None), pre-filter kind, {stage: kernel}, M of the notch, emulator tier
NOTCH_CASES = {
    "notch_c2": ({}, 1000.0, 1000, 2, None, None, {1: NOTCH_WC}, 2048, False),
    "notch_c7": ({}, 1000.0, 1000, 7, None, None, {1: NOTCH_WC}, 2048, False),
    "notch_c2_ref": ({}, 1000.0, 1000, 2, "mix", None, {1: NOTCH_WC}, 2048, False),
    "notch_c7_ref": ({}, 1000.0, 1000, 7, "car", None, {1: NOTCH_WC}, 2048, False),
    "notch_w901": ({}, 1000.0, 901, 5, None, None, {1: NOTCH_RT}, 2048, False),
    "notch_800": ({}, 800.0, 800, 8, "car", None, {1: NOTCH_RT}, 2048, False),
    "notch_2k": ({}, 2000.0, 2000, 3, None, None, {1: "nmx_kern_bank"}, 4000, True),
    "notch_one": ({"NMX_BANK_W64E": "0"}, 1000.0, 1000, 3, None, None, {1: "nmx_kern_notch_w64_rd64"}, 2048, True),
    "notch_one_ref": ({"NMX_BANK_W64E": "0"}, 1000.0, 1000, 3, "car", None, {1: "nmx_kern_notch_w64_rd64"}, 2048, True),
    "pre_bandstop": ({}, 1000.0, 1000, 3, None, "bandstop", {1: NOTCH_WC}, 2048, True),
    "pre_lowpass": ({}, 1000.0, 1000, 3, None, "lowpass", {1: NOTCH_WC}, 2048, True),
    "pre_highpass": ({}, 1000.0, 1000, 3, None, "highpass", {1: NOTCH_WC}, 2048, True),
}
EMU_NOTCH = [n for n, c in NOTCH_CASES.items() if c[8]]


def _ref_matrix(kind, C):
    if kind is None:
        return None
    return car_matrix(C) if kind == "car" else np.array([[1.0, -1.0], [-0.5, 1.0]])


def prep_reference(x, R, pre, notch, M, budget=BULK_ROWS):
    """(y64, y32, input rows of the notch) of re-reference -> pre-filters (zero padding, chained like
    oracle.nm_oracle.PreprocessingFilter) -> notch (odd reflection) on the fp32-exact rows `x` [.., C_in, W]."""
    x = np.asarray(x, np.float64)
    a64 = x if R is None else R @ x
    a32 = x.astype(np.float32) if R is None else R.astype(np.float32) @ x.astype(np.float32)
    shape = a64.shape
    a64, a32 = a64.reshape(-1, shape[-1]), a32.reshape(-1, shape[-1]).astype(np.float32)
    for h in pre:
        a64 = conv64(a64, live_taps(h, shape[-1]), budget=budget)
        a32 = conv32(a32, h, 2048)
    y64 = conv64(a64, notch, odd=True, budget=budget)
    y32 = conv32(a32, notch, M, odd=True)
    return y64.reshape(shape), y32.reshape(shape), a64.reshape(shape)


def notch_case(lib, name: str, classes=("impulse", "noise")) -> dict:
    """Impulses and noise of notch case `name` through preprocess_window.  -> {class: worst ratio}."""
    from py_neuromodulation_amd import NMSettings, fir_design

    env, sfreq, W, C, ref, pre_kind, kernels, M, _ = NOTCH_CASES[name]
    s = NMSettings.get_default()
    s.segment_length_features_ms = W * 1000.0 / sfreq
    notch = fir_design.notch_bank(sfreq, 50)
    R = _ref_matrix(ref, C)
    pre = [pre_taps(pre_kind, sfreq)] if pre_kind else []
    eng = build_engine(lib, env, s, [f"ch{i}" for i in range(C)], sfreq, features=["raw_hjorth"], notch_taps=notch,
                       ref_matrix=R, pre_taps=pre, window=W)
    worst: dict = {}
    try:
        half = (len(notch) - 1) // 2
        calls = [("impulse", x, None) for x in impulse_inputs(C, W, min(half, W - 1))]
        calls += [("noise", x, z) for x, z in noise_inputs(C, W, seed=len(name) + W + C)]
        for cls, x, zero in calls:
            if cls not in classes:
                continue
            eng.reset_state()   # (the constants a plan learns from its first window: every call is a first window)
            got = eng.preprocess_window(x)
            assert_kernels(lib, name, eng, kernels)
            if pre:
                assert_kernels(lib, name, eng, {1: ONE})
            y64, y32, xin = prep_reference(x, R, pre, notch, M)
            r = check_rows(name, cls, got, y64, y32, xin, zero if R is None else None)
            worst[cls] = max(worst.get(cls, 0.0), r)
    finally:
        eng.close()
        REPORT.flush(name)
    return worst


# ---- the notch in batches: tap ------------------------------------------------------------------------------------------
HOP = 100
# name -> env, C, hops, features, {stage: kernel}
TAP_CASES = {
    "tap_4x8": ({}, 4, 8, ["raw_hjorth"], {1: NOTCH_WC}),
    "tap_33x40": ({}, 33, 40, ["raw_hjorth"], {1: NOTCH_WC}),
    "tap_q": ({"NMX_BANK_W64E": "0"}, 64, 66, ["raw_hjorth"], {1: "nmx_kern_notch_w64q_rd64"}),
    "tap_qp": ({"NMX_BANK_W64E": "0"}, 256, 96, ["raw_hjorth"], {1: "nmx_kern_notch_w64qp_rd64"}),
    "tap_fused": ({}, 64, 66, ["bandpass_filter", "sharpwave_analysis"], {1: "nmx_kern_notch_bank_w64e_rd64<1000, 499, 1>", 6: ""}),
    "tap_fused2": ({"NMX_NOTCH_SW_FUSE": "2"}, 64, 66, ["bandpass_filter", "sharpwave_analysis"],
                   {1: "nmx_kern_notch_bank_w64e_rd64<1000, 499, 2>", 6: ""}),
    "tap_nofuse": ({"NMX_NOTCH_SW_FUSE": "0"}, 64, 66, ["bandpass_filter", "sharpwave_analysis"], {1: NOTCH_WC, 6: W64E0}),
    "tap_chunks": ({"NMX_CHUNK_WINDOWS": "16"}, 4, 40, ["raw_hjorth"], {1: NOTCH_WC}),
    "tap_4x40": ({}, 4, 40, ["raw_hjorth"], {1: NOTCH_WC}),
}


def tap_recording(C: int, hops: int, cls: str, seed: int) -> np.ndarray:
    """float32 [C, T]: noise with the channel pairs cycling through PAIR_PATTERNS (zero channels excepted: the common
    average fills them), or one unit impulse per channel every 997 samples from 41 c on -- the hops move it through
    the window."""
    W, T = 1000, 1000 + (hops - 1) * HOP
    if cls == "impulse":
        x = np.zeros((C, T), np.float32)
        for c in range(C):
            x[c, (41 * c) % 997::997] = 1.0
        return x
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, T)) * SIGMA
    for p in range(C // 2):
        a, b, lvl = PAIR_PATTERNS[p % 5]
        x[2 * p] = x[2 * p] * a + lvl
        x[2 * p + 1] *= b
    assert W <= T
    return x.astype(np.float32)


def tap_run(lib, name: str, x: np.ndarray) -> np.ndarray:
    """The tapped windows [hops, C, 1000] (float64, the carried constants back in them) of case `name` on recording `x`."""
    from py_neuromodulation_amd import NMSettings, fir_design

    env, C, hops, features, kernels = TAP_CASES[name]
    s = NMSettings.get_default()
    s.features.bandpass_filter = True
    eng = build_engine(lib, env, s, [f"ch{i}_avgref" for i in range(C)], 1000.0, features=features,
                       notch_taps=fir_design.notch_bank(1000.0, 50), ref_matrix=car_matrix(C))
    try:
        _, pre = eng.process_batch(x, np.arange(hops) * HOP, tap=True)
        assert_kernels(lib, name, eng, kernels)
    finally:
        eng.close()
    assert pre.shape == (hops, C, 1000)
    return np.asarray(pre, np.float64)


def tap_reference(x: np.ndarray, hops: int):
    """(y64, y32, notch input) [hops, C, 1000] of common average -> notch on every window of the float32 recording."""
    import scipy.fft as sf

    from py_neuromodulation_amd import fir_design

    C = x.shape[0]
    win = np.stack([x[:, h * HOP:h * HOP + 1000] for h in range(hops)]).astype(np.float64)
    with sf.set_workers(min(16, os.cpu_count() or 1)):   # (the transforms of the bulk reference and the yardstick, by rows)
        return prep_reference(win, car_matrix(C), [], fir_design.notch_bank(1000.0, 50), 2048)


def tap_case(lib, name: str, same_as=(), classes=("impulse", "noise")) -> dict:
    """Impulses and noise of tap case `name` against float64; the cases of `same_as` (the same shape, another plan) must
    return the same bytes.  -> {class: worst ratio}."""
    _, C, hops, _, _ = TAP_CASES[name]
    out = {}
    for cls in classes:
        x = tap_recording(C, hops, cls, seed=C * hops)
        got = tap_run(lib, name, x)
        y64, y32, xin = tap_reference(x, hops)
        n = hops * C
        out[cls] = check_rows(name, cls, got.reshape(n, 1000), y64.reshape(n, 1000), y32.reshape(n, 1000), xin.reshape(n, 1000))
        for other in same_as:
            assert TAP_CASES[other][1:3] == (C, hops)
            same_bytes(got, tap_run(lib, other, x), f"{name} against {other}, {cls}")
    REPORT.flush(name)
    return out


def same_bytes(a: np.ndarray, b: np.ndarray, what: str) -> None:
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum())} samples differ"
