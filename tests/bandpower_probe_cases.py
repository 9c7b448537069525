"""Per-entry probes of the band-pass power feature (`bandpass_filter`): the epilogues that turn the filtered series into
*_bandpass_activity_* / _mobility_* / _complexity_* columns, and the Kalman scan that smooths the activity.  Shared by the
emulator tier (test_bandpower_probes_cpu.py) and the MI355X tier (test_bandpower_probes_gpu.py).

tests/fir_sample_probe_cases.py stops at the filtered series; this module starts there.  The tail variance over
[W - seglen, W) is written out seven times (nmx_k_bank_w64.h, _w64c.h (shared with _w64e.h), _w64d.h, _w64x2.h, _w64p.h in
registers, each with its own "is this sample in the tail" index arithmetic and a one-pass sum with a mean-shifted redo;
nmx_hjorth in LDS for nmx_kern_bank in both forms and the MC path of the one-wave kernel).  The emulator's register form is
not the device's (skip / straddle against the branch-free `(unsigned)sb < span`): only the MI355X tier sees the latter.

How a case feeds the epilogue a series it knows: `bank_taps` of ONE tap per band (GAINS, all powers of two and all
different) make the bank a product y = g_b x -- up to the rounding of the kernel's transforms, which is why every exact
expectation is tied to the series the kernel stored (HotPathEngine.filter_window, same kernel asserted by name):

  +0.0 "outside the tail" is asserted bit for bit on every entry whose input tail is all zeros; where a kernel returns
  something else, the kernel's own series of that window must be non-zero in that tail (the transform's leak, which the
  LDS forms show at 1e-19 of the impulse's square) and the entry still meets the policy against 0.

Plans that identity taps move to another kernel than tests/fir_sample_probe_cases.BANK_CASES names (reach 0: an even W
with W + reach <= 1024 selects the M = 1024 pair kernel, W + reach <= 512 the LDS kernel, W + reach <= 2048 never the
M = 4096 one; the pair kernels hold 1024 samples): nmx_kern_bank_w64c_rd64 is probed with identity taps at the odd W = 901
and 999 and with designed taps at W = 1000 / 750; nmx_kern_bank_w64d_rd64<1> (W = 500) and nmx_kern_bank_w64x2_rd64<1>
(W = 2000) with designed taps only, their reference the float64 statistics of the series filter_window returns.  KINDS below is the table; the MI355X tier asserts every name.

Classes (profiles/bandpower_probes.md has the figures):
  a  where the tail starts: tails W, W - 1, 2, 1 and lo = W - seglen around every boundary of the kind's register layout;
     one impulse per channel moved through the window by `starts`, and fixed-seed noise
  b  cancellation and the redo: noise on an offset d sigma, the side of `n mean^2 / (4 SS)` asserted for every entry
     (<= 0.8 or >= 1.25), pairs (high, low), (low, high), (high, high), a zero channel in either half, a lone last high
     channel; log_transform on and off; designed taps with a level of 300 and 50 ms tails of the slow bands; a carried
     offset of 300 on the pair kernel
  c  end to end on noise, designed taps, default tails: against the float64 statistics of the kernel's own series
     (the epilogue alone) and of the float64 direct convolution (the whole stage); conditioning under +-1 ulp <= 1e-6
  d  mobility and complexity: tails 3, 4, 5, 63, 64, 65, W; alternating, ramp, constant, zero, noise; every subset of
     {activity, mobility, complexity}, keys compared by name; the reference places nan_to_num as bandpower.py does
  e  degenerate and rail windows: amplitudes 1e-16 .. 1e16, zero and constant channels under log_transform (classes of
     tests/parity_cases._rail_class), NaN / +-inf samples: the other channels bit for bit
  f  the Kalman scan against oracle.nm_oracle.KalmanWNA on float64(z), z what the same plan writes with the filter off

Limits.  a - e: tests/parity.tolerances of the key (rtol 1e-5; atol 1e-5 for a log activity, 1e-7 otherwise), no verifier,
nothing forgiven, no entry left out.  f: the kernel is float64 throughout and rounds once, at the store:
    |got - want| <= ulp32(want) + KALMAN_F64 * max(1, max|z|)
ulp32(want) = the spacing of float32 at |want| (one rounding is at most half of it; the other half covers a float64
difference that moves `want` across a rounding boundary); KALMAN_F64 = 1e-12: the kernel's recursion and filterpy's differ
in the order of about 40 float64 operations per hop (n00 / S against P H' inv(S), the Joseph form written out), each within
2^-53 = 1.1e-16 of quantities bounded by max|z|; the filter is contractive (|1 - k0| < 1), so the differences do not
accumulate beyond a few hundred roundings: 1e-12 is 10 000 of them.  rtol 1e-5 would be 1e5 times looser."""

from __future__ import annotations

import functools

import numpy as np

from tests import parity
from tests.fir_sample_probe_cases import (NO_PAIRS, TWO_BANDS, assert_kernels, build_engine, conv64, live_taps, noise_inputs,
                                          ran, same_bytes)
from tests.timedomain_probe_cases import perturbed

SIGMA = 50.0
GAINS = (1.0, 0.5, 2.0, 0.25, 4.0, 0.125, 8.0, 0.0625)
FLT_MAX = float(np.finfo(np.float32).max)
EPS32 = float(np.finfo(np.float32).eps)
COND_RTOL = 1e-6
KALMAN_F64 = 1e-12
W64C, ONE = "nmx_kern_bank_w64c_rd64", "nmx_kern_bank_w64_rd64"
D1, D0 = "nmx_kern_bank_w64d_rd64<1>", "nmx_kern_bank_w64d_rd64<0>"
X21, X20 = "nmx_kern_bank_w64x2_rd64<1>", "nmx_kern_bank_w64x2_rd64<0>"
PP1, PP0 = "nmx_kern_bank_w64pp_rd64<1>", "nmx_kern_bank_w64pp_rd64<0>"
LDS = "nmx_kern_bank"
GENERIC, PARTITIONED = {"NMX_BANK_W64": "0"}, {"NMX_BANK_W64": "0", "NMX_BANK_PARTITIONED": "1"}

# kind -> env, sfreq, W, C, taps ("identity" | "designed"), kernel, register-layout boundaries (sample indices), emulator tier,
#         bands per engine (the 4 k-channel kinds: two)
KINDS = {
    "w64c_901": ({}, 1000.0, 901, 5, "identity", W64C, (64, 512, 832, 896), False, 8),
    "w64c_999": ({}, 1000.0, 999, 7, "identity", W64C, (64, 512, 960), False, 8),
    "w64d_full": ({}, 600.0, 600, 5, "identity", D0, (64, 512, 576), False, 8),
    "w64d_1000": ({}, 1000.0, 1000, 7, "identity", D0, (64, 512, 960), False, 8),
    "one": (NO_PAIRS, 1000.0, 1000, 4, "identity", ONE, (2, 128, 512), False, 8),
    "x2_full": ({}, 1000.0, 2500, 5, "identity", X20, (4, 256, 1024, 2048), False, 8),
    "pp_half": (NO_PAIRS, 1000.0, 1000, 4099, "identity", PP1, (2, 128, 512), False, 2),
    "pp_full": (NO_PAIRS, 1000.0, 1100, 4096, "identity", PP0, (2, 512, 1024), False, 2),
    "generic": (GENERIC, 1000.0, 1000, 3, "identity", LDS, (64, 256), True, 8),
    "partitioned": (PARTITIONED, 1000.0, 1000, 3, "identity", LDS, (64, 256), True, 8),
    "partitioned_8k": ({"NMX_BANK_PARTITIONED": "1"}, 1000.0, 8000, 2, "identity", LDS, (2048, 4096), True, 8),
    "one_emu": ({}, 1000.0, 1000, 3, "identity", "", (2, 128, 512), True, 8),   # (the emulator's plan of the default shape)
    # designed taps: the plans of tests/fir_sample_probe_cases.BANK_CASES
    "w64c_1000_fir": ({}, 1000.0, 1000, 7, "designed", W64C, (), False, 8),
    "w64c_750_fir": ({}, 750.0, 750, 5, "designed", W64C, (), False, 8),
    "w64d_half_fir": ({}, 500.0, 500, 5, "designed", D1, (), False, 8),
    "w64d_full_fir": ({}, 600.0, 600, 5, "designed", D0, (), False, 8),
    "one_fir": (NO_PAIRS, 1000.0, 1000, 4, "designed", ONE, (), False, 8),
    "x2_half_fir": ({}, 2000.0, 2000, 5, "designed", X21, (), False, 8),
    "x2_full_fir": ({}, 2500.0, 2500, 5, "designed", X20, (), False, 8),
    "pp_half_fir": (NO_PAIRS, 1000.0, 1000, 4099, "designed", PP1, (), False, 2),
    "pp_full_fir": ({}, 1100.0, 1100, 4096, "designed", PP0, (), False, 2),
    "generic_fir": (GENERIC, 1000.0, 1000, 3, "designed", LDS, (), True, 8),
    "partitioned_fir": (PARTITIONED, 1000.0, 1000, 3, "designed", LDS, (), True, 8),
    "partitioned_8k_fir": ({}, 8000.0, 8000, 2, "designed", LDS, (), True, 2),
    "one_emu_fir": ({}, 1000.0, 1000, 3, "designed", "", (), True, 8),
}
KERNELS = {W64C, D1, D0, ONE, X21, X20, PP1, PP0, LDS}
IDENTITY = [k for k, v in KINDS.items() if v[4] == "identity"]
DESIGNED = [k for k, v in KINDS.items() if v[4] == "designed"]
REGISTER = [k for k, v in KINDS.items() if v[5] not in (LDS, "")]


def on_tier(lib, kinds):
    """The kinds of `kinds` this tier runs: the emulator (lib given) those whose plan it builds, the MI355X all but the
    emulator's own."""
    return [k for k in kinds if (KINDS[k][7] if lib is not None else k not in ("one_emu", "one_emu_fir"))]


# ---- report --------------------------------------------------------------------------------------------------------------
class Report:
    """Worst plain relative error |got - want| / |want| per (kind, class), next to the figure the policy allows at that
    entry; one line per (kind, class) when flushed (profiles/bandpower_probes.md)."""

    def __init__(self) -> None:
        self.seen: dict = {}

    def add(self, kind, cls, rel, allowed, n):
        r, a, m = self.seen.get((kind, cls), (0.0, 0.0, 0))
        if rel >= r:
            r, a = float(rel), float(allowed)
        self.seen[(kind, cls)] = (r, a, m + int(n))

    def flush(self, kind=None):
        for (k, cls), (r, a, n) in list(self.seen.items()):
            if kind is None or k == kind:
                print(f"BPPROBE {k:18s} {cls:14s} entries {n:7d}  worst rel {r:9.3e}  policy there {a:9.3e}")
                del self.seen[(k, cls)]


REPORT = Report()
REDO_ROWS: dict = {}     # (kind, class) -> (entries past the redo condition, entries)
SEEN_KERNELS: dict = {}  # kind -> kernel name asserted (MI355X tier)


# ---- settings and engines ------------------------------------------------------------------------------------------------
def ms_for(n: int, sfreq: float) -> int:
    """The segment length in ms (the settings hold whole milliseconds, as the reference's do) that
    int(floor(sfreq / 1000 * ms)) maps to n samples: at 750, 600 and 500 Hz not n * 1000 / sfreq as it rounds.  (1100, 2500
    and 8000 Hz reach only some n: those windows are probed at 1 kHz -- the kernel choice reads W, not the rate.)"""
    ms = int(np.ceil(n * 1000.0 / sfreq))
    assert int(np.floor(sfreq / 1000 * ms)) == n, (n, sfreq)
    return ms


def identity_settings(sfreq, W, lens, feats=("activity",), log=False):
    """One band b<i> per tail length, one-tap filters (identity_taps)."""
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bandpass_filter = True
    s.segment_length_features_ms = ms_for(W, sfreq)
    s.frequency_ranges_hz = {f"b{i}": [4 + 4 * i, 8 + 4 * i] for i in range(len(lens))}
    bp = s.bandpass_filter_settings
    bp.segment_lengths_ms = {f"b{i}": ms_for(n, sfreq) for i, n in enumerate(lens)}
    for f in ("activity", "mobility", "complexity"):
        setattr(bp.bandpower_features, f, f in feats)
    bp.log_transform = bool(log)
    return s.validate()


def designed_settings(sfreq, W, bands=None, log=True, short_slow=False):
    """The default bands and tails (theta, alpha at 50 ms with `short_slow`: the tail of a slow band is nearly a ramp)."""
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bandpass_filter = True
    if bands is not None:
        s.frequency_ranges_hz = {k: v for k, v in s.frequency_ranges_hz.items() if k in bands}
    bp = s.bandpass_filter_settings
    bp.log_transform = bool(log)
    if short_slow:
        bp.segment_lengths_ms = {**dict(bp.segment_lengths_ms), "theta": 50, "alpha": 50}
    return s.validate()


def identity_taps(n_bands: int) -> np.ndarray:
    return np.asarray(GAINS[:n_bands], np.float64)[:, None]


def channels(C: int) -> list[str]:
    return [f"ch{i}" for i in range(C)]


def amplitudes(C: int) -> np.ndarray:
    """One amplitude per channel, all different among any 16 neighbours and exact in float32: (1 + (c mod 13) / 4) 2^(c / 13 mod 3)."""
    c = np.arange(C)
    return (1.0 + (c % 13) / 4.0) * 2.0 ** ((c // 13) % 3)


def make_engine(lib, kind: str, s, taps=None):
    env, sfreq, W, C = KINDS[kind][:4]
    eng = build_engine(lib, env, s, channels(C), sfreq, features=["bandpass_filter"], bank_taps=taps, window=W)
    assert eng.W == W, (kind, eng.W)
    return eng


def tails_of(eng, s, sfreq) -> list[int]:
    """The plan's tail lengths by band, asserted against oracle.nm_oracle.BandPower's."""
    from oracle import nm_oracle as orc

    ob = orc.BandPower(s, eng.ch_names, sfreq, taps=np.zeros((len(s.frequency_ranges_hz), 1)))
    mine = {int(eng.desc.filters[i].bp_band_index): int(eng.desc.filters[i].bp_seglen) for i in range(int(eng.desc.n_filters))}
    got = [mine[b] for b in range(len(ob.band_names))]
    assert got == [min(n, eng.W) for n in ob.seglens], (got, ob.seglens)
    return got


def columns(eng, out: np.ndarray) -> dict:
    return {k: np.asarray(out[:, i], np.float64) for i, k in enumerate(eng.keys)}


def key_of(ch: str, feat: str, band: str) -> str:
    return f"{ch}_bandpass_{feat}_{band}"


def name_kernel(lib, kind: str, eng) -> None:
    want = KINDS[kind][5]
    assert_kernels(lib, kind, eng, {3: want} if want else {})
    if lib is None:
        SEEN_KERNELS[kind] = want


# ---- references ------------------------------------------------------------------------------------------------------------
def hjorth64(t: np.ndarray, log: bool):
    """(activity, mobility, complexity) of the tails t[..., n] in float64, nan_to_num placed as bandpower.py places it
    (mode 1 of nmx_hjorth): on the final values only."""
    import warnings

    from oracle import nm_oracle as orc

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (a tail of one sample has no differences: NaN, so 0)
        act, mob, comp = orc.hjorth_params(np.asarray(t, np.float64))
        if log:
            act = np.log10(act)
    return np.nan_to_num(act), np.nan_to_num(mob), np.nan_to_num(comp)


def redo_ratio(t: np.ndarray) -> np.ndarray:
    """The register forms' redo condition `mean^2 n > 4 tot` restated in float64: n mean^2 / (4 SS), > 1 past it."""
    t = np.asarray(t, np.float64)
    n = t.shape[-1]
    m = t.mean(-1)
    ss = ((t - m[..., None]) ** 2).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ss > 0, n * m * m / (4 * ss), np.where(m != 0, np.inf, 0.0))


def var32_lanes(t: np.ndarray, lanes: int) -> float:
    """nmx_var restated in float32: two passes, `lanes` strided accumulators each summed in order, then added up.  The
    emulator has one (NMX_NT = 1), the device kernels 64 or more."""
    t = np.asarray(t, np.float32)
    n = np.float32(len(t))

    def total(v):
        parts = [np.add.accumulate(v[i::lanes], dtype=np.float32)[-1] for i in range(min(lanes, len(v)))]
        return np.add.accumulate(np.asarray(parts, np.float32), dtype=np.float32)[-1]

    d = t - total(t) / n
    return float(total(d * d) / n)


UNRESOLVED: dict = {}     # (kind, class) -> mobility / complexity entries below float32's resolution (class d: the constant channel)
EMU_LEFT_OUT: dict = {}   # kind -> entries of class a the emulator's single accumulator cannot meet the policy on


def judge(kind, cls, key, got, want, s, sfreq, W, rows=None) -> None:
    """Every entry of `got` within tests/parity.tolerances(key) of `want`; nothing is forgiven."""
    rtol, atol = parity.tolerances(key, s, sfreq, 1.0, W)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{kind} {cls} {key}: non-finite entries"
    err, lim = np.abs(got - want), atol + rtol * np.abs(want)
    live = want != 0
    if live.any():
        rel = err[live] / np.abs(want[live])
        i = int(np.argmax(rel))
        REPORT.add(kind, cls, rel[i], lim[live][i] / abs(want[live][i]), live.sum())
    bad = np.flatnonzero(err > lim)
    assert bad.size == 0, (f"{kind} {cls} {key}: {bad.size} of {got.size} entries beyond rtol {rtol:g} atol {atol:g}; row "
                           f"{bad[0] if rows is None else rows[bad[0]]}: got {got[bad[0]]!r} want {want[bad[0]]!r}")


def series_of(lib, kind, eng, win32: np.ndarray) -> np.ndarray:
    """The series the bank kernel stored for one window, [C, n_filters, W] float64 (exact float32 values), in band order;
    the same kernel as the batch, by name."""
    y = eng.filter_window(np.asarray(win32, np.float64))
    name_kernel(lib, kind, eng)
    order = [int(eng.desc.filters[i].bp_band_index) for i in range(int(eng.desc.n_filters))]
    out = np.empty_like(y)
    for i, b in enumerate(order):
        out[:, b] = y[:, i]
    return out


# ---- class a: where the tail starts -------------------------------------------------------------------------------------------
def tail_lengths(kind: str) -> list[int]:
    """W, W - 1, 2, 1 and lo = W - seglen at every boundary of the kind's layout and one either side."""
    W, bounds = KINDS[kind][2], KINDS[kind][6]
    lens = [W, W - 1, 2, 1]
    for b in bounds:
        for lo in (b - 1, b, b + 1):
            if 0 < lo < W and W - lo not in lens:
                lens.append(W - lo)
    return lens


def impulse_positions(kind: str, lens) -> list[int]:
    W, bounds = KINDS[kind][2], KINDS[kind][6]
    p = {0, 1, W - 2, W - 1}
    for n in lens:
        p |= {W - n - 1, W - n, W - n + 1}
    for b in bounds:
        p |= {b - 2, b - 1, b, b + 1}
    return sorted(q for q in p if 0 <= q < W)


def chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


def class_a(lib, kind: str) -> int:
    """-> entries compared.  The 4 k-channel kinds: the tails W, 1 and the boundaries' own (two bands an engine), five
    positions each."""
    env, sfreq, W, C, _, _, bounds, _, per = KINDS[kind]
    lens = tail_lengths(kind)
    big = C > 64
    if big:
        lens = [W, 1, W - 1, 2] + [W - b for b in bounds if 0 < b < W][-2:]
    amp = amplitudes(C)
    shift = np.arange(C) % 7          # channel c carries its impulse `shift` samples later: neighbours see neighbouring positions
    n = 0
    for group in chunks(lens, per):
        s = identity_settings(sfreq, W, group)
        eng = make_engine(lib, kind, s, identity_taps(len(group)))
        try:
            assert tails_of(eng, s, sfreq) == list(group)
            pos = impulse_positions(kind, group)
            if big:
                pos = sorted({0, W - 1} | {W - g - 1 for g in group if g < W} | {W - g for g in group})[:6]
            T0 = W + 8
            x = np.zeros((C, 2 * W + 16), np.float32)
            x[np.arange(C), T0 + shift] = amp
            starts = np.array([T0 - p for p in pos], np.int64)
            n += _identity_rows(lib, kind, "a impulse", eng, s, x, starts, group, exact_zero=True)
            rng = np.random.default_rng(W + C)
            xn = (rng.standard_normal((C, W + 8)) * SIGMA * amp[:, None]).astype(np.float32)
            # noise: every tail against the float64 variance of the series the kernel stored (two samples of noise differ by
            # a fraction of sigma: their variance reads the transform's rounding, 1e-7 max|y|, at 1e-5 and more -- the FIR's
            # share, tests/fir_sample_probe_cases.py), tails of 100 samples and more against g^2 var64(x) as well
            wins = np.stack([xn[:, a:a + W] for a in ((0, 8) if big else (0, 3, 8))])
            n += _series_rows(lib, kind, "a noise", eng, s, wins, False)[0]
            long = [(b, g) for b, g in enumerate(group) if g >= 100]
            if long:
                n += _identity_rows(lib, kind, "a noise g^2 x", eng, s, xn, np.array([0, 3, 8], np.int64), group, only=[b for b, _ in long])
        finally:
            eng.close()
    REPORT.flush(kind)
    return n


def _identity_rows(lib, kind, cls, eng, s, x32, starts, lens, exact_zero=False, log=False, redo=False, only=None) -> int:
    """process_batch of the float32 recording against g^2 var64 (log10 of it) of the tail of every window."""
    sfreq, W = KINDS[kind][1:3]
    C = x32.shape[0]
    out = columns(eng, eng.process_batch(x32, starts))
    name_kernel(lib, kind, eng)
    win = np.stack([x32[:, a:a + W] for a in starts]).astype(np.float64)     # [rows, C, W]
    n, past, stored = 0, 0, {}
    for b, seglen in enumerate(lens):
        if only is not None and b not in only:
            continue
        t = GAINS[b] * win[:, :, W - seglen:]
        want, _, _ = hjorth64(t, log)
        if redo:
            r = redo_ratio(t)
            assert np.all((r <= 0.8) | (r >= 1.25)), f"{kind} {cls} band {b}: an entry sits at the redo condition ({r.min():.3g} .. {r.max():.3g})"
            past += int((r >= 1.25).sum())
        for c in range(C):
            key = key_of(f"ch{c}", "activity", f"b{b}")
            got = out[key]
            if exact_zero:
                zero = ~t[:, c].any(-1)
                for i in np.flatnonzero(zero & ~((got == 0) & ~np.signbit(got))):
                    if i not in stored:
                        stored[i] = series_of(lib, kind, eng, win[i])
                    y = stored[i][c, b, W - seglen:]
                    assert y.any(), f"{kind} {cls} {key} row {i}: {got[i]!r} from a tail of zeros (start {starts[i]})"
            keep = np.ones(len(got), bool)
            if exact_zero and lib is not None and KINDS[kind][5] == LDS:
                # (one accumulator adds 1e-6 to 1 a thousand times, every time rounded the same way: the stand-in's own
                # error, test_the_emulators_single_accumulator; the device tier leaves nothing out)
                rtol, atol = parity.tolerances(key, s, sfreq, 1.0, W)
                for i in range(len(got)):
                    if want[i, c] != 0 and abs(var32_lanes(t[i, c], 1) - want[i, c]) > 0.5 * (atol + rtol * want[i, c]):
                        keep[i] = False
                EMU_LEFT_OUT[kind] = EMU_LEFT_OUT.get(kind, 0) + int((~keep).sum())
            if log:
                _judge_log(kind, cls, key, got, want[:, c], s, sfreq, W)
            else:
                judge(kind, cls, key, got[keep], want[keep, c], s, sfreq, W, rows=starts[keep])
            n += int(keep.sum())
    if redo:
        a, m = REDO_ROWS.get((kind, cls), (0, 0))
        REDO_ROWS[(kind, cls)] = (a + past, m + n)
    return n


def _judge_log(kind, cls, key, got, want, s, sfreq, W):
    """A log activity: log10(0) is -FLT_MAX here against -DBL_MAX there -- the classes of tests/parity_cases._rail_class;
    ordinary entries by the policy."""
    from tests.parity_cases import _rail_class

    mine = np.array([_rail_class(v, key, s, True) for v in got])
    ref = np.array([_rail_class(v, key, s, False) for v in want])
    assert np.array_equal(mine, ref), f"{kind} {cls} {key}: rail classes {mine.tolist()} against {ref.tolist()}"
    ok = ref == 0
    if ok.any():
        judge(kind, cls, key, got[ok], want[ok], s, sfreq, W)
    assert np.all(got[~ok] == -FLT_MAX), f"{kind} {cls} {key}: {got[~ok]}"


# ---- class b: cancellation and the redo -----------------------------------------------------------------------------------
def offsets_b(C: int) -> np.ndarray:
    """d per channel, in sigmas (NaN: a zero channel): the pairs (high, low), (low, high), (high, high), (zero, high),
    (high, zero), far on either side (0, 1000), and a lone last channel that is high (odd C)."""
    pat = [3.0, 1.5, 1.5, 3.0, 3.0, 3.0, np.nan, 3.0, 3.0, np.nan, 0.0, 1000.0, 1000.0, 0.0]
    d = np.array([pat[c % len(pat)] for c in range(C)])
    d[-1] = 3.0
    if C > 64:   # (thousands of channels: the sample mean of a 100-sample tail strays 4 sigma / 10; 1.25 keeps 0.8 clear)
        d[d == 1.5] = 1.25
    return d


B_TAILS = {1000: (1000, 500, 333, 100), 999: (999, 500, 333, 100), 901: (901, 500, 333, 100), 1100: (1100, 550, 333, 110), 500: (500, 250, 166, 100),
           600: (600, 300, 200, 100), 2500: (2500, 1250, 832, 250), 8000: (8000, 4000, 2664, 800)}
B_CHANNELS = 15   # (odd: the last channel has no partner; the kernel choice of the small kinds does not depend on it)


def class_b_identity(lib, kind: str) -> int:
    env, sfreq, W, C0, _, _, _, _, per = KINDS[kind]
    C = C0 if C0 > 64 else B_CHANNELS
    d = offsets_b(C)
    rng = np.random.default_rng(3 * W + 1)
    x = rng.standard_normal((C, W + 4)) * SIGMA + np.nan_to_num(d)[:, None] * SIGMA
    x[np.isnan(d)] = 0.0
    x32 = x.astype(np.float32)
    n = 0
    for group in chunks(list(B_TAILS[W]), per):
        for log in (False, True):
            s = identity_settings(sfreq, W, group, log=log)
            eng = build_engine(lib, env, s, channels(C), sfreq, features=["bandpass_filter"], bank_taps=identity_taps(len(group)),
                               window=W)
            try:
                # (the reference reads the kernel's own series: at d = 1000 the transform's rounding of the level, 1e-7 of
                # 50 000 per sample and not white, moves the variance of g x by more than the policy -- the FIR's share)
                wins = np.stack([x32[:, a:a + W] for a in (0, 1, 4)])
                cls = f"b log={int(log)}"
                m, ratios = _series_rows(lib, kind, cls, eng, s, wins, log, want_redo=True)
                n += m
                for (i, c, band), r in ratios.items():
                    assert r <= 0.8 or r >= 1.25, f"{kind} {cls} row {i} ch{c} {band}: ratio {r:.3g} sits at the redo condition"
                    assert (r >= 1.25) == (d[c] >= 3.0), f"{kind} {cls} row {i} ch{c} {band}: ratio {r:.3g} on the wrong side for d = {d[c]}"
                a, k = REDO_ROWS.get((kind, cls), (0, 0))
                REDO_ROWS[(kind, cls)] = (a + sum(r >= 1.25 for r in ratios.values()), k + len(ratios))
            finally:
                eng.close()
    REPORT.flush(kind)
    return n


def _series_rows(lib, kind, cls, eng, s, wins32, log, feats=("activity",), bands=None, want_redo=False, rows=None):
    """process_batch of windows laid end to end against the float64 statistics of the series filter_window returns for
    each (the epilogue alone).  -> (entries, {(row, channel, band): redo ratio})."""
    sfreq, W = KINDS[kind][1:3]
    C = wins32.shape[1]
    x = np.ascontiguousarray(np.concatenate(list(wins32), axis=1))
    starts = np.arange(len(wins32), dtype=np.int64) * W
    out = columns(eng, eng.process_batch(x, starts))
    name_kernel(lib, kind, eng)
    lens = tails_of(eng, s, sfreq)
    names = list(s.frequency_ranges_hz)
    ys = np.stack([series_of(lib, kind, eng, w) for w in wins32])          # [rows, C, B, W]
    n, ratios = 0, {}
    for b, (band, seglen) in enumerate(zip(names, lens)):
        t = ys[:, :, b, W - seglen:]
        want = dict(zip(("activity", "mobility", "complexity"), hjorth64(t, log)))
        if want_redo:
            r = redo_ratio(t)
            for i in range(r.shape[0]):
                for c in range(C):
                    ratios[(i, c, band)] = float(r[i, c])
        # a ratio of variances is judged where float32 can resolve both: the mean a two-pass variance is shifted by is a
        # float32, off by up to one ulp of the series' level, which adds its square -- a variance below (eps32 level)^2 / rtol
        # (a constant through the transforms: 300 and their rounding) is not known to rtol; there mobility and complexity
        # must only be finite and not negative
        d1 = np.diff(t, axis=-1)
        res0 = np.var(t, axis=-1) * 1e-5 >= (EPS32 * np.abs(t).max(-1)) ** 2
        res1 = np.var(d1, axis=-1) * 1e-5 >= (EPS32 * np.abs(d1).max(-1)) ** 2 if d1.shape[-1] else res0
        zero = ~t.any(-1)                                  # (an all-zero tail: every ratio NaN, so 0 -- judged)
        ok = {"activity": res0 | zero, "mobility": res0 | zero, "complexity": (res0 & res1) | zero}
        cap = np.var(t, axis=-1) + 4 * (EPS32 * np.abs(t).max(-1)) ** 2 + 1e-7
        for c in range(C):
            for f in feats:
                key = key_of(f"ch{c}", f, band)
                got, k = out[key], ok[f][:, c]
                if f == "activity" and not k.all():   # (... and the activity no more than the variance and that square)
                    lin = 10.0 ** got[~k] if log else got[~k]
                    assert np.all(lin <= cap[~k, c]) and np.all(lin >= 0), (kind, cls, key, got[~k], cap[~k, c])
                if log and f == "activity":
                    _judge_log(kind, cls, key, got[k], want[f][k, c], s, sfreq, W)
                    UNRESOLVED[(kind, cls)] = UNRESOLVED.get((kind, cls), 0) + int((~k).sum())
                else:
                    judge(kind, cls, key, got[k], want[f][k, c], s, sfreq, W, rows=rows)
                    assert np.isfinite(got).all() and np.all(got >= 0), (kind, cls, key, got)
                    UNRESOLVED[(kind, cls)] = UNRESOLVED.get((kind, cls), 0) + int((~k).sum())
                n += int(k.sum())
    assert set(out) == {key_of(f"ch{c}", f, band) for c in range(C) for band in names for f in feats}
    return n, ratios


def class_b_designed(lib, kind: str) -> int:
    """Designed taps, the noise of the FIR probes (PAIR_PATTERNS: a level of 300 in the even channel of the first pair),
    theta and alpha at 50 ms: at least one entry past the redo condition."""
    env, sfreq, W, C, _, _, _, _, per = KINDS[kind]
    s = designed_settings(sfreq, W, TWO_BANDS if per == 2 else None, log=True, short_slow=True)
    eng = make_engine(lib, kind, s)
    try:
        wins = [x.astype(np.float32) for x, _ in noise_inputs(C, W, seed=7 + W + C)][:2 if C > 64 else None]
        n, ratios = _series_rows(lib, kind, "b designed", eng, s, np.stack(wins), True, want_redo=True)
    finally:
        eng.close()
    past = sum(r > 1.0 for r in ratios.values())
    REDO_ROWS[(kind, "b designed")] = (past, len(ratios))
    if KINDS[kind][5] not in (LDS, ""):
        assert past >= 1, f"{kind}: no entry past the redo condition (largest ratio {max(ratios.values()):.3g})"
    REPORT.flush(kind)
    return n


def class_b_carried(lib, kind: str = "w64c_999") -> int:
    """A carried offset of 300 on the pair kernel (the kernels' `dcf`): the recording handed over as float32 residual, the
    constants through set_offsets; the tails see x = u + 300 and every entry is past the redo condition."""
    env, sfreq, W, C = KINDS[kind][:4]
    lens = list(B_TAILS[W])
    s = identity_settings(sfreq, W, lens)
    eng = make_engine(lib, kind, s, identity_taps(len(lens)))
    try:
        assert eng.carries_offsets
        eng.set_offsets(np.full(C, 300.0))
        rng = np.random.default_rng(11)
        u = (rng.standard_normal((C, W + 4)) * SIGMA * amplitudes(C)[:, None] * 0.125).astype(np.float32)
        starts = np.array([0, 1, 4], np.int64)
        out = columns(eng, eng.process_batch(u, starts))
        name_kernel(lib, kind, eng)
        n = 0
        for b, seglen in enumerate(lens):
            t = np.stack([u[:, a + W - seglen:a + W] for a in starts]).astype(np.float64)
            # (u + 300 rounds to float32 in the kernel: the reference reads the float32 sums)
            t = GAINS[b] * (t.astype(np.float32) + np.float32(300.0)).astype(np.float64)
            assert redo_ratio(t).min() >= 1.25
            want, _, _ = hjorth64(t, False)
            for c in range(C):
                key = key_of(f"ch{c}", "activity", f"b{b}")
                judge(kind, "b carried", key, out[key], want[:, c], s, sfreq, W)
                n += len(starts)
        REDO_ROWS[(kind, "b carried")] = (n, n)
    finally:
        eng.close()
    REPORT.flush(kind)
    return n


# ---- class c: end to end on noise ----------------------------------------------------------------------------------------------
C_SEEDS: dict = {}      # kind -> seed used
C_ERRORS: dict = {}     # kind -> (worst rel error against the kernel's own series, against the float64 convolution)
C_PICK = 24             # channels of a 4 k-channel kind that get the float64 convolution (spread over the case)


def stage64(x32: np.ndarray, taps, lens, log: bool) -> np.ndarray:
    """[C, B]: float64 direct convolution (zero padding) of the float32 window, then the float64 tail statistic."""
    W = x32.shape[1]
    out = np.empty((x32.shape[0], len(taps)))
    for b, (h, seglen) in enumerate(zip(taps, lens)):
        y = conv64(x32.astype(np.float64), live_taps(h, W))
        out[:, b] = hjorth64(y[:, W - seglen:], log)[0]
    return out


def class_c(lib, kind: str) -> int:
    env, sfreq, W, C, _, _, _, _, per = KINDS[kind]
    s = designed_settings(sfreq, W, (("alpha", "high_beta") if W == 8000 else TWO_BANDS) if per == 2 else None, log=True)
    eng = make_engine(lib, kind, s)
    try:
        lens = tails_of(eng, s, sfreq)
        order = [int(eng.desc.filters[i].bp_band_index) for i in range(int(eng.desc.n_filters))]
        taps = [None] * len(order)
        for i, b in enumerate(order):
            taps[b] = np.asarray(eng.filter_taps[i], np.float64)
        pick = np.arange(C) if C <= 64 else np.unique(np.linspace(0, C - 1, C_PICK).astype(int))
        for seed in range(3):
            x32 = noise_inputs(C, W, seed=100 * seed + W + C)[0][0].astype(np.float32)
            want = stage64(x32[pick], taps, lens, True)
            moved = stage64(perturbed(x32[pick]), taps, lens, True)
            ok = np.abs(want) < 1e200
            with np.errstate(invalid="ignore"):
                k = float(np.max(np.abs(10.0 ** (moved[ok] - want[ok]) - 1.0)))
            if k <= COND_RTOL:
                break
        else:
            raise AssertionError(f"{kind}: no seed of three is well conditioned (last {k:.2e})")
        C_SEEDS[kind] = (seed, k)
        n, _ = _series_rows(lib, kind, "c own series", eng, s, x32[None], True)
        rel1 = REPORT.seen.get((kind, "c own series"), (0.0,))[0]
        out = columns(eng, eng.process_batch(x32, np.zeros(1, np.int64)))
        for bi, band in enumerate(s.frequency_ranges_hz):
            for j, c in enumerate(pick):
                key = key_of(f"ch{c}", "activity", band)
                _judge_log(kind, "c float64 conv", key, out[key], want[j:j + 1, bi], s, sfreq, W)
                n += 1
        C_ERRORS[kind] = (rel1, REPORT.seen.get((kind, "c float64 conv"), (0.0,))[0])
    finally:
        eng.close()
    REPORT.flush(kind)
    return n


# ---- class d: mobility and complexity ---------------------------------------------------------------------------------------------
D_KINDS = ("one", "generic", "partitioned", "one_emu")
D_TAILS = (3, 4, 5, 63, 64, 65, 1000)
D_SUBSETS = [f for m in range(1, 8) for f in [tuple(x for i, x in enumerate(("activity", "mobility", "complexity")) if m >> i & 1)]]


def series_d(W: int) -> np.ndarray:
    """float32 [5, W]: alternating +-3, a ramp, a constant, zeros, noise."""
    n = np.arange(W)
    rng = np.random.default_rng(5)
    return np.stack([3.0 * (1 - 2 * (n % 2)), 0.25 * n - 17.0, np.full(W, 300.0), np.zeros(W), rng.standard_normal(W) * SIGMA]).astype(np.float32)


def class_d(lib, kind: str, feats: tuple) -> int:
    env, sfreq, W, _, _, _, _, _, _ = KINDS[kind]
    C = 5
    s = identity_settings(sfreq, W, D_TAILS, feats=feats)
    eng = build_engine(lib, env, s, channels(C), sfreq, features=["bandpass_filter"], bank_taps=identity_taps(len(D_TAILS)), window=W)
    try:
        x = series_d(W + 1)
        wins = np.stack([x[:, :W], x[:, 1:W + 1]])
        n, _ = _series_rows(lib, kind, "d " + "+".join(f[:3] for f in feats), eng, s, wins, False, feats=feats)
    finally:
        eng.close()
    REPORT.flush(kind)
    return n


# ---- class e: degenerate and rail windows ----------------------------------------------------------------------------------------
E_KINDS = ("w64c_999", "w64d_1000", "one", "generic", "one_emu")
E_TAILS = (500, 333, 100, 64)
E_GAINS = np.array([[1.0], [0.5], [0.25], [0.125]])


def class_e_amplitudes(lib, kind: str) -> int:
    """Noise at amplitudes 1e-16 .. 1e16 (the sum of squares of 500 samples at 50e16 stays inside float32), a zero and a
    constant channel, log_transform on and off."""
    env, sfreq, W = KINDS[kind][:3]
    scales = [1e-16, 1e16, 1e-8, 1e8, 1.0, 0.0, 1e12, 1e-12, 1e16, 1e-16, 1e4, 0.0]
    C = len(scales)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((C, W + 2)) * SIGMA * np.asarray(scales)[:, None]
    x[-1] = 300.0                       # (a constant; channel 5 is zero)
    x32 = x.astype(np.float32)
    lens = [min(t, W) for t in E_TAILS]
    n = 0
    for log in (False, True):
        s = identity_settings(sfreq, W, lens, log=log)
        eng = build_engine(lib, env, s, channels(C), sfreq, features=["bandpass_filter"], bank_taps=E_GAINS, window=W)
        try:
            wins = np.stack([x32[:, :W], x32[:, 2:W + 2]])
            m, _ = _series_rows(lib, kind, f"e amplitudes log={int(log)}", eng, s, wins, log)
            n += m
        finally:
            eng.close()
    REPORT.flush(kind)
    return n


E_BAD = {"nan": (np.nan,), "inf": (np.inf, -np.inf)}
E_PARTNER: dict = {}    # (kind, which) -> worst |got - clean| of a pair partner's log activity


def class_e_bad_samples(lib, kind: str, which: str = "nan") -> int:
    """NaN (`which` = "nan") or +inf, -inf ("inf") in one sample of one channel, at lo - 1, lo, W - 1, 0 of the 333-sample
    tail, in the even and in the odd channel of a pair: every OTHER channel bit for bit what it is without the bad sample.
    In the channel-pair kernels the partner (c ^ 1) shares one complex transform with the bad channel, and with it the
    transform's roundings: it is held to the policy against the clean run, not to its bits.  A NaN sample is a zero sample
    (nan_to_num on load): the whole row is, bit for bit, the run with 0 there."""
    env, sfreq, W = KINDS[kind][:3]
    C = 5
    lens = [min(t, W) for t in E_TAILS]
    s = identity_settings(sfreq, W, lens, log=True)
    eng = build_engine(lib, env, s, channels(C), sfreq, features=["bandpass_filter"], bank_taps=identity_taps(4), window=W)
    n = 0
    pairs = KINDS[kind][5] in (W64C, D0, D1)   # two channels, c and c ^ 1, share one complex transform
    try:
        rng = np.random.default_rng(23)
        x32 = (rng.standard_normal((C, W)) * SIGMA * amplitudes(C)[:, None]).astype(np.float32)
        z = np.zeros(1, np.int64)
        clean = eng.process_batch(x32, z).copy()
        name_kernel(lib, kind, eng)
        per = len(lens)
        missed = []
        for ch in (2, 3):
            for p in (W - 333 - 1, W - 333, W - 1, 0):
                for bad in E_BAD[which]:
                    y = x32.copy()
                    y[ch, p] = bad
                    got = eng.process_batch(y, z)
                    assert np.isfinite(got).all(), (kind, ch, p, bad)
                    mate = ch ^ 1 if pairs else ch
                    others = np.ones(C * per, bool)
                    for k in {ch, mate}:
                        others[k * per:(k + 1) * per] = False
                    same_bytes(got[:, others], clean[:, others], f"{kind}: channels next to {bad} at sample {p} of channel {ch}")
                    if pairs:
                        sl = slice(mate * per, (mate + 1) * per)
                        dev = float(np.abs(got[0, sl].astype(np.float64) - clean[0, sl]).max())
                        E_PARTNER[(kind, which)] = max(E_PARTNER.get((kind, which), 0.0), dev)
                        rtol, atol = parity.tolerances(eng.keys[mate * per], s, sfreq, 1.0, W)
                        if dev > atol + rtol * float(np.abs(clean[0, sl]).min()):
                            missed.append((ch, p, bad, got[0, sl].tolist(), clean[0, sl].tolist()))
                    if np.isnan(bad):
                        y0 = x32.copy()
                        y0[ch, p] = 0.0
                        same_bytes(got, eng.process_batch(y0, z), f"{kind}: NaN at sample {p} of channel {ch} against 0 there")
                    n += got.size
        assert not missed, (f"{kind}: the pair partner of a channel with a bad sample left the policy in {len(missed)} of "
                            f"{8 * len(E_BAD[which])} runs; first (channel, sample, value, got, clean): {missed[0]}")
    finally:
        eng.close()
    return n


# ---- class f: the Kalman scan -----------------------------------------------------------------------------------------------
KW, KHOP, KSFREQ = 128, 16, 1000.0     # a short window: the LDS bank kernel on both tiers, the scan does not see the bank
K_DEFAULT = dict(Tp=0.1, sigma_w=0.7, sigma_v=1.0)
# name -> C, bands, mask (band indices; -1: a band that frequency_ranges_hz does not have), parameters, log, hops
KALMAN_CASES = {
    "default_63": dict(C=7, B=9, mask="all", par=K_DEFAULT, log=True, hops=40),
    "default_64": dict(C=8, B=8, mask="all", par=K_DEFAULT, log=True, hops=40),
    "default_65": dict(C=13, B=5, mask="all", par=K_DEFAULT, log=True, hops=40),
    "one_band_65": dict(C=65, B=1, mask="all", par=K_DEFAULT, log=True, hops=24),
    "threads_129": dict(C=43, B=3, mask="all", par=K_DEFAULT, log=True, hops=24),
    "mask_first": dict(C=3, B=5, mask=(0,), par=K_DEFAULT, log=True, hops=40),
    "mask_last": dict(C=3, B=5, mask=(4,), par=K_DEFAULT, log=True, hops=40),
    "mask_apart": dict(C=3, B=5, mask=(0, 2, 4), par=K_DEFAULT, log=True, hops=40),
    "mask_unknown": dict(C=3, B=5, mask=(1, -1, 3), par=K_DEFAULT, log=True, hops=40),
    "mask_mc": dict(C=3, B=4, mask=(1, 3), par=K_DEFAULT, log=True, hops=40, feats=("activity", "mobility", "complexity")),
    "Tp_small": dict(C=3, B=3, mask="all", par=dict(Tp=0.01, sigma_w=0.7, sigma_v=1.0), log=True, hops=60),
    "Tp_one": dict(C=3, B=3, mask="all", par=dict(Tp=1.0, sigma_w=0.7, sigma_v=1.0), log=True, hops=60),
    "Q_zero": dict(C=3, B=3, mask="all", par=dict(Tp=0.1, sigma_w=0.0, sigma_v=1.0), log=True, hops=60),
    "sigma_w_10": dict(C=3, B=3, mask="all", par=dict(Tp=0.1, sigma_w=10.0, sigma_v=1.0), log=True, hops=60),
    "sigma_v_small": dict(C=3, B=3, mask="all", par=dict(Tp=0.1, sigma_w=0.7, sigma_v=1e-3), log=True, hops=60),
    "sigma_v_100": dict(C=3, B=3, mask="all", par=dict(Tp=0.1, sigma_w=0.7, sigma_v=100.0), log=True, hops=60),
    "no_log": dict(C=3, B=3, mask="all", par=K_DEFAULT, log=False, hops=60),
}
KALMAN_WORST: dict = {}    # case -> (worst |got - want| / limit, worst |got - want|, limit there)


def kalman_settings(c: dict, on: bool):
    s = identity_settings(KSFREQ, KW, [KW - 5 * b for b in range(c["B"])], feats=c.get("feats", ("activity",)), log=c["log"])
    names = list(s.frequency_ranges_hz)
    s.bandpass_filter_settings.kalman_filter = bool(on)
    ks = s.kalman_filter_settings
    ks.Tp, ks.sigma_w, ks.sigma_v = c["par"]["Tp"], c["par"]["sigma_w"], c["par"]["sigma_v"]
    ks.frequency_bands = names if c["mask"] == "all" else [names[i] if i >= 0 else "no_such_band" for i in c["mask"]]
    return s.validate()


def kalman_taps(B: int) -> np.ndarray:
    """One tap per band, all different (nine bands: GAINS and 3)."""
    return np.asarray((GAINS + (3.0, 6.0, 1.5))[:B], np.float64)[:, None]


def kalman_recording(C: int, hops: int, seed: int = 0, dead=None) -> np.ndarray:
    """float32 [C, T]: noise whose amplitude wanders per channel (every filter a sequence of its own).  `dead`:
    {channel: (first hop, last hop)} -- zeros over every window of those hops."""
    T = KW + (hops - 1) * KHOP
    rng = np.random.default_rng(seed)
    env = np.exp(np.cumsum(rng.standard_normal((C, T)) * 0.02, axis=1) + rng.uniform(-1, 1, (C, 1)))
    x = rng.standard_normal((C, T)) * SIGMA * env
    for ch, (a, b) in (dead or {}).items():
        x[ch, a * KHOP:(b * KHOP + KW if b is not None else T)] = 0.0
    return x.astype(np.float32)


def kalman_engine(lib, c: dict, on: bool, env=None):
    s = kalman_settings(c, on)
    eng = build_engine(lib, env or {}, s, channels(c["C"]), KSFREQ, features=["bandpass_filter"], bank_taps=kalman_taps(c["B"]),
                       window=KW)
    return eng, s


def kalman_want(z: np.ndarray, par: dict) -> np.ndarray:
    """KalmanWNA.step over float64(z) [hops], then nan_to_num as bandpower.py places it."""
    from oracle import nm_oracle as orc

    kf = orc.KalmanWNA(par["Tp"], par["sigma_w"], par["sigma_v"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.nan_to_num(np.array([kf.step(float(v)) for v in np.asarray(z, np.float64)]))


def kalman_limit(want: np.ndarray, z: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + KALMAN_F64 * max(1.0, float(np.abs(z).max()))


def kalman_check(name, s, c, keys, z_out, k_out) -> int:
    """Masked activity columns against the oracle; every other column bit for bit the unfiltered run's."""
    names = list(s.frequency_ranges_hz)
    masked = set(names) if c["mask"] == "all" else {names[i] for i in c["mask"] if i >= 0}
    n = 0
    worst = KALMAN_WORST.get(name, (0.0, 0.0, 0.0))
    for i, key in enumerate(keys):
        band = key.rsplit("_", 1)[1]
        if "_activity_" in key and band in masked:
            z = z_out[:, i].astype(np.float64)
            want = kalman_want(z, c["par"])
            lim = kalman_limit(want, z)
            err = np.abs(k_out[:, i].astype(np.float64) - want)
            j = int(np.argmax(err / lim))
            if err[j] / lim[j] > worst[0]:
                worst = (float(err[j] / lim[j]), float(err[j]), float(lim[j]))
            assert np.all(err <= lim), f"kalman {name} {key}: hop {j}: got {k_out[j, i]!r} want {want[j]!r}: {err[j]:.3e} > {lim[j]:.3e}"
            n += len(z)
        else:
            same_bytes(k_out[:, i], z_out[:, i], f"kalman {name} {key}: a column the scan must not touch")
    KALMAN_WORST[name] = worst
    return n


def class_f(lib, name: str) -> int:
    c = KALMAN_CASES[name]
    x = kalman_recording(c["C"], c["hops"], seed=len(name))
    starts = np.arange(c["hops"], dtype=np.int64) * KHOP
    outs = []
    for on in (False, True):
        eng, s = kalman_engine(lib, c, on)
        try:
            outs.append(eng.process_batch(x, starts).copy())
            assert_kernels(lib, name, eng, {3: LDS})
            if lib is None:
                assert ran(eng.kernels(3), "nmx_kern_kalman") == on, eng.kernels(3)
            keys = list(eng.keys)
        finally:
            eng.close()
    n = kalman_check(name, s, c, keys, outs[0], outs[1])
    w = KALMAN_WORST[name]
    print(f"BPPROBE kalman {name:14s} entries {n:6d}  worst error {w[1]:.3e} = {w[0]:.3f} of the limit {w[2]:.3e}")
    return n


CARRY = dict(C=2, B=3, mask=(0, 2), par=K_DEFAULT, log=True, hops=700)


@functools.lru_cache(maxsize=None)
def carry_recording():
    return kalman_recording(CARRY["C"], CARRY["hops"], seed=99)


def class_f_carry(lib) -> int:
    """One sequence of 700 hops, six ways, bit-identical; reset_state reproduces the first rows."""
    c, x = CARRY, carry_recording()
    starts = np.arange(c["hops"], dtype=np.int64) * KHOP

    def run(env, how):
        eng, s = kalman_engine(lib, c, True, env)
        try:
            return how(eng)
        finally:
            eng.close()

    def split(eng):
        return np.concatenate([eng.process_batch(x, starts[:1]), eng.process_batch(x, starts[1:18]), eng.process_batch(x, starts[18:])])

    def single(eng):
        first = np.stack([eng.process_window(x[:, a:a + KW].astype(np.float64)) for a in starts[:20]])
        return np.concatenate([first, eng.process_batch(x, starts[20:])])

    def moved(eng):
        a = eng.process_batch(x, starts[:333]).copy()
        blob = eng.export_state()
        other, _ = kalman_engine(lib, c, True)
        try:
            other.import_state(blob)
            b = other.process_batch(x, starts[333:]).copy()
        finally:
            other.close()
        return np.concatenate([a, b])

    def again(eng):
        a = eng.process_batch(x, starts).copy()
        eng.reset_state()
        b = eng.process_batch(x, starts[:50])
        same_bytes(b, a[:50], "kalman carry: the first rows after reset_state")
        return a

    whole = run({}, again)
    ways = {"batches of 1, 17 and the rest": run({}, split), "process_window for 20 hops": run({}, single),
            "export_state / import_state at hop 333": run({}, moved),
            "host chunks of 8 and 32": run({"NMX_HOST_FIRST_CHUNK": "8", "NMX_HOST_CHUNK_WINDOWS": "32"}, lambda e: e.process_batch(x, starts).copy()),
            "NMX_CHUNK_WINDOWS=16": run({"NMX_CHUNK_WINDOWS": "16"}, lambda e: e.process_batch(x, starts).copy())}
    for what, got in ways.items():
        same_bytes(got, whole, f"kalman carry: {what} against one batch")
    # ... and the one batch against the oracle
    eng, s = kalman_engine(lib, c, False)
    try:
        z = eng.process_batch(x, starts).copy()
        keys = list(eng.keys)
    finally:
        eng.close()
    return kalman_check("carry_700", s, c, keys, z, whole)


def class_f_dead(lib) -> int:
    """A channel that is zero over hops 5 - 7 and one dead from the start: log10f(0) = -inf enters the filter raw; -FLT_MAX at
    the first dead hop, 0 for ever after (the reference: -inf once, NaN for ever).  The other filters bit for bit a run
    without the dead channels; the state survives export / import with its NaN."""
    c = dict(C=4, B=2, mask="all", par=K_DEFAULT, log=True, hops=30)
    starts = np.arange(c["hops"], dtype=np.int64) * KHOP
    live = kalman_recording(c["C"], c["hops"], seed=5)
    # (zero over every sample the windows of hops 5 .. 7 read, and no other window in full)
    dead = live.copy()
    dead[1, 5 * KHOP:7 * KHOP + KW] = 0.0
    dead[3, :] = 0.0
    eng, s = kalman_engine(lib, c, True)
    try:
        a = eng.process_batch(live, starts).copy()
        eng.reset_state()
        b = eng.process_batch(dead, starts[:12]).copy()
        blob = eng.export_state()
        other, _ = kalman_engine(lib, c, True)
        try:
            other.import_state(blob)
            assert other.export_state() == blob, "the state blob changed in the round trip"
            b = np.concatenate([b, other.process_batch(dead, starts[12:])])
        finally:
            other.close()
        keys = list(eng.keys)
    finally:
        eng.close()
    off, s = kalman_engine(lib, c, False)
    try:
        z = off.process_batch(dead, starts).astype(np.float64)
    finally:
        off.close()
    n = 0
    for i, key in enumerate(keys):
        if key.startswith(("ch1_", "ch3_")):
            first = 5 if key.startswith("ch1_") else 0
            assert z[first, i] == -FLT_MAX and np.all(z[:first, i] > -1e30), (key, z[:, i])
            zi = np.where(z[:, i] == -FLT_MAX, -np.inf, z[:, i])     # (the scan reads the raw log10f(0))
            want = kalman_want(zi, c["par"])
            assert want[first] < -1e300 and not want[first + 1:].any()
            assert b[first, i] == np.float32(-FLT_MAX) and not b[first + 1:, i].any(), (key, b[:, i])
            if first:
                lim = kalman_limit(want[:first], zi[:first])
                assert np.all(np.abs(b[:first, i] - want[:first]) <= lim), (key, b[:first, i], want[:first])
        else:
            same_bytes(b[:, i], a[:, i], f"kalman dead {key}: a filter next to a dead channel")
        n += len(b)
    # the oracle agrees on the classes: -inf once, NaN afterwards
    w = kalman_want(np.array([1.0, 2.0, -np.inf, 1.0, 2.0]), K_DEFAULT)
    assert w[2] < -1e300 and not w[3:].any()
    return n
