"""Per-window probes of the time-domain statistics (Hjorth activity / mobility / complexity, LineLength, Raw), shared by the
emulator tier (test_timedomain_probes_cpu.py) and the MI355X tier (test_timedomain_probes_gpu.py).

Six implementations compute these five numbers (the table below); the rest of the suite sees them as three extra columns
of well-scaled noise at W = 1000 with window starts that are multiples of four.  A probe case names ONE implementation,
asserts it by the kernel the plan reports (`eng.kernels(2)` against `timeosc_kind`, the plan's precedence restated here and
tied to the source text by the CPU tier), and compares every (window, channel) of the batch with a float64 restatement of
hjorth_raw.py / linelength.py over `sliding_window_view` (`reference`; tied to oracle.Hjorth / LineLength / Raw, exactly
equal, on a subset of windows of every case) applied to nan_to_num of the float32 samples the engine was given (the input
minus the constants the engine split off, `eng.offsets()`), widened exactly.

Policy: tests/parity.compare with the family tolerances (hjorth / linelength 1e-5 relative + 1e-9 max(amp, 1); raw 1e-6
relative + 1e-6 amp), amp per channel, and NO verifier: nothing can be forgiven, tests/accepted_miss_budget.json has no
entry for these families and gets none.  Two places are STRICTER than the policy, none is wider:
  * mobility and complexity do not scale with the input, so they are compared with amp = 1 (an atol of 1e-9 whatever the
    amplitude; at 1e14 the policy's own atol would be 1e5 and the comparison empty);
  * where the reference's mobility is exactly 0 (a constant window, an exact ramp) the atol is not used at all: the kernel's
    first differences are exact there and its mean of them carries one float32 rounding, so
    |mobility| <= 2^-22 |step| / sqrt(activity), computed from the reference's numbers (`zero_mobility_bound`); complexity
    must then be 0 within the policy's atol.
A window that holds an infinity sits on the rail: +-FLT_MAX in the engine's float32, +-DBL_MAX in the reference's float64.
Its activity and line length (and raw, when the last sample is the one) are rail-derived on both scales: every entry must
fall in the reference's class -- tests/parity_cases.py: `_rail_class`, the classes of case_inf_members: ordinary, rail-derived
with the same sign (beyond 1e25 here, beyond 1e200 there), NaN -- and every ordinary entry of such a window (mobility and
complexity: 0 on both scales) goes through the policy like any other.  The `e_rail_*` cases put the bad sample in front of a
common-average re-reference: every channel of the group then holds a FINITE +-1e38 in that sample (the member itself
FLT_MAX, the others -FLT_MAX / 3), the window passes the cleaning untouched and leaves the packed form by its
`!(fabsf(p0) < 1e30f)` exit; their reference is the float64 pipeline (nan_to_num, processing/rereference.py's row minus
the mean of the others, the features) on the input, the re-referenced samples differing from the engine's by one float32
rounding each.

Conditioning is a condition on the INPUT, checked on the CPU before any kernel sees it (`draw`): the float32 samples are
perturbed by +-1 ulp (fixed seed) and every entry of the float64 reference must move by less than 1e-6 relative, a tenth
of the tolerance; a white-noise recording that fails is redrawn with the next seed.

    implementation                        where                     variant (VARIANTS)           kernels
    two-pass LDS item                     nmx_k_timeosc.h           two_pass                     nmx_kern_timeosc, ..._fixed128
    long-window item                      nmx_k_timeosc_long.h      long                         nmx_kern_timeosc_long
    packed registers, runtime W           nmx_k_td.h                td_emit<0>                   nmx_kern_scan, ..._w510 (W % 4 == 0)
    packed registers, W = 1000            nmx_k_td.h                td_load<1000>                nmx_kern_timeosc_w1000
                                                                    td_load<1000> SUM4 off / on  (the <4> and the SPEC-folded build)
                                                                    td_load_x + td_rest_from_x   nmx_kern_timeosc_w1000_low (SUM4 off: <4>;
                                                                                                 on: the two SPEC builds)
    scalar DPP form                       nmx_k_scan.h              scan                         nmx_kern_scan (W % 4 != 0 or W < 8),
                                                                                                 ..._w510 at W = 510, every NaN / inf window
    single pass about a four-sample pivot nmx_k_specmm.h            specmm                       nmx_kern_specmm_w1000 (+ ..._w1000_todo)

Classes (`CASES`; the figures observed are in profiles/timedomain_probes.md)
  a  lengths on the scan kernel: packed W in PACKED_W, scalar W in SCALAR_W, 1028 (no scan kernel any more); float64
     input with offsets of 100 spreads, so that the constants travel as dcf
  b  odd hops: window starts of every residue mod 4 on the scan kernel (256, 1000, 1023), w1000, w1000_low, w510 (1020
     and 510); the first hops through process_window too, bit for bit
  c  every kernel of the table on one recording (1 kHz, W = 1000, sigma 50, offsets +-300); W = 2000 and 13 655 for the
     two kernels that do not take 1000 samples
  d  the persistent kernel's item loop: more items than the grid holds (`persistent_launches`, asserted in the test)
  e  values: amplitudes on both sides of the 1e-30 / 1e30 switches, degenerate windows, NaN / +inf / -inf in single
     windows of a batch, plain and in front of a re-reference (a channel group on the rail)
  f  artifacts of 1e2, 1e3, 1e4 sigma on the matrix-pipe kernel's pivot samples, on every W = 1000 kernel of class c"""

from __future__ import annotations

import re

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import parity
from tests.fir_sample_probe_cases import build_engine, car_matrix
from tests.spectral_probe_cases import generic_layout_fits, probe_settings

TD = ["raw_hjorth", "linelength", "return_raw"]
LOW4 = {"theta": (4, 8), "alpha": (8, 12), "low_beta": (13, 20), "high_beta": (20, 35)}
HIGH4 = {"theta": (4, 8), "alpha": (8, 12), "low_beta": (13, 20), "high_gamma": (90, 200)}
PACKED_W = (8, 12, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024)
SCALAR_W = (4, 5, 7, 9, 255, 257, 510, 1001, 1022, 1023)
COND_RTOL = 1e-6
RAIL64 = 1e200   # (tests/parity_cases.py: _rail_class -- the reference's side)
# host batches go out in chunks of NMX_HOST_FIRST_CHUNK (128), then NMX_HOST_CHUNK_WINDOWS (512) hops; class d wants the
# launches of a device-resident batch -- NMX_CHUNK_WINDOWS = 1024 hops -- and says so
CHUNK_ENV = {"NMX_HOST_FIRST_CHUNK": "1024", "NMX_HOST_CHUNK_WINDOWS": "1024"}
ONE_LAUNCH_ENV = {"NMX_HOST_FIRST_CHUNK": "4096", "NMX_HOST_CHUNK_WINDOWS": "4096", "NMX_CHUNK_WINDOWS": "4096"}


# ---- the plan's choice, restated (nmx_engine_plan_spectral.inc: timeosc_kind; test_timedomain_probes_cpu.py ties it to the text)
def _bins(bands: dict, n: int, sfreq: float):
    """[k_lo, k_hi) over every band of an n-point transform at sfreq (oscillatory.py: f >= lo and f < hi)."""
    f = np.arange(n // 2 + 1) * (np.floor(sfreq) / n)
    sel = [np.flatnonzero((f >= lo) & (f < hi)) for lo, hi in bands.values()]
    sel = [s for s in sel if s.size]
    return (int(min(s[0] for s in sel)), int(max(s[-1] for s in sel)) + 1) if sel else (0, 0)


def timeosc_kind(c: dict) -> str:
    """The kernel kind build_timeosc chooses for case c on the device, in timeosc_kind's order of precedence."""
    W, sfreq, feats, env = c["W"], c["sfreq"], c["features"], c["env"]
    on = lambda k, d=1: int(env.get(k, d)) != 0   # noqa: E731
    fft, welch, stft = "fft" in feats, "welch" in feats, "stft" in feats
    n_fft = int(np.floor(c["fft_ms"] / 1000 * sfreq)) if fft else 0
    n_welch = int(sfreq) if welch else 0
    n_stft = int(c["stft_ms"]) if stft else 0
    nb = len(c["bands"])
    if W > 16384 or (not stft and (fft or welch) and
                     not generic_layout_fits(W, max(n_fft, n_welch), max(_bins(c["bands"], n, sfreq)[1] - _bins(c["bands"], n, sfreq)[0]
                                                                         for n in (n_fft, n_welch) if n))):
        return "LONG"
    if not (fft or welch or stft) and 3 <= W <= 1024 and on("NMX_SCAN_KERNEL"):
        return "SCAN"
    w500 = (W == 1000 or (stft and not (fft or welch) and n_stft == 500 and W <= 2048)) and on("NMX_TIMEOSC_W1000")
    k_lo, k_hi = _bins(c["bands"], n_fft, sfreq) if fft else (0, 0)
    if (W == 1000 and fft and not welch and not stft and n_fft == 1000 and k_lo >= 1 and k_hi - k_lo <= 32 and k_hi <= 500
            and on("NMX_SPECMM") and w500 and 1 <= nb <= 8):
        return "SPECMM"
    if w500 and W == 1000 and nb <= 8 and (not fft or n_fft == 1000) and (not welch or n_welch == 1000) and \
            (not stft or n_stft == 500) and (fft or welch or stft):
        low = not stft and (not fft or k_hi <= 100) and (not welch or _bins(c["bands"], n_welch, sfreq)[1] + 1 <= 100)
        return "W1000_LOW" if low and on("NMX_TOW_PERSISTENT") else "W1000"
    if w500 and stft and not (fft or welch) and n_stft == 500:
        return "STFT500"
    if on("NMX_TIMEOSC_W510") and 510 <= W <= 1024 and nb <= 8 and not welch and ((fft and n_fft == 510) or (stft and n_stft == 510)) \
            and (not fft or n_fft == 510) and (not stft or n_stft == 510 or n_stft <= 64):
        return "W510"
    return "FIXED128" if W <= 1024 else "GENERIC"


SPEC_BITS = {"raw_hjorth": 1 << 0, "return_raw": 1 << 1, "stft": 1 << 3, "fft": 1 << 4, "welch": 1 << 5, "linelength": 1 << 8}
SPEC_NAMES = {65809: "C2", 196915: "DEFAULT", 196923: "ALL"}


def tow_spec(c: dict, feature_bits: dict = SPEC_BITS) -> int:
    """nmx_tow_spec: the enabled features, bit 16 / 17 the log transform of the FFT / Welch family (on in every case)."""
    v = sum(feature_bits[f] for f in c["features"])
    return v | (1 << 16 if "fft" in c["features"] else 0) | (1 << 17 if "welch" in c["features"] else 0)


def kernel_name(c: dict, feature_bits: dict = SPEC_BITS) -> str:
    """The name eng.kernels(2) reports for case c (the launchers of nmx_wave.hip, nmx_specmm.hip, nmx_timeosc*.hip)."""
    kind, nb = timeosc_kind(c), 4 if len(c["bands"]) <= 4 else 8
    spec = tow_spec(c, feature_bits)
    if kind == "W1000_LOW":
        return f"nmx_kern_timeosc_w1000_low<4, {spec}u>" if nb == 4 and spec in (65809, 196915) else f"nmx_kern_timeosc_w1000_low<{nb}>"
    if kind == "W1000":
        return f"nmx_kern_timeosc_w1000<4, {spec}u>" if nb == 4 and spec == 196923 else f"nmx_kern_timeosc_w1000<{nb}>"
    return {"LONG": "nmx_kern_timeosc_long", "SCAN": "nmx_kern_scan", "SPECMM": f"nmx_kern_specmm_w1000<{nb}>",
            "W510": f"nmx_kern_timeosc_w510<{nb}>", "FIXED128": "nmx_kern_timeosc_fixed128", "GENERIC": "nmx_kern_timeosc",
            "STFT500": f"nmx_kern_timeosc_stft500<{nb}>"}[kind]


def variant(c: dict) -> str:
    """The implementation of the module docstring's table a CLEAN window of case c runs."""
    kind, W = timeosc_kind(c), c["W"]
    packed = W % 4 == 0 and 8 <= W <= 1024
    if kind in ("SCAN", "W510"):
        return "td_emit<0>" if packed else "scan"
    if kind == "W1000":
        return "td_load<1000> SUM4 " + ("on" if tow_spec(c) == 196923 and len(c["bands"]) <= 4 else "off")
    if kind == "W1000_LOW":
        return "td_load_x + td_rest_from_x SUM4 " + ("on" if "u>" in kernel_name(c) else "off")
    return {"SPECMM": "specmm", "LONG": "long"}.get(kind, "two_pass")


VARIANTS = {"two_pass", "long", "td_emit<0>", "scan", "specmm", "td_load<1000> SUM4 on", "td_load<1000> SUM4 off",
            "td_load_x + td_rest_from_x SUM4 on", "td_load_x + td_rest_from_x SUM4 off"}
KERNELS = {"nmx_kern_scan", "nmx_kern_timeosc_fixed128", "nmx_kern_timeosc", "nmx_kern_timeosc_long", "nmx_kern_timeosc_w510<4>",
           "nmx_kern_timeosc_w1000<4>", "nmx_kern_timeosc_w1000<4, 196923u>", "nmx_kern_timeosc_w1000_low<4>",
           "nmx_kern_timeosc_w1000_low<4, 65809u>", "nmx_kern_timeosc_w1000_low<4, 196915u>", "nmx_kern_specmm_w1000<4>"}


def persistent_launches(n_cu: int, C: int, hops: int, env: dict) -> list:
    """[(items, grid, passes)] of the launches of nmx_kern_timeosc_w1000_low over a host batch of `hops` hops
    (batch_chunk_sizes; nmx_wave_launch_timeosc_w1000_low: 12 one-wave workgroups per CU, rounded down to a multiple of C)."""
    big = min(int(env.get("NMX_CHUNK_WINDOWS", 1024)), int(env.get("NMX_HOST_CHUNK_WINDOWS", 512)))
    first = min(big, int(env.get("NMX_HOST_FIRST_CHUNK", 128)))
    out, w0 = [], 0
    while w0 < hops:
        nw = min(first if w0 == 0 else big, hops - w0)
        grid = n_cu * 12
        if grid > C and grid % C:
            grid -= grid % C
        grid = min(grid, nw * C)
        out.append((nw * C, grid, -(-nw * C // grid)))
        w0 += nw
    return out


# ---- recordings -----------------------------------------------------------------------------------------------------------
def noise(seed: int, C: int, T: int, sigma: float = 50.0, offsets=None) -> np.ndarray:
    x = np.random.default_rng(seed).standard_normal((C, T)) * sigma
    if offsets is not None:
        x = x + np.resize(np.asarray(offsets, float), C)[:, None]
    return x


def _T(c):
    return c["W"] + (c["hops"] - 1) * c["hop"]


def data_noise(c, seed):
    x = noise(seed, c["C"], _T(c), c.get("sigma", 50.0), c.get("offsets"))
    return x if c.get("f64", True) else x.astype(np.float32)


AMPS = (1e-16, 1e-14, 1e-6, 1.0, 1e4, 1e14, 1e16)


def data_amps(c, seed):
    """One channel per amplitude: the variances lie on both sides of the 1e-30 / 1e30 switches, everything stays finite."""
    x = np.random.default_rng(seed).standard_normal((len(AMPS), _T(c))) * np.asarray(AMPS)[:, None]
    return x.astype(np.float32)


def degenerate_rows(W: int, a: float = 37.5) -> list:
    """Exactly representable windows: constant; ramp of step 0.5; alternating +-a; flat but for the last two / the first two
    samples (the telescoped means read exactly those); a step at a group boundary (sample 255 | 256, or the middle)."""
    n = np.arange(W, dtype=np.float64)
    k = 256 if W > 256 else W // 2
    tail, head = np.full(W, 12.0), np.full(W, 12.0)
    tail[-2:], head[:2] = (12.0 + a, 12.0 - 3 * a), (12.0 - a, 12.0 + 2 * a)
    return [np.full(W, 100.0), 0.5 * n - 64.0, np.where(n % 2 == 0, a, -a), tail, head, np.where(n < k, 0.0, a),
            np.zeros(W), -0.5 * n + 7.0]


def data_degenerate(c, seed):
    """hops x C non-overlapping windows (hop = W): item (h, ch) = row h C + ch."""
    rows = degenerate_rows(c["W"])
    assert len(rows) == c["hops"] * c["C"] and c["hop"] == c["W"]
    x = np.stack(rows).reshape(c["hops"], c["C"], c["W"])
    return np.ascontiguousarray(np.concatenate(list(x), axis=1), dtype=np.float32)


def bad_positions(W: int) -> list:
    """Sample 0, W - 1, both sides of the first group boundary, the first sample of the ragged group."""
    ragged = 256 * ((W - 1) // 256) if W % 256 else W - 256
    return sorted({0, W - 1, min(255, W - 2), min(256, W - 1), ragged})


def data_bad(c, seed):
    """Channel 0 NaN, 1 +inf, 2 -inf: one bad sample in every second window (hop = W: the windows do not overlap), so that
    the neighbours of a flagged window stay on the packed path."""
    W, pos = c["W"], bad_positions(c["W"])
    assert c["C"] == 3 and c["hops"] == 2 * len(pos) + 1 and c["hop"] == W
    x = noise(seed, 3, _T(c), 50.0, (300.0, -300.0, 150.0)).astype(np.float32)
    for i, p in enumerate(pos):
        for ch, v in enumerate((np.nan, np.inf, -np.inf)):
            x[ch, (2 * i + 1) * W + p] = v
    return x


def data_rail(c, seed):
    """Four zero-mean channels in front of a common-average re-reference; bad window j (every second window, hop = W) holds
    one NaN (j % 3 == 0, channel 0), +inf (1, channel 1) or -inf (2, channel 2) at bad_positions[j // 3]."""
    W, pos = c["W"], bad_positions(c["W"])
    assert c["C"] == 4 and c["hops"] == 6 * len(pos) + 1 and c["hop"] == W and c["reref"]
    x = noise(seed, 4, _T(c), 50.0).astype(np.float32)
    for j in range(3 * len(pos)):
        x[j % 3, (2 * j + 1) * W + pos[j // 3]] = (np.nan, np.inf, -np.inf)[j % 3]
    return x


def rereferenced(x: np.ndarray) -> np.ndarray:
    """processing/rereference.py on cleaned float64 rows, every row to the average of the others."""
    xc = np.nan_to_num(np.asarray(x).astype(np.float64))
    with np.errstate(all="ignore"):
        return np.stack([xc[i] - np.mean(np.delete(xc, i, axis=0), axis=0) for i in range(xc.shape[0])])


# (burst: 17 samples at either end and 34 across the centre -- an artifact under the pivot's samples AND many more, so that
# the cancellation ratio stays near the flag's threshold, 14 - 15 against 8, where the other sets reach 116 - 250)
ART_SETS = {"centre": (499, 500), "ends": (0, 999), "all4": (0, 499, 500, 999), "control": (300, 301),
            "burst": tuple(range(0, 17)) + tuple(range(483, 517)) + tuple(range(983, 1000))}


def data_artifacts(c, seed):
    """White noise sigma 50 + offsets; window h (hop = W) carries artifacts of art[h % 3] sigma at the samples of `where`,
    signs alternating from channel to channel."""
    x = noise(seed, c["C"], _T(c), 50.0, c.get("offsets"))
    for h in range(c["hops"]):
        for ch in range(c["C"]):
            for p in ART_SETS[c["where"]]:
                x[ch, h * c["W"] + p] += (-1) ** ch * 50.0 * (1e2, 1e3, 1e4)[h % 3]
    return x


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _case(cls, W, features, *, C=3, hops=5, hop=None, sfreq=1000.0, env=None, bands=LOW4, fft_ms=None, stft_ms=500, data=data_noise,
          seed=1, white=True, window_calls=0, reref=False, **kw):
    c = {"cls": cls, "W": W, "features": list(features), "C": C, "hops": hops, "hop": W // 4 + 1 if hop is None else hop,
         "sfreq": float(sfreq), "env": dict(env or {}), "bands": dict(bands), "fft_ms": 1000.0 if fft_ms is None else fft_ms,
         "stft_ms": stft_ms, "data": data, "seed": seed, "white": white, "window_calls": window_calls, "reref": reref}
    c.update(kw)
    return c


NO_SMM, SMM = {"NMX_SPECMM": "0"}, {"NMX_SPECMM": "1"}
# the feature sets of the W = 1000 kernels (classes c, f; b picks three of them)
W1000_KERNELS = {
    "scan": (TD, {}, LOW4),
    "fixed128": (TD, {"NMX_SCAN_KERNEL": "0"}, LOW4),
    "w1000": (TD + ["fft", "welch"], {}, HIGH4),
    "w1000_all": (TD + ["fft", "welch", "stft"], {}, LOW4),
    "low_c2": (["raw_hjorth", "linelength", "fft"], NO_SMM, LOW4),
    "low_default": (TD + ["fft", "welch"], {}, LOW4),
    "low": (TD + ["fft"], NO_SMM, LOW4),
    "specmm": (TD + ["fft"], SMM, LOW4),
}
OFF100 = (5000.0, -5000.0, 2500.0, -7500.0)   # 100 spreads and more: beyond 64, the host splits them off (engine.py: _host_offsets)
OFF300 = (300.0, -300.0, 150.0, -75.0)

CASES: dict = {}
for _W in PACKED_W + SCALAR_W + (1028,):
    CASES[f"a_W{_W}"] = _case("a", _W, TD, C=3, hops=6, offsets=OFF100, seed=100 + _W)
CASES.update({
    "b_scan256": _case("b", 256, TD, hop=33, hops=9, offsets=OFF300, seed=201, window_calls=4),
    "b_scan1000": _case("b", 1000, TD, hop=33, hops=9, offsets=OFF300, seed=202, window_calls=4),
    "b_scan1023": _case("b", 1023, TD, hop=33, hops=9, offsets=OFF300, seed=203, window_calls=4),
    "b_w1000": _case("b", 1000, *W1000_KERNELS["w1000"][:1], env=W1000_KERNELS["w1000"][1], bands=HIGH4, hop=33, hops=9,
                     offsets=OFF300, seed=204, window_calls=4),
    "b_low": _case("b", 1000, W1000_KERNELS["low_default"][0], hop=33, hops=9, offsets=OFF300, seed=205, window_calls=4),
    "b_w510_1020": _case("b", 1020, TD + ["fft", "stft"], fft_ms=510.0, stft_ms=510, hop=33, hops=9, offsets=OFF300, seed=206,
                         window_calls=4),
    "b_w510_510": _case("b", 510, TD + ["fft"], sfreq=30000.0, fft_ms=17.0, bands={"lo": (100, 1000), "hi": (1000, 5000)}, hop=33,
                        hops=9, offsets=OFF300, seed=207, window_calls=4),
})
for _k, (_f, _e, _b) in W1000_KERNELS.items():
    CASES[f"c_{_k}"] = _case("c", 1000, _f, C=4, hops=6, hop=100, env=_e, bands=_b, offsets=OFF300, seed=300)
CASES.update({
    "c_generic2000": _case("c", 2000, TD + ["fft"], C=4, hops=3, hop=100, offsets=OFF300, seed=300),
    "c_long13655": _case("c", 13655, TD + ["fft"], sfreq=13655.0, C=2, hops=2, hop=1365, offsets=OFF300, seed=301),
    "d_c7": _case("d", 1000, TD + ["fft"], C=7, hops=1100, hop=25, env={**NO_SMM, **CHUNK_ENV}, offsets=OFF300, seed=400, min_passes=3),
    "d_c1": _case("d", 1000, TD + ["fft"], C=1, hops=3100, hop=8, env={**NO_SMM, **ONE_LAUNCH_ENV}, offsets=OFF300, seed=401, min_passes=2),
})
for _k, _W, _f, _e in (("scan1000", 1000, TD, {}), ("scan260", 260, TD, {}), ("w1000", 1000, W1000_KERNELS["w1000"][0], {})):
    _b = HIGH4 if _k == "w1000" else LOW4
    CASES[f"e_amps_{_k}"] = _case("e", _W, _f, C=len(AMPS), hops=4, env=_e, bands=_b, data=data_amps, seed=500)
    CASES[f"e_degenerate_{_k}"] = _case("e", _W, _f, C=4, hops=2, hop=_W, env=_e, bands=_b, data=data_degenerate, white=False)
    CASES[f"e_bad_{_k}"] = _case("e", _W, _f, C=3, hops=2 * len(bad_positions(_W)) + 1, hop=_W, env=_e, bands=_b, data=data_bad, seed=510)
    CASES[f"e_rail_{_k}"] = _case("e", _W, _f, C=4, hops=6 * len(bad_positions(_W)) + 1, hop=_W, env=_e, bands=_b, data=data_rail, seed=520,
                                  reref=True)
for _k, (_f, _e, _b) in W1000_KERNELS.items():
    for _w in ART_SETS:
        CASES[f"f_{_k}_{_w}"] = _case("f", 1000, _f, C=2, hops=6, hop=1000, env=_e, bands=_b, data=data_artifacts, where=_w,
                                      offsets=OFF300, seed=600)


def case_settings(c: dict):
    return probe_settings(c["features"], c["bands"], c["W"] * 1000.0 / c["sfreq"], fft_ms=c["fft_ms"] if "fft" in c["features"] else None,
                          stft_ms=c["stft_ms"] if "stft" in c["features"] else None)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def reference(x32: np.ndarray, starts, W: int) -> dict:
    """hjorth_raw.py:24-42, 51-57 and linelength.py:11-21 in float64 over every window of x32 [C, T] (float32, widened
    exactly, then nan_to_num -- the reference cleans float64 data) -> {name: [n, C]}.  Windows are copied to contiguous
    rows: NumPy's pairwise sums over them are the ones oracle.Hjorth / LineLength take over a [C, W] array."""
    x32 = np.asarray(x32)
    xc = x32 if x32.dtype == np.float64 else np.nan_to_num(x32.astype(np.float32).astype(np.float64))   # (float64: cleaned by the caller)
    v = np.ascontiguousarray(sliding_window_view(xc, W, axis=1)[:, np.asarray(starts, np.int64), :])   # [C, n, W]
    with np.errstate(all="ignore"):
        d1 = np.diff(v, axis=-1)
        v0, v1, v2 = np.var(v, axis=-1), np.var(d1, axis=-1), np.var(np.diff(d1, axis=-1), axis=-1)
        act = np.nan_to_num(v0)
        mob = np.nan_to_num(np.sqrt(v1 / v0))
        comp = np.nan_to_num(np.sqrt(v2 / v1) / mob)
        ll = np.mean(np.abs(d1) / (W - 1), axis=-1)
        step = np.abs(d1).max(axis=-1)
    return {"RawHjorth_Activity": act.T, "RawHjorth_Mobility": mob.T, "RawHjorth_Complexity": comp.T, "LineLength": ll.T,
            "raw": v[:, :, -1].T, "_step": step.T}


def oracle_rows(x32: np.ndarray, starts, W: int, ch_names, features) -> list:
    """The same windows through oracle.Hjorth / Raw / LineLength: [{key: value}] per start."""
    from oracle import nm_oracle as orc

    xc = np.nan_to_num(np.asarray(x32, np.float32).astype(np.float64))
    objs = [orc._FEATURE_CLS[f](None, ch_names, 1000.0) for f in features if f in TD]
    out = []
    for a in starts:
        row: dict = {}
        with np.errstate(all="ignore"):
            for o in objs:
                row.update(o.calc_feature(np.ascontiguousarray(xc[:, a:a + W])))
        out.append(row)
    return out


def td_key(key: str):
    """(channel, name) of a time-domain key, None for any other."""
    for name in ("RawHjorth_Activity", "RawHjorth_Mobility", "RawHjorth_Complexity", "LineLength", "raw"):
        if key.endswith("_" + name):
            return key[:-len(name) - 1], name
    return None


def zero_mobility_bound(step: float, act: float) -> float:
    """Module docstring: one float32 rounding (two, as a bound) of the mean of exact first differences.  A constant window
    (step 0) and a window on the rail (inf / inf in both precisions) give exactly 0."""
    return 2.0 ** -22 * step / np.sqrt(act) if 0 < act < RAIL64 and step > 0 else 0.0


def perturbed(x32: np.ndarray, seed: int = 12345) -> np.ndarray:
    up = np.random.default_rng(seed).integers(0, 2, x32.shape).astype(bool)
    y = np.where(up, np.nextafter(x32, np.float32(np.inf)), np.nextafter(x32, np.float32(-np.inf))).astype(np.float32)
    return np.where(np.isfinite(x32), y, x32)


def conditioning(x32: np.ndarray, starts, W: int) -> float:
    """Largest relative move of a reference entry under +-1 ulp on every sample (entries of rail windows and exact zeros
    left out: they do not move)."""
    a, b = reference(x32, starts, W), reference(perturbed(x32), starts, W)
    worst = 0.0
    for k in a:
        if k.startswith("_"):
            continue
        ok = np.isfinite(a[k]) & (np.abs(a[k]) < RAIL64) & (a[k] != 0)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(b[k][ok] - a[k][ok]) / np.abs(a[k][ok]))))
    return worst


def starts_of(c: dict) -> np.ndarray:
    return np.arange(c["hops"], dtype=np.int64) * c["hop"]


def split(x: np.ndarray, dc) -> np.ndarray:
    """The float32 samples the engine is given: the input minus the host's constants, in float64, then the cast."""
    if x.dtype == np.float32:
        assert dc is None or not np.any(dc)
        return x
    return (x - (0.0 if dc is None else np.asarray(dc)[:, None])).astype(np.float32)


def host_offsets(x: np.ndarray):
    """engine.py: _host_offsets for finite float64 data of a plan that carries offsets -- the means of the first 256
    samples, when some row's level is beyond 64 spreads.  (run_case checks it against eng.offsets().)"""
    if x.dtype != np.float64:
        return None
    seg = x[:, :min(x.shape[1], 256)]
    m, sd = seg.mean(1), seg.std(1)
    return m if np.any(np.abs(m) > 64.0 * sd) else None


def draw(name: str, carries: bool = True):
    """The recording of a case: for white-noise cases the first seed (seed, seed + 1000, ...) whose float32 samples pass the
    conditioning check.  -> (x as handed to the engine, seed, conditioning)."""
    c = CASES[name]
    st = starts_of(c)
    if not c["white"]:
        return c["data"](c, c["seed"]), c["seed"], 0.0
    for seed in range(c["seed"], c["seed"] + 5000, 1000):
        x = c["data"](c, seed)
        k = conditioning(split(x, host_offsets(x) if carries else None), st, c["W"])
        if k < COND_RTOL:
            return x, seed, k
    raise AssertionError(f"{name}: no seed in five passes the conditioning check (last {k:.2e})")


class Report:
    def __init__(self):
        self.worst, self.n, self.zero_mob, self.rail, self.left_out = {}, 0, 0, 0, 0

    def line(self, name, extra=""):
        w = " ".join(f"{k} {v:.1e}" for k, v in sorted(self.worst.items()))
        print(f"TDPROBE {name:24s} items {self.n:5d}  worst relative error: {w} {extra}")


def compare_rows(name: str, c: dict, keys, got: np.ndarray, ref: dict, amp: np.ndarray, settings, rep: Report, leave_out=(), on_rail=None) -> None:
    """got [n, n_outputs] against ref: every time-domain entry of every (window, channel) but the items `leave_out`.
    on_rail [n, C]: the (window, channel) items that hold a sample on the rail -- a statement about the input: only their
    entries are read by class.  rep.worst: the largest plain relative error |got - want| / |want| per family over the
    ordinary non-zero entries."""
    from tests.parity_cases import _rail_class

    ch_names = [f"ch{i}" for i in range(c["C"])]
    cols = [(i, ch_names.index(t[0]), t[1]) for i, k in enumerate(keys) for t in [td_key(k)] if t is not None]
    want_names = {"raw_hjorth": 3, "linelength": 1, "return_raw": 1}
    assert len(cols) == c["C"] * sum(want_names[f] for f in c["features"] if f in want_names), (name, len(cols))
    bad = []
    for h in range(got.shape[0]):
        for ci in range(c["C"]):
            if (h, ci) in leave_out:
                rep.left_out += 1
                continue
            rep.n += 1
            for scale_free in (False, True):
                sel = [(i, nm) for i, cc, nm in cols if cc == ci and (nm in ("RawHjorth_Mobility", "RawHjorth_Complexity")) == scale_free]
                if not sel:
                    continue
                ks, g, w = [keys[i] for i, _ in sel], [got[h, i] for i, _ in sel], [ref[nm][h, ci] for _, nm in sel]
                skip = set()
                for (i, nm), gv, wv in zip(sel, g, w):
                    cw = _rail_class(float(wv), keys[i], settings, False) if on_rail is not None and on_rail[h, ci] else 0
                    if cw != 0 or (on_rail is not None and on_rail[h, ci] and _rail_class(float(gv), keys[i], settings, True) != 0):
                        skip.add(keys[i])
                        rep.rail += 1
                        if _rail_class(float(gv), keys[i], settings, True) != cw or cw == 2:
                            bad.append(f"hop {h} {keys[i]}: got {gv!r} in another class than the reference's {wv!r}")
                    elif nm == "RawHjorth_Mobility" and wv == 0.0:
                        skip.add(keys[i])
                        rep.zero_mob += 1
                        lim = zero_mobility_bound(float(ref["_step"][h, ci]), float(ref["RawHjorth_Activity"][h, ci]))
                        if not abs(float(gv)) <= lim:
                            bad.append(f"hop {h} {keys[i]}: got {gv!r}, reference 0, limit {lim:.3g}")
                n_bad, report, worst = parity.compare(ks, g, w, settings, c["sfreq"], 1.0 if scale_free else float(amp[ci]), c["W"],
                                                      skip=lambda k: k in skip, verifier=None)
                for k, gv, wv in zip(ks, g, w):
                    if k not in skip and wv != 0:
                        fam = parity.family_of(k)
                        rep.worst[fam] = max(rep.worst.get(fam, 0.0), abs(float(gv) - float(wv)) / abs(float(wv)))
                if n_bad:
                    bad.append(f"hop {h}:\n{report}")
    assert not bad, f"{name}: {len(bad)} (window, channel) groups beyond the policy\n" + "\n".join(bad[:10])


# ---- the matrix-pipe kernel's single pass, restated (nmx_k_specmm.h) -------------------------------------------------------
SMM_CANCEL = 8.0      # NMX_SMM_CANCEL: q0 / (q0 - s0^2 / W) beyond which a window goes to the two-pass redo
SMM_ROUNDINGS = 2.0   # the error model's roundings per unit of that ratio (rms; the derivation stands next to the define)
SMM_PIVOT = (0, 999, 499, 500)


def specmm_cancellation(x32: np.ndarray) -> np.ndarray:
    """q0 / (q0 - s0^2 / W) of every 1000-sample row of x32 in float32 as nmx_specmm_item_emu forms it: the pivot (mean of
    four samples), 64 partial sums per statistic, a tree.  (inf where nothing is left of the difference.)"""
    f32 = np.float32
    x = np.asarray(x32, f32)
    assert x.shape[1] == 1000
    a, b, c, d = (x[:, i] for i in SMM_PIVOT)
    p = (f32(0.25) * ((a + b) + (c + d))).astype(f32)
    u = np.zeros((x.shape[0], 1024), f32)
    u[:, :1000] = x - p[:, None]
    u = u.reshape(-1, 16, 64)
    s, q = np.zeros((x.shape[0], 64), f32), np.zeros((x.shape[0], 64), f32)
    for k in range(16):
        s, q = s + u[:, k], q + u[:, k] * u[:, k]
    h = 32
    while h >= 1:
        s[:, :h], q[:, :h] = s[:, :h] + s[:, h:2 * h], q[:, :h] + q[:, h:2 * h]
        h //= 2
    cw = q[:, 0] - s[:, 0] * s[:, 0] * (f32(1) / f32(1000))
    with np.errstate(all="ignore"):
        return np.where(cw > 0, q[:, 0] / cw, np.where(q[:, 0] > 0, np.inf, 1.0)).astype(np.float64)


def two_pass_f32(x32: np.ndarray, lanes: int):
    """Activity / mobility / complexity of one float32 window by the two-pass formulas of nmx_time_osc_item, sample i summed
    by accumulator i % lanes, the accumulators by a tree: lanes = 128 is the device kernel's order, lanes = 1 the
    single-thread emulator's."""
    f32 = np.float32

    def total(t):
        acc = np.zeros(lanes, f32)
        for a in range(0, t.size, lanes):
            blk = t[a:a + lanes]
            acc[:blk.size] = acc[:blk.size] + blk
        while acc.size > 1:
            acc = acc[:acc.size // 2] + acc[acc.size // 2:]
        return acc[0]

    x = np.asarray(x32, f32)
    d1 = x[1:] - x[:-1]
    d2 = d1[1:] - d1[:-1]
    out = []
    for t in (x, d1, d2):
        m = total(t) / f32(t.size)
        e = t - m
        out.append(total(e * e) / f32(t.size))
    with np.errstate(all="ignore"):
        mob = np.nan_to_num(np.sqrt(out[1] / out[0]))
        return float(np.nan_to_num(out[0])), float(mob), float(np.nan_to_num(np.sqrt(out[2] / out[1]) / mob))


# The emulator is one thread: it adds a window's 1000 terms one after the other.  On exactly representable windows whose
# terms repeat (a step: 744 times the same square; flat but for two samples: 997 times 0.0014 onto 18 000) every addition
# rounds the same way and the sum drifts by 1e-5 of itself -- the summation order of the stand-in, not of any kernel (128
# accumulators and a tree stay at 1e-7: test_timedomain_probes_cpu.py shows both on these rows).  The emulator tier leaves
# exactly those two items -- (hop, channel): flat but for the first two samples, the step -- out of these two cases and
# compares the other six rows; the MI355X tier compares all eight; W = 260 is short enough for either order.
EMU_CANNOT = {"e_degenerate_scan1000": ((1, 0), (1, 1)), "e_degenerate_w1000": ((1, 0), (1, 1))}


def emu_trace(lib, fn):
    """fn() between nmx_emu_trace_begin / _end (tests/emu/nmx_emu.cpp) -> (fn's result, the backend operations it issued)."""
    import ctypes

    lib.lib.nmx_emu_trace_begin()
    try:
        out = fn()
        n = lib.lib.nmx_emu_trace_end(None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.lib.nmx_emu_trace_end(buf, n)
    finally:
        lib.lib.nmx_emu_trace_end(None, 0)
    return out, [ln.split()[1] for ln in buf.raw.decode(errors="replace").splitlines() if ln.startswith("op ")]


def cu_count() -> int:
    """The device's compute units, read the way the plan reads them (hipDeviceAttributeMultiprocessorCount)."""
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run_case(lib, name: str) -> Report:
    """Case `name` on the device library (lib None) or the emulator: the kernel by name, every item against the reference."""
    c = CASES[name]
    ch_names = [f"ch{i}" for i in range(c["C"])]
    s = case_settings(c)
    kw = {"ref_matrix": car_matrix(c["C"])} if c["reref"] else {}
    eng = build_engine(lib, c["env"], s, ch_names, c["sfreq"], features=c["features"], window=c["W"], **kw)
    rep = Report()
    try:
        assert eng.W == c["W"]
        x, seed, cond = draw(name, eng.carries_offsets and not c["reref"])
        st = starts_of(c)
        assert st[-1] + c["W"] == x.shape[1]
        if lib is None:
            got = eng.process_batch(x, st).astype(np.float64)
            names = set(eng.kernels(2).split(" + "))
            assert names == {kernel_name(c)}, f"{name}: stage 2 ran {sorted(names)}, wanted {kernel_name(c)}"
        else:
            # the emulator names no kernels; its trace says whether the plan handed the items to the matrix-pipe kernel's
            # restatement: only that choice is followed by the launch of the redo pass (launch_timeosc_stage)
            got, ops = emu_trace(lib, lambda: eng.process_batch(x, st).astype(np.float64))
            assert "be_launch_timeosc" in ops, ops
            assert ("be_launch_timeosc_redo" in ops) == (timeosc_kind(c) == "SPECMM"), f"{name}: {sorted(set(ops))}"
        assert got.shape == (c["hops"], len(eng.keys))
        d_in, d_pre = eng.offsets()
        want_dc = host_offsets(x) if eng.carries_offsets and not c["reref"] else None
        np.testing.assert_array_equal(d_in, np.zeros(c["C"]) if want_dc is None else want_dc)
        np.testing.assert_array_equal(d_pre, d_in)
        if lib is None and c.get("min_passes"):   # the persistent kernel's item loop must iterate: say so when it cannot
            launches = persistent_launches(cu_count(), c["C"], c["hops"], c["env"])
            print(f"TDPROBE {name}: launches (items, grid, passes) {launches}")
            assert launches[0][2] >= c["min_passes"], f"{name}: {launches[0][0]} items on a grid of {launches[0][1]}: the loop does not iterate"
            rep.launches = launches
        x32 = split(x, want_dc)
        ref = reference(rereferenced(x32) if c["reref"] else x32, st, c["W"])
        ref["raw"] = ref["raw"] + d_in[None, :]
        fin = np.where(np.isfinite(x32), x32, 0.0).astype(np.float64) + d_in[:, None]
        amp = np.abs(rereferenced(fin) if c["reref"] else fin).max(axis=1)
        inf_at = ~np.isfinite(np.nan_to_num(x32, nan=0.0, posinf=np.inf, neginf=-np.inf))   # (a NaN is cleaned to 0: no rail)
        if c["reref"]:
            inf_at = np.broadcast_to(inf_at.any(axis=0), inf_at.shape)
        on_rail = sliding_window_view(inf_at, c["W"], axis=1)[:, st, :].any(axis=-1).T
        compare_rows(name, c, eng.keys, got, ref, amp, s, rep, EMU_CANNOT.get(name, ()) if lib is not None else (), on_rail)
        if c["reref"]:   # the case is about windows on the rail: they must be there, in every channel of the group
            assert rep.rail >= 2 * c["C"] * 2 * len(bad_positions(c["W"])), rep.rail
        if c["window_calls"]:   # the one-window call: the same kernel choice, the same bits
            eng2 = build_engine(lib, c["env"], s, ch_names, c["sfreq"], features=c["features"], window=c["W"], **kw)
            try:
                if want_dc is not None:
                    eng2.set_offsets(want_dc)
                for h in range(c["window_calls"]):
                    one = eng2.process_window(np.asarray(x[:, st[h]:st[h] + c["W"]], np.float64))
                    np.testing.assert_array_equal(one, eng.process_batch(x, st[h:h + 1])[0], err_msg=f"{name} hop {h}")
                    np.testing.assert_array_equal(one.astype(np.float64), got[h], err_msg=f"{name} hop {h}: one hop against the batch")
            finally:
                eng2.close()
    finally:
        eng.close()
    rep.line(name, f"{kernel_name(c)} seed {seed} conditioning {cond:.1e}")
    return rep


def source_ties(csrc) -> None:
    """timeosc_kind, nmx_tow_spec, the launchers' names and the chunk sizes as restated above, against the source text."""
    plan = (csrc / "nmx_engine_plan_spectral.inc").read_text()
    body = plan[plan.index("NmxTimeOscKind timeosc_kind("):plan.index("int build_timeosc(")]
    order = re.findall(r"return (?:[^;]*\? )?(NMX_TO_\w+)(?: : (NMX_TO_\w+))?;", body)
    assert [t for pair in order for t in pair if t] == ["NMX_TO_LONG", "NMX_TO_SCAN", "NMX_TO_SPECMM", "NMX_TO_W1000_LOW", "NMX_TO_W1000",
                                                        "NMX_TO_STFT500", "NMX_TO_W510", "NMX_TO_FIXED128", "NMX_TO_GENERIC"], order
    for line in ('if (A.long_mode) return NMX_TO_LONG;',
                 'if (!A.fft.enabled && !A.welch.enabled && !A.stft.enabled && A.W <= 1024 && A.W >= 3 && env_int("NMX_SCAN_KERNEL", 1)) return NMX_TO_SCAN;',
                 'if (A.smm_tab && nmx_specmm_ok(A)) return NMX_TO_SPECMM;',
                 'return nmx_timeosc_w1000_low_ok(A) && env_int("NMX_TOW_PERSISTENT", 1) ? NMX_TO_W1000_LOW : NMX_TO_W1000;',
                 'if (A.w510_tab && nmx_timeosc_w510_ok(A, A.w510_tab)) return NMX_TO_W510;',
                 'if (P.timeosc.nt == 128) return NMX_TO_FIXED128;', 'S.nt = d.window <= 1024 ? 128 : 256;',
                 'bool lng = d.window > 16384;',
                 'lng = ((long long)al4(d.window) + 2ll * al4(2 * gc) + al4(gs) + 64) * 4 > 160 * 1024;',
                 'if ((d.window == 1000 || stft500) && env_int("NMX_TIMEOSC_W1000", 1)) {',
                 'A.fft.k_hi - A.fft.k_lo <= 32 && A.fft.k_hi <= 500 && env_int("NMX_SPECMM", 1)) {'):
        assert line in plan, line
    w1000 = (csrc / "nmx_k_timeosc_w1000.h").read_text()
    for line in ('if (A.fft.enabled && A.fft.k_hi > 100) return false;', 'if (A.welch.enabled && A.welch.k_hi + 1 > 100) return false;',
                 'if (A.stft.enabled || !(A.fft.enabled || A.welch.enabled)) return false;',
                 '#define NMX_TOW_SPEC_LOG_FFT (1u << 16)', '#define NMX_TOW_SPEC_LOG_WELCH (1u << 17)',
                 'const bool fast = nmx_td_emit<1000, (!LOW || SPEC != 0), (SPEC & NMX_TOW_FEATS)>'):
        assert line in w1000, line
    common = (csrc / "nmx_common.h").read_text()
    bits = {f: int(re.search(rf"#define NMXD_F_{n}\s+\(?1u? ?<< ?(\d+)\)?", common).group(1))
            for f, n in (("raw_hjorth", "HJORTH"), ("return_raw", "RAW"), ("linelength", "LINELENGTH"), ("fft", "FFT"), ("welch", "WELCH"),
                         ("stft", "STFT"))}
    assert {f: 1 << b for f, b in bits.items()} == SPEC_BITS, bits
    wave = (csrc / "nmx_wave.hip").read_text()
    for line in ('int grid = n_cu * 12;', 'if (grid > C && grid % C) grid -= grid % C;', 'if (grid > n_items) grid = n_items;',
                 'static_assert(NMX_TOW_SPEC_C2 == 65809u && NMX_TOW_SPEC_DEFAULT == 196915u && NMX_TOW_SPEC_ALL == 196923u, "reported kernel names");',
                 'NMX_LAUNCH(nmx_kern_scan,', 'nmx_td_load<1000>(A, w, c, R);', 'nmx_td_rest_from_x<1000>(R);'):
        assert line in wave, line
    td = (csrc / "nmx_k_td.h").read_text()
    assert 'NMX_DEV bool nmx_td_ok(const NmxTimeOscArgs& A) { return (A.W & 3) == 0 && A.W >= 8 && A.W <= 1024; }' in td
    abi, run = (csrc / "nmx_engine_abi.inc").read_text(), (csrc / "nmx_engine_run.inc").read_text()
    for line in ('P->host_chunk_windows = std::max(1, env_int("NMX_HOST_CHUNK_WINDOWS", 512));',
                 'P->host_first_chunk = std::max(1, env_int("NMX_HOST_FIRST_CHUNK", 128));', 'P->chunk_windows = env_int("NMX_CHUNK_WINDOWS", 1024);'):
        assert line in abi, line
    for line in ('z.host_big = std::min<int64_t>(P.chunk_windows, P.host_chunk_windows);',
                 'z.host_first = std::min<int64_t>(z.host_big, P.host_first_chunk);'):
        assert line in run, line
