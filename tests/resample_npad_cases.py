"""Per-sample probes of the resampler's FIXED padding mode (``resample_npad`` = n samples per side; nmx_k_resample.h with
GEN = 1, build_resample), shared by the emulator tier (test_resample_npad_cpu.py) and the MI355X tier
(test_resample_npad_gpu.py).  The style, the inputs and the limit are those of the resampler part of
tests/front_probe_cases.py, whose `_pad_rows`, `resample64`, `check_resampled`, `FACTOR` and `YARD_CAP` this module imports.

Reference: `resample64` on the plan dict of `npad_plan` (build_resample's arithmetic for the fixed pad, restated), which the
CPU tier ties to tests/resample_npad_oracle.py at 1e-12.  Yardstick (`chain` in float32): the kernel's chain at the plan's
transform lengths with scipy.fft on float32 -- the padded row packed as n_pad / 2 complex points (n_pad points when n_pad is
odd), or q polyphase components of m points, two per transform (the last alone when q is odd), summed with a table of n_pad
roots; the kept bins, the Nyquist scale, the transform back, the scale, the crop.  Limit, as there:

    max_n |y - y64| <= FACTOR max(e32[row], eps32 rms(x_row)),   FACTOR = 4,

the yardstick itself within YARD_CAP eps32 of the row's scale; rows without input exactly 0.

OWN FACTORS (`OWN_FACTORS`, impulse rows only; every other class of every case holds FACTOR).  On an impulse row the
yardstick's error e32 is ONE store rounding: the output peak adds n_new / 2 roots of unity in phase, the yardstick reads each
from a correctly rounded table, so at the peak it is 0 or half an ulp of the peak (eps32 / 2, relative) by the luck of the
last rounding -- not a statistic of an fp32 chain (front_probe_cases.FACTORS, profiles/front_probes.md).
  * 8, front_probe_cases' own figure and reason: nmx_fft's radix-3/4/5 stages form w^2 .. w^4 from the table's w by
    multiplication, an eps32 per root and stage, 2 - 4 ulp of the peak against the yardstick's half.
  * a prime radix R is a DIRECT fp32 sum: every output adds (R - 1) / 2 pairs one after the other.  At the peak the terms are
    in phase, partial sum i is i terms long and its rounding at most eps32 / 2 of it: independent roundings leave
    (eps32 / 2) sqrt(sum i^2) / n = (eps32 / 2) sqrt(n / 3) of the peak, n = (R - 1) / 2, at one sigma.  Two sigma against the
    yardstick's half ulp:  factor(R) = 2 sqrt((R - 1) / 6).  R = 1049 (prime_new: n_new itself is prime): 26.4.
The factors follow from R and the number formats, not from what the kernel gives; the figures are in
profiles/resample_npad.md.

C = 3, one engine per case, a few windows each.
"""

from __future__ import annotations

import numpy as np

from tests import fir_sample_probe_cases as fir
from tests import front_probe_cases as fc
from tests.front_probe_cases import FACTOR, YARD_CAP, _pad_rows, check_resampled, resample64  # noqa: F401

EPS32 = fc.EPS32
SIGMA = fc.SIGMA
KERNEL = "nmx_kern_resample_npad"     # the fixed pad's kernel (nmx_api.hip); "auto" keeps nmx_kern_resample
LDS_BYTES = 160 * 1024
C = 3


def prime_radix_factor(R: int) -> float:
    """Impulse rows through a direct R-term fp32 sum (module docstring): 2 sqrt((R - 1) / 6) yardsticks."""
    return 2.0 * float(np.sqrt((R - 1) / 6.0))


# (case, class) -> the factor in force where it is not FACTOR.  check_resampled looks its factors up in
# front_probe_cases.FACTORS by (case, class): this module's cases go there as "npad/<case>", so that no entry of either
# table is taken for the other's (both have a poly_44k).
OWN_FACTORS = {
    ("prime_new", "impulse"): prime_radix_factor(1049),   # n_new = 1049: the whole inverse transform is one direct sum
    ("poly_16k", "impulse"): 8.0,                         # m = 2025 = 3^4 5^2: six radix-3/5 stages forward
    ("poly_44k", "impulse"): 8.0,                         # as front_probe_cases' poly_44k
}
fc.FACTORS.update({(f"npad/{n}", c): f for (n, c), f in OWN_FACTORS.items()})


def _al4(n: int) -> int:
    return (n + 3) & ~3


def _max_prime(n: int) -> int:
    big, p = 1, 2
    while p * p <= n:
        while n % p == 0:
            big, n = max(big, p), n // p
        p += 1
    return max(big, n)


def npad_plan(sf_old: float, sf_new: float, Wr: int, npad: int = 100, forced: bool = False) -> dict:
    """build_resample's arithmetic for the fixed pad, restated (Python's round is round-half-even, as nearbyint).
    ValueError where the library refuses to build the plan."""
    ratio = float(sf_new) / float(sf_old)
    if Wr + 2 * npad > 65536:
        raise ValueError(f"raw window {Wr} + 2 x npad {npad} exceeds 65 536")
    W_new = int(round(ratio * Wr))
    n_pad = Wr + 2 * npad
    n_new = max(int(round(ratio * n_pad)), 1)
    crop_l = int(round(ratio * npad))
    assert crop_l + W_new <= n_new
    inv_full = n_new & 1
    use_len = min(n_new, n_pad)
    n_inv = n_new if inv_full else n_new // 2

    def fits(n_fwd, keep_x):
        cmax = max(n_fwd, n_inv)
        return ((_al4(Wr) if keep_x else 0) + 2 * _al4(2 * cmax) + _al4(2 * (n_new // 2 + 1))) * 4 <= LDS_BYTES

    if _max_prime(n_new) > 4096:
        raise ValueError(f"n_new {n_new} has a prime factor > 4096")
    fwd_full = n_pad & 1
    n_fwd = n_pad if fwd_full else n_pad // 2
    q = m = 0
    if not (1 <= n_fwd <= 32768 and fits(n_fwd, 1) and _max_prime(n_fwd) <= 4096 and not forced):
        fwd_full = 0
        q = next((t for t in range(2, min(256, n_pad - 1) + 1) if n_pad % t == 0 and n_pad // t <= 2048 and fits(n_pad // t, 0)), 0)
        if not q:
            raise ValueError(f"no polyphase split of n_pad {n_pad} (raw window {Wr}, n_new {n_new})")
        m = n_pad // q
    return dict(ratio=ratio, W=Wr, W_new=W_new, n_pad=n_pad, pad_l=npad, pad_r=npad, n_new=n_new, crop_l=crop_l,
                crop_r=n_new - W_new - crop_l, inv_full=inv_full, fwd_full=fwd_full,
                nyq_bin=use_len // 2 if use_len % 2 == 0 else -1, nyq_scale=2.0 if n_new < n_pad else 0.5,
                scale=np.float32(ratio / n_new), poly_q=q, poly_m=m, npad=npad)


def chain(x: np.ndarray, p: dict, rdt) -> np.ndarray:
    """The kernel's chain in the real type `rdt` (module docstring).  rdt = float32: the yardstick; float64: resample64's value."""
    import scipy.fft as sf

    cdt = np.complex64 if rdt == np.float32 else np.complex128
    x = np.atleast_2d(np.asarray(x, rdt))
    xe = _pad_rows(x, p)
    N, n_new, q, m = p["n_pad"], p["n_new"], p["poly_q"], p["poly_m"]
    nh, kmax = N // 2, n_new // 2
    kuse = min(kmax, nh)
    half, j1 = rdt(0.5), cdt(1j)
    Xn = np.zeros((len(x), kmax + 1), cdt)
    k = np.arange(kuse + 1)
    if q == 0 and p["fwd_full"]:
        Xn[:, :kuse + 1] = sf.fft(xe.astype(cdt), axis=-1)[:, :kuse + 1]
    elif q == 0:
        Z = sf.fft((xe[:, 0::2] + j1 * xe[:, 1::2]).astype(cdt), axis=-1)
        Zk, Zc = Z[:, k % nh], np.conj(Z[:, (nh - k) % nh])
        Xn[:, :kuse + 1] = half * (Zk + Zc) - j1 * fc._roots(N, kuse + 1, -1.0, cdt)[None, :] * (half * (Zk - Zc))
    else:
        tab = fc._roots(N, N, -1.0, cdt)
        for r in range(0, q, 2):
            if r + 1 < q:
                Z = sf.fft((xe[:, r::q] + j1 * xe[:, r + 1::q]).astype(cdt), axis=-1)
                Zk, Zc = Z[:, k % m], np.conj(Z[:, (m - k % m) % m])
                f0, f1 = half * (Zk + Zc), -j1 * (half * (Zk - Zc))
                Xn[:, :kuse + 1] += tab[(k * r) % N][None, :] * f0 + tab[(k * (r + 1)) % N][None, :] * f1
            else:   # q odd: the last component alone
                Z = sf.fft(xe[:, r::q].astype(cdt), axis=-1)
                Xn[:, :kuse + 1] += tab[(k * r) % N][None, :] * Z[:, k % m]
            assert Z.shape[1] == m
    assert Xn.dtype == cdt
    if p["nyq_bin"] >= 0:
        Xn[:, p["nyq_bin"]] *= rdt(p["nyq_scale"])
    Xn[:, 0] = Xn[:, 0].real   # (C2R: the imaginary part of the DC bin does not contribute)
    if not p["inv_full"]:
        mh = kmax
        Xn[:, mh] = Xn[:, mh].real
        kk = np.arange(mh)
        Xk, Xc = Xn[:, kk], np.conj(Xn[:, mh - kk])
        z = (Xk + Xc) + j1 * fc._roots(n_new, mh, +1.0, cdt)[None, :] * (Xk - Xc)
        zt = sf.ifft(z.astype(cdt), axis=-1, norm="forward")
        y = np.empty((len(x), n_new), rdt)
        y[:, 0::2], y[:, 1::2] = zt.real, zt.imag
    else:
        full = np.concatenate([Xn, np.conj(Xn[:, :0:-1])], axis=1)
        assert full.shape[1] == n_new
        y = sf.ifft(full.astype(cdt), axis=-1, norm="forward").real
    assert y.dtype == rdt
    y = y * (p["scale"] if rdt == np.float32 else rdt(p["ratio"] / n_new))
    assert y.dtype == rdt
    return y[:, p["crop_l"]:p["crop_l"] + p["W_new"]]


def chain32(x: np.ndarray, p: dict) -> np.ndarray:
    return chain(x, p, np.float32)


POLY = {"NMX_RESAMPLE_POLY": "1"}
# name -> (sf_old, sf_new, W, npad, env, what the case pins: {field of npad_plan: value})
CASES = {
    "down_2200": (2000.0, 1000.0, 2000, 100, {}, dict(n_pad=2200, n_new=1100, crop_l=50, inv_full=0, fwd_full=0, nyq_bin=550, nyq_scale=2.0, poly_q=0)),
    "up_450": (250.0, 1000.0, 250, 100, {}, dict(n_pad=450, n_new=1800, crop_l=400, W_new=1000, nyq_bin=225, nyq_scale=0.5, poly_q=0)),
    "odd_pad": (999.0, 1000.0, 999, 100, {}, dict(n_pad=1199, n_new=1200, fwd_full=1, inv_full=0, nyq_bin=-1, W_new=1000, crop_l=100, poly_q=0)),
    "odd_both": (1375.0, 1000.0, 1375, 100, {}, dict(n_pad=1575, n_new=1145, fwd_full=1, inv_full=1, nyq_bin=-1, crop_l=73, poly_q=0)),
    "prime_new": (4096.0, 1000.0, 4096, 100, {}, dict(n_pad=4296, n_new=1049, inv_full=1, fwd_full=0, nyq_bin=-1, poly_q=0)),
    "tiny_4": (1000.0, 2000.0, 4, 100, {}, dict(n_pad=204, n_new=408, W_new=8, crop_l=200, nyq_bin=102, nyq_scale=0.5, poly_q=0)),
    "npad0_64": (2000.0, 1000.0, 64, 0, {}, dict(n_pad=64, pad_l=0, pad_r=0, n_new=32, W_new=32, crop_l=0, crop_r=0, poly_q=0)),
    "tie_crop": (8000.0, 1000.0, 8000, 100, {}, dict(n_pad=8200, n_new=1025, crop_l=12, inv_full=1, fwd_full=0, nyq_bin=-1, poly_q=0)),
    "one_12k": (12000.0, 1000.0, 12000, 100, {}, dict(n_pad=12200, n_new=1017, inv_full=1, fwd_full=0, poly_q=0)),
    "poly_forced_240": (2000.0, 1000.0, 40, 100, POLY, dict(n_pad=240, n_new=120, crop_l=50, W_new=20, poly_q=2, poly_m=120)),
    "poly_16k": (16000.0, 1000.0, 16000, 100, {}, dict(n_pad=16200, n_new=1012, poly_q=8, poly_m=2025, inv_full=0)),
    "poly_30k": (30000.0, 1000.0, 30000, 100, {}, dict(n_pad=30200, n_new=1007, poly_q=20, poly_m=1510, inv_full=1, crop_l=3)),
    "poly_44k": (44100.0, 1000.0, 44100, 100, {}, dict(n_pad=44300, n_new=1005, poly_q=25, poly_m=1772, inv_full=1)),
    "poly_max": (65336.0, 1000.0, 65336, 100, {}, dict(n_pad=65536, n_new=1003, poly_q=32, poly_m=2048, inv_full=1)),
}
# raw windows that must build at 1 kHz with npad = 100
REQUIRED_WINDOWS = [2000, 2048, 4000, 4096, 5000, 8000, 10000, 12000, 16000, 20000, 22050, 24000, 24414, 25000, 30000, 32000,
                    40000, 44100, 48000, 48828]


def case_plan(name: str) -> dict:
    sf_old, sf_new, Wr, npad, env, cls = CASES[name]
    p = npad_plan(sf_old, sf_new, Wr, npad, forced=bool(env))
    for k, v in cls.items():
        assert p[k] == v, f"{name}: restated {k} = {p[k]}, the case table says {v}"
    return p


def positions(p: dict, every: bool = False) -> list[int]:
    """The structural positions: both ends, around the reach of the pads' reflections, the middle; in the long form the first
    and last samples of the first, the second and the last polyphase component (the unpaired one when q is odd) and the
    window samples whose reflections land there.  A few windows per case."""
    Wr, pl, pr, q, m, N = p["W"], p["pad_l"], p["pad_r"], p["poly_q"], p["poly_m"], p["n_pad"]
    if every:
        return list(range(Wr))
    s = {0, 1, 2, pl - 1, pl, pl + 1, Wr - 2 - pr, Wr - 1 - pr, Wr - pr, Wr - 2, Wr - 1, Wr // 2, Wr // 2 + 1}
    if q:
        padded = {q * j + r for j in (0, 1, m - 2, m - 1) for r in (0, 1, q - 2, q - 1)}
        for i in padded:
            j = i - pl
            if j < 0:
                j = -j
            elif j >= Wr:
                j = 2 * (Wr - 1) - j
            s.add(j)
    return sorted(t for t in s if 0 <= t < Wr)


# Impulse positions a case leaves out, with the reason.  poly_max, the window's last sample: under a pad of 100 at W = 65 336
# the odd reflection of a unit impulse there is a step of 2 that ends just outside the crop (crop_r = 1 output sample); the
# output is that step's ringing, 0.09 at most, while the transforms carry the step.  The single-precision CHAIN ITSELF --
# this module's and front_probe_cases.resample32 on the "auto" plan of the same lengths alike -- then stands 18.9 eps32 of
# the row's scale from float64: beyond YARD_CAP, so the yardstick cannot referee that row (found on the yardstick against
# float64, no kernel involved).  The last sample is probed at every other length, poly_44k (8.5 eps32 at most) included, and
# poly_max's noise rows end on a live sample.
LEFT_OUT = {"poly_max": {65335}}


def inputs(name: str, p: dict) -> list[tuple[str, np.ndarray]]:
    """[(class, float32 [C, W])]: impulses, noise with an offset row and a NaN, the Nyquist tone where there is one."""
    Wr = p["W"]
    out = []
    pos = [t for t in positions(p, every=name == "poly_forced_240") if t not in LEFT_OUT.get(name, ())]
    for i in range(0, len(pos), C):
        x = np.zeros((C, Wr), np.float32)
        for c in range(C):
            x[c, pos[(i + c) % len(pos)]] = 1.0
        out.append(("impulse", x))
    x = np.random.default_rng(Wr + p["n_new"]).standard_normal((C, Wr)) * SIGMA
    x[1] += 300.0
    x = x.astype(np.float32)
    x[2, Wr // 3] = np.nan
    out.append(("noise", x))
    if p["nyq_bin"] >= 0:
        ph = 2.0 * np.pi * p["nyq_bin"] * (np.arange(Wr) + p["pad_l"]) / p["n_pad"]
        x = np.zeros((C, Wr))
        x[0], x[1] = SIGMA * np.cos(ph), SIGMA * np.sin(ph)
        if not np.abs(x[1]).max() > 1e-6:
            x[1] = 0.0
        x[2] = x[0] + x[1]
        out.append(("tone", x.astype(np.float32)))
    return out


def engine(lib, env, sf_old, sf_new, Wr, n_ch, npad, notch=None, **kw):
    from py_neuromodulation_amd import NMSettings

    return fir.build_engine(lib, env, NMSettings.get_default(), [f"c{i}" for i in range(n_ch)], sf_new, features=["return_raw"],
                            resample_from=sf_old, raw_window=Wr, window=int(round(sf_new / sf_old * Wr)), notch_taps=notch,
                            resample_npad=npad, **kw)


def run_case(lib, name: str) -> dict:
    """The inputs of case `name` through preprocess_window.  -> {class: worst ratio}."""
    sf_old, sf_new, Wr, npad, env, _ = CASES[name]
    p = case_plan(name)
    eng = engine(lib, env, sf_old, sf_new, Wr, C, npad)
    worst: dict = {}
    try:
        assert (eng.W_in, eng.W, eng.resample_npad) == (Wr, p["W_new"], npad), f"{name}: the plan's windows {eng.W_in} -> {eng.W}"
        assert (eng.desc.resample_npad_mode, eng.desc.resample_npad) == (1, npad)
        for cls, x in inputs(name, p):
            got = eng.preprocess_window(x.astype(np.float64))
            fir.assert_kernels(lib, name, eng, {1: KERNEL})
            xc = np.nan_to_num(x)
            r = check_resampled(f"npad/{name}", cls, got, resample64(xc, p), chain32(xc, p), xc, p)
            worst[cls] = max(worst.get(cls, 0.0), r)
    finally:
        eng.close()
        fc.REPORT.flush(f"npad/{name}")
    return worst


def both_modes_case(lib) -> dict:
    """poly_max's lengths are those of "auto" (65 336 + 200 = 2^16): the noise window through a plan of either mode, both
    against the same float64 series under the same limit."""
    sf_old, sf_new, Wr, npad, env, _ = CASES["poly_max"]
    p = case_plan("poly_max")
    pa = fc.resample_plan(sf_old, sf_new, Wr)
    for k in ("n_pad", "pad_l", "pad_r", "n_new", "crop_l", "W_new", "inv_full", "nyq_bin", "poly_q", "poly_m"):
        assert p[k] == pa[k], (k, p[k], pa[k])
    x = dict(inputs("poly_max", p))["noise"]
    xc = np.nan_to_num(x)
    y64, y32 = resample64(xc, p), chain32(xc, p)
    out = {}
    for mode, kernel in (("auto", fc.RESAMPLE), (npad, KERNEL)):
        eng = engine(lib, env, sf_old, sf_new, Wr, C, mode)
        try:
            got = eng.preprocess_window(x.astype(np.float64))
            fir.assert_kernels(lib, "poly_max", eng, {1: kernel})
            out[mode] = check_resampled("npad/poly_max", f"noise/{mode}", got, y64, y32, xc, p)
        finally:
            eng.close()
    fc.REPORT.flush("npad/poly_max")
    return out


def batch_case(lib, with_notch: bool, npad: int = 100) -> float:
    """front_probe_cases.batch_resample_case with the fixed pad: 2000 -> 1000, 5 channels, 9 ragged hops through the tap, the
    resampler alone or behind the notch at the raw rate; the batch equals its windows one by one, byte for byte."""
    from py_neuromodulation_amd import fir_design

    name = "npad_batch_notch" if with_notch else "npad_batch"
    BW, BC, hops = fc.BATCH_W, fc.BATCH_C, fc.BATCH_HOPS
    p = npad_plan(2000.0, 1000.0, BW, npad)
    notch = fir_design.notch_bank(2000.0, 50) if with_notch else None
    starts = np.arange(hops, dtype=np.int64) * fc.BATCH_HOP + fc.BATCH_RAGGED
    T = int(starts[-1]) + BW + 7
    x = np.random.default_rng(12).standard_normal((BC, T)) * SIGMA
    x[1] += 300.0
    x[3] *= 1e-3
    x = x.astype(np.float32)
    x[2, int(starts[4]) + 5] = np.nan
    eng = engine(lib, {}, 2000.0, 1000.0, BW, BC, npad, notch)
    try:
        _, mask, pre = eng.process_batch(x, starts, want_nan_mask=True, tap=True)
        names = eng.kernels(1) if lib is None else ""
        assert lib is not None or fir.ran(names, KERNEL), names
        assert pre.shape == (hops, BC, p["W_new"])
        assert np.array_equal(mask, fc.windows_of(np.isnan(x), starts, BW).any(axis=2))
    finally:
        eng.close()
    n = hops * BC
    rows = fc.windows_of(np.nan_to_num(x), starts, BW).reshape(n, BW)
    a64, a32 = rows.astype(np.float64), rows
    if with_notch:
        a64 = fir.conv64(a64, notch, odd=True)
        a32 = fir.conv32(rows, notch, 4000, odd=True)
    r = check_resampled(name, "noise", np.asarray(pre, np.float64).reshape(n, -1), resample64(a64, p), chain32(a32, p), a64, p)
    eng = engine(lib, {}, 2000.0, 1000.0, BW, BC, npad, notch)   # a fresh plan
    try:
        for h, a in enumerate(starts):
            one = eng.preprocess_window(x[:, a:a + BW].astype(np.float64))
            fir.same_bytes(np.asarray(pre[h], np.float64), one, f"{name}: hop {h} of the batch against preprocess_window")
    finally:
        eng.close()
        fc.REPORT.flush(name)
    return r


# ---- the stand-alone float64 Resampler ---------------------------------------------------------------------------------------
# (fs, to, samples): the case lengths, and the reference's own test shape (tests/test_nm_resample.py: 10 s at 4 kHz -> 1 kHz)
F64_SHAPES = [(sf_old, sf_new, Wr, npad) for sf_old, sf_new, Wr, npad, _, _ in CASES.values()] + [(4000.0, 1000.0, 40000, 100)]


def standalone_case(lib, fs: float, to: float, T: int, npad: int) -> float:
    """processing.Resampler(fs, to, npad=...) and nmx_resample_f64_npad against the float64 restatement, under the limit of the
    existing float64 resampler test (parity_cases.case_standalone_resampler_float64): atol = 1e-12 max|want|.  -> the error
    in units of that limit."""
    from py_neuromodulation_amd.processing import Resampler
    from tests import resample_npad_oracle as oracle
    from tests.parity_cases import _default_library

    rng = np.random.default_rng(92 + T)
    x = rng.standard_normal((3, T)) * 10 + rng.uniform(-1e3, 1e3, (3, 1))
    want = oracle.resample(x, up=to / fs, down=1.0, npad=npad)
    with _default_library(lib):
        got = Resampler(fs, to, npad=npad).process(x)
        assert got.shape == want.shape and got.dtype == np.float64
        tol = 1e-12 * np.abs(want).max()
        err = float(np.abs(got - want).max())
        assert err <= tol, f"Resampler({fs:g}, {to:g}, npad={npad}) on {T} samples: error {err:.3e}, limit {tol:.3e}"
        from py_neuromodulation_amd._lib import get_library

        L = get_library()
        y = np.empty_like(want)
        L.check(L.lib.nmx_resample_f64_npad(0, x.ctypes.data, T, 3, T, to / fs, y.ctypes.data, max(y.shape[1], 1), y.shape[1], npad))
        assert np.array_equal(y, got), "nmx_resample_f64_npad and Resampler.process differ"
    return err / max(tol, 1e-300)


# ---- the reference's own tables -------------------------------------------------------------------------------------------
STREAM_TAGS = ("down_2k", "up_250", "odd_1375")


def stream_case(lib, tag: str) -> None:
    """tests/golden/resample_npad.npz (make_golden_resample_npad.py: the reference's own Stream.run with mne.filter.resample
    restated at its own default, npad=100) against ``Stream(..., resample_npad=100).run``: the column list equal, every row
    through parity.compare WITH NO VERIFIER (the conditioning verifier restates the "auto" pipeline and cannot speak for this
    mode), n_bad == 0 with no entry skipped.  The same recording with NMX_RESAMPLE_NPAD=100 and no keyword gives the identical
    frame; on two plans (``devices=[0, 0]``) the frame meets the same table under the same policy."""
    import os

    from py_neuromodulation_amd.stream import Stream
    from tests import parity
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("resample_npad")
    sf, data = float(g[f"{tag}_sfreq"]), g[f"{tag}_data"]
    s = settings_from_json(g[f"{tag}_settings_json"])
    cols = [str(c) for c in g[f"{tag}_columns"]]
    want = g[f"{tag}_values"]
    W_new = int(round(1000.0 / sf * int(sf)))

    def meets(df, what):
        assert list(df.columns) == cols, what
        got = df.to_numpy(dtype=np.float64)
        assert got.shape == want.shape, what
        np.testing.assert_array_equal(got[:, -1], want[:, -1])
        for r in range(len(got)):
            n_bad, rep, _ = parity.compare(cols[:-1], got[r, :-1], want[r, :-1], s, sf, float(np.abs(data).max()), W_new)
            assert n_bad == 0, f"{tag} {what} row {r}\n{rep}"
        return got

    old = os.environ.pop("NMX_RESAMPLE_NPAD", None)
    try:
        st = Stream(sfreq=sf, data=data, settings=s, line_noise=50, lib=lib, resample_npad=100)
        assert st.data_processor.sfreq_raw == sf and st.data_processor.engine.resample_npad == 100
        one = meets(st.run(save_csv=False), "keyword")
        meets(Stream(sfreq=sf, data=data, settings=s, line_noise=50, lib=lib, resample_npad=100, devices=[0, 0]).run(save_csv=False),
              "two plans")
        auto = Stream(sfreq=sf, data=data, settings=s, line_noise=50, lib=lib).run(save_csv=False).to_numpy(dtype=np.float64)
        assert not np.array_equal(auto, one), f"{tag}: the two padding modes gave the same frame"
        os.environ["NMX_RESAMPLE_NPAD"] = "100"
        env = Stream(sfreq=sf, data=data, settings=s, line_noise=50, lib=lib).run(save_csv=False)
        assert list(env.columns) == cols
        assert env.to_numpy(dtype=np.float64).tobytes() == one.tobytes(), f"{tag}: NMX_RESAMPLE_NPAD=100 and the keyword differ"
    finally:
        os.environ.pop("NMX_RESAMPLE_NPAD", None)
        if old is not None:
            os.environ["NMX_RESAMPLE_NPAD"] = old
