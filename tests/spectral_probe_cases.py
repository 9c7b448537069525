"""Per-bin probes of the spectral kernels (FFT / Welch / STFT), shared by the emulator tier (test_spectral_probes_cpu.py)
and the MI355X tier (test_spectral_probes_gpu.py).

Every other spectral test reads band MEANS over the default bands: a band of 200 log values divides a one-bin error by 200
(0.1 % in one bin is 2e-6 in the column, inside the 1e-5 policy), and the default bands end at bin 400.  A probe gives
every requested bin a band of its own -- [f_k - 0.4 df, f_k + 0.4 df], df the family's bin spacing, which under the
reference's rule (f >= lo and f < hi; <= hi for the STFT) holds exactly that bin -- on fixed-seed WHITE noise, so that
every bin carries signal (a random walk leaves the high bins ill-conditioned, and the policy would forgive exactly the
entries under test).  The reference of every comparison is oracle.run_stream, float64, computed in the test; the
tolerance is tests/parity.compare's 1e-5, a miss accepted only on the conditioning report of a PipelineVerifiers row, and
every accepted miss is returned to the caller, per family.

Long-window kernel (nmx_k_timeosc_long.h): LONG_LENGTHS holds one length per class of the plan's `long_split`, restated
here (long_split) together with the LDS / slab decision of build_timeosc (long_form).  spread_bins / cluster_bins place
the probes where the kernel's index arithmetic changes: k mod M wraps at M, the conjugate branch starts above M / 2, the
twiddle index (r k) mod N is exercised up to r = D - 1 at k = N / 2 - 1.

Generic LDS transform (nmx_k_timeosc.h, nmx_device.h: nmx_fft_auto over the stages of build_fft): SPECTRUM_LENGTHS are
compared bin by bin through return_spectrum.  build_fft takes the factors 4, 2, 5, 3 first, then every odd prime as a
direct DFT stage, largest radix first; an even length is transformed as n / 2 packed complex points, an odd one as n:

    window   transform   stages (radix)              what it exercises
    853      853         853                         one prime direct DFT (the resampler's length)
    901      901         53 17                       two prime stages, complex_full
    1000     500         5 5 5 4                     the default length on the generic item
    1024     512         4 4 4 4 2                   radix 4 with one radix 2
    1331     1331        11 11 11                    a repeated odd prime, complex_full
    3998     1999        1999                        the largest prime stage in the list, behind the real-transform split
    4096     2048        4 4 4 4 4 2                 six stages
    8008     4004        13 11 7 4                   three different primes and a radix 4
    11680    5840        73 5 4 4 4                  the largest layout that fits with every bin kept (see below)

13 000 samples is the largest generic layout with the DEFAULT bands; with return_spectrum the spectrum (n / 2 + 1 floats)
joins the window and the two buffers in LDS and the layout ends at 11 684 samples: beyond it the plan goes to the
long-window kernel, which refuses return_spectrum.  13 000 (transform 6500 = 13 5 5 5 4) is therefore probed through
single-bin bands (SPREAD_13000: two plans, each within the 1896 bins the layout has room for), every bin through
return_spectrum up to 11 680."""

from __future__ import annotations

import math

import numpy as np

from tests import parity
from tests.sharpwave_long_recording import recording

MAX_STAGES = 12        # nmx_common.h: NMX_MAX_STAGES
MAX_BANDS = 16         # nmx_common.h: NMX_MAX_BANDS_DEV
LDS_BYTES = 160 * 1024


# ---- the plan's arithmetic, restated ------------------------------------------------------------------------------
def long_split(n: int) -> int:
    """nmx_engine_plan_spectral.inc: long_split -- the smallest D <= 64 that divides n and leaves M = n / D samples whose
    transform (M / 2 complex points, M when M is odd) has at most 8192 points, prime factors <= 4096 and at most
    MAX_STAGES stages (one per odd prime factor, radix 4 for pairs of twos).  0: none."""
    for D in range(1, 65):
        if n % D:
            continue
        M = n // D
        if M < 2:
            break
        nc = M if M & 1 else M // 2
        if nc > 8192:
            continue
        twos = stages = 0
        while nc % 2 == 0:
            nc //= 2
            twos += 1
        ok, p = True, 3
        while nc > 1 and ok:
            if nc % p == 0:
                nc //= p
                stages += 1
                ok = p <= 4096
            elif p * p > nc:
                p = nc
            else:
                p += 2
        if ok and stages + (twos + 1) // 2 <= MAX_STAGES:
            return D
    return 0


def _al4(x: int) -> int:
    return (x + 3) & ~3


def long_form(W: int, n: int, spans) -> str:
    """build_timeosc's layout of a long-window plan whose families all transform n samples and evaluate the bins
    `spans` = [(k_lo, k_hi), ...]: "lds" when the accumulators and the spectrum (3 floats per bin) fit behind the two
    transform buffers of one subsequence, "slab" when they go to the workgroup's slab of device memory."""
    M = n // long_split(n)
    nc = M if M & 1 else M // 2
    nb = max(_al4(hi - lo) for lo, hi in spans)
    end = 2 * _al4(2 * nc) + 3 * nb
    return "slab" if (max(end, _al4(W)) + 64) * 4 > LDS_BYTES else "lds"


def generic_layout_fits(W: int, n: int, bins: int, segments: int = 1) -> bool:
    """build_timeosc: window + two transform buffers + spectrum + 64 floats within 160 KiB (the plan is long otherwise)."""
    nc = n if n & 1 else n // 2
    return (_al4(W) + 2 * _al4(2 * nc) + _al4(bins * segments) + 64) * 4 <= LDS_BYTES


# N: (D, M, "spread" layout's form, class)
LONG_LENGTHS = {
    13655: (5, 2731, "lds", "smallest long length; prime M (one direct-DFT stage); W <= 16 384 route"),
    13847: (61, 227, "lds", "largest D"),
    16384: (1, 16384, "slab", "largest unsplit; 8192-point buffers"),
    16388: (2, 8194, "slab", "first split length"),
    20001: (3, 6667, "slab", "odd M = 59 x 113"),
    24579: (9, 2731, "slab", "composite D"),
    32768: (2, 16384, "slab", "8192 complex points per subsequence, seven stages"),
    36015: (5, 7203, "slab", "odd M = 3 x 7^4, five stages"),
    39974: (11, 3634, "slab", "even M, D > 4"),
    39995: (5, 7999, "slab", "odd M = 19 x 421 at the upper limit"),
    40000: (4, 10000, "slab", "a fixture length, now at high bins"),
}
WIDE_LENGTHS = (20001, 36015, 39974)
SWEEP = range(13655, 40001, 97)


def spread_bins(N: int) -> list[int]:
    """At most 15 bins below N / 2 where the subsequence arithmetic changes: the ends of the grid, around M / 2 (the
    conjugate branch), around M and 2 M (k mod M wraps), 3 M / 2, around (D / 2) M, the last bins below Nyquist."""
    D = long_split(N)
    M = N // D
    half = [M // 2 - 1, M // 2, M // 2 + 1] if M % 2 == 0 else [(M - 1) // 2, (M + 1) // 2]
    three = [3 * M // 2] if M % 2 == 0 else [(3 * M - 1) // 2, (3 * M + 1) // 2]
    cand = [1, 2] + half + [M - 1, M, M + 1] + three + [2 * M - 1, 2 * M, 2 * M + 1,
                                                        (D // 2) * M - 1, (D // 2) * M + 1, N // 2 - 2, N // 2 - 1]
    bins = sorted({k for k in cand if 1 <= k < N / 2})
    for drop in (2, 2 * M + 1, 2 * M - 1):   # (16 - 17 candidates survive for an odd M with D >= 5)
        if len(bins) > 15 and drop in bins:
            bins.remove(drop)
    assert 0 < len(bins) <= 15, (N, bins)
    return bins


def cluster_bins(N: int) -> dict:
    """Three plans whose bins lie within +-3 of M / 2, of M and of N / 2 - 4: k_lo is large, the accumulators stay in
    LDS and every access carries a non-zero k - k_lo."""
    M = N // long_split(N)
    out = {}
    for name, c in (("half", M // 2), ("wrap", M), ("top", N // 2 - 4)):
        b = sorted({k for k in range(c - 3, c + 4) if 1 <= k < N / 2})
        if b:   # (an unsplit length has no bin at M)
            out[name] = b
    return out


CLUSTERS = [(n, w) for n in LONG_LENGTHS for w in cluster_bins(n)]

SPECTRUM_LENGTHS = (853, 901, 1000, 1024, 1331, 2 * 1999, 4096, 7 * 11 * 13 * 8, 11680)
# (next to a 13 000-sample window and its two buffers the generic layout has room for a span of 1896 bins)
SPREAD_13000 = {"low": [1, 2, 99, 100, 948, 1624, 1625, 1626, 1895, 1896],
                "top": [4604, 4605, 4875, 5000, 5001, 6497, 6498, 6499]}


# ---- settings, input ------------------------------------------------------------------------------------------------
def band_of(k: int, df: float) -> list:
    return [(k - 0.4) * df, (k + 0.4) * df]


def probe_settings(features, bands: dict, window_ms: float, *, estimators=("mean",), feat_hz: float = 10,
                   fft_ms: float | None = None, stft_ms: float | None = None, return_spectrum: bool = False):
    from py_neuromodulation_amd import NMSettings

    base = NMSettings.get_default().to_dict()
    base["frequency_ranges_hz"] = {name: [float(lo), float(hi)] for name, (lo, hi) in bands.items()}
    s = NMSettings(**base)
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    for f in features:
        setattr(s.features, f, True)
    s.segment_length_features_ms = window_ms
    s.sampling_rate_features_hz = feat_hz
    for o in (s.fft_settings, s.welch_settings, s.stft_settings):
        o.features.disable_all()
        for e in estimators:
            setattr(o.features, e, True)
    if fft_ms is not None:
        s.fft_settings.windowlength_ms = fft_ms
    if stft_ms is not None:
        s.stft_settings.windowlength_ms = stft_ms
    s.fft_settings.return_spectrum = bool(return_spectrum)
    return s


def white(seed: int, channels: int, T: int) -> np.ndarray:
    """(channels, T) unit white noise, exactly representable in float32: sharpwave_long_recording's "white" rows, two per
    seed (seed, seed + 1, ...)."""
    rows = [recording(seed + i, T, "white", hops=1) for i in range((channels + 1) // 2)]
    return np.concatenate(rows)[:channels]


def samples_for(hops: int, sfreq: float, feat_hz: float, window_ms: float) -> int:
    """The shortest recording whose window schedule (stream/generator.py: float stride, int() truncation) has `hops`
    windows."""
    return int(sfreq / feat_hz * (hops - 1) + window_ms / 1000 * sfreq)


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def ran_kernel(names: str, kernel) -> bool:
    """`names`: HotPathEngine.kernels(stage), "a + b<4> + ..."; `kernel`: a name without template arguments, or several
    (any of them)."""
    want = (kernel,) if isinstance(kernel, str) else tuple(kernel)
    return any(t == k or t.startswith(k + "<") for t in names.split(" + ") for k in want)


def run_and_compare(lib, tag, sfreq, s, x, *, kernel=None, env=None):
    """Stream.run against oracle.run_stream, every row under parity.compare with a PipelineVerifiers row.
    -> (accepted misses per family, worst relative error per family, the oracle's per-family bin selection)."""
    import os

    from oracle import nm_oracle as orc
    from py_neuromodulation_amd import channels as chmod
    from py_neuromodulation_amd.stream import Stream

    ch = chmod.get_default_channels_from_data(x)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:   # (the plan reads its switches when it is built)
        st = Stream(float(sfreq), channels=ch, settings=s, line_noise=50, **_kw(lib))
        df = st.run(x, save_csv=False)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if kernel is not None and lib is None:   # (the emulator names no kernels: it runs the generic or the long item)
        names = st.data_processor.engine.kernels(2)
        assert ran_kernel(names, kernel), f"{tag}: wanted {kernel}, ran {names}"
    rows = orc.run_stream(x, float(sfreq), s, ch, line_noise=50)
    starts, ends, _ = orc.window_schedule(x.shape[1], float(sfreq), s.sampling_rate_features_hz, s.segment_length_features_ms)
    cols = list(df.columns)
    assert len(rows) == len(starts) == len(df) and all(list(r) == cols for r in rows), tag
    got = df.to_numpy(float)
    want = np.array([[r[c] for c in cols] for r in rows])
    assert cols[-1] == "time"
    np.testing.assert_array_equal(got[:, -1], want[:, -1])
    W = int(ends[0] - starts[0])
    pv = parity.PipelineVerifiers(s, ch, float(sfreq), x, starts, W, line_noise=50, ends=ends)
    amp = float(np.nanmax(np.abs(x)))
    before = dict(parity.STATS["forgiven"])
    worst: dict = {}
    for i in range(len(starts)):
        n_bad, rep, w = parity.compare(cols[:-1], got[i, :-1], want[i, :-1], s, float(sfreq), amp, W, verifier=pv.row(i))
        for fam, v in w.items():
            worst[fam] = max(worst.get(fam, 0.0), v)
        assert n_bad == 0, f"{tag} hop {i}\n{rep}"
    after = parity.STATS["forgiven"]
    acc = {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}
    print(f"PROBE {tag}: {len(starts)} hops, accepted {acc}, worst relative error "
          + ", ".join(f"{f} {v:.1e}" for f, v in sorted(worst.items())))
    return acc, worst


def oracle_bins(s, sfreq, family) -> dict:
    """{band: bin indices} as the oracle's feature class of `family` selects them."""
    from oracle import nm_oracle as orc

    cls = {"fft": orc.FFT, "welch": orc.Welch, "stft": orc.STFT}[family]
    return {b: [int(k) for k in idx] for b, idx in cls(s, ["c"], float(sfreq)).idx_range}


def family_df(family, sfreq, s) -> float:
    if family == "fft":
        return math.floor(sfreq) / math.floor(s.fft_settings.windowlength_ms / 1000 * sfreq)
    if family == "welch":
        return 1.0
    return sfreq / int(s.stft_settings.windowlength_ms)


def probe(lib, sfreq, window_ms, features, bins, *, kernel=None, seed, channels=2, hops=3, estimators=("mean",),
          grid="fft", wide=None, feat_hz=10, fft_ms=None, stft_ms=None, env=None, tag=None):
    """One single-bin band per entry of `bins` (bins of the family `grid`; every enabled family with the same spacing
    must select exactly that bin, checked against the oracle's own selection), `wide` = further (name, lo_bin, hi_bin)
    bands; `channels` x `hops` of white noise through Stream.run, against oracle.run_stream.
    -> (accepted misses per family, worst relative error per family)."""
    spectral = [f for f in features if f in ("fft", "welch", "stft")]
    assert grid in spectral, (grid, features)
    s0 = probe_settings(features, {"x": (1, 2)}, window_ms, fft_ms=fft_ms, stft_ms=stft_ms)
    df = family_df(grid, sfreq, s0)
    bands = {f"b{k}": band_of(k, df) for k in bins}
    for name, lo, hi in wide or ():
        bands[name] = [(lo - 0.4) * df, (hi + 0.4) * df]
    assert len(bands) <= MAX_BANDS
    s = probe_settings(features, bands, window_ms, estimators=estimators, feat_hz=feat_hz, fft_ms=fft_ms, stft_ms=stft_ms)
    for fam in spectral:
        sel = oracle_bins(s, sfreq, fam)
        same = abs(family_df(fam, sfreq, s) - df) < 1e-9 * df
        for k in bins:
            assert len(sel[f"b{k}"]) == 1, f"{fam}: band of bin {k} holds bins {sel[f'b{k}']}"
            if same:
                assert sel[f"b{k}"] == [k], (fam, k, sel[f"b{k}"])
        for name, lo, hi in wide or ():
            if same:
                assert sel[name] == list(range(lo, hi + 1)), (fam, name)
    x = white(seed, channels, samples_for(hops, sfreq, feat_hz, window_ms))
    tag = tag or f"{sfreq:g} Hz {window_ms:g} ms {'+'.join(features)} bins {bins[0]}..{bins[-1]}"
    return run_and_compare(lib, tag, sfreq, s, x, kernel=kernel, env=env)


# ---- long-window kernel ---------------------------------------------------------------------------------------------
LONG = "nmx_kern_timeosc_long"


def check_class(N: int) -> None:
    D, M, form, _ = LONG_LENGTHS[N]
    assert long_split(N) == D and N // D == M and D * M == N, (N, long_split(N))
    assert not generic_layout_fits(N, N, 1), N       # (even a one-bin plan of this length is a long-window plan)
    b = spread_bins(N)
    assert long_form(N, N, [(b[0], b[-1] + 1)]) == form, N
    for name, c in cluster_bins(N).items():
        assert long_form(N, N, [(c[0], c[-1] + 1)]) == "lds", (N, name)


def long_spread(lib, N, seed=None):
    """fft + welch on 1000 ms windows at sfreq = N: the spread layout (slab form where LONG_LENGTHS says so)."""
    check_class(N)
    return probe(lib, float(N), 1000, ["fft", "welch"], spread_bins(N), kernel=LONG, seed=N if seed is None else seed,
                 estimators=("mean", "max"), tag=f"long {N} spread")


def long_cluster(lib, N, which, seed=None):
    check_class(N)
    return probe(lib, float(N), 1000, ["fft", "welch"], cluster_bins(N)[which], kernel=LONG,
                 seed=N + 1 if seed is None else seed, estimators=("mean", "max"), tag=f"long {N} cluster {which}")


def long_wide(lib, N, seed=None):
    """A near-full-range band [3, N / 2 - 2] beside one single bin (M + 1): the slab form with every bin evaluated."""
    M = N // long_split(N)
    assert long_form(N, N, [(3, N // 2 - 1)]) == "slab", N
    return probe(lib, float(N), 1000, ["fft", "welch"], [M + 1], wide=[("wide", 3, N // 2 - 2)], kernel=LONG,
                 seed=N + 2 if seed is None else seed, estimators=("mean", "max"), tag=f"long {N} wide")


def long_two_seconds(lib, seed=27310):
    """sfreq 13 655, 2000 ms: W = 27 310, Welch averages 3 segments of 13 655 samples (odd M = 2731), the FFT reads the
    window's last 13 655 samples."""
    N = 13655
    return probe(lib, float(N), 2000, ["fft", "welch"], spread_bins(N), kernel=LONG, seed=seed,
                 estimators=("mean", "max"), tag="long 13655 x 2 s")


def sweep_construction(lib):
    """A plan for every 97th length: construction succeeds exactly where long_split finds a split, and the refusal names
    the length otherwise.  Construction only."""
    import pytest

    from py_neuromodulation_amd.engine import HotPathEngine

    s = probe_settings(["fft", "welch"], {"b": (4, 30)}, 1000)
    built = refused = 0
    for N in SWEEP:
        if long_split(N):
            HotPathEngine(s, ["a", "b"], float(N), window=N, **_kw(lib)).close()
            built += 1
        else:
            with pytest.raises(ValueError, match=f"{N:,}".replace(",", " ")):
                HotPathEngine(s, ["a", "b"], float(N), window=N, **_kw(lib))
            refused += 1
    assert built and refused, (built, refused)
    return built, refused


# ---- generic LDS transform: every bin ---------------------------------------------------------------------------------
def full_spectrum(lib, N, seed=None, kernel=None):
    """return_spectrum of the FFT over one N-sample window at sfreq = N (1 Hz per bin: the psd keys are the bins), every
    bin against the oracle."""
    assert generic_layout_fits(N, N, N // 2 + 1), N
    s = probe_settings(["fft"], {"low": (1, N / 4)}, 1000, return_spectrum=True)
    x = white(N if seed is None else seed, 2, samples_for(1, float(N), 10, 1000))
    assert x.shape[1] == N
    return run_and_compare(lib, f"spectrum {N}", float(N), s, x, kernel=kernel)


def generic_13000(lib, which, kernel=None):
    bins = SPREAD_13000[which]
    assert generic_layout_fits(13000, 13000, bins[-1] + 1 - bins[0]) and not generic_layout_fits(13000, 13000, 1897)
    return probe(lib, 13000.0, 1000, ["fft", "welch"], bins, seed=13000, estimators=("mean", "max"), kernel=kernel,
                 tag=f"generic 13000 {which}")


# ---- wave-level kernels of the default shapes (device only) -----------------------------------------------------------
TIME_DOMAIN = ["raw_hjorth", "return_raw", "linelength"]
GENERIC = ("nmx_kern_timeosc_fixed128", "nmx_kern_timeosc")
LOW_BINS = [1, 2, 49, 50, 63, 64, 65, 98]                 # Welch evaluates k_hi + 1 <= 100 bins: 98 is the last
W1000_BINS = [99, 100, 101, 249, 250, 251, 498, 499]      # the first bins the low-band form refuses, N / 4, below Nyquist
STFT_BINS = [1, 2, 124, 125, 126, 248, 249]               # of the 500-point segments: 2 Hz per bin at 1 kHz
W510_BINS = ([1, 2, 29, 30, 31, 50, 51], [127, 128, 169, 170, 253, 254])
SPECMM_SPANS = (1, 234, 468)                              # 32 consecutive bins from here; 468 + 32 = N / 2


def device_probe(features, bins, *, kernel, seed, sfreq=1000.0, window_ms=1000, **kw):
    """4 channels x 17 hops: partly filled waves, workgroups and 16-window tiles."""
    return probe(None, sfreq, window_ms, features, bins, kernel=kernel, seed=seed, channels=4, hops=17, **kw)


def w1000_low():
    return device_probe(["fft", "welch"] + TIME_DOMAIN, LOW_BINS, kernel="nmx_kern_timeosc_w1000_low", seed=101, tag="w1000_low")


def w1000(extra_bins=(), estimators=("mean",), kernel="nmx_kern_timeosc_w1000", tag="w1000"):
    return device_probe(["fft", "welch"] + TIME_DOMAIN, W1000_BINS + list(extra_bins), kernel=kernel, seed=102,
                        estimators=estimators, tag=tag)


def w1000_with_stft():
    return device_probe(["fft", "welch", "stft"] + TIME_DOMAIN, STFT_BINS, grid="stft", kernel="nmx_kern_timeosc_w1000",
                        seed=103, tag="w1000 + stft")


def stft500(window_ms):
    """STFT alone on windows of OTHER lengths than 1000 (at 1000 samples the one-wave kernel of the default shape takes
    the plan first: timeosc_kind): 600 samples -- a zero-padded last segment -- and 1500 -- none."""
    return device_probe(["stft"], STFT_BINS, grid="stft", window_ms=window_ms, kernel="nmx_kern_timeosc_stft500",
                        seed=104, tag=f"stft500 W {window_ms}")


def w510_fft_30k(part):
    """30 kHz, 17 ms: 510-sample windows, the FFT over all of them (the STFT of this shape has 17-sample segments, whose
    9 bins no band of an FFT bin holds)."""
    return device_probe(["fft"] + TIME_DOMAIN, W510_BINS[part], sfreq=30000.0, window_ms=17, fft_ms=17, feat_hz=1000,
                        kernel="nmx_kern_timeosc_w510", seed=105 + part, tag=f"w510 30 kHz part {part}")


def w510_fft_stft(part):
    """1 kHz, 1020-sample windows, FFT over the last 510 samples and STFT with five 510-sample segments: both
    prime-factor paths of the kernel, two real sequences per transform."""
    return device_probe(["fft", "stft"] + TIME_DOMAIN, W510_BINS[part], window_ms=1020, fft_ms=510, stft_ms=510,
                        kernel="nmx_kern_timeosc_w510", seed=107 + part, tag=f"w510 fft + stft part {part}")


def specmm(start):
    bins = [start + i for i in (0, 1, 2, 15, 16, 17, 30, 31)]
    return device_probe(["fft"] + TIME_DOMAIN, bins, kernel="nmx_kern_specmm_w1000", seed=109 + start,
                        env={"NMX_SPECMM": "1"}, tag=f"specmm from bin {start}")
