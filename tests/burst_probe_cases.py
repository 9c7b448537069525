"""Probes of the bursts chain (Hilbert envelope -> threshold walk -> run statistics), shared by the emulator tier
(test_burst_probes_cpu.py) and the MI355X tier (test_burst_probes_gpu.py).

tests/parity.py holds burst amplitudes to 1e-5 relative (about 80 eps32) and forgives every entry of a (channel, band) whose
float64 envelope comes near its threshold anywhere in the window; the golden tables compare bytes with bytes of this code's
parent; the C++ tests run host restatements.  A probe compares what the chain stores with a float64 restatement under limits
derived from the number formats, with nothing forgiven.

Outlets (calls that exist; nothing is exported for the probes)
  rows        six outputs per (hop, channel, band) of process_batch
  state blob  export_state(): its first section is top[C][Bb][K] (descending float32) | counts[C][Bb][2] (int64: samples
              appended, windows seen) -- burst_state_export.  The list holds the kernel's OWN envelope samples bit for bit:
              every appended sample (window 0 whole, the last `overlap` samples of each later hop) while K >= samples
              appended, the top K of them otherwise.  The k-th largest of a multiset is 1-Lipschitz in the sup norm, so a
              rank-by-rank comparison with the float64 list carries the per-sample limit.  Entries behind the filled length
              are the +0.f bytes burst_state_reset left (no walk writes there).  The blob is exported after EVERY batch.
  kernels(4)  the kernel names of the last batch's first chunk

Reference: float64 direct convolution (fir_sample_probe_cases.conv64_direct) of the float32 input with the plan's taps,
oracle.nm_oracle.analytic_envelope, Bursts.update_threshold, burst_stats.  `stats_of` restates burst_stats per run (it needs
the runs for the limits) and is tied to it at 1e-13 in the CPU tier, as the convolution is tied to fir_bank_apply at 1e-12.

Yardstick: the same chain on the same float32 input in single precision -- conv32 at the kind's transform length M, the
hand-off rounded to float32, the analytic signal by complex64 FFT / IFFT at length W, the modulus in float32;
e32[row] = max_n |env32 - env64|, which must itself stay within YARD_CAP eps32 of the row's scale max(rms(y), max env).

Limits
  envelope      L_env(row) = F max(e32[row], eps32 rms(y_row)), F = FACTOR = 4 (FACTORS: a case's own factor, at most 8)
  list          |top[r] - top64[r]| <= max L_env over the rows that fed the (channel, band), every rank below the filled
                length; counts equal; descending; the rest exactly zero
  in_burst            equal
  duration_max        2 eps32 |v|    (float)mlen / sfreq: one rounding, + 1
  duration_mean       3 eps32 |v|    (fa / (float)num_bursts) / sfreq: two roundings, + 1
  burst_rate_per_s    5 eps32 |v|    dmean / seg_s: three roundings, seg_s itself rounded to float32, + 1
  amplitude_max       L_env
  amplitude_mean      per run L_env + (len - 1) eps32 mean|v| + 2 eps32 |mean| (any summation order, v_rcp_f32, one multiply);
                      over nv runs the largest of them + (nv - 1) eps32 mean + 2 eps32 |result|
  (nmx_burst_stat_item_reg lines 95 - 101 and nmx_burst_stat_item lines 1248 - 1254 hold the same expressions.)
The outputs are compared with the REFERENCE's decisions (env64 >= thr64).  No verifier, no accepted miss.

Inputs
  (a) constructed (`constructed_stream`): a two-level pattern (Lo 100, Hi 300) periodic in W, each hop block holding exactly
      pb = (1 - q) hop high samples in runs of 2 samples and up, low-passed circularly below 0.24 W bins (raised cosine over
      0.1 W bins), times a carrier at bin W // 4: every window of the stream is a rotation of one analytic signal, its
      envelope the smoothed pattern, and every threshold of the fill regime lies in the Lo - Hi gap.  Identity taps: band 0
      [1.0], band 1 [0.5] -- band 1's amplitudes must be half of band 0's (exact: a power of two) and everything else equal,
      which checks the (window, channel, band) item arithmetic without the oracle.  Channels: a pattern each, scales 1, 1e3,
      1e-3.  Pattern 0 has a run that wraps the period (a run from sample 0, a run ending at W - 1, and a run of 2 pb samples
      -- four lanes and more -- when the seam is inside a window); pattern 1 a run ending at hop - 2 and one starting at 1;
      the W = 20 000 patterns put run ends on both sides of sample 2048.  The rotation by `hop` moves every run through
      further residues; test_burst_probes_cpu.py asserts the classes reached (lane boundaries of 16 / 32, the last partly
      filled lane, two runs in one lane, the 2048 seams, odd transition counts, a row without a run).
      Condition (asserted on every row in the CPU tier): decisions equal the pattern, margin min|env - thr| >= MARGIN max env.
      Sensitivity (CPU tier): moving any one run boundary of the decision vector by one sample changes duration_mean,
      duration_max or amplitude_mean by at least SENS_RATIO limits.
  (b) full ring, then quieter (`quieter_stream`): the pattern fills a 2 s / 5 s ring exactly, then the stream is scaled to 0.6
      over a 20-sample raised-cosine ramp inside a Lo stretch: the threshold steps once into the gap between the new Hi and the
      old one; windows straddling the ramp have bursts in their older part only, later rows are all zero.  Sparse envelope
      storage on (the `_sparse` kernels asserted by name) and off; the rows of both equal the reference.
  (c) noise: fixed-seed white noise sigma 50 + 17 / 27 Hz lines, default taps.  Every list check applies to every row.  The
      outputs of a row are compared unless min|env64 - thr64| < 2 L_env(row); at most NOISE_LEFT_OUT = 5 % may be left out,
      the share is printed and asserted.

    case          rate   W      C x hops (batches)   stage 4: Hilbert, walk of each batch, statistics         regime
    envelope + list + run edges, fresh state, K >= samples appended (constructed, 30 s ring, q = 1 - pb / hop)
    w1000         1000   1000   3 x 12 (12)          w500_sparse, fill_sort + fill_walk, stat_reg_sparse<16>      q = 0.75
    w1000_hops    1000   1000   3 x 12 (12 x 1)      w500_sparse, thr<32> in every call, stat_reg_sparse<16>      one-hop calls
    w1000_fixed   1000   1000   3 x 12 (12)          fixed128, fill_sort + fill_walk, stat_reg<16>                NMX_HILBERT_W500=0
    w1000_dense   1000   1000   3 x 12 (12)          w500, fill_sort + fill_walk, stat_reg<16>                    NMX_BURST_ENV_SPARSE=0
    w1000_q50     1000   1000   3 x 12 (12)          as w1000                                                     q = 0.5: runs up to 100
    w1000_q10     1000   1000   3 x 12 (12)          as w1000                                                     q = 0.1: runs up to 180, 11 lanes
    w2000 / w2000_dense  2000  2000  3 x 6 (6)       w1000_sparse / w1000, fill, stat_reg_sparse<32> / stat_reg<32>
    w800          800    800    3 x 8  (8)           fixed128, fill, stat_reg<16>                                 even W: half-length path
    w901          1000   901    2 x 6  (6)           fixed128, fill, burst_stat                                   odd W, hop 53: full complex path
    w2500         2500   2500   2 x 6  (6)           fixed128, fill, burst_stat                                   LDS statistics above 2048
    w14000        14000  14000  2 x 2  (2)           hilbert_long, fill, burst_stat                               K = 105 001 >= 15 400 appended
    w20000        20000  20000  2 x 2  (2)           hilbert_long, fill, stat_scan                                NMX_LONG_BURSTS=1, staged tiles
    walk forms through the list (noise, default taps; 5 s ring: K = 1251, full at 41 absorbed hops)
    ring5         1000   1000   2 x 90 (30, 30, 30)  fill; thr<32> + thr_wave<2, true>; thr_wave<2, true>
    ring5_l2                                         ... thr_wave<2, false>                                       NMX_THR_LIST_LDS=0
    ring5_global                                     as ring5, the workgroup walk's list in L2                    NMX_THR_LIST_GLOBAL=1
    ring5_nofill                                     thr<32>; ...                                                 NMX_THR_FILL=0
    ring5_fill1                                      nmx_kern_burst_fill; ...                                     NMX_FILL_SPLIT=0
    ring5_nowave                                     fill; thr<32>; thr<32>                                       NMX_THR_WAVE=0
    ring5_chunk9                                     fill; thr<32>; thr_wave<2, true>              NMX_CHUNK_WINDOWS=9: fills inside a chunk
    rate2000      2000   2000   2 x 90 (30, 30, 30)  w1000_sparse, fill; thr<32> + thr_wave<4, false>; thr_wave<4, false>, stat_reg_sparse<32>
    ring2         1000   1000   2 x 60 (30, 30)      fill; thr<32>                                                K = 501: never one-wave
    k64 / k128    1000   1000   2 x 6  (3, 3)        fill; thr<64> / thr<128>                                     40 / 100 s ring: K = 10 001 / 25 001
    wide          1000   1000   2 x 6  (3, 3)        fill; thr_wide                                               135 s ring: K = 33 751
    tiled         1000   1000   2 x 6  (3, 3)        fill; thr_tiled                                              270 s ring: K = 67 501
    quieter after a full ring (constructed)
    quiet2 / quiet2_dense  1000  1000  3 x 26 (13, 13)  fill; thr<32>;  w500_sparse + stat_reg_sparse<16> / w500 + stat_reg<16>
    quiet5 / quiet5_dense  1000  1000  3 x 56 (45, 11)  fill + thr_wave<2, true>; thr_wave<2, true>;  the same Hilbert and statistics kernels

The kernels of stage 4 are asserted as a SET after every batch (`walk` table + the Hilbert and statistics kernels of plan_choice);
the plan stores sparse rows whenever the one-wave Hilbert kernels run, so the `_sparse` forms run from the first hop on.  The
emulator tier runs every case on the forms its plans build (the workgroup walk, tiled beyond 65 536 entries; the Hilbert item of
its bank; the LDS statistics and their tiled scan): it validates inputs, conditions, glue and limits.  Not reachable through
these outlets: a `frac` error inside the threshold's interpolation (no sample still in a window lies strictly between s[lo]
and s[lo + 1] of its own history), and the order of equal list entries.  Figures: profiles/burst_probes.md."""

from __future__ import annotations

import functools

import numpy as np

from tests.fir_sample_probe_cases import EPS32, FACTOR, YARD_CAP, assert_kernels, build_engine, conv32, conv64_direct, live_taps, rms

FACTORS: dict = {}       # case -> envelope factor where it is not FACTOR (at most 8; profiles/burst_probes.md)
MARGIN = 1e-3            # decision margin of a constructed row, in units of its largest envelope sample
NOISE_LEFT_OUT = 0.05
SENS_RATIO = 10.0
LO, HI = 100.0, 300.0
BANDS = ("low_beta", "high_beta")
SLOTS = ("duration_mean", "duration_max", "amplitude_mean", "amplitude_max", "burst_rate_per_s", "in_burst")
K_EPS = {"duration_max": 2, "duration_mean": 3, "burst_rate_per_s": 5}   # roundings + 1 (module docstring)

_H = "nmx_kern_hilbert_"
_B = "nmx_kern_burst_"
FILL2 = (_B + "fill_sort", _B + "fill_walk")


# ---- the plan's choices, restated (build_bursts, build_hilbert, nmx_burst_walk_plan; the CPU tier ties them to the source) ----
def plan_choice(W: int, sfreq: float, duration_s: float, threshold: float, feat_hz: float = 10.0, seg_s: float | None = None,
                env: dict | None = None, n_seq: int = 4) -> dict:
    env = env or {}
    flag = lambda k, d: int(env.get(k, d))   # noqa: E731
    q = threshold / 100.0
    n_ring = int(sfreq * duration_s)
    K = min(int(np.floor((1.0 - q) * (n_ring - 1))) + 2, n_ring)
    seg_s = W / sfreq if seg_s is None else seg_s
    overlap = int(sfreq * seg_s / feat_hz)
    if overlap == 0 or overlap > W:
        overlap = W
    al4 = lambda n: (n + 3) & ~3   # noqa: E731
    lds = (2 * al4(2 * W) if W & 1 else 2 * al4(W + 2) + al4(W)) * 4
    wave = flag("NMX_HILBERT_W500", 1) != 0
    hil = "long" if lds > 160 * 1024 else "w500" if wave and W == 1000 else "w1000" if wave and W == 2000 else "fixed128"
    sparse = flag("NMX_BURST_ENV_SPARSE", 1) != 0 and hil in ("w500", "w1000")
    stat = "stat_scan" if W > 16384 else "stat" if (W & 3) or W > 2048 else \
        ("stat_reg_sparse" if sparse else "stat_reg") + ("<16>" if W <= 1024 else "<32>")
    tiled = K > 65536
    thr = "thr_tiled" if tiled else "thr_wide" if -(-K // 256) > 128 else f"thr<{32 if -(-K // 256) <= 32 else 64 if -(-K // 256) <= 64 else 128}>"
    nr = 2 if overlap <= 128 else 4
    lo_ring = int(np.floor(q * (n_ring - 1)))
    ia = n_ring - 1 - lo_ring
    wave_from = None
    if flag("NMX_THR_WAVE", 1) and 1 <= overlap <= 256 and overlap + 8 < 192 * nr and K > 512 * nr and K - 3 <= ia < K:
        short = n_ring - W
        wave_from = 1 if short <= 0 else 1 + -(-short // overlap)
    lds_list = (5376 + K // 64 + 4) * 4 + 4 * K   # nmx_burst_thrw_lds(2, K, true): NMX_THRW_LDS_FLOATS_OF(2, true) = 5376
    list_lds = bool(flag("NMX_THR_LIST_LDS", 1) and nr == 2 and lds_list <= 80 * 1024 and n_seq <= 2 * 256 * ((160 * 1024) // lds_list))
    return {"K": K, "n_ring": n_ring, "overlap": overlap, "hilbert": _H + hil + ("_sparse" if sparse else ""), "stat": _B + stat, "thr": _B + thr,
            "fill": flag("NMX_THR_FILL", 1) != 0, "fill_split": flag("NMX_FILL_SPLIT", 1) != 0, "wave_from": wave_from, "nr": nr,
            "wave": _B + f"thr_wave<{nr}, {'true' if list_lds else 'false'}>"}


# ---- constructed streams -------------------------------------------------------------------------------------------------
def _block(rng, hop: int, pb: int, n: int | None, first=None, last=None, first_len=None, last_len=None, tight=False) -> np.ndarray:
    """One hop block with exactly pb high samples in n runs of 2 and up; first / last: the gaps in front of the first and
    behind the last run; first_len / last_len: those runs' lengths; tight: the first two runs are 2 samples each, 2 apart."""
    n = int(rng.integers(1, 4)) if n is None else n
    for _ in range(1000):
        lens = rng.multinomial(pb - 2 * n, np.ones(n) / n) + 2
        gm = 1 if 2 * pb <= hop else 2   # (low stretches between runs: 2 samples and up where the highs are the majority)
        g = rng.multinomial(hop - pb - gm * (n - 1), np.ones(n + 1) / (n + 1))
        g[1:n] += gm
        if tight:
            lens[2] += lens[0] + lens[1] - 4
            lens[0] = lens[1] = 2
            g[2] += g[1] - 2
            g[1] = 2
        if first_len is not None:
            lens[-1] += lens[0] - first_len
            lens[0] = first_len
        if last_len is not None:
            lens[0] += lens[-1] - last_len
            lens[-1] = last_len
        if first is not None:
            g[n if last is None else 1] += g[0] - first
            g[0] = first
        if last is not None:
            g[0 if first is None else 1] += g[n] - last
            g[n] = last
        if lens.min() >= 2 and g.min() >= 0 and (n == 1 or g[1:n].min() >= 1):
            break
    else:
        raise AssertionError("no such block")
    b = np.zeros(hop, bool)
    p = g[0]
    for ln, gap in zip(lens, g[1:]):
        b[p:p + ln] = True
        p += ln + gap
    assert b.sum() == pb and p - g[n] <= hop
    return b


def pattern(W: int, hop: int, pb: int, seed: int, variant: int) -> np.ndarray:
    """bool[W]: W / hop blocks of exactly pb highs.  variant 0: the last block ends and the first begins with one run (a run
    across the period's seam); 1: a run ending at hop - 2 in block 1, one starting at 1 in block 2; 2: two 2-sample runs two
    samples apart in block 1, a 3-sample run at the end of block 2 (it starts in the window's last lane when that block is
    the window's last); windows beyond 4096 samples: a run [2046, 2048) (variants 0, 2) or one starting at 2048 (1);
    others: random."""
    assert W % hop == 0
    nb = W // hop
    rng = np.random.default_rng(seed)
    force: dict = {}
    if variant == 0:
        force = {0: dict(n=1, first=0), nb - 1: dict(n=1, last=0)}
    elif variant == 1:
        force = {1: dict(n=2, last=1), 2: dict(n=2, first=1)}
    elif variant == 2:
        force = {1: dict(n=3, tight=True), 2: dict(n=2, last=0, last_len=3)}
    if W > 4096:   # (the 2048-sample tiles of the scan statistics)
        k = 2048 // hop
        force[k] = dict(n=2, first=2048 - k * hop - 2, first_len=2) if variant != 1 else dict(n=2, first=2048 - k * hop)
    return np.concatenate([_block(rng, hop, pb, **force.get(i, dict(n=None))) for i in range(nb)])


def series(b: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(one period of the signal, its envelope): the pattern's levels low-passed circularly, times the carrier."""
    W = b.size
    kcut, roll = 0.24 * W, 0.1 * W
    k = np.abs(np.fft.fftfreq(W, 1.0 / W))
    g = np.where(k <= kcut - roll, 1.0, np.where(k >= kcut, 0.0, 0.5 * (1 + np.cos(np.pi * (k - (kcut - roll)) / roll))))
    A = np.fft.ifft(np.fft.fft(np.where(b, HI, LO)) * g).real
    return A * np.cos(2 * np.pi * (W // 4) * np.arange(W) / W), A


SCALES = (1.0, 1e3, 1e-3)


def constructed_stream(W: int, hop: int, pb: int, C: int, hops: int, seed: int):
    """(x float32[C, T], patterns bool[C, W]): channel c repeats its own period, scaled by SCALES[c]."""
    T = W + (hops - 1) * hop
    pats = np.stack([pattern(W, hop, pb, seed + 17 * c, c) for c in range(C)])
    x = np.stack([np.tile(series(p)[0], T // W + 2)[:T] * SCALES[c % 3] for c, p in enumerate(pats)])
    return x.astype(np.float32), pats


def quieter_stream(n_ring: int, C: int, hops: int, seed: int, W: int = 1000, hop: int = 100, pb: int = 25, to: float = 0.6, ramp: int = 20):
    """Stream (b): the first and last 30 samples of every period are low (the highs they displace go to the middle of their
    block); the ring is full when the hop that appends sample `n_ring` comes, and from that sample on the stream is scaled
    to `to` over `ramp` samples."""
    assert n_ring % W == 0
    T = W + (hops - 1) * hop
    pats = []
    for c in range(C):
        b = pattern(W, hop, pb, seed + 17 * c, 3)
        b[:30] = False
        b[-30:] = False
        for a in (0, W - hop):
            blk = b[a:a + hop]
            idx = np.flatnonzero(~blk[35:65])[:pb - blk.sum()] + 35
            blk[idx] = True
            assert blk.sum() == pb
        pats.append(b)
    pats = np.stack(pats)
    t = np.clip((np.arange(T) - n_ring) / ramp, 0.0, 1.0)
    sc = 1 + (to - 1) * 0.5 * (1 - np.cos(np.pi * t))
    x = np.stack([np.tile(series(p)[0], T // W + 2)[:T] * sc * SCALES[c % 3] for c, p in enumerate(pats)])
    return x.astype(np.float32), pats


def noise_stream(sfreq: float, W: int, hop: int, C: int, hops: int, seed: int) -> np.ndarray:
    T = W + (hops - 1) * hop
    t = np.arange(T) / sfreq
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, T)) * 50.0 + 10 * np.sin(2 * np.pi * 17 * t) + 10 * np.sin(2 * np.pi * 27 * t + 0.7)
    return x.astype(np.float32)


# ---- cases ---------------------------------------------------------------------------------------------------------------
def _case(kind, sfreq=1000.0, W=1000, C=3, batches=(12,), duration=30.0, pb=25, hop=None, env=None, walk=(), absent=(), M=None,
          seed=1, feat_hz=10.0):
    hop = hop if hop is not None else int(sfreq * (W / sfreq) / feat_hz)
    return dict(kind=kind, sfreq=float(sfreq), W=W, C=C, batches=tuple(batches), duration=float(duration), pb=pb, hop=hop, env=env or {},
                walk=tuple(walk), absent=tuple(absent), M=M, seed=seed, feat_hz=float(feat_hz),
                threshold=100.0 * (1.0 - pb / hop) if kind != "noise" else 75.0)


def _m1536(W, half):
    return 1536 if W + half <= 1536 else 2048


_ONE = tuple([1] * 12)
_R5 = dict(kind="noise", C=2, batches=(30, 30, 30), duration=5.0, M=_m1536, seed=11)
FILL1, THR32, THR64, THR128, WIDE, TILED = (_B + "fill", _B + "thr<32>", _B + "thr<64>", _B + "thr<128>", _B + "thr_wide", _B + "thr_tiled")
WAVE2T, WAVE2F, WAVE4F = _B + "thr_wave<2, true>", _B + "thr_wave<2, false>", _B + "thr_wave<4, false>"
_WAVES = (WAVE2T, WAVE2F, WAVE4F)
_FILLS = FILL2 + (FILL1,)
_SPARSE_OFF = {"NMX_BURST_ENV_SPARSE": "0"}
# `walk`: per batch, the walk kernels of its first chunk (the Hilbert and statistics kernels follow plan_choice); `absent`: never
CASES = {
    "w1000": _case("constructed", walk=(FILL2,), absent=(THR32,)),
    "w1000_hops": _case("constructed", batches=_ONE, walk=((THR32,),) * 12, absent=_FILLS),
    "w1000_fixed": _case("constructed", env={"NMX_HILBERT_W500": "0"}, walk=(FILL2,)),
    "w1000_dense": _case("constructed", env=_SPARSE_OFF, walk=(FILL2,)),
    "w1000_q50": _case("constructed", pb=50, walk=(FILL2,), seed=2),
    "w1000_q10": _case("constructed", pb=90, walk=(FILL2,), seed=3),
    "w2000": _case("constructed", sfreq=2000, W=2000, C=3, batches=(6,), pb=50, walk=(FILL2,)),
    "w2000_dense": _case("constructed", sfreq=2000, W=2000, C=3, batches=(6,), pb=50, env=_SPARSE_OFF, walk=(FILL2,)),
    "w800": _case("constructed", sfreq=800, W=800, C=3, batches=(8,), pb=20, walk=(FILL2,)),
    "w901": _case("constructed", W=901, C=2, batches=(6,), pb=13, hop=53, feat_hz=17.0, walk=(FILL2,)),
    "w2500": _case("constructed", sfreq=2500, W=2500, C=2, batches=(6,), pb=50, walk=(FILL2,)),
    "w14000": _case("constructed", sfreq=14000, W=14000, C=2, batches=(2,), pb=350, walk=(FILL2,)),
    "w20000": _case("constructed", sfreq=20000, W=20000, C=2, batches=(2,), pb=500, env={"NMX_LONG_BURSTS": "1"}, walk=(FILL2,)),
    "ring5": _case(**_R5, walk=(FILL2, (THR32, WAVE2T), (WAVE2T,)), absent=(WAVE2F,)),
    "ring5_l2": _case(**_R5, env={"NMX_THR_LIST_LDS": "0"}, walk=(FILL2, (THR32, WAVE2F), (WAVE2F,)), absent=(WAVE2T,)),
    "ring5_global": _case(**_R5, env={"NMX_THR_LIST_GLOBAL": "1"}, walk=(FILL2, (THR32, WAVE2T), (WAVE2T,))),
    "ring5_nofill": _case(**_R5, env={"NMX_THR_FILL": "0"}, walk=((THR32,), (THR32, WAVE2T), (WAVE2T,)), absent=_FILLS),
    "ring5_fill1": _case(**_R5, env={"NMX_FILL_SPLIT": "0"}, walk=((FILL1,), (THR32, WAVE2T), (WAVE2T,)), absent=FILL2),
    "ring5_nowave": _case(**_R5, env={"NMX_THR_WAVE": "0"}, walk=(FILL2, (THR32,), (THR32,)), absent=_WAVES),
    "ring5_chunk9": _case(**_R5, env={"NMX_CHUNK_WINDOWS": "9"}, walk=(FILL2, (THR32,), (WAVE2T,))),
    "rate2000": _case("noise", sfreq=2000, W=2000, C=2, batches=(30, 30, 30), duration=5.0, M=lambda W, half: 4096, seed=12,
                      walk=(FILL2, (THR32, WAVE4F), (WAVE4F,)), absent=(WAVE2T, WAVE2F)),
    "ring2": _case("noise", C=2, batches=(30, 30), duration=2.0, M=_m1536, seed=13, walk=(FILL2, (THR32,)), absent=_WAVES),
    "k64": _case("noise", C=2, batches=(3, 3), duration=40.0, M=_m1536, seed=16, walk=(FILL2, (THR64,)), absent=_WAVES),
    "k128": _case("noise", C=2, batches=(3, 3), duration=100.0, M=_m1536, seed=17, walk=(FILL2, (THR128,)), absent=_WAVES),
    "wide": _case("noise", C=2, batches=(3, 3), duration=135.0, M=_m1536, seed=14, walk=(FILL2, (WIDE,)), absent=_WAVES),
    "tiled": _case("noise", C=2, batches=(3, 3), duration=270.0, M=_m1536, seed=15, walk=(FILL2, (TILED,)), absent=_WAVES),
    "quiet2": _case("quieter", batches=(13, 13), duration=2.0, walk=(FILL2, (THR32,))),
    "quiet2_dense": _case("quieter", batches=(13, 13), duration=2.0, env=_SPARSE_OFF, walk=(FILL2, (THR32,))),
    "quiet5": _case("quieter", batches=(45, 11), duration=5.0, walk=(FILL2 + (WAVE2T,), (WAVE2T,))),
    "quiet5_dense": _case("quieter", batches=(45, 11), duration=5.0, env=_SPARSE_OFF, walk=(FILL2 + (WAVE2T,), (WAVE2T,))),
}
EMU_CASES = list(CASES)
CONSTRUCTED = [n for n, c in CASES.items() if c["kind"] != "noise"]
ALL_KERNELS = {_H + k for k in ("fixed128", "long", "w500", "w500_sparse", "w1000", "w1000_sparse")} | \
              {_B + k for k in ("stat", "stat_scan", "stat_reg<16>", "stat_reg<32>", "stat_reg_sparse<16>", "stat_reg_sparse<32>")} | \
              set(_FILLS + _WAVES + (THR32, THR64, THR128, WIDE, TILED))


def walk_kernels(name: str) -> tuple:
    """The walk launches of the first chunk of every batch of a case: nmx_burst_walk_schedule, be_launch_burst_fill and
    be_launch_burst_thr restated on the case's plan_choice (the CPU tier holds the `walk` tables to it)."""
    c, ch = CASES[name], case_choice(name)
    chunk = int(c["env"].get("NMX_CHUNK_WINDOWS", 1024))
    never = 1 << 62
    wave_from = never if ch["wave_from"] is None else ch["wave_from"]
    out, seen = [], 0
    for n in c["batches"]:
        nw, done, k = min(n, chunk), 0, []
        if ch["fill"] and seen == 0 and nw >= 2 and c["W"] <= 32768:
            m = min(nw, (32768 - c["W"]) // ch["overlap"] + 1, wave_from)
            if m >= 2:
                k += list(FILL2) if ch["fill_split"] else [FILL1]
                done = m
        if done < nw and wave_from > seen + done:
            k.append(ch["thr"])
            done += min(wave_from - (seen + done), nw - done)
        if done < nw:
            k.append(ch["wave"] if seen + done < 4096 else ch["wave"].replace("true", "false"))
        out.append(tuple(k))
        seen += n
    return tuple(out)


def expected_kernels(name: str) -> set:
    """Every kernel a case asserts in stage 4: its walk table, and the Hilbert and statistics kernels of its plan."""
    ch = case_choice(name)
    return {k for b in CASES[name]["walk"] for k in b} | {ch["hilbert"], ch["stat"]}


def n_hops(c) -> int:
    return sum(c["batches"])


def case_choice(name: str) -> dict:
    c = CASES[name]
    seg_s = c["W"] / c["sfreq"] if c["W"] != 901 else 0.901
    return plan_choice(c["W"], c["sfreq"], c["duration"], c["threshold"], c["feat_hz"], seg_s, c["env"], 2 * c["C"])


def case_settings(c):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bursts = True
    s.segment_length_features_ms = 901 if c["W"] == 901 else 1000
    s.sampling_rate_features_hz = c["feat_hz"]
    s.bursts_settings.threshold = c["threshold"]
    s.bursts_settings.time_duration_s = c["duration"]
    s.bursts_settings.frequency_bands = list(BANDS)
    return s.validate()


def identity_taps(settings) -> np.ndarray:
    """bank_taps, one row per frequency band: [1.0], and [0.5] for the second burst band."""
    names = list(settings.frequency_ranges_hz)
    t = np.ones((len(names), 1))
    t[names.index(BANDS[1]), 0] = 0.5
    return t


@functools.lru_cache(maxsize=None)
def case_input(name: str):
    """(x float32[C, T], patterns or None) of a case; cases that differ only in selectors share it (and the reference)."""
    c = CASES[name]
    hops = n_hops(c)
    if c["kind"] == "constructed":
        return constructed_stream(c["W"], c["hop"], c["pb"], c["C"], hops, c["seed"])
    if c["kind"] == "quieter":
        return quieter_stream(int(c["sfreq"] * c["duration"]), c["C"], hops, c["seed"])
    return noise_stream(c["sfreq"], c["W"], c["hop"], c["C"], hops, c["seed"]), None


def _ref_key(name: str):
    c = CASES[name]
    return (c["kind"], c["sfreq"], c["W"], c["C"], n_hops(c), c["duration"], c["pb"], c["hop"], c["seed"], c["feat_hz"])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def env32_of(y32: np.ndarray) -> np.ndarray:
    """The analytic envelope in single precision: complex64 FFT / IFFT at length W, the modulus in float32."""
    import scipy.fft as sf

    W = y32.shape[-1]
    h = np.zeros(W, np.float32)
    if W % 2 == 0:
        h[0] = h[W // 2] = 1
        h[1:W // 2] = 2
    else:
        h[0] = 1
        h[1:(W + 1) // 2] = 2
    z = sf.ifft(sf.fft(np.asarray(y32, np.float32).astype(np.complex64), axis=-1) * h, axis=-1)
    assert z.dtype == np.complex64
    return np.sqrt(z.real * z.real + z.imag * z.imag).astype(np.float32)


def band_series(x: np.ndarray, taps, M) -> tuple[np.ndarray, np.ndarray]:
    """(y64, y32) [C, B, W] of the float32-exact window x [C, W]."""
    C, W = x.shape
    y64 = np.empty((C, len(taps), W))
    y32 = np.empty((C, len(taps), W), np.float32)
    for b, h in enumerate(taps):
        hl = live_taps(h, W)
        if len(hl) == 1:   # (one tap: a product, exact in float64; the yardstick rounds it once)
            y64[:, b] = hl[0] * x
            y32[:, b] = (np.float32(hl[0]) * x.astype(np.float32)).astype(np.float32)
        else:
            y64[:, b] = conv64_direct(x, hl)
            y32[:, b] = conv32(x, h, M(W, (len(hl) - 1) // 2))
    return y64, y32


def runs_of(b: np.ndarray):
    """(starts, exclusive ends of the finished runs, transitions) of a decision vector, as burst_stats counts them."""
    d = np.diff(np.concatenate(([False], b)).astype(np.int8))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1), int(np.count_nonzero(d))


def stats_of(env: np.ndarray, b: np.ndarray, sfreq: float, seg_s: float, L: float) -> dict:
    """{slot: (value, limit)} of one row from its decisions b: oracle.nm_oracle.burst_stats restated run by run."""
    starts, ends, n_trans = runs_of(b)
    nb = n_trans // 2
    dmean = float(b.sum()) / nb / sfreq if nb else 0.0
    out = {"duration_mean": dmean, "duration_max": 0.0, "amplitude_mean": 0.0, "amplitude_max": float((env * b).max()),
           "burst_rate_per_s": dmean / seg_s, "in_burst": float(b[-1])}
    lim = {k: K_EPS[k] * EPS32 * abs(out[k]) for k in K_EPS}
    lim["amplitude_max"], lim["in_burst"], lim["amplitude_mean"] = L, 0.0, 0.0
    nv = len(ends)
    if nv:
        lens = ends - starts[:nv]
        out["duration_max"] = float(lens.max()) / sfreq
        lim["duration_max"] = K_EPS["duration_max"] * EPS32 * out["duration_max"]
        means = np.array([env[s:e].mean() for s, e in zip(starts[:nv], ends)])
        per_run = [L + (e - s - 1) * EPS32 * float(np.abs(env[s:e]).mean()) + 2 * EPS32 * abs(m) for s, e, m in zip(starts[:nv], ends, means)]
        r = float(means.mean())
        out["amplitude_mean"] = r
        lim["amplitude_mean"] = max(per_run) + (nv - 1) * EPS32 * float(np.abs(means).mean()) + 2 * EPS32 * abs(r)
    return {k: (out[k], lim[k]) for k in SLOTS}


@functools.lru_cache(maxsize=None)
def _reference(key, name: str):
    """Per hop of the stream of case `name` (shared by every case of the same key): env64, thr64, y rms, e32, the descending
    float64 list, margins.  `factor` is not in it: limits are formed by the caller."""
    from oracle import nm_oracle as orc

    c = CASES[name]
    x, _ = case_input(name)
    s = case_settings(c)
    W, hop, C = c["W"], c["hop"], c["C"]
    from py_neuromodulation_amd.engine import HotPathEngine

    dry = HotPathEngine(s, [f"ch{i}" for i in range(C)], c["sfreq"], features=["bursts"], window=W, dry_run=True,
                        bank_taps=identity_taps(s) if c["kind"] != "noise" else None)
    taps = dry.filter_taps
    assert len(taps) == 2
    M = c["M"] or (lambda W, half: 0)
    ob = orc.Bursts(s, [f"ch{i}" for i in range(C)], c["sfreq"], taps=np.zeros((2, 1)))
    K = case_choice(name)["K"]
    assert ob.samples_overlap == hop and ob.n_ring == case_choice(name)["n_ring"], (ob.samples_overlap, hop)
    hops = []
    for h in range(n_hops(c)):
        xw = x[:, h * hop:h * hop + W].astype(np.float64)
        y64, y32 = band_series(xw, taps, M)
        env = orc.analytic_envelope(y64)
        e32 = np.abs(env32_of(y32).astype(np.float64) - env).max(-1)
        thr = ob.update_threshold(env[:, :, -(W if h == 0 else hop):])
        top = -np.sort(-ob.buffer, axis=-1)[:, :, :K]
        hops.append(dict(env=env, thr=thr, rms=rms(y64), e32=e32, top=top, margin=np.abs(env - thr[..., None]).min(-1),
                         emax=env.max(-1), total=W + h * hop))
    return dict(hops=hops, seg_s=ob.seg_s, taps=taps, K=K)


def reference(name: str) -> dict:
    return _reference(_ref_key(name), name)


def env_limits(name: str, ref: dict) -> np.ndarray:
    """L_env [hops, C, B]; asserts the yardstick's own cap on every row."""
    f = FACTORS.get(name, FACTOR)
    e32 = np.stack([h["e32"] for h in ref["hops"]])
    r = np.stack([h["rms"] for h in ref["hops"]])
    cap = YARD_CAP * EPS32 * np.maximum(r, np.stack([h["emax"] for h in ref["hops"]]))
    assert np.all(e32 <= cap), f"{name}: the single-precision yardstick is {float(np.max(e32 / cap)) * YARD_CAP:.1f} eps32 of the " \
                               f"row's scale from the float64 envelope: one of the two is wrong"
    return f * np.maximum(e32, EPS32 * r)


class Report:
    """Worst error / limit per family of one case (profiles/burst_probes.md)."""

    def __init__(self, name):
        self.name, self.worst, self.rows, self.left = name, {}, 0, 0

    def add(self, fam, ratio):
        self.worst[fam] = max(self.worst.get(fam, 0.0), float(ratio))

    def line(self, extra=""):
        w = " ".join(f"{k} {v:.3f}" for k, v in sorted(self.worst.items()))
        print(f"BURSTPROBE {self.name:14s} rows {self.rows:4d} left out {self.left:3d}  worst error / limit: {w} {extra}")


def parse_blob(blob: bytes, C: int, K: int):
    """(top float32[C, 2, K], counts int64[C, 2, 2]): the bursts section is the blob's first."""
    n = C * 2 * K
    top = np.frombuffer(blob, np.float32, n).reshape(C, 2, K)
    counts = np.frombuffer(blob, np.int64, C * 2 * 2, offset=4 * n).reshape(C, 2, 2)
    return top, counts


def check_list(name: str, blob: bytes, ref: dict, L: np.ndarray, seen: int, rep: Report) -> None:
    """The state behind `seen` hops against the float64 list, rank by rank."""
    C, K = L.shape[1], ref["K"]
    top, counts = parse_blob(blob, C, K)
    hop = ref["hops"][seen - 1]
    n = min(hop["total"], K)
    assert np.all(counts[..., 0] == hop["total"]) and np.all(counts[..., 1] == seen), f"{name}: counts {counts.tolist()} behind {seen} hops"
    assert not top[:, :, n:].tobytes().strip(b"\0"), f"{name}: entries behind the filled length {n} are not the reset's zero bytes"
    got = top[:, :, :n].astype(np.float64)
    assert np.isfinite(got).all() and np.all(np.diff(got, axis=-1) <= 0), f"{name}: the list is not descending"
    lim = L[:seen].max(0)
    err = np.abs(got - hop["top"][:, :, :n]).max(-1)
    ratio = err / lim
    rep.add("list", ratio.max())
    rep.add("envelope(yardsticks)", ratio.max() * FACTORS.get(name, FACTOR))
    assert np.all(err <= lim), f"{name} behind {seen} hops: list entry {ratio.max():.2f} limits off " \
                               f"({ratio.max() * FACTORS.get(name, FACTOR):.2f} yardsticks); per (channel, band): {np.round(ratio, 2).tolist()}"


def check_rows(name: str, out: np.ndarray, keys, first: int, ref: dict, L: np.ndarray, rep: Report) -> None:
    """The rows of hops [first, first + len(out)) against the reference's statistics under the reference's decisions."""
    c = CASES[name]
    col = {k: i for i, k in enumerate(keys)}
    assert len(col) == c["C"] * 2 * 6
    bad = []
    for i, row in enumerate(np.asarray(out, np.float64)):
        hp = ref["hops"][first + i]
        for ci in range(c["C"]):
            got_b = []
            for bi, band in enumerate(BANDS):
                rep.rows += 1
                got = {s: row[col[f"ch{ci}_bursts_{band}_{s}"]] for s in SLOTS}
                got_b.append(got)
                lim = L[first + i, ci, bi]
                if c["kind"] == "noise" and hp["margin"][ci, bi] < 2 * lim:
                    rep.left += 1
                    continue
                want = stats_of(hp["env"][ci, bi], hp["env"][ci, bi] >= hp["thr"][ci, bi], c["sfreq"], ref["seg_s"], lim)
                for s, (v, lm) in want.items():
                    e = abs(got[s] - v)
                    if lm > 0:
                        rep.add(s, e / lm)
                    if not (np.isfinite(got[s]) and e <= lm):
                        bad.append(f"hop {first + i} ch {ci} {band} {s}: got {got[s]!r}, reference {v!r}, error {e:.3g}, limit {lm:.3g}")
            if c["kind"] != "noise":   # band 1 = 0.5 x band 0: amplitudes halve exactly, the rest is equal
                for s in SLOTS:
                    f = 0.5 if s.startswith("amplitude") else 1.0
                    if got_b[1][s] != f * got_b[0][s]:
                        bad.append(f"hop {first + i} ch {ci} {s}: band 1 {got_b[1][s]!r} is not {f} x band 0 {got_b[0][s]!r}")
    assert not bad, f"{name}: {len(bad)} outputs beyond their limits\n  " + "\n  ".join(bad[:12])


def check_conditions(name: str) -> float:
    return _check_conditions(_ref_key(name), name)


@functools.lru_cache(maxsize=None)
def _check_conditions(key, name: str) -> float:
    """The conditions on a constructed case, on the reference alone: decisions equal the pattern (stream (a)), every row's margin
    >= MARGIN max env, the sensitivity of the statistics to one moved run boundary.  -> smallest margin / max env."""
    c = CASES[name]
    ref = reference(name)
    L = env_limits(name, ref)
    _, pats = case_input(name)
    worst = np.inf
    for h, hp in enumerate(ref["hops"]):
        m = hp["margin"] / hp["emax"]
        worst = min(worst, float(m.min()))
        assert np.all(m >= MARGIN), f"{name} hop {h}: margin {m.min():.3g} max env"
        for ci in range(c["C"]):
            for bi in range(2):
                env, b = hp["env"][ci, bi], hp["env"][ci, bi] >= hp["thr"][ci, bi]
                if c["kind"] == "constructed":
                    assert np.array_equal(b, np.roll(pats[ci], -h * c["hop"])), f"{name} hop {h} ch {ci}: decisions leave the pattern"
                if bi == 0:
                    check_sensitivity(f"{name} hop {h} ch {ci}", env, b, c["sfreq"], ref["seg_s"], L[h, ci, bi])
    return worst


def check_sensitivity(what: str, env, b, sfreq, seg_s, L) -> None:
    base = stats_of(env, b, sfreq, seg_s, L)
    d = np.flatnonzero(np.diff(np.concatenate(([False], b)).astype(np.int8)))
    for t in d:
        for flip in (t, t - 1):
            if flip < 0:
                continue
            b2 = b.copy()
            b2[flip] = not b2[flip]
            alt = stats_of(env, b2, sfreq, seg_s, L)
            moved = max(abs(alt[s][0] - base[s][0]) / max(base[s][1], alt[s][1], 1e-300)
                        for s in ("duration_mean", "duration_max", "amplitude_mean") if alt[s][0] != base[s][0])
            assert moved >= SENS_RATIO, f"{what}: boundary {t} moved to {flip}: the statistics move by {moved:.2f} limits"


def noise_left_out(name: str) -> float:
    """Share of the rows of a noise case the reference alone leaves out."""
    ref = reference(name)
    L = env_limits(name, ref)
    m = np.stack([h["margin"] for h in ref["hops"]])
    return float((m < 2 * L).mean())


# ---- a case on a library ------------------------------------------------------------------------------------------------
def run_table(lib, name: str) -> np.ndarray:
    """The rows of every batch of a case, in order."""
    return run_case(lib, name).table


def run_case(lib, name: str) -> Report:
    c = CASES[name]
    x, _ = case_input(name)
    ref = reference(name)
    L = env_limits(name, ref)
    s = case_settings(c)
    W, hop, C = c["W"], c["hop"], c["C"]
    eng = build_engine(lib, c["env"], s, [f"ch{i}" for i in range(C)], c["sfreq"], features=["bursts"], window=W,
                       bank_taps=identity_taps(s) if c["kind"] != "noise" else None)
    rep = Report(name)
    ran: set = set()
    tables = []
    choice = case_choice(name)
    try:
        assert eng.W == W and len(eng.filter_taps) == 2
        at = 0
        for bi, n in enumerate(c["batches"]):
            seg = np.ascontiguousarray(x[:, at * hop:(at + n - 1) * hop + W])
            out = eng.process_batch(seg, np.arange(n, dtype=np.int64) * hop)
            assert out.dtype == np.float32 and out.shape == (n, len(eng.keys))
            if lib is None:
                names = set(eng.kernels(4).split(" + "))
                ran |= names
                want = set(c["walk"][bi]) | {choice["hilbert"], choice["stat"]}
                for k in sorted(want):
                    assert_kernels(lib, f"{name} batch {bi}", eng, {4: k})
                assert names == want, f"{name} batch {bi}: stage 4 ran {sorted(names)}, wanted {sorted(want)}"
            check_list(name, eng.export_state(), ref, L, at + n, rep)
            check_rows(name, out, eng.keys, at, ref, L, rep)
            tables.append(out)
            at += n
        assert not ran & set(c["absent"]), f"{name}: stage 4 ran {sorted(ran & set(c['absent']))}"
        rep.table = np.concatenate(tables)
    finally:
        eng.close()
    share = rep.left / max(rep.rows, 1)
    rep.line(f"kernels {' + '.join(sorted(ran))}" if ran else "")
    if c["kind"] == "noise":
        print(f"BURSTPROBE {name:14s} rows left out {rep.left} of {rep.rows} = {100 * share:.2f} %")
        assert share <= NOISE_LEFT_OUT, f"{name}: {100 * share:.1f} % of the rows left out"
    else:
        assert rep.left == 0
    return rep


# ---- what the constructed rows reach (asserted by the CPU tier) ---------------------------------------------------------------
def lane_width(name: str) -> int:
    """Samples per lane of the statistics kernel of a case: 16 / 32 in registers, ceil(W / 64) in LDS, 32 within a 2048-sample
    tile of the scan form."""
    stat, W = case_choice(name)["stat"], CASES[name]["W"]
    return 16 if "<16>" in stat else 32 if "<32>" in stat or stat.endswith("scan") else -(-W // 64)


def edge_classes(name: str) -> set:
    """The run-edge classes the reference's decisions reach in the rows of a constructed case (band 0; band 1 decides the same)."""
    c, ref = CASES[name], reference(name)
    W, ch = c["W"], lane_width(name)
    kind = case_choice(name)["stat"].replace(_B, "").replace("_sparse", "")
    seen = set()
    for hp in ref["hops"]:
        for ci in range(c["C"]):
            b = hp["env"][ci, 0] >= hp["thr"][ci, 0]
            starts, ends, n_trans = runs_of(b)
            last = np.concatenate([ends, [W]])[:len(starts)] - 1   # last sample of every run, the open one included
            seen.add((kind, "no run") if not b.any() else (kind, "runs"))
            if n_trans & 1:
                seen.add((kind, "odd transitions"))
            if b[0]:
                seen.add((kind, "run from 0"))
            if b[-1]:
                seen.add((kind, "run ending at W - 1"))
            if b[-2] and not b[-1]:
                seen.add((kind, "run ending at W - 2"))
            seen |= {(kind, "start", int(r)) for r in starts % ch} | {(kind, "end", int(r)) for r in last % ch}
            lanes = starts // ch
            if np.any(np.diff(lanes) == 0):
                seen.add((kind, "two runs in one lane"))
            if np.any(last // ch - lanes >= 3):
                seen.add((kind, "four lanes"))
            tail = (W - 1) // ch * ch
            if W % ch and np.any(starts >= tail):
                seen.add((kind, "start in the last partly filled lane"))
            if W % ch and np.any((ends > tail) & (ends < W)):
                seen.add((kind, "end in the last partly filled lane"))
            if W > 2048:
                seen |= {(kind, "seam", w) for w, hit in (("start at it", np.any((starts % 2048 == 0) & (starts > 0))),
                                                         ("end before it", np.any(ends % 2048 == 0)),
                                                         ("across", np.any(starts // 2048 < last // 2048))) if hit}
    return seen
