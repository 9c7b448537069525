"""Per-sample probes of the front end (the re-reference kernels, the offset shift and the offset split around them, the NaN
mask) and of the window-wise resampler, shared by the emulator tier (test_front_probes_cpu.py) and the MI355X tier
(test_front_probes_gpu.py).

These stages produce the samples every other kernel reads.  tests/prep_stage_cases.py pins their bytes (a guard against
change, no statement on correctness, 6 channels); case_reref_structured_matrices allows 1e-6 max|x| with an offset ten times
the signal inside max|x|; case_resampler allows 2e-5 max|x|; the device forms nmx_car_tile<16>, nmx_car_tile<4> and
nmx_reref_struct_tile were reached through feature parity only.  A probe compares EVERY sample of EVERY row a kernel stores
with a float64 restatement.  No row and no sample is left out, no verifier, no accepted miss.

Outlets (calls that exist; nothing is exported for the probes):
  preprocess_window                      the one-window front end; float64, the carried constants added back in float64
  process_batch(want_nan_mask, tap=True) the stream front end over a chunk's sample range: the tapped windows + offsets()[1]
  offsets()                              the constants themselves

1. Re-reference kernels (nmx_k_prep.h).  Reference R @ u + D in float64:
     u   the plan not splitting: nan_to_num(x) of the fp32 input; splitting: float32(x) - float32(sub) formed in np.float32
         as nmx_clean_sub forms it, a NaN becomes -float32(d_in)
     D   (R_exact @ d_in) x the notch gain
   twice: (a) with the coefficients the plan uploads -- R.astype(float32) (dense), float32(diag) and float32(off) (common
   average), float32(val - o) and float32(o) per row (structured: find_reref_structure restated in `struct_decompose`) --
   and (b) with the exact float64 R, which is what the reference project computes.
   Limits (derived: the kernels multiply fp32 by fp32 in float64, which is exact, add in float64, round once at the store):
     (a)  |got - want| <= 0.5 eps32 |want - D| (1 + 1e-6) + C_in 2^-52 sum_j |R_ij u_j| + 2^-149  [+ F64]
     (b)  the same + eps32 sum_j (|R_ij| + |o_i|) |u_j|     (o_i: the row's repeated value, on the members of its group;
          0 in the dense kernel) -- the rounding of the coefficients
   F64 = C_in 2^-52 sum_j |R_ij d_j| + 2^-52 |want|: both outlets hand the samples over as float64 with D added back in
   float64 (the plan's own D is a float64 dot product, the sum y + D rounds at |y + D|), so no implementation of these
   outlets can meet a limit below the float64 spacing of what it returns.  The term is 0 without offsets and, with offsets
   of 1e5 times the signal, 2e-11 of the signal -- 3000 times below half an fp32 ulp: the limits stay relative to the signal
   u, never to an offset, which is what makes the offset split testable.  Each case runs four times: noise, noise on
   per-row offsets of 1e5 times the row's signal (fp32 input: the learned split engages; the SAME limits), the same with
   NMX_DC_SPLIT=0 ((b) only, u = x), and impulses.
   Inputs: fixed-seed noise of sigma 50, the rows cycling through the amplitudes 1, 1e4, 1e-3 and a zero row; one unit
   impulse per input row, each at its own sample (an output there is the matrix entry itself); NaN samples at t = 0, 63,
   64, 255, 256, T - 1 and at the first and the last sample of a window.
   Shapes: `return_raw` only, 1 kHz, W = 200, hop 100, 12 hops: the range of a stream call is 1300 samples (no multiple of
   64 or 256).  Every case runs through BOTH outlets (the tap, then preprocess_window of the first and the last window).

    case                    C x C_in        kernel asserted (stage 1)   form / what it exercises
    car_cN, N < 64          N x N           nmx_kern_car               NW = 4 (C < 64): N = 2 3 5 12 13 16 17 29 33 63: every
                                                                       combination of the three tail terms, 0 - 4 trips of the
                                                                       16-stride loop
    car_cN, N >= 64         N x N           nmx_kern_car               NW = 16 (range <= 4096 and C >= 64; preprocess_window
                                                                       and the 1300-sample range): N = 64 65 79 80 97 113 128
                                                                       129 257: 1, 2, 4 trips of the 64-stride loop, 0 - 3
                                                                       terms of the 16-stride tail (97: the tail of two)
    car_long_c65 / _c129    65 / 129        nmx_kern_car               NW = 4 at C >= 64: 45 hops, range 4600 > 4096; `short`: the
                                                                       first 30 hops of the same recording, range 3100: NW = 16
    car_bytes_c65 / _c129   65 / 129        nmx_kern_car               no notch, NMX_DC_SPLIT=0, no offsets: the tapped windows of
                                                                       the 4600-sample range (NW = 4), of the 3100-sample range
                                                                       (NW = 16) and preprocess_window (NW = 16), BYTE FOR BYTE
    struct_sub40            5 x 40          nmx_kern_reref_struct      rows 8 - 12 of a 40-channel average: one group, C != C_in
    struct_g1               7 x 33          nmx_kern_reref_struct      one group of 33; bipolar rows of 2 and 3 taps, a pass-through
    struct_g2               9 x 13          nmx_kern_reref_struct      groups of 5 and 6 + 2 (a row of a group plus extra taps)
    struct_g3               5 x 54          nmx_kern_reref_struct      groups of 16, 17, 21
    struct_g4               9 x 60          nmx_kern_reref_struct      groups of 5, 6, 16, 33; bipolar rows, a pass-through
    struct_taps             5 x 3           nmx_kern_reref_struct      no group at all: every row is taps
    struct_g5               7 x 60          nmx_kern_reref             FIVE groups: the search gives up, the dense product runs
    dense_cN_in300          N x 300         nmx_kern_reref             N = 1 15 16 17 33: both sides of NMX_REREF_ROWS = 16
    dense_cN_in3            N x 3           nmx_kern_reref             the same N with NMX_REREF_STRUCT=0 (3 entries per row are taps
                                                                       to the search: without it this is struct_taps' kernel)
    dense_car17             17 x 17         nmx_kern_reref             the CAR matrix, NMX_CAR_FAST=0 NMX_REREF_STRUCT=0
    shift_c4                4 (no matrix)   nmx_kern_shift + the notch no matrix, notch on, W = 1000, offsets 1e5 times the signal:
                                                                       a NaN becomes -d in the split domain; reference u -> the FIR
                                                                       probes' float64 odd-reflection convolution, limit: theirs
    chunks_car / _struct    13 / 9 x 13     as car_c13 / struct_g2      NMX_CHUNK_WINDOWS=4: three chunks (lo > 0 in launch_front),
                                                                       bytes == the one-chunk run

   The emulator tier runs the `_sample` forms of the same cases (nmx_car_sample, nmx_reref_struct_sample; one summation
   order whatever C is): the `_tile` forms and their NW exist on the device only.

2. Learned constants and the NaN mask
    learned      5 x 5 CAR      offsets()[0] == the rule of dc_prepare restated in NumPy, EXACTLY: rows at 3.9 and 4.1 times their
                                spread, a row with NaN and inf in the first window, an all-NaN first window, a zero row;
                                12 hops in one batch and 12 one-hop batches store the same tapped bytes
    nanmask      5 x 7 struct   nmx_kern_nanmask (be_launch_nanmask is its only launch; the launcher records no name, so the kernel
                                cannot be asserted through kernels(): test_front_probes_cpu.py reads the launcher's source):
                                a NaN at start - 1, start, start + 63, start + 64, start + W - 1, start + W, each on its own input
                                row, ragged starts, C_in != C; mask == isnan(x[:, a:a + W]).any(1) per hop

3. Resampler (nmx_k_resample.h, build_resample).  Reference oracle.mne_restated.resample in float64 (`resample64`, an explicit
   restatement -- pad, rfft, bins, irfft --, is tied to it at 1e-12 on every case).  Yardstick (`resample32`): the same chain
   on the same fp32 input in single precision -- the padding in float32, scipy.fft on float32 / complex64 at the plan's
   lengths, for the polyphase form a float32 table w_N and a complex64 accumulation over the q components, the bins' scale
   and `scale` in float32, every hand-off rounded to float32.  Limit, as the FIR probes':
   max_n |y - y64| <= FACTOR max(e32[row], eps32 rms(x_row)), FACTOR = 4 (8 on the impulse rows of the six cases of FACTORS,
   where e32 is one store rounding: the reason stands at the table); the yardstick itself within YARD_CAP eps32 of the row's
   scale as the transforms see it -- max(rms(x_row), rms(padded row), max|y64|) -- checked on every case on the CPU.  `resample_plan` restates build_resample's arithmetic; every case asserts
   its class.  C = 3, one window; kernel asserted: nmx_kern_resample (the name does not tell the forms apart: poly_q > 0
   when n_pad > 8192, or the LDS layout does not fit, or NMX_RESAMPLE_POLY=1; inv_full when n_new is odd).

    case             rates, W               n_pad  n_new  form, inverse        class
    down_even        2000 -> 1000, 2000     4096   2048   one, even            Nyquist bin 1024 doubled
    down_odd         1375 -> 500, 1375      2048   745    one, odd             odd W (pad_l 336 != pad_r 337), full complex inverse
    up_even          1000 -> 2000, 500      1024   2048   one, even            bin n_pad / 2 halved, zero-extended spectrum
    up_odd           1024 -> 1125, 800      1024   1125   one, odd             up-sampling with the full inverse
    tiny_4 / tiny_9  2000 -> 1000, 4 / 9    4 / 16 2 / 8  one, even            pad = 0; pads of 3 and 4 (W_new = round(4.5) = 4)
    one_8192         7000 -> 1000, 7000     8192   1170   one, even            the largest one-transform plan
    poly_forced_40   2000 -> 1000, 40       64     32     poly q = 2, even     NMX_RESAMPLE_POLY=1; an impulse at EVERY position
    poly_forced_4k   4000 -> 1000, 4000     8192   2048   poly q = 4, even     forced; one_4k is the unforced plan: the same limit
    poly_8k          8000 -> 1000, 8000     16384  2048   poly q = 8, even
    poly_24k         24000 -> 1000, 24000   32768  1365   poly q = 16, odd
    poly_44k         44100 -> 1000, 44100   65536  1486   poly q = 32, even
    tie_down / _up   2000 -> 1000, 1001 / 1003   2048  1024   one, even        500.5 -> 500, crop 261.5 -> 262 / 501.5 -> 502

   The emulator tier runs every case, poly_24k and poly_44k included (1 and 2 seconds there).
   Inputs: unit impulses, one per row, at 0, 1, 2, pad_l - 1 .. pad_l + 1, W - 2 - pad_r .. W - pad_r, W - 2, W - 1, W / 2, for
   polyphase plans 0 .. 2 q + 1 and the samples whose reflections are the padded points q j + r of j = 0, 1, m - 2, m - 1 (the
   first and last points of every component lie in the pads), cycling through calls of C positions; noise of sigma 50 with a
   level of 300 on one row and one NaN (clean on load); one tone exactly on the kept Nyquist bin of the padded length, in
   cosine and in sine phase.
   Batch outlet (batch_resample, batch_notch_resample): 2000 -> 1000, C = 5, 9 hops with ragged starts through the tap, the
   resampler alone and behind the notch at the raw rate (reference: the FIR probes' float64 notch, then resample64; the same
   yardstick rule); the tapped windows of a hop == preprocess_window of that window on a fresh plan, byte for byte.

The figures observed are in profiles/front_probes.md."""

from __future__ import annotations

import numpy as np

from tests import fir_sample_probe_cases as fir

EPS32 = fir.EPS32
FACTOR = fir.FACTOR       # the resampler's limit in units of the yardstick's error
YARD_CAP = fir.YARD_CAP   # the yardstick's own error, in eps32 of the row's scale
# (case, input class) -> factor in force where it is not FACTOR (at most 8; the reasons: profiles/front_probes.md).  Impulse rows
# only: there e32 is ONE store rounding -- the output peak adds n_new / 2 roots of unity in phase, the yardstick reads each root
# from a correctly rounded table, so its error at the peak is 0 or half an ulp of the peak by the luck of the last rounding, not
# a statistic of an fp32 chain -- while a transform that forms w^2 .. w^4 from the table's w by multiplication (nmx_fft's radix-4
# and radix-5 stages) carries an eps32 per root and stage and comes out 2 - 4 ulp of the peak away.
FACTORS: dict = {(n, "impulse"): 8.0 for n in ("one_4k", "poly_forced_4k", "poly_8k", "poly_44k", "tie_down", "tie_up")}
SIGMA = fir.SIGMA
SFREQ, W, HOP, HOPS = 1000.0, 200, 100, 12
LONG_HOPS, SHORT_HOPS = 45, 30          # ranges of 4600 (> 4096: NW = 4) and 3100 samples
AMPS = (1.0, 1e4, 1e-3, 0.0)            # the rows' amplitudes, cycling
OFFSET = 1e5                            # per-row offsets, in units of the row's signal
NAN_T = (0, 63, 64, 255, 256)
CAR = "nmx_kern_car"
STRUCT = "nmx_kern_reref_struct"
DENSE = "nmx_kern_reref"
SHIFT = "nmx_kern_shift"
RESAMPLE = "nmx_kern_resample"
F2_52, F2_149 = 2.0 ** -52, 2.0 ** -149


class Report:
    """Per (case, variant): samples compared and the worst err / limit (profiles/front_probes.md).  One line per entry when a
    case ends."""

    def __init__(self) -> None:
        self.seen: dict = {}

    def add(self, case, what, ratio, n, extra=""):
        r, m, e = self.seen.get((case, what), (0.0, 0, ""))
        self.seen[(case, what)] = (max(r, float(ratio)), m + int(n), extra or e)

    def flush(self, case):
        for (c, what), (r, n, e) in list(self.seen.items()):
            if c == case:
                print(f"FRONTPROBE {c:22s} {what:22s} samples {n:9d}  worst err / limit {r:6.3f}  {e}")
                del self.seen[(c, what)]


REPORT = Report()


# ---- 1. re-reference: matrices ----------------------------------------------------------------------------------------
def car_matrix(C: int) -> np.ndarray:
    return fir.car_matrix(C)


def _avg_row(Cin: int, G, i: int) -> np.ndarray:
    """The reference's "average" row of channel i over the type group G (processing/rereference.py:61-63)."""
    r = np.zeros(Cin)
    r[list(G)] = -1.0 / (len(G) - 1)
    r[i] = 1.0
    return r


def _taps_row(Cin: int, taps: dict) -> np.ndarray:
    r = np.zeros(Cin)
    for j, v in taps.items():
        r[j] = v
    return r


def _groups(sizes):
    out, a = [], 0
    for n in sizes:
        out.append(range(a, a + n))
        a += n
    return out, a


def struct_matrix(name: str) -> np.ndarray:
    if name == "struct_sub40":
        return car_matrix(40)[8:13]
    if name == "struct_g1":
        (G,), Cin = _groups([33])
        return np.stack([_avg_row(Cin, G, 0), _avg_row(Cin, G, 1), _avg_row(Cin, G, 5), _avg_row(Cin, G, 32),
                         _taps_row(Cin, {3: 1.0, 30: -1.0}), _taps_row(Cin, {4: 1.0, 5: -0.5, 6: -0.5}), _taps_row(Cin, {7: 1.0})])
    if name == "struct_g2":
        (A, B), Cin = _groups([5, 6])
        Cin += 2   # two channels outside both groups: the extra taps
        plus = _avg_row(Cin, B, 6) + _taps_row(Cin, {11: 0.25, 12: -0.125})
        return np.stack([_avg_row(Cin, A, 0), _avg_row(Cin, A, 4), _avg_row(Cin, A, 2), _avg_row(Cin, B, 5), _avg_row(Cin, B, 10),
                         plus, _taps_row(Cin, {11: 1.0, 12: -1.0}), _taps_row(Cin, {12: 1.0}), _avg_row(Cin, A, 3)])
    if name == "struct_g3":
        (A, B, Cg), Cin = _groups([16, 17, 21])
        return np.stack([_avg_row(Cin, A, 0), _avg_row(Cin, A, 15), _avg_row(Cin, B, 16), _avg_row(Cin, Cg, 53), _avg_row(Cin, B, 32)])
    if name in ("struct_g4", "struct_g5"):
        (A, B, Cg, Dg), Cin = _groups([5, 6, 16, 33])
        rows = [_avg_row(Cin, A, 1), _avg_row(Cin, B, 5), _avg_row(Cin, Cg, 11), _avg_row(Cin, Dg, 27), _avg_row(Cin, Dg, 59)]
        if name == "struct_g4":
            rows += [_taps_row(Cin, {0: 1.0, 59: -1.0}), _taps_row(Cin, {2: 1.0, 3: -0.5, 40: -0.5}), _taps_row(Cin, {58: 1.0}),
                     _avg_row(Cin, Cg, 26)]
        else:   # a fifth group: the members of A and B together
            rows += [_avg_row(Cin, range(0, 11), 3), _taps_row(Cin, {58: 1.0})]
        return np.stack(rows)
    if name == "struct_taps":
        return np.array([[1.0, -1.0, 0.0], [-0.5, 1.0, -0.5], [0.0, 0.0, 1.0], [0.3, 0.3, 0.4], [0.0, -2.0, 1.0]])
    raise KeyError(name)


def struct_decompose(R: np.ndarray):
    """find_reref_structure restated.  -> [(taps {j: value}, group members or None, o)] per row, or None where the plan
    falls back to the dense product (a row of more than NMX_RS_TAPS entries beside its repeated value, a fifth group)."""
    rows, groups = [], {}
    for row in np.asarray(R, np.float64):
        nz = np.flatnonzero(row)
        if len(nz) <= 4:
            rows.append(({int(j): float(row[j]) for j in nz}, None, 0.0))
            continue
        vals, counts = np.unique(row[nz], return_counts=True)   # ascending: the first of the most frequent values
        o = float(vals[int(np.argmax(counts))])
        if len(nz) - int(counts.max()) > 4:
            return None
        key = tuple(int(j) for j in nz)
        if key not in groups:
            if len(groups) == 4:
                return None
            groups[key] = len(groups)
        rows.append(({int(j): float(row[j]) - o for j in nz if row[j] != o}, key, o))
    return rows


def is_car(R: np.ndarray) -> bool:
    """build_front's exact common-average test."""
    C, Cin = R.shape
    if C != Cin or C < 2:
        return False
    want = np.full((C, C), R[0, 1])
    np.fill_diagonal(want, R[0, 0])
    return bool(np.all(np.abs(R - want) <= 1e-12))


def front_kernel(R: np.ndarray, env: dict) -> str:
    """The kernel build_front chooses for matrix R under the selectors of `env`."""
    if env.get("NMX_CAR_FAST", "1") != "0" and is_car(R):
        return CAR
    if env.get("NMX_REREF_STRUCT", "1") != "0" and struct_decompose(R) is not None:
        return STRUCT
    return DENSE


def uploaded(R: np.ndarray, kernel: str):
    """(R_a, O): the matrix the kernel's fp32 coefficients amount to, in float64, and |o_i| on the members of row i's group
    (zeros where the row has none)."""
    R = np.asarray(R, np.float64)
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    O = np.zeros(R.shape)
    if kernel == DENSE:
        return R.astype(np.float32).astype(np.float64), O
    if kernel == CAR:
        d, o = f32(R[0, 0]), f32(R[0, 1])
        Ra = np.full(R.shape, o)
        Ra[np.diag_indices(len(R))] += d - o   # y_i = (d - o) u_i + o sum_j u_j
        return Ra, np.full(R.shape, abs(R[0, 1]))
    Ra = np.zeros(R.shape)
    for i, (taps, G, o) in enumerate(struct_decompose(R)):
        for j, v in taps.items():
            Ra[i, j] += f32(v)
        if G is not None:
            Ra[i, list(G)] += f32(o)
            O[i, list(G)] = abs(o)
    return Ra, O


def struct_rebuilt(R: np.ndarray) -> np.ndarray:
    """The decomposition with exact coefficients, put together again (the CPU test: == R at 1e-12)."""
    out = np.zeros(R.shape)
    for i, (taps, G, o) in enumerate(struct_decompose(R)):
        for j, v in taps.items():
            out[i, j] += v
        if G is not None:
            out[i, list(G)] += o
    return out


def _dense(C: int, Cin: int) -> np.ndarray:
    return np.random.default_rng(100 * C + Cin).standard_normal((C, Cin))


NO_STRUCT = {"NMX_REREF_STRUCT": "0"}
# name -> (matrix, env, kernel, hops)
REREF_CASES: dict = {}
for _c in (2, 3, 5, 12, 13, 16, 17, 29, 33, 63, 64, 65, 79, 80, 97, 113, 128, 129, 257):
    REREF_CASES[f"car_c{_c}"] = (lambda c=_c: car_matrix(c), {}, CAR, HOPS)
for _c in (65, 129):
    REREF_CASES[f"car_long_c{_c}"] = (lambda c=_c: car_matrix(c), {}, CAR, LONG_HOPS)
for _n in ("struct_sub40", "struct_g1", "struct_g2", "struct_g3", "struct_g4", "struct_taps"):
    REREF_CASES[_n] = (lambda n=_n: struct_matrix(n), {}, STRUCT, HOPS)
REREF_CASES["struct_g5"] = (lambda: struct_matrix("struct_g5"), {}, DENSE, HOPS)
for _c in (1, 15, 16, 17, 33):
    REREF_CASES[f"dense_c{_c}_in300"] = (lambda c=_c: _dense(c, 300), {}, DENSE, HOPS)
    REREF_CASES[f"dense_c{_c}_in3"] = (lambda c=_c: _dense(c, 3), NO_STRUCT, DENSE, HOPS)
REREF_CASES["dense_car17"] = (lambda: car_matrix(17), {"NMX_CAR_FAST": "0", "NMX_REREF_STRUCT": "0"}, DENSE, HOPS)
CAR_NW4 = [f"car_c{c}" for c in (2, 3, 5, 12, 13, 16, 17, 29, 33, 63)]
CAR_NW16 = [f"car_c{c}" for c in (64, 65, 79, 80, 97, 113, 128, 129, 257)]
CAR_LONG = ["car_long_c65", "car_long_c129"]
STRUCT_CASES = [n for n in REREF_CASES if n.startswith("struct")]
DENSE_CASES = [n for n in REREF_CASES if n.startswith("dense")]


def car_waves(C: int, n_range: int) -> int:
    """be_launch_car: waves per workgroup of the device form."""
    return 16 if n_range <= 4096 and C >= 64 else 4


# ---- 1. re-reference: inputs, reference, limits -------------------------------------------------------------------------
def starts_of(hops: int) -> np.ndarray:
    return np.arange(hops, dtype=np.int64) * HOP


def row_scales(Cin: int) -> np.ndarray:
    return np.array([AMPS[j % len(AMPS)] for j in range(Cin)])


def nan_places(Cin: int, T: int, window: int = W) -> list[tuple[int, int]]:
    """(row, t): the block boundaries of the kernels, the end of the range, the first and the last sample of a window."""
    ts = [t for t in NAN_T if t < T] + [T - 1]
    if T > window:
        ts += [3 * HOP, 3 * HOP + window - 1]
    return [((5 * k + 1) % Cin, t) for k, t in enumerate(dict.fromkeys(ts))]


def recording(Cin: int, T: int, cls: str, seed: int, offsets: bool = False, window: int = W) -> np.ndarray:
    """float32 [C_in, T] of input class `cls` ("noise", "impulse"), NaN samples included."""
    if cls == "impulse":
        x = np.zeros((Cin, T))
        step = next(s for s in (11, 13, 17, 19, 23) if np.gcd(s, T) == 1)
        x[np.arange(Cin), (3 + step * np.arange(Cin)) % T] = 1.0   # (distinct samples while C_in <= T)
    else:
        sc = row_scales(Cin)
        x = np.random.default_rng(seed).standard_normal((Cin, T)) * SIGMA * sc[:, None]
        if offsets:
            sign = np.where(np.arange(Cin) % 3 == 1, -1.0, 1.0)
            x += (sign * OFFSET * SIGMA * np.where(sc > 0, sc, 1.0))[:, None]
    x = x.astype(np.float32)
    for j, t in nan_places(Cin, T, window):
        x[j, t] = np.nan
    return x


def split_u(x32: np.ndarray, d_in: np.ndarray) -> np.ndarray:
    """What the kernels multiply: nmx_clean_sub restated in np.float32 (sub = float32(d_in): nothing is set by the host in
    these plans).  float64 [C_in, T] of fp32 values."""
    assert x32.dtype == np.float32
    sub = np.asarray(d_in, np.float64).astype(np.float32)
    assert np.array_equal(sub.astype(np.float64), d_in), "learned constants are fp32 values"
    bad = np.isnan(x32)
    fmax = np.finfo(np.float32).max
    u = np.clip(np.where(bad, np.float32(0), x32), -fmax, fmax) - sub[:, None]   # (nmx_clean: +-inf are +-FLT_MAX)
    assert u.dtype == np.float32
    return np.where(bad, -sub[:, None], u).astype(np.float64)


def windows_of(y: np.ndarray, starts: np.ndarray, window: int) -> np.ndarray:
    """[C, T] -> [hops, C, window]"""
    idx = np.asarray(starts)[:, None] + np.arange(window)[None, :]
    return y[:, idx].transpose(1, 0, 2)


def reref_check(case: str, what: str, got: np.ndarray, u: np.ndarray, R: np.ndarray, kernel: str, d_in: np.ndarray,
                starts: np.ndarray, window: int, only_b: bool = False, gain: float = 1.0) -> dict:
    """Every sample of `got` [hops, C, window] against R @ u + D under the limits (a) and (b) of the module docstring.
    -> {"a": worst err / limit, "b": ...}."""
    Cin = u.shape[0]
    Rb = np.asarray(R, np.float64)
    Ra, O = uploaded(Rb, kernel)
    D = (Rb @ d_in) * gain
    f64 = Cin * F2_52 * (np.abs(Rb) @ np.abs(d_in)) * abs(gain)
    au = np.abs(u)
    got = np.asarray(got, np.float64)
    assert got.shape == (len(starts), R.shape[0], window), got.shape
    assert np.isfinite(got).all(), f"{case} {what}: non-finite samples"
    out = {}
    for tag, Rm, coef in (("a", Ra, 0.0), ("b", Rb, EPS32 * ((np.abs(Rb) + O) @ au))):
        if tag == "a" and only_b:
            continue
        want = Rm @ u
        full = want + D[:, None]
        lim = (0.5 * EPS32 * np.abs(want) * (1 + 1e-6) + Cin * F2_52 * (np.abs(Rm) @ au) + F2_149 + coef
               + f64[:, None] + F2_52 * np.abs(full))
        err = np.abs(got - windows_of(full, starts, window))
        ratio = err / windows_of(lim, starts, window)
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        out[tag] = float(ratio[k])
        REPORT.add(case, f"{what} ({tag})", ratio[k], err.size)
        assert ratio[k] <= 1.0, (f"{case} {what} limit ({tag}): hop {k[0]} row {k[1]} sample {k[2]}: got {got[k]!r}, want "
                                 f"{windows_of(full, starts, window)[k]!r}: error {err[k]:.3e} is {ratio[k]:.3f} limits; "
                                 f"{int((ratio > 1).sum())} of {err.size} samples beyond")
    return out


def reref_engine(lib, env: dict, R, window: int = W, notch=None, C: int | None = None):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.segment_length_features_ms = window * 1000.0 / SFREQ
    n = R.shape[0] if R is not None else C
    return fir.build_engine(lib, env, s, [f"ch{i}" for i in range(n)], SFREQ, features=["return_raw"], ref_matrix=R,
                            notch_taps=notch, window=window)


def _run_outlets(lib, case, what, eng, x, R, kernel, hops, only_b, expect_split):
    """One recording through the tap (the stream's range) and through preprocess_window (first and last window), each on a
    plan that has seen nothing."""
    starts = starts_of(hops)
    eng.reset_state()
    _, mask, pre = eng.process_batch(x, starts, want_nan_mask=True, tap=True)
    fir.assert_kernels(lib, case, eng, {1: kernel})
    d_in = eng.offsets()[0]
    assert bool(d_in.any()) == expect_split, f"{case} {what}: the plan learned {d_in}"
    assert np.array_equal(mask, windows_of(np.isnan(x), starts, W).any(axis=2)), f"{case} {what}: NaN mask"
    worst = reref_check(case, f"{what} tap", pre, split_u(x, d_in), R, kernel, d_in, starts, W, only_b)
    for a in (int(starts[0]), int(starts[-1])):
        eng.reset_state()
        xw = np.ascontiguousarray(x[:, a:a + W])
        got = eng.preprocess_window(xw.astype(np.float64))
        fir.assert_kernels(lib, case, eng, {1: kernel})
        d_in = eng.offsets()[0]
        assert bool(d_in.any()) == expect_split, f"{case} {what}: the plan learned {d_in} from one window"
        w2 = reref_check(case, f"{what} window", got[None], split_u(xw, d_in), R, kernel, d_in, np.zeros(1, np.int64), W, only_b)
        worst = {k: max(v, w2[k]) for k, v in worst.items()}
    return worst


def reref_case(lib, name: str) -> dict:
    """Noise, noise on offsets (the split engaged), the same with NMX_DC_SPLIT=0, impulses -- through both outlets.
    -> {variant: {"a": worst ratio, "b": ...}}."""
    make, env, kernel, hops = REREF_CASES[name]
    R = make()
    assert front_kernel(R, env) == kernel, f"{name}: the restated choice is {front_kernel(R, env)}"
    Cin = R.shape[1]
    T = W + (hops - 1) * HOP
    assert T % 64 and T % 256
    seed = 1000 + sum(map(ord, name))
    out = {}
    eng = reref_engine(lib, env, R)
    try:
        out["noise"] = _run_outlets(lib, name, "noise", eng, recording(Cin, T, "noise", seed), R, kernel, hops, False, False)
        if hops == LONG_HOPS:   # the same recording over a range <= 4096: NW = 16 over a chunk
            out["short"] = _run_outlets(lib, name, "short", eng, recording(Cin, T, "noise", seed), R, kernel, SHORT_HOPS, False, False)
        out["offsets"] = _run_outlets(lib, name, "offsets", eng, recording(Cin, T, "noise", seed, offsets=True), R, kernel, hops,
                                      False, True)
        out["impulse"] = _run_outlets(lib, name, "impulse", eng, recording(Cin, T, "impulse", seed), R, kernel, hops, False, False)
    finally:
        eng.close()
    eng = reref_engine(lib, dict(env, NMX_DC_SPLIT="0"), R)
    try:
        out["nosplit"] = _run_outlets(lib, name, "nosplit", eng, recording(Cin, T, "noise", seed, offsets=True), R, kernel, hops,
                                      True, False)
    finally:
        eng.close()
        REPORT.flush(name)
    return out


def car_bytes_case(lib, C: int) -> None:
    """The average over NW = 4 waves (a 4600-sample range), over NW = 16 (a 3100-sample range of the same recording) and
    in preprocess_window (NW = 16): the same bytes.  No notch, NMX_DC_SPLIT=0, input without offsets."""
    name = f"car_bytes_c{C}"
    R = car_matrix(C)
    T = W + (LONG_HOPS - 1) * HOP
    assert car_waves(C, T) == 4 and car_waves(C, W + (SHORT_HOPS - 1) * HOP) == 16 and car_waves(C, W) == 16
    x = recording(C, T, "noise", 77 + C)
    eng = reref_engine(lib, {"NMX_DC_SPLIT": "0"}, R)
    try:
        _, long_ = eng.process_batch(x, starts_of(LONG_HOPS), tap=True)
        fir.assert_kernels(lib, name, eng, {1: CAR})
        _, short = eng.process_batch(x, starts_of(SHORT_HOPS), tap=True)
        assert long_.dtype == short.dtype == np.float32 and not eng.offsets()[1].any()
        fir.same_bytes(long_[:SHORT_HOPS], short, f"{name}: the 4600-sample range against the 3100-sample range")
        for h in range(LONG_HOPS):
            one = eng.preprocess_window(x[:, h * HOP:h * HOP + W].astype(np.float64))
            fir.same_bytes(long_[h].astype(np.float64), one, f"{name}: hop {h} of the stream against preprocess_window")
        REPORT.add(name, "bytes", 0.0, long_.size)
    finally:
        eng.close()
        REPORT.flush(name)


def chunks_case(lib, name: str) -> None:
    """Three chunks of four hops (lo > 0 in launch_front) store the bytes of the one-chunk run, offsets carried."""
    make, env, kernel, hops = REREF_CASES[name]
    R = make()
    x = recording(R.shape[1], W + (hops - 1) * HOP, "noise", 5, offsets=True)
    got = []
    for e in ({}, {"NMX_CHUNK_WINDOWS": "4"}):
        eng = reref_engine(lib, dict(env, **e), R)
        try:
            _, mask, pre = eng.process_batch(x, starts_of(hops), want_nan_mask=True, tap=True)
            fir.assert_kernels(lib, name, eng, {1: kernel})
            assert eng.offsets()[0].any()
            got.append((np.asarray(pre, np.float64), mask))
        finally:
            eng.close()
    fir.same_bytes(got[0][0], got[1][0], f"chunks of {name}")
    assert np.array_equal(got[0][1], got[1][1])


# ---- 1. the shift -------------------------------------------------------------------------------------------------------
SHIFT_W, SHIFT_C, SHIFT_HOPS = 1000, 4, 4
SHIFT_RAGGED = np.array([0, 3, 3, 7])


def shift_case(lib) -> dict:
    """No matrix, the notch on, offsets of 1e5 times the signal: the learned split runs in nmx_kern_shift, a NaN becomes -d.
    Reference: u, then the FIR probes' float64 odd-reflection convolution; limit and yardstick: theirs (M = 2048)."""
    from py_neuromodulation_amd import fir_design

    name = "shift_c4"
    notch = fir_design.notch_bank(SFREQ, 50)
    gain = float(np.sum(np.asarray(notch, np.float64)))
    starts = np.arange(SHIFT_HOPS, dtype=np.int64) * HOP + SHIFT_RAGGED
    T = int(starts[-1]) + SHIFT_W + 5
    x = recording(SHIFT_C, T, "noise", 31, offsets=True, window=SHIFT_W)
    eng = reref_engine(lib, {}, None, SHIFT_W, notch, SHIFT_C)
    out = {}
    try:
        def check(what, got, xin):
            d_in, d_pre = eng.offsets()
            assert d_in.all(), f"{name} {what}: the plan learned {d_in}"
            assert np.abs(d_pre - d_in * gain).max() <= 1e-12 * np.abs(d_in).max()
            u = split_u(xin, d_in)
            n = got.shape[0] * SHIFT_C
            rows = u if what == "window" else windows_of(u, starts, SHIFT_W).reshape(n, SHIFT_W)
            y64 = fir.conv64(rows, notch, odd=True)
            y32 = fir.conv32(rows.astype(np.float32), notch, 2048, odd=True)
            g = (np.asarray(got, np.float64) - d_pre[None, :, None]).reshape(n, SHIFT_W)
            out[what] = fir.check_rows(name, what, g, y64, y32, rows, ~rows.any(axis=1))   # (a constant row: u = 0, output +-0)

        _, mask, pre = eng.process_batch(x, starts, want_nan_mask=True, tap=True)
        if lib is None:
            assert fir.ran(eng.kernels(1), SHIFT), f"{name}: stage 1 ran {eng.kernels(1)!r}"
        assert np.array_equal(mask, windows_of(np.isnan(x), starts, SHIFT_W).any(axis=2))
        check("tap", pre, x)
        eng.reset_state()
        xw = np.ascontiguousarray(x[:, :SHIFT_W])
        got = eng.preprocess_window(xw.astype(np.float64))
        if lib is None:
            assert fir.ran(eng.kernels(1), SHIFT), f"{name}: stage 1 ran {eng.kernels(1)!r}"
        check("window", got[None], xw)
    finally:
        eng.close()
        fir.REPORT.flush(name)
    return out


# ---- 2. learned constants and the NaN mask ------------------------------------------------------------------------------
def learned_rule(first: np.ndarray) -> np.ndarray:
    """dc_prepare restated: per row of the first window [C_in, W] (float32), over the finite samples, summed in order in
    float64: the mean as fp32 where |mean| > 4 x the spread about it, else 0."""
    out = np.zeros(len(first))
    for j, row in enumerate(np.asarray(first, np.float32).astype(np.float64)):
        ok = row[np.isfinite(row)]
        s = 0.0
        for v in ok:
            s += float(v)
        m = s / len(ok) if len(ok) else 0.0
        q = 0.0
        for v in ok:
            q += (float(v) - m) * (float(v) - m)
        sd = float(np.sqrt(q / len(ok))) if len(ok) else 0.0
        mf = np.float32(m)
        out[j] = float(mf) if np.isfinite(mf) and abs(m) > 4.0 * sd else 0.0
    return out


def learned_recording(hops: int = HOPS) -> np.ndarray:
    """float32 [5, T]: rows at 3.9 and 4.1 times their spread in the first window, a row with NaN and inf there (its level
    at 1e5 spreads), an all-NaN first window, a zero row."""
    T = W + (hops - 1) * HOP
    z = np.random.default_rng(9).standard_normal((5, T))
    z[:2] -= z[:2, :W].mean(axis=1, keepdims=True)
    z[:2] /= z[:2, :W].std(axis=1, keepdims=True)
    x = np.zeros((5, T))
    x[0] = SIGMA * (z[0] + 3.9)
    x[1] = SIGMA * (z[1] - 4.1)
    x[2] = SIGMA * (z[2] + 1e5)
    x[3] = SIGMA * (z[3] + 1e5)
    x = x.astype(np.float32)
    x[2, [0, 17, W - 1]] = np.nan
    x[2, [5, 64]] = [np.inf, -np.inf]
    x[3, :W] = np.nan
    return x


def learned_case(lib) -> None:
    x = learned_recording()
    first = x[:, :W].astype(np.float64)
    fin = np.where(np.isfinite(first), first, np.nan)
    level = np.abs(np.nanmean(fin[:3], axis=1)) / np.nanstd(fin[:3], axis=1)
    assert 3.85 < level[0] < 3.95 and 4.05 < level[1] < 4.15 and level[2] > 1e4, level
    want = learned_rule(x[:, :W])
    assert want[0] == 0 and want[1] != 0 and want[2] != 0 and want[3] == 0 and want[4] == 0, want
    R = car_matrix(5)
    eng = reref_engine(lib, {}, R)
    try:
        _, pre = eng.process_batch(x, starts_of(HOPS), tap=True)
        d_in = eng.offsets()[0]
        assert d_in.tobytes() == want.tobytes(), f"learned {d_in!r}, the rule restated {want!r}"
        # (the constants stay: the batch's later windows -- row 3 is finite there -- are held to the same limits)
        reref_check("learned", "tap", pre, split_u(x, d_in), R, CAR, d_in, starts_of(HOPS), W)
        eng.reset_state()
        one = []
        for a in starts_of(HOPS):
            one.append(np.asarray(eng.process_batch(x, np.array([a]), tap=True)[1], np.float64))
            assert eng.offsets()[0].tobytes() == want.tobytes(), "learned once: a later batch changed the constants"
        fir.same_bytes(np.asarray(pre, np.float64), np.concatenate(one), "12 hops in one batch against 12 one-hop batches")
    finally:
        eng.close()
        REPORT.flush("learned")


def nanmask_case(lib) -> None:
    """A NaN at start - 1, start, start + 63, start + 64, start + W - 1, start + W of hop 2, each on its own input row; ragged
    starts; a 5 x 7 structured matrix (C_in != C)."""
    Cin, hops = 7, 6
    R = np.stack([_taps_row(Cin, {i: 1.0, i + 1: -1.0}) for i in range(5)])
    starts = starts_of(hops) + np.array([0, 3, 3, 7, 7, 8])
    T = int(starts[-1]) + W + 3
    x = (np.random.default_rng(4).standard_normal((Cin, T)) * SIGMA).astype(np.float32)
    a = int(starts[2])
    for j, t in enumerate((a - 1, a, a + 63, a + 64, a + W - 1, a + W)):
        x[j, t] = np.nan
    eng = reref_engine(lib, {}, R)
    try:
        _, mask, pre = eng.process_batch(x, starts, want_nan_mask=True, tap=True)
        fir.assert_kernels(lib, "nanmask", eng, {1: STRUCT})
        want = windows_of(np.isnan(x), starts, W).any(axis=2)
        assert mask.shape == (hops, Cin) and mask.dtype == bool
        assert np.array_equal(mask, want), f"mask {mask.astype(int).tolist()}, want {want.astype(int).tolist()}"
        assert not want[:, 6].any() and want[:, :6].any(axis=0).all()
        assert set(want[2].nonzero()[0]) == {1, 2, 3, 4} and want[1, 0] and want[3, 5], "the placements no longer straddle hop 2"
        reref_check("nanmask", "tap", pre, split_u(x, np.zeros(Cin)), R, STRUCT, np.zeros(Cin), starts, W)
    finally:
        eng.close()
        REPORT.flush("nanmask")


# ---- 3. resampler -------------------------------------------------------------------------------------------------------
def _al4(n: int) -> int:
    return (n + 3) & ~3


def resample_plan(sf_old: float, sf_new: float, Wr: int, forced: bool = False) -> dict:
    """build_resample's arithmetic restated (Python's round is round-half-even, as nearbyint)."""
    ratio = float(sf_new) / float(sf_old)
    W_new = int(round(ratio * Wr))
    n_pad = 1
    while n_pad < Wr + min(Wr // 8, 100) * 2:
        n_pad <<= 1
    pad_l = (n_pad - Wr) // 2
    n_new = max(int(round(ratio * n_pad)), 1)
    crop_l = int(round(ratio * pad_l))
    assert crop_l + W_new <= n_new
    inv_full = n_new & 1
    use_len = min(n_new, n_pad)
    n_inv = n_new if inv_full else n_new // 2

    def fits(n_fwd, keep_x):
        cmax = max(n_fwd, n_inv)
        return ((_al4(Wr) if keep_x else 0) + 2 * _al4(2 * cmax) + _al4(2 * (n_new // 2 + 1))) * 4 <= 160 * 1024

    q = m = 0
    if not (n_pad <= 8192 and fits(n_pad // 2, 1) and not forced):
        m = min(2048, n_pad // 2)
        assert fits(m, 0)
        q = n_pad // m
    return dict(ratio=ratio, W=Wr, W_new=W_new, n_pad=n_pad, pad_l=pad_l, pad_r=n_pad - Wr - pad_l, n_new=n_new, crop_l=crop_l,
                inv_full=inv_full, nyq_bin=use_len // 2 if use_len % 2 == 0 else -1, nyq_scale=2.0 if n_new < n_pad else 0.5,
                scale=np.float32(ratio / n_new), poly_q=q, poly_m=m)


def _pad_rows(x: np.ndarray, p: dict) -> np.ndarray:
    """The odd ("reflect_limited") reflection about both ends in the dtype of `x`, zeros beyond W - 1 samples."""
    Wr, pl, pr = p["W"], p["pad_l"], p["pad_r"]
    two = x.dtype.type(2)
    zl = np.zeros((len(x), max(pl - Wr + 1, 0)), x.dtype)
    zr = np.zeros((len(x), max(pr - Wr + 1, 0)), x.dtype)
    xe = np.concatenate([zl, two * x[:, :1] - x[:, pl:0:-1], x, two * x[:, -1:] - x[:, -2:-pr - 2:-1], zr], axis=1)
    assert xe.shape[1] == p["n_pad"] and xe.dtype == x.dtype
    return xe


def resample64(x: np.ndarray, p: dict) -> np.ndarray:
    """mne.filter.resample (fft, boxcar, reflect_limited) restated step by step in float64 on rows [.., W]."""
    import scipy.fft as sf

    x = np.atleast_2d(np.asarray(x, np.float64))
    X = sf.rfft(_pad_rows(x, p), axis=-1)
    n_new = p["n_new"]
    Xn = np.zeros((len(x), n_new // 2 + 1), np.complex128)
    k = min(n_new // 2, p["n_pad"] // 2) + 1
    Xn[:, :k] = X[:, :k]
    if p["nyq_bin"] >= 0:
        Xn[:, p["nyq_bin"]] *= p["nyq_scale"]
    y = sf.irfft(Xn, n=n_new, axis=-1) * p["ratio"]
    return y[:, p["crop_l"]:p["crop_l"] + p["W_new"]]


def _roots(n: int, count: int, sign: float, cdt) -> np.ndarray:
    """exp(sign 2 pi i j / n), j < count: computed in float64, the parts rounded to the real type of `cdt` (the plan's tables)."""
    a = sign * 2.0 * np.pi * np.arange(count) / n
    rdt = np.float32 if cdt == np.complex64 else np.float64
    return (np.cos(a).astype(rdt) + 1j * np.sin(a).astype(rdt)).astype(cdt)


def resample_chain(x: np.ndarray, p: dict, rdt) -> np.ndarray:
    """The kernel's chain at the plan's transform lengths in the real type `rdt`: the padded row packed as n_pad / 2 complex
    points, one complex transform, the split into the bins of the real transform with a table of 2 n_pad / 2 roots -- or, in
    the polyphase form, q / 2 transforms of m points, two components each, split by their Hermitian symmetry and summed with
    a table of n_pad roots --, the kept bins and the Nyquist scale, the pre-twiddle and one complex transform of n_new / 2
    points back (n_new odd: the Hermitian extension and n_new points), `scale`, the crop.  Every intermediate array has the
    type `rdt` / its complex twin.  rdt = float32: the yardstick.  rdt = float64: the same value as resample64 (the CPU test
    ties them at 1e-12)."""
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
    if q == 0:
        Z = sf.fft((xe[:, 0::2] + j1 * xe[:, 1::2]).astype(cdt), axis=-1)
        Zk, Zc = Z[:, k % nh], np.conj(Z[:, (nh - k) % nh])
        Xn[:, :kuse + 1] = half * (Zk + Zc) - j1 * _roots(N, kuse + 1, -1.0, cdt)[None, :] * (half * (Zk - Zc))
    else:
        tab = _roots(N, N, -1.0, cdt)
        for r in range(0, q, 2):
            Z = sf.fft((xe[:, r::q] + j1 * xe[:, r + 1::q]).astype(cdt), axis=-1)
            assert Z.shape[1] == m
            Zk, Zc = Z[:, k % m], np.conj(Z[:, (m - k % m) % m])
            f0, f1 = half * (Zk + Zc), -j1 * (half * (Zk - Zc))
            Xn[:, :kuse + 1] += tab[(k * r) % N][None, :] * f0 + tab[(k * (r + 1)) % N][None, :] * f1
    assert Xn.dtype == cdt
    if p["nyq_bin"] >= 0:
        Xn[:, p["nyq_bin"]] *= rdt(p["nyq_scale"])
    Xn[:, 0] = Xn[:, 0].real   # (C2R: the imaginary part of the DC bin does not contribute)
    if not p["inv_full"]:
        mh = kmax
        Xn[:, mh] = Xn[:, mh].real
        kk = np.arange(mh)
        Xk, Xc = Xn[:, kk], np.conj(Xn[:, mh - kk])
        z = (Xk + Xc) + j1 * _roots(n_new, mh, +1.0, cdt)[None, :] * (Xk - Xc)
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


def resample32(x: np.ndarray, p: dict) -> np.ndarray:
    """The yardstick: the chain in single precision (module docstring)."""
    return resample_chain(x, p, np.float32)


POLY = {"NMX_RESAMPLE_POLY": "1"}
# name -> (sf_old, sf_new, W, env, class asserted on resample_plan: {field: value}, emulator tier)
RESAMPLE_CASES = {
    "down_even": (2000.0, 1000.0, 2000, {}, dict(n_pad=4096, n_new=2048, inv_full=0, nyq_bin=1024, nyq_scale=2.0, poly_q=0), True),
    "down_odd": (1375.0, 500.0, 1375, {}, dict(n_pad=2048, pad_l=336, pad_r=337, n_new=745, inv_full=1, nyq_bin=-1, poly_q=0), True),
    "up_even": (1000.0, 2000.0, 500, {}, dict(n_pad=1024, n_new=2048, inv_full=0, nyq_bin=512, nyq_scale=0.5, poly_q=0), True),
    "up_odd": (1024.0, 1125.0, 800, {}, dict(n_pad=1024, n_new=1125, inv_full=1, nyq_bin=512, nyq_scale=0.5, poly_q=0), True),
    "tiny_4": (1000.0, 2000.0, 4, {}, dict(n_pad=4, pad_l=0, pad_r=0, n_new=8, W_new=8, nyq_bin=2, nyq_scale=0.5, poly_q=0), True),
    "tiny_9": (2000.0, 1000.0, 9, {}, dict(n_pad=16, pad_l=3, pad_r=4, n_new=8, W_new=4, crop_l=2, poly_q=0), True),
    "one_8192": (7000.0, 1000.0, 7000, {}, dict(n_pad=8192, n_new=1170, inv_full=0, nyq_bin=585, poly_q=0), True),
    "one_4k": (4000.0, 1000.0, 4000, {}, dict(n_pad=8192, n_new=2048, inv_full=0, nyq_bin=1024, poly_q=0), True),
    "poly_forced_40": (2000.0, 1000.0, 40, POLY, dict(n_pad=64, n_new=32, inv_full=0, poly_q=2, poly_m=32), True),
    "poly_forced_4k": (4000.0, 1000.0, 4000, POLY, dict(n_pad=8192, n_new=2048, inv_full=0, poly_q=4, poly_m=2048), True),
    "poly_8k": (8000.0, 1000.0, 8000, {}, dict(n_pad=16384, n_new=2048, inv_full=0, poly_q=8, poly_m=2048), True),
    "poly_24k": (24000.0, 1000.0, 24000, {}, dict(n_pad=32768, n_new=1365, inv_full=1, nyq_bin=-1, poly_q=16, poly_m=2048), True),
    "poly_44k": (44100.0, 1000.0, 44100, {}, dict(n_pad=65536, n_new=1486, inv_full=0, nyq_bin=743, poly_q=32, poly_m=2048), True),
    "tie_down": (2000.0, 1000.0, 1001, {}, dict(n_pad=2048, pad_l=523, crop_l=262, W_new=500, n_new=1024, poly_q=0), True),
    "tie_up": (2000.0, 1000.0, 1003, {}, dict(n_pad=2048, pad_l=522, crop_l=261, W_new=502, n_new=1024, poly_q=0), True),
}
EMU_RESAMPLE = [n for n, c in RESAMPLE_CASES.items() if c[5]]
RESAMPLE_C = 3


def case_plan(name: str) -> dict:
    sf_old, sf_new, Wr, env, cls, _ = RESAMPLE_CASES[name]
    p = resample_plan(sf_old, sf_new, Wr, forced=bool(env))
    for k, v in cls.items():
        assert p[k] == v, f"{name}: restated {k} = {p[k]}, the case table says {v}"
    return p


def resample_positions(p: dict, every: bool = False) -> list[int]:
    Wr, pl, pr, q, m = p["W"], p["pad_l"], p["pad_r"], p["poly_q"], p["poly_m"]
    if every:
        return list(range(Wr))
    s = {0, 1, 2, pl - 1, pl, pl + 1, Wr - 2 - pr, Wr - 1 - pr, Wr - pr, Wr - 2, Wr - 1, Wr // 2}
    if q:
        s |= set(range(2 * q + 2))
        # the padded indices q j + r of j = 0, 1 and of j = m - 2, m - 1 (the first and last points of every component) lie in
        # the pads: the window samples whose reflections land there
        N = p["n_pad"]
        s |= {pl - i for i in range(2 * q + 2)} | {2 * (Wr - 1) + pl - i for i in range(N - 2 * q - 1, N)}
        s |= {q * j + r - pl for j in (m - 2, m - 1) for r in range(q)}   # (inside the window where the pads are short)
    return sorted(t for t in s if 0 <= t < Wr)


def resample_inputs(name: str, p: dict) -> list[tuple[str, np.ndarray]]:
    """[(class, float32 [C, W])]"""
    Wr, C = p["W"], RESAMPLE_C
    out = []
    pos = resample_positions(p, every=name == "poly_forced_40")
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
        if not np.abs(x[1]).max() > 1e-6:   # (the window's own Nyquist: the sine is zero at every sample)
            x[1] = 0.0
        x[2] = x[0] + x[1]
        out.append(("tone", x.astype(np.float32)))
    return out


def check_resampled(case: str, cls: str, got, y64, y32, x_rows, p: dict) -> float:
    """Every row of `got` within FACTOR yardsticks of y64; rows without input exactly 0 (fir.check_rows' rule, this module's
    FACTORS).  The yardstick's cap is relative to the row's scale AS THE TRANSFORMS SEE IT: the odd reflection of a row that
    ends on a unit impulse is a pad of 2s, a thousand samples long -- max(rms(x_row), rms(padded row), max|y64|).
    -> worst ratio."""
    got = np.asarray(got, np.float64).reshape(y64.shape)
    assert np.isfinite(got).all(), f"{case} {cls}: non-finite samples"
    e32 = np.abs(y32.astype(np.float64) - y64).max(axis=-1)
    scale = fir.rms(x_rows)
    floor = np.maximum(e32, EPS32 * scale)
    seen = np.maximum(scale, fir.rms(_pad_rows(np.atleast_2d(np.asarray(x_rows, np.float64)), p)))
    cap = YARD_CAP * EPS32 * np.maximum(seen, np.abs(y64).max(axis=-1))
    yard = float(np.max(e32 / np.maximum(cap, 1e-300)) * YARD_CAP)
    assert np.all(e32 <= cap), (f"{case} {cls}: the single-precision yardstick is {yard:.1f} eps32 of the row's scale from the "
                                f"float64 reference: one of the two is wrong")
    err = np.abs(got - y64).max(axis=-1)
    live = floor > 0
    assert np.all(err[~live] == 0), f"{case} {cls}: output on rows without input"
    ratio = np.zeros(len(err))
    ratio[live] = err[live] / floor[live]
    factor = FACTORS.get((case, cls), FACTOR)
    worst = int(np.argmax(ratio))
    REPORT.add(case, cls, ratio.max(), got.size, f"yardstick e32 {yard:5.2f} eps32")
    assert ratio.max() <= factor, (f"{case} {cls}: row {worst} of {len(err)}: sample {int(np.argmax(np.abs(got - y64)[worst]))}: "
                                   f"error {err[worst]:.3e} is {ratio[worst]:.2f} yardsticks (e32 {e32[worst]:.3e}, eps32 rms "
                                   f"{EPS32 * scale[worst]:.3e}); {int((ratio > factor).sum())} rows beyond {factor:g}")
    return float(ratio.max())


def resample_engine(lib, env, sf_old, sf_new, Wr, C, notch=None):
    from py_neuromodulation_amd import NMSettings

    return fir.build_engine(lib, env, NMSettings.get_default(), [f"c{i}" for i in range(C)], sf_new, features=["return_raw"],
                            resample_from=sf_old, raw_window=Wr, window=int(round(sf_new / sf_old * Wr)), notch_taps=notch)


def resample_case(lib, name: str) -> dict:
    """Impulses, noise and the Nyquist tone of resampler case `name` through preprocess_window.  -> {class: worst ratio}."""
    sf_old, sf_new, Wr, env, _, _ = RESAMPLE_CASES[name]
    p = case_plan(name)
    eng = resample_engine(lib, env, sf_old, sf_new, Wr, RESAMPLE_C)
    worst: dict = {}
    try:
        assert (eng.W_in, eng.W) == (Wr, p["W_new"]), f"{name}: the plan's windows {eng.W_in} -> {eng.W}"
        for cls, x in resample_inputs(name, p):
            got = eng.preprocess_window(x.astype(np.float64))
            fir.assert_kernels(lib, name, eng, {1: RESAMPLE})
            xc = np.nan_to_num(x)
            r = check_resampled(name, cls, got, resample64(xc, p), resample32(xc, p), xc, p)
            worst[cls] = max(worst.get(cls, 0.0), r)
    finally:
        eng.close()
        REPORT.flush(name)
    return worst


BATCH_C, BATCH_HOPS, BATCH_W, BATCH_HOP = 5, 9, 2000, 200
BATCH_RAGGED = np.array([0, 0, 3, 3, 3, 7, 7, 7, 8])


def batch_resample_case(lib, with_notch: bool) -> float:
    """2000 -> 1000, 5 channels, 9 ragged hops through the tap: the resampler alone, or behind the notch at the raw rate."""
    from py_neuromodulation_amd import fir_design

    name = "batch_notch_resample" if with_notch else "batch_resample"
    p = resample_plan(2000.0, 1000.0, BATCH_W)
    notch = fir_design.notch_bank(2000.0, 50) if with_notch else None
    starts = np.arange(BATCH_HOPS, dtype=np.int64) * BATCH_HOP + BATCH_RAGGED
    T = int(starts[-1]) + BATCH_W + 7
    x = np.random.default_rng(12).standard_normal((BATCH_C, T)) * SIGMA
    x[1] += 300.0
    x[3] *= 1e-3
    x = x.astype(np.float32)
    x[2, int(starts[4]) + 5] = np.nan
    eng = resample_engine(lib, {}, 2000.0, 1000.0, BATCH_W, BATCH_C, notch)
    try:
        _, mask, pre = eng.process_batch(x, starts, want_nan_mask=True, tap=True)
        names = eng.kernels(1) if lib is None else ""
        assert lib is not None or fir.ran(names, RESAMPLE), names
        if with_notch and lib is None:
            assert fir.ran(names, "nmx_kern_bank"), names
        assert pre.shape == (BATCH_HOPS, BATCH_C, p["W_new"]) and not eng.offsets()[1].any()
        assert np.array_equal(mask, windows_of(np.isnan(x), starts, BATCH_W).any(axis=2))
    finally:
        eng.close()
    n = BATCH_HOPS * BATCH_C
    rows = windows_of(np.nan_to_num(x), starts, BATCH_W).reshape(n, BATCH_W)
    a64, a32 = rows.astype(np.float64), rows
    if with_notch:
        a64 = fir.conv64(a64, notch, odd=True)
        a32 = fir.conv32(rows, notch, 4000, odd=True)
    r = check_resampled(name, "noise", np.asarray(pre, np.float64).reshape(n, -1), resample64(a64, p), resample32(a32, p), a64, p)
    eng = resample_engine(lib, {}, 2000.0, 1000.0, BATCH_W, BATCH_C, notch)   # a fresh plan
    try:
        for h, a in enumerate(starts):
            one = eng.preprocess_window(x[:, a:a + BATCH_W].astype(np.float64))
            fir.same_bytes(np.asarray(pre[h], np.float64), one, f"{name}: hop {h} of the batch against preprocess_window")
    finally:
        eng.close()
        REPORT.flush(name)
    return r
