// nmx_k_nolds.h -- sample entropy of the nolds feature (features/nolds.py): one workgroup per (window, series, channel).
//
// Reference arithmetic (Nolds.calc_nolds -> nolds.sampen with its defaults: emb_dim = 2, lag = 1, Chebyshev distance, open
// comparison), for a series x of N samples:
//   the value is 0 when x.sum() is exactly zero; otherwise, with tol = factor * std(x, ddof) and the T = N - 2 templates
//   i = 0 .. T - 1 (the same rows for both lengths),
//     B = #{i < j : max(|x_i - x_j|, |x_{i+1} - x_{j+1}|) < tol}
//     A = #{i < j : max(|x_i - x_j|, |x_{i+1} - x_{j+1}|, |x_{i+2} - x_{j+2}|) < tol}
//   -ln(A / B) when both counts are positive, +inf when only A is zero, NaN when both are (a constant series: tol = 0;
//   N < 4: no pair of templates).
// `factor` (nolds: 0.1164 (0.5627 ln 2 + 1.3334)) and `ddof` come from the plan description: what the host could have
// recalled wrongly about nolds sits in one place there, not in this kernel.
//
// The series sits in LDS (a 40 000-sample window: 160 000 of the CU's 163 840 bytes).  Mean and variance in float64, two
// passes; tol is rounded once to float32 and every comparison is a float32 one, on float32 differences of the float32
// samples.  The pairs are walked along the diagonals j - i = k, k = 1 .. T - 1: a lane owns a diagonal and carries
// |x_{i+1} - x_{i+1+k}| and |x_{i+2} - x_{i+2+k}| forward in registers, so a pair costs one new absolute difference, two
// maxima and two compare-adds; x[i + 2] is an LDS broadcast, x[i + 2 + k] a unit-stride read across the lanes.  Diagonal k
// holds T - k pairs: a lane takes k and T - k together (T pairs each; T / 2 alone when T is even), so every lane of every
// wave walks the same number of pairs.  Counts are uint32 (T (T - 1) / 2 < 2^32 up to N = 40 000), reduced by the wave
// reduction and one LDS pass.  A constant offset the engine carries next to the window (dcf, nmx_engine_dc.inc) changes
// neither a difference nor the variance; the sum takes it in float64.
//
// Included by nmx_engine.inc: the HIP build gets the kernel and its launcher, the host emulator (NMX_HOST_EMU) a launcher
// that loops the same item code.
#pragma once

#include "nmx_device.h"

#define NMX_NOLDS_MAX_N 40000   // series length bound: the series + 64 floats of reduction scratch in 160 KiB of LDS

struct NmxNoldsArgs {
  const float* x;           // pre-processed windows (as NmxTimeOscArgs): the "raw" series
  long long ch_stride;
  long long win_stride;
  const long long* starts;
  int clean_on_load;
  const float* dcf;         // [n_channels] constant the windows were split from, or NULL (enters the sum only)
  const float* yb;          // [n_windows][n_channels][n_band][W] band series from the FIR stage (clean), or NULL
  float* out;               // [n_windows][n_outputs]
  int n_outputs;
  int n_channels;
  int W;                    // samples per series
  int raw;                  // series 0 is the window itself
  int n_band;               // band series behind it
  double tol_factor;
  int ddof;
  NmxCols cols;             // column = base + ch * ch_stride + series * a_stride
  unsigned* probe;          // [item][4]: A, B, bits of tol, sum == 0 -- or NULL
  float* series_out;        // [item][W]: the series as the walk read it (cleaned samples / band series) -- or NULL
  int lds_floats;
};

#ifdef NMX_HOST_EMU
NMX_DEV double nmx_nolds_sum_d(double v, float*) { return v; }
NMX_DEV unsigned nmx_nolds_sum_u(unsigned v, float*) { return v; }
NMX_DEV float nmx_nolds_max(float a, float b) { return a > b ? a : b; }
#else
// float64 sum over the workgroup: wave butterfly, then one LDS pass (red: 16 doubles)
NMX_DEV double nmx_nolds_sum_d(double v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int nw = (NMX_NT + 63) >> 6;
  if (nw == 1) return v;
  double* r = (double*)red;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = r[0];
  for (int i = 1; i < nw; ++i) t += r[i];
  return t;
}
NMX_DEV unsigned nmx_nolds_sum_u(unsigned v, float* red) {
  return nmx_block_reduce(v, 0u, red, [](unsigned a, unsigned b) { return a + b; });
}
NMX_DEV float nmx_nolds_max(float a, float b) { return nmx_vmax(a, b); }   // (the samples are finite: no NaN to order)
#endif

// the pairs (i, i + k), i = 0 .. T - k - 1, of diagonal k
NMX_DEV void nmx_nolds_diag(const float* xs, int T, int k, float tol, unsigned& a, unsigned& b) {
  const float* xk = xs + k;
  float d1 = fabsf(xs[0] - xk[0]), d2 = fabsf(xs[1] - xk[1]);
  const int n = T - k;
  for (int i = 0; i < n; ++i) {
    const float d3 = fabsf(xs[i + 2] - xk[i + 2]);   // (i + 2 + k <= T + 1 = N - 1)
    const float m2 = nmx_nolds_max(d1, d2);
    b += m2 < tol ? 1u : 0u;
    a += nmx_nolds_max(m2, d3) < tol ? 1u : 0u;
    d1 = d2;
    d2 = d3;
  }
}

// item = (w * n_series + s) * n_channels + c
NMX_DEV void nmx_nolds_item(const NmxNoldsArgs& A, int item, float* smem) {
  const int n_series = A.raw + A.n_band, C = A.n_channels, N = A.W;
  const int c = item % C, s = (item / C) % n_series, w = item / (C * n_series);
  float* xs = smem;
  float* red = smem + ((N + 3) & ~3);
  const bool is_raw = A.raw && s == 0;
  double dc = 0.0;
  if (is_raw) {
    const float* src = A.x + (long long)c * A.ch_stride + (long long)w * A.win_stride + (A.starts ? A.starts[w] : 0ll);
    const int clean = A.clean_on_load;
    for (int i = NMX_TID; i < N; i += NMX_NT) { const float v = src[i]; xs[i] = clean ? nmx_clean(v) : v; }
    if (A.dcf) dc = (double)A.dcf[c];
  } else {
    const float* src = A.yb + (((long long)w * C + c) * A.n_band + (s - A.raw)) * N;
    for (int i = NMX_TID; i < N; i += NMX_NT) xs[i] = src[i];
  }
  NMX_SYNC();
  if (A.series_out) {
    float* dst = A.series_out + (long long)item * N;
    for (int i = NMX_TID; i < N; i += NMX_NT) dst[i] = xs[i];
  }

  // ---- sum, mean, variance (float64, two passes), tol ------------------------------------------------------------------
  double sum = 0.0;
  for (int i = NMX_TID; i < N; i += NMX_NT) sum += (double)xs[i];
  sum = nmx_nolds_sum_d(sum, red);
  const double mean = sum / (double)N;
  double ss = 0.0;
  for (int i = NMX_TID; i < N; i += NMX_NT) { const double d = (double)xs[i] - mean; ss += d * d; }
  ss = nmx_nolds_sum_d(ss, red);
  // (N <= ddof: 0 / 0 or a negative variance -> NaN, no pair passes, the result is NaN)
  const float tol = (float)(sqrt(ss / (double)(N - A.ddof)) * A.tol_factor);
  const bool zero = sum + (double)N * dc == 0.0;

  // ---- the walk ------------------------------------------------------------------------------------------------------------
  const int T = N - 2;
  unsigned a = 0u, b = 0u;
  for (int u = 1 + NMX_TID; u <= T / 2; u += NMX_NT) {
    nmx_nolds_diag(xs, T, u, tol, a, b);
    if (T - u != u) nmx_nolds_diag(xs, T, T - u, tol, a, b);
  }
  a = nmx_nolds_sum_u(a, red);
  b = nmx_nolds_sum_u(b, red);

  if (NMX_TID == 0) {
    float r;
    if (zero) r = 0.f;
    else if (a > 0u && b > 0u) r = (float)(-log((double)a / (double)b));
    else if (b > 0u) r = INFINITY;
    else r = NAN;
    A.out[(long long)w * A.n_outputs + A.cols.base + c * A.cols.ch_stride + s * A.cols.a_stride] = r;
    if (A.probe) {
      unsigned* p = A.probe + (long long)item * 4;
      unsigned tb;
      memcpy(&tb, &tol, 4);
      p[0] = a; p[1] = b; p[2] = tb; p[3] = zero ? 1u : 0u;
    }
  }
}

// threads per workgroup: one wave up to 256 samples, four up to 8192, sixteen beyond
static inline int nmx_nolds_threads(int n) { return n <= 256 ? 64 : (n <= 8192 ? 256 : 1024); }

#ifdef NMX_HOST_EMU
static void be_launch_nolds(const NmxNoldsArgs& A, int n_items, be_stream_t st) {
#ifdef NMX_TR
  NMX_TR(st);
#endif
  (void)st;
  std::vector<float> sm((size_t)A.lds_floats + 16);
  for (int it = 0; it < n_items; ++it) nmx_nolds_item(A, it, sm.data());
}
#else
extern __shared__ __attribute__((aligned(16))) float nmx_smem[];
__global__ void __launch_bounds__(1024) nmx_kern_nolds_sampen(const NmxNoldsArgs A) {
  nmx_nolds_item(A, (int)blockIdx.x, nmx_smem);
}
static void be_launch_nolds(const NmxNoldsArgs& A, int n_items, be_stream_t s) {
  NMX_LAUNCH(nmx_kern_nolds_sampen, dim3(n_items), dim3(nmx_nolds_threads(A.W)), (size_t)A.lds_floats * 4, s, A);
}
#endif
