// nmx_k_nolds.h -- sample entropy, detrended fluctuation analysis (below: nmx_nolds_dfa_item) and the rescaled-range Hurst
// exponent (nmx_nolds_hurst_item) of the nolds feature (features/nolds.py): one workgroup per (window, series, channel).
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
// Included by nmx_engine.inc: the HIP build gets the kernels and their launchers, the host emulator (NMX_HOST_EMU) launchers
// that loop the same item code.
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

// The series of item = (w * n_series + s) * n_channels + c into xs (and into A.series_out); -> the constant carried next to it
NMX_DEV double nmx_nolds_load(const NmxNoldsArgs& A, int item, float* xs) {
  const int n_series = A.raw + A.n_band, C = A.n_channels, N = A.W;
  const int c = item % C, s = (item / C) % n_series, w = item / (C * n_series);
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
  return dc;
}

// item = (w * n_series + s) * n_channels + c
NMX_DEV void nmx_nolds_item(const NmxNoldsArgs& A, int item, float* smem) {
  const int n_series = A.raw + A.n_band, C = A.n_channels, N = A.W;
  const int c = item % C, s = (item / C) % n_series, w = item / (C * n_series);
  float* xs = smem;
  float* red = smem + ((N + 3) & ~3);
  const double dc = nmx_nolds_load(A, item, xs);

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

// ---- detrended fluctuation analysis (nolds.dfa with fit_trend = "poly", order 1, overlap, fit_exp = "poly") -----------------
// For a series x of N samples and the plan's scale table n_0 .. n_{S-1} (formed on the host: plan_desc.dfa_scales):
//   walk = cumsum(x - mean(x)); for every scale n the chunks walk[i : i + n], i = 0, n / 2, 2 (n / 2), ... < N - n;
//   fluc = sqrt(sum of squared residuals of the chunk's least-squares line / n); F(n) = mean of fluc over the chunks;
//   alpha = least-squares slope of ln F on ln n over the scales with F(n) != 0 -- NaN with fewer than two of them (nolds
//   would hand back the minimum-norm solution of the under-determined fit for exactly one); 0 when x.sum() is exactly zero.
// One workgroup per (window, series, channel), the series in LDS as for the sample entropy.  A WAVE owns a scale (every scale
// visits about 2 N samples, whatever n), a lane a chunk: the chunk's walk is accumulated in float64 from x - mean starting
// at 0 -- a line fit does not see a constant, so the profile itself (sigma sqrt(N)) is never formed -- in two passes over
// the chunk: the sums of the fit, then the residuals themselves (the closed form sum y^2 - n ybar^2 - Sty^2 / Stt cancels
// to the square root of float64's rounding on chunks that are nearly straight).  The lanes' sums meet in the wave butterfly
// and F(n) lands in LDS: every sum has one fixed order, a result does not depend on the batch around it.  Thread 0 fits
// the S points in float64.
#define NMX_NOLDS_DFA_MAX_SCALES 64

struct NmxNoldsDfaArgs {
  NmxNoldsArgs s;           // the series and the row as for the sample entropy; cols: the DFA columns; probe unused
  const int* scales;        // [n_scales] chunk lengths, 2 <= n < W
  int n_scales;
  double* probe;            // [item][n_scales + 3]: F(n) of every scale, alpha, sum == 0, scales kept -- or NULL
  int lds_floats;           // series + 64 floats of reduction scratch + n_scales doubles
};

#ifdef NMX_HOST_EMU
#define NMX_DFA_LANE 0
#define NMX_DFA_LANES 1
#define NMX_DFA_WAVE 0
#define NMX_DFA_WAVES 1
NMX_DEV double nmx_nolds_wave_sum_d(double v) { return v; }
#else
#define NMX_DFA_LANE ((int)(threadIdx.x & 63))
#define NMX_DFA_LANES 64
#define NMX_DFA_WAVE nmx_uniform_i((int)(threadIdx.x >> 6))
#define NMX_DFA_WAVES ((int)(blockDim.x >> 6))
NMX_DEV double nmx_nolds_wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
#endif

// fluc of the chunk p[0 .. n): the walk y_0 = 0, y_j = y_{j-1} + (p[j] - mean)
NMX_DEV double nmx_nolds_dfa_chunk(const float* p, int n, double mean, double tm, double inv_n, double inv_stt) {
  double y = 0.0, sy = 0.0, sty = 0.0;
  for (int j = 1; j < n; ++j) {
    y += (double)p[j] - mean;
    sy += y;
    sty += (double)j * y;
  }
  const double slope = (sty - tm * sy) * inv_stt, icpt = sy * inv_n - slope * tm;
  double r = icpt * icpt;   // (j = 0: y = 0)
  y = 0.0;
  for (int j = 1; j < n; ++j) {
    y += (double)p[j] - mean;
    const double e = y - (icpt + slope * (double)j);
    r += e * e;
  }
  return sqrt(r * inv_n);
}

NMX_DEV void nmx_nolds_dfa_item(const NmxNoldsDfaArgs& D, int item, float* smem) {
  const NmxNoldsArgs& A = D.s;
  const int n_series = A.raw + A.n_band, C = A.n_channels, N = A.W, S = D.n_scales;
  const int c = item % C, s = (item / C) % n_series, w = item / (C * n_series);
  float* xs = smem;
  float* red = smem + ((N + 3) & ~3);
  double* F = (double*)(red + 64);
  const double dc = nmx_nolds_load(A, item, xs);

  double sum = 0.0;
  for (int i = NMX_TID; i < N; i += NMX_NT) sum += (double)xs[i];
  sum = nmx_nolds_sum_d(sum, red);
  const double mean = sum / (double)N;
  const bool zero = sum + (double)N * dc == 0.0;

  for (int k = NMX_DFA_WAVE; k < S; k += NMX_DFA_WAVES) {
    const int n = nmx_uniform_i(D.scales[k]), step = n >> 1;
    const int n_chunks = (N - n + step - 1) / step;   // starts 0, step, 2 step, ... < N - n: the last sample read is < N - 1
    const double tm = 0.5 * (double)(n - 1), inv_n = 1.0 / (double)n;
    const double inv_stt = 12.0 / ((double)n * ((double)n * (double)n - 1.0));
    double acc = 0.0;
    for (int q = NMX_DFA_LANE; q < n_chunks; q += NMX_DFA_LANES) acc += nmx_nolds_dfa_chunk(xs + q * step, n, mean, tm, inv_n, inv_stt);
    acc = nmx_nolds_wave_sum_d(acc);
    if (NMX_DFA_LANE == 0) F[k] = acc / (double)n_chunks;
  }
  NMX_SYNC();

  if (NMX_TID == 0) {
    int kept = 0;
    double mx = 0.0, my = 0.0;
    for (int k = 0; k < S; ++k)
      if (F[k] > 0.0) { ++kept; mx += log((double)D.scales[k]); my += log(F[k]); }
    double alpha = NAN;
    if (kept >= 2) {
      mx /= (double)kept;
      my /= (double)kept;
      double sxx = 0.0, sxy = 0.0;
      for (int k = 0; k < S; ++k)
        if (F[k] > 0.0) { const double dx = log((double)D.scales[k]) - mx; sxx += dx * dx; sxy += dx * (log(F[k]) - my); }
      alpha = sxy / sxx;
    }
    A.out[(long long)w * A.n_outputs + A.cols.base + c * A.cols.ch_stride + s * A.cols.a_stride] = zero ? 0.f : (float)alpha;
    if (D.probe) {
      double* p = D.probe + (long long)item * (S + 3);
      for (int k = 0; k < S; ++k) p[k] = F[k];
      p[S] = alpha; p[S + 1] = zero ? 1.0 : 0.0; p[S + 2] = (double)kept;
    }
  }
}

// a wave per scale: no more waves than scales
static inline int nmx_nolds_dfa_threads(int n, int n_scales) { return std::min(nmx_nolds_threads(n), 64 * std::max(n_scales, 1)); }

// ---- Hurst exponent by rescaled range (nolds.hurst_rs with nvals = logmid_n(N, 1/4, 15), corrected, unbiased, fit = "poly") --
// For a series x of N samples and the plan's tables n_0 .. n_{S-1}, ln E(n_k) (formed on the host: plan_desc.hurst_scales,
// plan_desc.hurst_expected_rs):
//   per scale n the N / n whole chunks x[q n : (q + 1) n] (the tail is dropped); per chunk d = x - mean(chunk), y = cumsum(d),
//   r = max y - min y over y_0 .. y_{n-1}, s = sqrt(sum d^2 / (n - 1)); chunks with r == 0 are left out; (R/S)_n = mean of
//   r / s over the rest, NaN when none is left;
//   H = 0.5 + least-squares slope of ln (R/S)_n - ln E(n) on ln n over the scales that are not NaN -- NaN with fewer than
//   two of them (nolds would hand back the minimum-norm solution for exactly one); 0 when x.sum() is exactly zero.
// One workgroup per (window, series, channel), the series in LDS as for the other two kernels.  Every scale visits the same
// N - N % n samples, so the work is split evenly BY SCALE: the workgroup is cut into teams of L = threads / 16 adjacent lanes
// (4, 16 or 64: nmx_nolds_hurst_lanes), team k owns scale k and lane l of it the chunks l, l + L, ...  A whole wave per scale
// (as the DFA kernel has it, whose chunks overlap and number 2 N / n) would leave most lanes idle: at N = 1000 thirteen of
// the fifteen scales have fewer than 64 chunks.  A lane walks its chunks in ONE loop over (chunk, pass, sample) -- two passes
// per chunk: the mean, then walk, extrema and sum of squares together -- so that teams with different n in one wave do not
// wait on each other's inner loops: every lane runs about 2 N / L iterations.  All of it in float64; r == 0 is an exact
// comparison (a constant chunk of float32 samples has an exact float64 mean).  A lane adds its chunks in ascending order,
// the lanes' sums and kept counts meet in the team's butterfly, (R/S)_n lands in LDS: every sum has one fixed order, the
// count is an integer sum, and a result does not depend on the batch around it.  Thread 0 fits the <= 15 points.
#define NMX_NOLDS_HURST_MAX_SCALES 15

struct NmxNoldsHurstArgs {
  NmxNoldsArgs s;           // the series and the row as for the sample entropy; cols: the Hurst columns; probe unused
  const int* scales;        // [n_scales] chunk lengths, 2 <= n < W
  const double* log_e;      // [n_scales] ln E(n)
  int n_scales;
  int lanes;                // lanes per team (a power of two <= 64 that divides the workgroup)
  double* probe;            // [item][2 n_scales + 3]: (R/S)_n, kept chunks per scale, H, sum == 0, scales kept -- or NULL
  int lds_floats;           // series + 64 floats of reduction scratch + n_scales doubles + n_scales ints
};

#ifdef NMX_HOST_EMU
#define NMX_HURST_LANE(L) 0
#define NMX_HURST_LANES(L) 1
#define NMX_HURST_TEAM(L) 0
#define NMX_HURST_TEAMS(L) 1
NMX_DEV double nmx_nolds_team_sum_d(double v, int) { return v; }
NMX_DEV int nmx_nolds_team_sum_i(int v, int) { return v; }
#else
#define NMX_HURST_LANE(L) ((int)(threadIdx.x & ((L) - 1)))
#define NMX_HURST_LANES(L) (L)
#define NMX_HURST_TEAM(L) ((int)(threadIdx.x / (L)))
#define NMX_HURST_TEAMS(L) ((int)(blockDim.x / (L)))
// sums over the L adjacent lanes of a team (L a power of two <= 64: the exchanges stay inside the team)
NMX_DEV double nmx_nolds_team_sum_d(double v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
NMX_DEV int nmx_nolds_team_sum_i(int v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
#endif

NMX_DEV void nmx_nolds_hurst_item(const NmxNoldsHurstArgs& D, int item, float* smem) {
  const NmxNoldsArgs& A = D.s;
  const int n_series = A.raw + A.n_band, C = A.n_channels, N = A.W, S = D.n_scales, L = D.lanes;
  const int c = item % C, s = (item / C) % n_series, w = item / (C * n_series);
  float* xs = smem;
  float* red = smem + ((N + 3) & ~3);
  double* RS = (double*)(red + 64);
  int* kept_chunks = (int*)(RS + S);
  const double dc = nmx_nolds_load(A, item, xs);

  double sum = 0.0;
  for (int i = NMX_TID; i < N; i += NMX_NT) sum += (double)xs[i];
  sum = nmx_nolds_sum_d(sum, red);
  const bool zero = sum + (double)N * dc == 0.0;

  // (k is the same for the whole team, and the butterfly exchanges inside the team only)
  for (int k = NMX_HURST_TEAM(L); k < S; k += NMX_HURST_TEAMS(L)) {
    const int n = D.scales[k], m = N / n;   // (q n + j <= m n - 1 <= N - 1)
    const double dn = (double)n, dn1 = (double)(n - 1);
    double acc = 0.0;
    int cnt = 0;
    int q = NMX_HURST_LANE(L), j = 0, pass = 0;
    double csum = 0.0, mean = 0.0, y = 0.0, ss = 0.0, hi = 0.0, lo = 0.0;
    while (q < m) {
      const double v = (double)xs[q * n + j];
      if (pass == 0) {
        csum += v;
      } else {
        const double d = v - mean;
        y += d;
        ss += d * d;
        hi = (j == 0 || y > hi) ? y : hi;
        lo = (j == 0 || y < lo) ? y : lo;
      }
      if (++j == n) {
        j = 0;
        if (pass == 0) {
          mean = csum / dn;   // (a division: n equal float32 samples sum exactly, and the quotient is then the sample)
          y = 0.0; ss = 0.0;
          pass = 1;
        } else {
          const double r = hi - lo;
          if (r != 0.0) { acc += r / sqrt(ss / dn1); ++cnt; }
          csum = 0.0;
          pass = 0;
          q += NMX_HURST_LANES(L);
        }
      }
    }
    acc = nmx_nolds_team_sum_d(acc, L);
    cnt = nmx_nolds_team_sum_i(cnt, L);
    if (NMX_HURST_LANE(L) == 0) { RS[k] = cnt > 0 ? acc / (double)cnt : (double)NAN; kept_chunks[k] = cnt; }
  }
  NMX_SYNC();

  if (NMX_TID == 0) {
    int kept = 0;
    double mx = 0.0, my = 0.0;
    for (int k = 0; k < S; ++k)
      if (kept_chunks[k] > 0) { ++kept; mx += log((double)D.scales[k]); my += log(RS[k]) - D.log_e[k]; }
    double h = NAN;
    if (kept >= 2) {
      mx /= (double)kept;
      my /= (double)kept;
      double sxx = 0.0, sxy = 0.0;
      for (int k = 0; k < S; ++k)
        if (kept_chunks[k] > 0) {
          const double dx = log((double)D.scales[k]) - mx;
          sxx += dx * dx;
          sxy += dx * (log(RS[k]) - D.log_e[k] - my);
        }
      h = sxy / sxx + 0.5;
    }
    A.out[(long long)w * A.n_outputs + A.cols.base + c * A.cols.ch_stride + s * A.cols.a_stride] = zero ? 0.f : (float)h;
    if (D.probe) {
      double* p = D.probe + (long long)item * (2 * S + 3);
      for (int k = 0; k < S; ++k) { p[k] = RS[k]; p[S + k] = (double)kept_chunks[k]; }
      p[2 * S] = h; p[2 * S + 1] = zero ? 1.0 : 0.0; p[2 * S + 2] = (double)kept;
    }
  }
}

// sixteen teams in the workgroup the other kernels would use -- 4, 16 or 64 lanes each -- and no more waves than the table
// has teams for
static inline int nmx_nolds_hurst_lanes(int n) { return nmx_nolds_threads(n) / 16; }
static inline int nmx_nolds_hurst_threads(int n, int n_scales) {
  return std::min(nmx_nolds_threads(n), (std::max(n_scales, 1) * nmx_nolds_hurst_lanes(n) + 63) & ~63);
}

#ifdef NMX_HOST_EMU
static void be_launch_nolds(const NmxNoldsArgs& A, int n_items, be_stream_t st) {
#ifdef NMX_TR
  NMX_TR(st);
#endif
  (void)st;
  std::vector<float> sm((size_t)A.lds_floats + 16);
  for (int it = 0; it < n_items; ++it) nmx_nolds_item(A, it, sm.data());
}
static void be_launch_nolds_dfa(const NmxNoldsDfaArgs& D, int n_items, be_stream_t st) {
#ifdef NMX_TR
  NMX_TR(st);
#endif
  (void)st;
  std::vector<float> sm((size_t)D.lds_floats + 16);
  for (int it = 0; it < n_items; ++it) nmx_nolds_dfa_item(D, it, sm.data());
}
static void be_launch_nolds_hurst(const NmxNoldsHurstArgs& D, int n_items, be_stream_t st) {
#ifdef NMX_TR
  NMX_TR(st);
#endif
  (void)st;
  std::vector<float> sm((size_t)D.lds_floats + 16);
  for (int it = 0; it < n_items; ++it) nmx_nolds_hurst_item(D, it, sm.data());
}
#else
extern __shared__ __attribute__((aligned(16))) float nmx_smem[];
__global__ void __launch_bounds__(1024) nmx_kern_nolds_sampen(const NmxNoldsArgs A) {
  nmx_nolds_item(A, (int)blockIdx.x, nmx_smem);
}
static void be_launch_nolds(const NmxNoldsArgs& A, int n_items, be_stream_t s) {
  NMX_LAUNCH(nmx_kern_nolds_sampen, dim3(n_items), dim3(nmx_nolds_threads(A.W)), (size_t)A.lds_floats * 4, s, A);
}
__global__ void __launch_bounds__(1024) nmx_kern_nolds_dfa(const NmxNoldsDfaArgs D) {
  nmx_nolds_dfa_item(D, (int)blockIdx.x, nmx_smem);
}
static void be_launch_nolds_dfa(const NmxNoldsDfaArgs& D, int n_items, be_stream_t s) {
  NMX_LAUNCH(nmx_kern_nolds_dfa, dim3(n_items), dim3(nmx_nolds_dfa_threads(D.s.W, D.n_scales)), (size_t)D.lds_floats * 4, s, D);
}
__global__ void __launch_bounds__(1024) nmx_kern_nolds_hurst(const NmxNoldsHurstArgs D) {
  nmx_nolds_hurst_item(D, (int)blockIdx.x, nmx_smem);
}
static void be_launch_nolds_hurst(const NmxNoldsHurstArgs& D, int n_items, be_stream_t s) {
  NMX_LAUNCH(nmx_kern_nolds_hurst, dim3(n_items), dim3(nmx_nolds_hurst_threads(D.s.W, D.n_scales)), (size_t)D.lds_floats * 4, s, D);
}
#endif
