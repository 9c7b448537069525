// nmx_k_coh.h -- coherence between channel pairs (features/coherence.py): one workgroup per (window, pair).
//
// Reference arithmetic (CoherenceObject.get_coh):
//   Pxx, Pyy = welch(x / y, fs, "hann", nperseg), Pxy = csd(x, y, ...): periodic Hann, noverlap = nperseg // 2, constant
//   detrend per segment, mean over the segments;  coh = |Pxy|^2 / (Pxx Pyy),  icoh = Im Pxy / sqrt(Pxx Pyy).
// Every scale factor of the estimators (density scale, one-sided doubling, 1 / nseg) cancels in both ratios, so the
// kernel accumulates plain sums over the segments:  Sxx = sum |X|^2,  Syy = sum |Y|^2,  Sxy = sum conj(X) Y.
// Both channels go through ONE complex transform, z = x + i y:  X[k] ~ Z[k] + conj(Z[n - k]),  Y[k] ~ -i (Z[k] - conj(Z[n - k]))
// (the common factor 1/2 cancels as well).  Before packing, each channel is scaled by a power of two near the inverse of its
// RMS over the window (exact, and both ratios are invariant to a positive rescaling of either channel): a quiet channel's
// spectrum then does not sit in the rounding of a loud one's, and the sums stay far from the fp32 range limits.
// Samples are taken relative to the window's first sample before any sum: a channel that is constant within the window
// detrends to exact zeros (0 / 0 = NaN, as in the reference).  The window's carried offset (NmxTimeOscArgs::dcf) is not
// needed: the per-segment detrend removes a constant exactly.
//
// Reductions per method (coh, icoh): band mean and band maximum over the bins [bin_lo, bin_hi) the host resolved with the
// reference's strict edges (f > lo & f < hi; mean of nothing = NaN, np.max propagates NaN), and f[argmax] over ALL bins
// (np.argmax: a NaN is the maximum, the first index wins).
//
// Included by nmx_engine.inc: the HIP build gets the kernel and its launcher, the host emulator (NMX_HOST_EMU) a launcher
// that loops the same item code.
#pragma once

#include "nmx_device.h"

#define NMX_COH_MAX_N 4096   // segment length bound: two complex buffers + four per-bin sums in LDS

struct NmxCohArgs {
  const float* x;           // input samples (as NmxTimeOscArgs)
  long long ch_stride;
  long long win_stride;
  const long long* starts;
  float* out;               // [n_windows][n_outputs]
  int n_outputs;
  int clean_on_load;
  int n_pairs;
  const int* pairs;         // [n_pairs][2] channel indices
  int W;                    // window samples
  int n, nseg, step, nfreq; // segment length (after the clamp to W), segment count, hop, one-sided bins
  int n_bands;
  int bin_lo[NMX_MAX_BANDS_DEV], bin_hi[NMX_MAX_BANDS_DEV];
  unsigned feats;           // bit 0 mean_fband, bit 1 max_fband, bit 2 max_allfbands
  unsigned methods;         // bit 0 coh, bit 1 icoh
  double df;                // frequency of bin k = k * df (numpy's rfftfreq in float64)
  NmxCols cols;             // column = base + pair * a_stride + method * b_stride + slot
  NmxFft fft;               // complex length n
  const float* win;         // [n] periodic Hann
  int off_a, off_b, off_acc, off_red, lds_floats;
};

// power of two near 1 / sqrt(ss / cnt) (1 when the sum of squares is zero or not finite)
NMX_DEV float nmx_coh_pow2_scale(float ss, int cnt) {
  const float ms = ss / (float)cnt;
  if (!(ms > 0.f) || !(ms < INFINITY)) return 1.f;
  int e = (int)rintf(-0.5f * log2f(ms));
  e = e < -120 ? -120 : (e > 120 ? 120 : e);
  return ldexpf(1.f, e);
}

NMX_DEV void nmx_coh_item(const NmxCohArgs& A, int w, int p, float* smem) {
  float2* bufA = (float2*)(smem + A.off_a);
  float2* bufB = (float2*)(smem + A.off_b);
  float* acc = smem + A.off_acc;          // [4][nfreq]: Sxx, Syy, Re Sxy, Im Sxy
  float* red = smem + A.off_red;
  const int N = A.n, nf = A.nfreq, W = A.W;
  float* sxx = acc;
  float* syy = acc + nf;
  float* sre = acc + 2 * nf;
  float* sim = acc + 3 * nf;
  const long long st = A.starts ? A.starts[w] : 0ll;
  const float* sx = A.x + (long long)A.pairs[2 * p] * A.ch_stride + (long long)w * A.win_stride + st;
  const float* sy = A.x + (long long)A.pairs[2 * p + 1] * A.ch_stride + (long long)w * A.win_stride + st;
  const int clean = A.clean_on_load;
  auto ld = [&](const float* s, int i) -> float { const float v = s[i]; return clean ? nmx_clean(v) : v; };
  const float x0 = ld(sx, 0), y0 = ld(sy, 0);

  // ---- window-level power-of-two scales (two passes: mean, then centred sum of squares) -------------------------------
  float m[2] = {0.f, 0.f};
  int moves = 0;   // bit 0: x is not constant within the window, bit 1: y is not
  for (int i = NMX_TID; i < W; i += NMX_NT) {
    const float a = ld(sx, i), b = ld(sy, i);
    m[0] += a - x0;
    m[1] += b - y0;
    moves |= (a != x0 ? 1 : 0) | (b != y0 ? 2 : 0);
  }
  nmx_block_sum_n<2>(m, red);
  moves = nmx_block_or(moves, red);
  // a channel that is constant within the window detrends to exact zeros: its spectrum is zero, not the rounding the
  // other channel's transform leaks into its half of the packed spectrum (0 / 0 = NaN, as in the reference)
  const float keep_x = (moves & 1) ? 1.f : 0.f, keep_y = (moves & 2) ? 1.f : 0.f;
  const float mx = m[0] / (float)W, my = m[1] / (float)W;
  float q[2] = {0.f, 0.f};
  for (int i = NMX_TID; i < W; i += NMX_NT) {
    const float a = (ld(sx, i) - x0) - mx, b = (ld(sy, i) - y0) - my;
    q[0] += a * a;
    q[1] += b * b;
  }
  nmx_block_sum_n<2>(q, red);
  const float gx = nmx_coh_pow2_scale(q[0], W), gy = nmx_coh_pow2_scale(q[1], W);

  // ---- segments: detrend, window, one packed complex transform, per-bin sums ------------------------------------------
  for (int sg = 0; sg < A.nseg; ++sg) {
    const int s0 = sg * A.step;
    float sm[2] = {0.f, 0.f};
    for (int i = NMX_TID; i < N; i += NMX_NT) {
      sm[0] += (ld(sx, s0 + i) - x0) * gx;
      sm[1] += (ld(sy, s0 + i) - y0) * gy;
    }
    nmx_block_sum_n<2>(sm, red);
    const float ax = sm[0] / (float)N, ay = sm[1] / (float)N;
    for (int i = NMX_TID; i < N; i += NMX_NT) {
      const float wv = A.win[i];
      bufB[i] = make_float2(((ld(sx, s0 + i) - x0) * gx - ax) * wv, ((ld(sy, s0 + i) - y0) * gy - ay) * wv);
    }
    NMX_SYNC();
    const float2* Z = nmx_fft_auto<-1>(A.fft, bufB, bufA, bufB);
    for (int k = NMX_TID; k < nf; k += NMX_NT) {
      const float2 zk = Z[k], zc = Z[k == 0 ? 0 : N - k];
      const float xr = zk.x + zc.x, xi = zk.y - zc.y;   // 2 X[k]
      const float yr = zk.y + zc.y, yi = zc.x - zk.x;   // 2 Y[k]
      const float pxx = (xr * xr + xi * xi) * keep_x, pyy = (yr * yr + yi * yi) * keep_y;
      const float kxy = keep_x * keep_y;
      const float pre = (xr * yr + xi * yi) * kxy, pim = (xr * yi - xi * yr) * kxy;   // conj(X) Y
      if (sg == 0) {
        sxx[k] = pxx; syy[k] = pyy; sre[k] = pre; sim[k] = pim;
      } else {
        sxx[k] += pxx; syy[k] += pyy; sre[k] += pre; sim[k] += pim;
      }
    }
    NMX_SYNC();
  }
  // coh into sxx, icoh into syy (each thread rewrites only the bins it accumulated)
  for (int k = NMX_TID; k < nf; k += NMX_NT) {
    const float a = sxx[k], b = syy[k], re = sre[k], im = sim[k];
    const float den = a * b;
    sxx[k] = (re * re + im * im) / den;
    syy[k] = im / sqrtf(den);
  }
  NMX_SYNC();

  // ---- reductions and output ---------------------------------------------------------------------------------------------
  float* out_row = A.out + (long long)w * A.n_outputs + A.cols.base + (long long)p * A.cols.a_stride;
  const int nfb = (int)(A.feats & 1u) + (int)((A.feats >> 1) & 1u);
  const int n_meth = (A.methods & 2u) ? 2 : 1;
  int* ridx = (int*)(red + 64);
  float* rval = red + 64 + NMX_NT;
  for (int mth = 0; mth < n_meth; ++mth) {
    const float* v = mth == 0 ? sxx : syy;
    float* o = out_row + mth * A.cols.b_stride;
    for (int b = 0; b < A.n_bands; ++b) {
      const int lo = A.bin_lo[b], hi = A.bin_hi[b], cnt = hi - lo;
      int slot = b * nfb;
      if (A.feats & 1u) {
        float s = 0.f;
        for (int k = lo + NMX_TID; k < hi; k += NMX_NT) s += v[k];
        s = nmx_block_sum(s, red);
        if (NMX_TID == 0) o[slot] = cnt > 0 ? s / (float)cnt : NAN;
        ++slot;
      }
      if (A.feats & 2u) {
        float s = -INFINITY;
        for (int k = lo + NMX_TID; k < hi; k += NMX_NT) s = nmx_nanmax(s, v[k]);
        s = nmx_block_max(s, red);
        if (NMX_TID == 0) o[slot] = cnt > 0 ? s : NAN;
      }
    }
    if (A.feats & 4u) {
      // per thread: first NaN, else first index of the maximum, over its strided bins; then thread 0 merges in index order
      float bv = -INFINITY;
      int bk = -1;
      for (int k = NMX_TID; k < nf; k += NMX_NT) {
        const float x = v[k];
        if (bk >= 0 && bv != bv) break;
        if (bk < 0 || x != x || x > bv) { bv = x; bk = k; }
      }
      ridx[NMX_TID] = bk;
      rval[NMX_TID] = bv;
      NMX_SYNC();
      if (NMX_TID == 0) {
        float gv = -INFINITY;
        int gk = -1;
        for (int t = 0; t < NMX_NT; ++t) {
          const int k = ridx[t];
          if (k < 0) continue;
          const float x = rval[t];
          const bool gnan = gk >= 0 && gv != gv, xnan = x != x;
          bool take;
          if (gk < 0) take = true;
          else if (gnan) take = xnan && k < gk;
          else if (xnan) take = true;
          else take = x > gv || (x == gv && k < gk);
          if (take) { gv = x; gk = k; }
        }
        o[A.n_bands * nfb] = (float)((double)(gk < 0 ? 0 : gk) * A.df);
      }
      NMX_SYNC();
    }
  }
}

#ifdef NMX_HOST_EMU
static void be_launch_coh(const NmxCohArgs& A, int n_items, be_stream_t) {
  std::vector<float> sm((size_t)A.lds_floats + 16);
  for (int it = 0; it < n_items; ++it) nmx_coh_item(A, it / A.n_pairs, it % A.n_pairs, sm.data());
}
#else
extern __shared__ __attribute__((aligned(16))) float nmx_smem[];
__global__ void __launch_bounds__(128) nmx_kern_coh(const NmxCohArgs A) {
  const int item = (int)blockIdx.x;
  nmx_coh_item(A, item / A.n_pairs, item % A.n_pairs, nmx_smem);
}
// one workgroup per (window, pair): 64 threads up to 512-point segments, 128 beyond
static void be_launch_coh(const NmxCohArgs& A, int n_items, be_stream_t s) {
  const int nt = A.n <= 512 ? 64 : 128;
  NMX_LAUNCH(nmx_kern_coh, dim3(n_items), dim3(nt), (size_t)A.lds_floats * 4, s, A);
}
#endif
