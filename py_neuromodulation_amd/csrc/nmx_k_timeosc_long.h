// nmx_k_timeosc_long.h -- the time / oscillatory item for windows whose generic LDS layout (window + two transform
// buffers + spectrum, nmx_k_timeosc.h) does not fit 160 KiB: up to 40 000 samples, FFT and Welch segments as long as the
// window.  Same NmxTimeOscArgs, same columns, same arithmetic conventions as nmx_time_osc_item; no return_spectrum of
// FFT / Welch (the plan refuses it for this kernel); STFT behind NMX_LONG_STFT=1 (nmx_plan_create).  Included at the end of
// nmx_k_timeosc.h.
//
// Phase 1: the window is staged in LDS once, for the rail test and the time-domain features (nmx_tol_time_domain: the
//   arithmetic of nmx_time_osc_item, a thread's sums closed every NMX_TOL_CHUNK terms).
// Phase 2: the transform buffers take the window's LDS.  A real transform of N samples is split into D = O.split_d
//   interleaved subsequences x_r[m] = x[m D + r] of M = N / D samples (re-read from the input with a stride of D floats:
//   the window is resident in L2 by then), each transformed with the LDS machinery (nmx_fft_auto on M / 2 packed complex
//   points, or M when M is odd), and only the bins some band reads are combined:
//       X[k] = sum_r w_N^(r k) X_r[k mod M],  X_r[M - j] = conj(X_r[j]),  w_N from a float64-built table of N entries.
//   The accumulators (k_hi - k_lo complex) and the spectrum (k_hi - k_lo floats) sit behind the buffers in LDS, or -- when
//   the band range is too wide for that -- in the workgroup's slab of device memory (A.long_spec_slab).  Every thread
//   owns the same bins k = k_lo + tid + j nt in every loop over bins, so the accumulators need no barrier of their own;
//   the spectrum is read by all threads in nmx_emit_bands, behind NMX_SYNC() -- in a multi-wave workgroup
//   __syncthreads(), which also orders the global stores of the slab form.
// Phase 3 (STFT): segments read from the input through the even-extension map, centred on the window mean phase 1 took;
//   one of four segment classes (NMX_TOL_STFT_*), the spectrum [(k - k_lo) nseg + segment] in LDS or in the slab.
#pragma once

// A thread's running sums are closed into its total every NMX_TOL_CHUNK terms.  On the device a thread of the 512-wide
// workgroup has at most 79 terms -- one chunk, the plain loop.  The single-thread emulator would add 40 000 terms into one
// fp32 accumulator (a rounding walk of ~200 ulp, the whole 1e-5 budget); chunked it stays at the level of the device's
// 512 partial sums.
#define NMX_TOL_CHUNK 128

// Hjorth + LineLength + Raw of the window xs[0..W) in LDS: nmx_time_osc_item's arithmetic -- sums first, then mean-shifted
// squares, the same nan_to_num placement, raw = last sample + dcv
NMX_DEV void nmx_tol_time_domain(const NmxTimeOscArgs& A, const float* xs, int W, int c, float dcv, float* out_row, float* red) {
  if (A.features & (NMXD_F_HJORTH | NMXD_F_LINELENGTH)) {
    // pass 1: sums of x, dx, d2x (for the means) and of |dx| (line length)
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = NMX_TID; i0 < W; i0 += NMX_NT * NMX_TOL_CHUNK) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0, i = i0; j < NMX_TOL_CHUNK && i < W; ++j, i += NMX_NT) {
        const float x0 = xs[i];
        a[0] += x0;
        if (i + 1 < W) {
          const float d1 = xs[i + 1] - x0;
          a[1] += d1;
          a[3] += fabsf(d1);
          if (i + 2 < W) a[2] += (xs[i + 2] - xs[i + 1]) - d1;
        }
      }
      for (int k = 0; k < 4; ++k) p[k] += a[k];
    }
    nmx_block_sum_n<4>(p, red);
    const float m0 = p[0] / (float)W, m1 = p[1] / (float)(W - 1), m2 = p[2] / (float)(W - 2);
    const float ll = p[3];
    // pass 2: mean-shifted sums of squares (np.var is two-pass)
    float q[3] = {0.f, 0.f, 0.f};
    for (int i0 = NMX_TID; i0 < W; i0 += NMX_NT * NMX_TOL_CHUNK) {
      float a[3] = {0.f, 0.f, 0.f};
      for (int j = 0, i = i0; j < NMX_TOL_CHUNK && i < W; ++j, i += NMX_NT) {
        const float x0 = xs[i];
        const float e0 = x0 - m0;
        a[0] += e0 * e0;
        if (i + 1 < W) {
          const float d1 = xs[i + 1] - x0;
          const float e1 = d1 - m1;
          a[1] += e1 * e1;
          if (i + 2 < W) {
            const float e2 = ((xs[i + 2] - xs[i + 1]) - d1) - m2;
            a[2] += e2 * e2;
          }
        }
      }
      for (int k = 0; k < 3; ++k) q[k] += a[k];
    }
    nmx_block_sum_n<3>(q, red);
    if (NMX_TID == 0) {
      if (A.features & NMXD_F_HJORTH) {
        const float v0 = q[0] / (float)W, v1 = q[1] / (float)(W - 1), v2 = q[2] / (float)(W - 2);
        // hjorth_raw.py:24-34: complexity divides by the nan_to_num'ed mobility
        const float mob = nmx_nan_to_num(sqrtf(v1 / v0));
        const float comp = nmx_nan_to_num(sqrtf(v2 / v1) / mob);
        const int col = A.hjorth_cols.base + c * A.hjorth_cols.ch_stride;
        out_row[col] = nmx_nan_to_num(v0);
        out_row[col + A.hjorth_cols.a_stride] = mob;
        out_row[col + 2 * A.hjorth_cols.a_stride] = comp;
      }
      if (A.features & NMXD_F_LINELENGTH) {
        const float wm1 = (float)(W - 1);
        out_row[A.ll_cols.base + c * A.ll_cols.ch_stride] = ll / wm1 / wm1;
      }
    }
  }
  if ((A.features & NMXD_F_RAW) && NMX_TID == 0)
    out_row[A.raw_cols.base + c * A.raw_cols.ch_stride] = xs[W - 1] + dcv;
}

// bin j (0 <= j < M) of the spectrum of one real subsequence from its transform Z
NMX_DEV float2 nmx_tol_sub_bin(const NmxOsc& O, const float2* Z, int j) {
  if (O.complex_full) return Z[j];
  const int n = O.fft.n;   // M / 2
  if (j <= n) return nmx_rfft_bin(Z, O.fft.twr, n, j);
  const float2 t = nmx_rfft_bin(Z, O.fft.twr, n, O.sub_m - j);
  return make_float2(t.x, -t.y);
}

// acc[k - k_lo] = X[k], k in [k_lo, k_hi), of the segment whose centred sample i in [0, N) is sample(i), times win[i]
// (win = NULL: 1)
template <typename F>
NMX_DEV void nmx_tol_segment_of(const NmxOsc& O, F sample, float2* bufA, float2* bufB, float2* acc) {
  const int D = O.split_d, M = O.sub_m, N = O.n;
  const float* NMX_RESTRICT win = O.win;
  for (int r = 0; r < D; ++r) {
    auto v = [&](int m) -> float {
      const int i = m * D + r;
      const float x = sample(i);
      return win ? x * win[i] : x;
    };
    if (O.complex_full) {
      for (int i = NMX_TID; i < M; i += NMX_NT) bufB[i] = make_float2(v(i), 0.f);
    } else {
      for (int i = NMX_TID; i < M / 2; i += NMX_NT) bufB[i] = make_float2(v(2 * i), v(2 * i + 1));
    }
    NMX_SYNC();
    const float2* Z = nmx_osc_fft(O, bufA, bufB);
    for (int k = O.k_lo + NMX_TID; k < O.k_hi; k += NMX_NT) {
      float2 X = nmx_tol_sub_bin(O, Z, k % M);
      if (r) {
        const int t = (r * k) % N;   // (r < 64, k <= 20 000)
        X = nmx_cadd(acc[k - O.k_lo], nmx_cmul(X, O.tw_n[t]));
      }
      acc[k - O.k_lo] = X;
    }
    NMX_SYNC();   // (the next subsequence overwrites the buffers Z lives in)
  }
}

// the same of the segment seg[0..N) in memory: (clean(seg[i]) - mean) * win[i]
NMX_DEV void nmx_tol_segment(const NmxOsc& O, const float* seg, int clean, float mean, float2* bufA, float2* bufB, float2* acc) {
  nmx_tol_segment_of(O, [=](int i) -> float { return (clean ? nmx_clean(seg[i]) : seg[i]) - mean; }, bufA, bufB, acc);
}

// STFT segment classes of the long-window item, chosen when the plan is built (build_timeosc, NmxTimeOscArgs::long_stft) and
// compiled in by the kernel's template argument (nmx_timeosc_long.hip)
enum { NMX_TOL_STFT_NONE = 0, NMX_TOL_STFT_WAVE500 = 1, NMX_TOL_STFT_DIRECT = 2, NMX_TOL_STFT_LDS = 3, NMX_TOL_STFT_SPLIT = 4 };

// `stft_cls`: a compile-time constant on the device (0: the kernel of plans without STFT), A.long_stft in the emulator
NMX_DEV void nmx_time_osc_long_item(const NmxTimeOscArgs& A, int w, int c, float* smem, float* slab, int stft_cls) {
  float* xs = smem + A.off_x;
  float2* bufA = (float2*)(smem + A.off_a);
  float2* bufB = (float2*)(smem + A.off_b);
  float* red = smem + A.off_red;
  float* sp = A.long_spec_slab ? slab : smem + A.off_spec;
  float2* acc = (float2*)sp;          // [long_nb] complex
  float* spec = sp + 2 * A.long_nb;   // [long_nb]
  const int W = A.W, clean = A.clean_on_load;
  float* out_row = A.out + (long long)w * A.n_outputs;
  const float dcv = A.dcf ? A.dcf[c] : 0.f;
  const float* src = A.x + (long long)c * A.ch_stride + (long long)w * A.win_stride + (A.starts ? A.starts[w] : 0ll);

  // ---- phase 1: the window in LDS -- rail test, time-domain features -------------------------------------------------
  nmx_stage_row(src, W, [=](int i, float v) { xs[i] = clean ? nmx_clean(v) : v; });
  NMX_SYNC();
  bool rail = false;
  if (A.fft.enabled || A.welch.enabled || (stft_cls && A.stft.enabled)) {
    int any = 0;
    for (int i = NMX_TID; i < W; i += NMX_NT) any |= !(fabsf(xs[i]) < 1e30f);
    rail = nmx_block_or(any, red) != 0;
    NMX_SYNC();
  }
  nmx_tol_time_domain(A, xs, W, c, dcv, out_row, red);
  // the segment sums while the window is still there: FFT tail, Welch segments (a few: nperseg is a second of signal)
  float xsum = 0.f;
  if (A.fft.enabled) {
    float sm = 0.f;
    for (int i = NMX_TID; i < A.fft.n; i += NMX_NT) sm += xs[W - A.fft.n + i];
    xsum = nmx_block_sum(sm, red);
  }
  // the window mean the STFT segments are centred on (nmx_time_osc_item), a thread's sum closed like the sums above
  float wmean = 0.f;
  if (stft_cls && A.stft.enabled) {
    float sm = 0.f;
    for (int i0 = NMX_TID; i0 < W; i0 += NMX_NT * NMX_TOL_CHUNK) {
      float a = 0.f;
      for (int j = 0, i = i0; j < NMX_TOL_CHUNK && i < W; ++j, i += NMX_NT) a += xs[i];
      sm += a;
    }
    wmean = nmx_block_sum(sm, red) / (float)W;
  }
  NMX_SYNC();   // xs is dead from here on: [off_a, off_spec) becomes the transform buffers

  // ---- FFT band power ------------------------------------------------------------------------------------------------
  if (A.fft.enabled) {
    const NmxOsc& O = A.fft;
    const int N = O.n;
    nmx_tol_segment(O, src + (W - N), clean, xsum / (float)N, bufA, bufB, acc);
    for (int k = O.k_lo + NMX_TID; k < O.k_hi; k += NMX_NT) {
      float2 X = acc[k - O.k_lo];
      if (k == 0) X = make_float2(xsum + (float)N * dcv, 0.f);
      float v = nmx_sqrt_fast(X.x * X.x + X.y * X.y);
      if (O.log_transform) v = nmx_log10_fast(v);
      spec[k - O.k_lo] = v;
    }
    NMX_SYNC();
    nmx_emit_bands(O, spec, 1, A.n_bands, out_row, c, red, rail);
    NMX_SYNC();
  }

  // ---- Welch -----------------------------------------------------------------------------------------------------------
  if (A.welch.enabled) {
    const NmxOsc& O = A.welch;
    const int N = O.n;
    for (int sgi = 0; sgi < O.nseg; ++sgi) {
      const float* seg = src + sgi * O.step;
      float sm = 0.f;
      for (int i = NMX_TID; i < N; i += NMX_NT) sm += clean ? nmx_clean(seg[i]) : seg[i];
      const float mean = nmx_block_sum(sm, red) / (float)N;
      NMX_SYNC();
      nmx_tol_segment(O, seg, clean, mean, bufA, bufB, acc);
      for (int k = O.k_lo + NMX_TID; k < O.k_hi; k += NMX_NT) {
        const float2 X = acc[k - O.k_lo];
        float p = (X.x * X.x + X.y * X.y) * O.scale;
        const bool edge = (k == 0) || ((N % 2 == 0) && k == N / 2);
        if (!edge) p *= 2.f;
        spec[k - O.k_lo] = (sgi == 0) ? p : spec[k - O.k_lo] + p;
      }
    }
    const float inv = 1.f / (float)O.nseg;
    for (int k = NMX_TID; k < O.k_hi - O.k_lo; k += NMX_NT) {
      float v = spec[k] * inv;
      if (O.log_transform) v = nmx_log10_fast(v);
      spec[k] = v;
    }
    NMX_SYNC();
    nmx_emit_bands(O, spec, 1, A.n_bands, out_row, c, red, rail);
    NMX_SYNC();
  }

  // ---- STFT ------------------------------------------------------------------------------------------------------------
  // nmx_time_osc_item's arithmetic; the samples come from the input (resident in L2) through the even-extension map, as the
  // FFT and Welch phases read theirs.  Spectrum [(k - k_lo) nseg + segment] behind the accumulators of the split form.
  if (stft_cls && A.stft.enabled) {
    const NmxOsc& O = A.stft;
    const int N = O.n, h = O.half;
    float* sspec = sp + A.long_stft_acc;
    const float mean = wmean;
    auto xe = [&](int e) -> float {   // centred sample e of the window extended evenly by h, zero padding beyond
      int i;
      if (e < h) i = h - e;
      else if (e < h + W) i = e - h;
      else if (e < 2 * h + W) i = W - 2 - (e - h - W);
      else return 0.f;
      const float v = src[i];
      return (clean ? nmx_clean(v) : v) - mean;
    };
    const int seg_padded = O.nadd ? O.nseg - 1 : -1;
    auto put = [&](float2 X, int sgi, int k) {
      const float2 t = O.wdc[(sgi == seg_padded ? O.nfreq : 0) + k];
      X = make_float2(X.x + (mean + dcv) * t.x, X.y + (mean + dcv) * t.y);
      float v = nmx_sqrt_fast(X.x * X.x + X.y * X.y) * O.scale;
      if (O.log_transform) v = nmx_log10_fast(v);
      sspec[(k - O.k_lo) * O.nseg + sgi] = v;
    };
#ifndef NMX_HOST_EMU
    if (stft_cls == NMX_TOL_STFT_WAVE500) {
      // nperseg 500: every wave takes whole segments and runs its own 250-point transform in its own slice of the buffers
      // (build_timeosc sizes them for NMX_NT / 64 slices) -- no workgroup barrier inside the segment loop
      const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63), nwv = NMX_NT >> 6;
      float2* wA = bufA + wv * 250;
      float2* wB = bufB + wv * 250;
      for (int sgi = wv; sgi < O.nseg; sgi += nwv) {
        const int s0 = sgi * O.step;
        for (int i = lane; i < 250; i += 64)
          wB[i] = make_float2(xe(s0 + 2 * i) * O.win[2 * i], xe(s0 + 2 * i + 1) * O.win[2 * i + 1]);
        NMX_WAVE_FENCE();
        const float2* Z = nmx_fft4_wave<-1, 250, 5, 5, 5, 2>(wB, wA, wB, O.fft.tw);
        for (int k = O.k_lo + lane; k < O.k_hi; k += 64) put(nmx_rfft_bin(Z, O.fft.twr, 250, k), sgi, k);
        NMX_WAVE_FENCE();
      }
    }
#endif
    if (stft_cls == NMX_TOL_STFT_DIRECT) {
      // segments of at most 64 samples: one (segment, bin) pair per thread, direct N-term DFT
      const int nb = O.k_hi - O.k_lo;
      for (int idx = NMX_TID; idx < O.nseg * nb; idx += NMX_NT) {
        const int sgi = idx / nb, k = O.k_lo + (idx - sgi * nb);
        const int s0 = sgi * O.step;
        float re = 0.f, im = 0.f;
        for (int i = 0; i < N; ++i) {
          float sn, cs;
#ifdef NMX_HOST_EMU
          const double ang = -2.0 * 3.14159265358979323846 * (double)((k * i) % N) / (double)N;
          sn = (float)sin(ang); cs = (float)cos(ang);
#else
          sincospif(-2.f * (float)((k * i) % N) / (float)N, &sn, &cs);
#endif
          const float v = xe(s0 + i) * O.win[i];
          re += v * cs;
          im += v * sn;
        }
        put(make_float2(re, im), sgi, k);
      }
    }
    if (stft_cls == NMX_TOL_STFT_LDS) {
      // one unsplit LDS transform per segment
      for (int sgi = 0; sgi < O.nseg; ++sgi) {
        const int s0 = sgi * O.step;
        if (O.complex_full) {
          for (int i = NMX_TID; i < N; i += NMX_NT) bufB[i] = make_float2(xe(s0 + i) * O.win[i], 0.f);
        } else {
          for (int i = NMX_TID; i < N / 2; i += NMX_NT)
            bufB[i] = make_float2(xe(s0 + 2 * i) * O.win[2 * i], xe(s0 + 2 * i + 1) * O.win[2 * i + 1]);
        }
        NMX_SYNC();
        const float2* Z = nmx_osc_fft(O, bufA, bufB);
        for (int k = O.k_lo + NMX_TID; k < O.k_hi; k += NMX_NT) put(nmx_osc_bin(O, Z, k), sgi, k);
        NMX_SYNC();   // (the next segment overwrites the buffers Z lives in)
      }
    }
    if (stft_cls == NMX_TOL_STFT_SPLIT) {
      // segments beyond one LDS transform: interleaved subsequences, as the FFT and Welch phases (a thread owns its bins)
      for (int sgi = 0; sgi < O.nseg; ++sgi) {
        const int s0 = sgi * O.step;
        nmx_tol_segment_of(O, [&](int i) -> float { return xe(s0 + i); }, bufA, bufB, acc);
        for (int k = O.k_lo + NMX_TID; k < O.k_hi; k += NMX_NT) put(acc[k - O.k_lo], sgi, k);
      }
    }
    NMX_SYNC();
    nmx_emit_bands(O, sspec, O.nseg, A.n_bands, out_row, c, red, rail);
    if (O.return_spectrum)
      for (int k = NMX_TID; k < O.nfreq; k += NMX_NT) {
        float s = 0.f;
        for (int m = 0; m < O.nseg; ++m) s += sspec[k * O.nseg + m];
        out_row[O.psd_cols.base + c * O.psd_cols.ch_stride + k * O.psd_cols.a_stride] = s / (float)O.nseg;
      }
    NMX_SYNC();
  }
}
