// nmx_k_hilbert_long.h -- the Hilbert envelope for series whose two full-length LDS buffers (nmx_hilbert_item: 3 W + 4
// floats) do not fit 160 KiB: up to 40 000 samples, even or odd.  Same NmxHilbertArgs, same result --
// |ifft(fft(y, W) h)| at exactly length W (scipy.signal.hilbert) --, every row stored whole.  Included at the end of
// nmx_k_bank_w64.h; nmx_hilbert_item hands its item over when A.long_mode is set.
//
// W = D M (D = A.split_d <= 64, M = A.sub_m <= 8192 complex points: two LDS buffers of at most 64 KiB).  Both length-W
// transforms are D transforms of M points with the LDS machinery (nmx_fft_auto), split so that neither needs
// accumulators: a transform's result goes straight to where it is read.
//   forward (decimation in frequency): the bins k = j D + r of Y come from ONE M-point transform,
//       Y[j D + r] = FFT_M{ w_W^(n1 r) sum_n2 y[n1 + M n2] w_D^(n2 r) }[j],   n1 < M, n2 < D
//     (contiguous reads of the series, which is resident in L2 after the first r).  Only the bins 0 < k < (W + 1) / 2 are
//     kept, weighted 2 / W, in the workgroup's slab of device memory: the analytic signal's one-sided spectrum without its
//     DC and Nyquist bins -- those two are real and reach only the real part, which IS y.
//   inverse (the same split of the spectrum's index): the samples n = m D + r come from ONE M-point transform,
//       a[m D + r] = IFFT_M{ w_W^(-k1 r) sum_k2 A[k1 + M k2] w_D^(-k2 r) }[m],   k1 < M, k2 < D
//     (contiguous reads of the slab), and env[n] = sqrt(y[n]^2 + Im(a[n])^2).
// Cost beside the transforms: each of the 2 D passes forms a D-term sum per point, D W multiply-adds per direction -- small
// against the transforms for the D = 2 .. 5 of lengths with many divisors (14 000, 16 385, 20 000, 30 000, 40 000; measured:
// profiles/bursts_long.md), quadratic in D for a length like 37 x 1009, whose smallest split is D = 37.  Nothing above D = 5
// has been measured.
// w_W = exp(-2 pi i / W) from A.tw_n, W entries built in float64 on the host; w_D^j = w_W^(j M).
// NMX_SYNC() separates the phases: in a multi-wave workgroup __syncthreads(), which with NMX_GLOBAL_FENCE() in front of it
// also orders the workgroup's stores to its slab before the loads of the inverse.
#pragma once

NMX_DEV void nmx_hilbert_long_item(const NmxHilbertArgs& A, long long item, float* smem, float* slab) {
  float2* bufA = (float2*)(smem + A.off_a);
  float2* bufB = (float2*)(smem + A.off_b);
  const int W = A.W, D = A.split_d, M = A.sub_m;
  const int nh = (W + 1) / 2;   // bins [1, nh) carry weight 2
  const float* src = A.y + item * W;
  float* dst = A.env + item * W;
  const float2* NMX_RESTRICT tw = A.tw_n;
  float2* S = (float2*)slab;    // [nh] one-sided spectrum x 2 / W
  const float sc = 2.f / (float)W;

  for (int r = 0; r < D; ++r) {
    for (int n1 = NMX_TID; n1 < M; n1 += NMX_NT) {
      float2 acc = make_float2(0.f, 0.f);
      int t = 0;   // (n2 r) mod D
      for (int n2 = 0; n2 < D; ++n2) {
        const float yv = src[n1 + M * n2];
        const float2 w = tw[t * M];
        acc.x += yv * w.x;
        acc.y += yv * w.y;
        t += r;
        if (t >= D) t -= D;
      }
      bufB[n1] = r ? nmx_cmul(acc, tw[(int)(((long long)n1 * r) % W)]) : acc;
    }
    NMX_SYNC();
    const float2* Z = nmx_fft_auto<-1>(A.hil_c, bufB, bufA, bufB);
    for (int j = NMX_TID; j < M; j += NMX_NT) {
      const int k = j * D + r;
      if (k < nh) S[k] = k ? make_float2(Z[j].x * sc, Z[j].y * sc) : make_float2(0.f, 0.f);
    }
    NMX_SYNC();   // (the next r overwrites the buffers Z lives in)
  }
  NMX_GLOBAL_FENCE();
  NMX_SYNC();

  for (int r = 0; r < D; ++r) {
    for (int k1 = NMX_TID; k1 < M; k1 += NMX_NT) {
      float2 acc = make_float2(0.f, 0.f);
      int t = 0;   // (k2 r) mod D
      for (int k2 = 0; k2 < D && k1 + M * k2 < nh; ++k2) {
        const float2 a = S[k1 + M * k2];
        const float2 w = tw[t * M];
        acc = nmx_cadd(acc, nmx_cmul(a, make_float2(w.x, -w.y)));
        t += r;
        if (t >= D) t -= D;
      }
      if (r) {
        const float2 w = tw[(int)(((long long)k1 * r) % W)];
        acc = nmx_cmul(acc, make_float2(w.x, -w.y));
      }
      bufB[k1] = acc;
    }
    NMX_SYNC();
    const float2* z = nmx_fft_auto<+1>(A.hil_c, bufB, bufA, bufB);
    for (int m = NMX_TID; m < M; m += NMX_NT) {
      const int n = m * D + r;
      const float re = src[n], im = z[m].y;
      dst[n] = nmx_sqrt_fast(re * re + im * im);
    }
    NMX_SYNC();
  }
}
