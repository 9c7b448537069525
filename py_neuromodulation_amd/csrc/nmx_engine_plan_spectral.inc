// nmx_engine_plan_spectral.inc -- plan building, part 1: FFT factorisation / twiddle tables, the oscillatory families
// (FFT / Welch / STFT bin tables, windows), the wave-level 500- and 510-point tables.  Included by nmx_engine.inc.
// ---- FFT plan ---------------------------------------------------------------------------
bool smooth5(int n) {
  for (int p : {2, 3, 5}) while (n % p == 0) n /= p;
  return n == 1;
}

int build_fft(Plan& P, int n, NmxFft* out, bool allow10 = false) {
  const int key = allow10 ? -n : n;
  auto it = P.fft_cache.find(key);
  if (it != P.fft_cache.end()) { *out = it->second; return 0; }
  NMX_REQUIRE(n >= 1 && n <= 32768, "FFT length out of range");
  NmxFft f{};
  f.n = n;
  std::vector<int> radices;
  int r = n;
  if (allow10)
    while (r % 10 == 0) { radices.push_back(10); r /= 10; }   // fewer LDS passes (1000 = 10^3)
  while (r % 4 == 0) { radices.push_back(4); r /= 4; }
  while (r % 2 == 0) { radices.push_back(2); r /= 2; }
  while (r % 5 == 0) { radices.push_back(5); r /= 5; }
  while (r % 3 == 0) { radices.push_back(3); r /= 3; }
  for (int p = 7; r > 1; p += 2) {
    while (r % p == 0) { radices.push_back(p); r /= p; }
    if (p * p > r && r > 1) { radices.push_back(r); r = 1; }
  }
  // (a prime radix is a direct O(R^2) DFT, (R - 1) / 2 real-coefficient terms per output pair: fine for the odd lengths
  // MNE's padded resampling produces -- 853 = round(2048 * 250 / 600) -- but a 1e-5 result needs R <= 4096 in fp32)
  for (int p : radices) NMX_REQUIRE(p <= 4096, "FFT length has a prime factor > 4096 (unsupported)");
  // large/odd radices first (their strided writes are cheapest while Ns is small)
  std::sort(radices.begin(), radices.end(), [](int a, int b) { return a > b; });
  NMX_REQUIRE((int)radices.size() <= NMX_MAX_STAGES, "too many FFT stages");
  f.nstages = (int)radices.size();
  int ns = 1;
  for (int s = 0; s < f.nstages; ++s) {
    NmxFftStage& st = f.st[s];
    st.radix = radices[s];
    st.ns = ns;
    st.m = n / st.radix;
    st.magic = (unsigned)((1ull << 32) / (unsigned long long)ns + 1ull);
    st.tw_step = n / (ns * st.radix);
    if (ns > 1)
      for (int j = 0; j < st.m; ++j) {
        const unsigned q = (unsigned)(((unsigned long long)j * st.magic) >> 32);
        NMX_REQUIRE((int)q == j / ns, "internal: magic division mismatch");
      }
    ns *= st.radix;
  }
  std::vector<float> tw(2 * (size_t)n), twr(2 * (size_t)(n + 1));
  for (int k = 0; k < n; ++k) {
    const double a = -2.0 * kPi * (double)k / (double)n;
    tw[2 * k] = (float)std::cos(a);
    tw[2 * k + 1] = (float)std::sin(a);
  }
  for (int k = 0; k <= n; ++k) {
    const double a = -2.0 * kPi * (double)k / (double)(2 * n);
    twr[2 * k] = (float)std::cos(a);
    twr[2 * k + 1] = (float)std::sin(a);
  }
  f.tw = (const float2*)upload(P, tw.data(), tw.size() * sizeof(float));
  f.twr = (const float2*)upload(P, twr.data(), twr.size() * sizeof(float));
  if (!f.tw || !f.twr) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  P.fft_cache[key] = f;
  *out = f;
  return 0;
}



int al4(int x) { return (x + 3) & ~3; }

NmxCols cv(const nmx_cols& c) { return NmxCols{c.base, c.ch_stride, c.a_stride, c.b_stride}; }

int popcount4(unsigned e) { return (int)((e & 1) + ((e >> 1) & 1) + ((e >> 2) & 1) + ((e >> 3) & 1)); }

// ---- oscillatory family ---------------------------------------------------------------
// the bins [lo, hi) a family evaluates: the union of its bands (all bins with return_spectrum)
void osc_bin_range(const nmx_plan_desc& d, const nmx_osc_desc& s, int* k_lo, int* k_hi) {
  const int nfreq = s.n / 2 + 1;
  *k_lo = 0;
  *k_hi = nfreq;
  if (s.return_spectrum) return;
  int lo = nfreq, hi = 0;
  for (int b = 0; b < d.n_bands && b < NMX_MAX_BANDS_DEV; ++b)
    if (s.bin_hi[b] > s.bin_lo[b]) { lo = std::min(lo, s.bin_lo[b]); hi = std::max(hi, s.bin_hi[b]); }
  if (hi > lo) { *k_lo = lo; *k_hi = hi; } else { *k_lo = 0; *k_hi = 1; }
}

std::string spaced(int n) {   // 39989 -> "39 989"
  std::string t = std::to_string(n);
  for (int i = (int)t.size() - 3; i > 0; i -= 3) t.insert((size_t)i, " ");
  return t;
}

// Long-window kernel (nmx_k_timeosc_long.h): the smallest D that divides n and leaves a subsequence of M = n / D samples
// whose transform -- M / 2 complex points, M when M is odd -- has at most 8192 points (two LDS buffers of 64 KiB, 31 KiB
// left for the accumulators and the spectrum of a few thousand bins) and factors the FFT engine supports.  0: none.
int long_split(int n) {
  for (int D = 1; D <= 64; ++D) {
    if (n % D) continue;
    const int M = n / D;
    if (M < 2) break;
    int nc = (M & 1) ? M : M / 2, twos = 0, stages = 0;
    if (nc > 8192) continue;
    while (nc % 2 == 0) { nc /= 2; ++twos; }
    bool ok = true;
    for (int p = 3; nc > 1 && ok; ) {   // (build_fft: one stage per odd prime factor, radix 4 for pairs of twos)
      if (nc % p == 0) { nc /= p; ++stages; if (p > 4096) ok = false; }
      else if ((long long)p * p > nc) p = nc;
      else p += 2;
    }
    if (ok && stages + (twos + 1) / 2 <= NMX_MAX_STAGES) return D;
  }
  return 0;
}

// kind: 0 FFT, 1 Welch, 2 STFT.  lng: for the long-window kernel -- `fft` / `complex_full` describe one subsequence
int build_osc(Plan& P, const nmx_osc_desc& s, int kind, NmxOsc* o, int* cplx_len, int* spec_len, bool lng = false) {
  const nmx_plan_desc& d = P.d;
  const int W = d.window;
  std::memset(o, 0, sizeof(*o));
  o->enabled = 1;
  o->n = s.n;
  NMX_REQUIRE(s.n >= 2 && s.n <= W, "oscillatory window must satisfy 2 <= n <= W "
              "(Welch needs W >= int(sfreq): scipy would shrink nperseg and the reference's "
              "frequency grid would no longer match)");
  o->nfreq = s.n / 2 + 1;
  o->complex_full = s.n & 1;
  o->log_transform = s.log_transform;
  o->estimators = s.estimators;
  o->n_est = popcount4(s.estimators);
  o->return_spectrum = s.return_spectrum;
  NMX_REQUIRE(d.n_bands <= NMX_MAX_BANDS_DEV, "too many bands");
  for (int b = 0; b < d.n_bands; ++b) {
    o->bin_lo[b] = s.bin_lo[b];
    o->inv_bins[b] = s.bin_hi[b] > s.bin_lo[b] ? (float)(1.0 / (double)(s.bin_hi[b] - s.bin_lo[b])) : NAN;
    o->bin_hi[b] = s.bin_hi[b];
    NMX_REQUIRE(0 <= s.bin_lo[b] && s.bin_lo[b] <= s.bin_hi[b] && s.bin_hi[b] <= o->nfreq,
                "band bin range outside the frequency grid");
  }
  o->cols = cv(s.cols);
  o->psd_cols = cv(s.psd_cols);
  // only the bins some band reads are evaluated (|X|, log10) and kept in LDS
  osc_bin_range(d, s, &o->k_lo, &o->k_hi);
  int nc = o->complex_full ? s.n : s.n / 2;
  if (lng) {
    const char* fam = kind == 0 ? "fft" : kind == 1 ? "welch" : "stft";
    if (s.return_spectrum && kind != 2)   // (the STFT phase has it: new code behind NMX_LONG_STFT)
      return nmx_fail(NMX_E_UNSUPPORTED, std::string(fam) + ": return_spectrum is not implemented in the long-window time/oscillatory "
                      "kernel (windows above 16 384 samples, or segments whose transform buffers do not fit LDS next to the window)");
    const int D = long_split(s.n);
    NMX_REQUIRE(D > 0, std::string(fam) + ": no supported split of a " + spaced(s.n) + "-point transform (the long-window kernel "
                "needs a divisor D <= 64 with n / D <= 16 384, or <= 8192 when odd, and prime factors <= 4096)");
    o->split_d = D;
    o->sub_m = s.n / D;
    o->complex_full = o->sub_m & 1;
    nc = o->complex_full ? o->sub_m : o->sub_m / 2;
    auto it = P.twn_cache.find(s.n);
    if (it == P.twn_cache.end()) {
      std::vector<float> t(2 * (size_t)s.n);
      for (int k = 0; k < s.n; ++k) {
        const double a = -2.0 * kPi * (double)k / (double)s.n;
        t[2 * k] = (float)std::cos(a);
        t[2 * k + 1] = (float)std::sin(a);
      }
      const float2* p = (const float2*)upload(P, t.data(), t.size() * sizeof(float));
      if (!p) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
      it = P.twn_cache.emplace(s.n, p).first;
    }
    o->tw_n = it->second;
  }
  int rc = build_fft(P, nc, &o->fft);
  if (rc) return rc;
  *cplx_len = nc;
  std::vector<float> win(s.n);
  if (kind == 0) {
    o->nseg = 1;
    o->step = s.n;
    o->scale = 1.f;
  } else if (kind == 1) {  // scipy.signal.welch(window="hann", noverlap=None), density scaling
    double sw2 = 0;
    for (int i = 0; i < s.n; ++i) {
      const double w = 0.5 - 0.5 * std::cos(2.0 * kPi * i / s.n);
      win[i] = (float)w;
      sw2 += w * w;
    }
    o->step = s.n - s.n / 2;
    o->nseg = (W - s.n) / o->step + 1;
    o->scale = (float)(1.0 / (std::floor(d.sfreq) * sw2));
  } else {  // scipy.signal.stft(window="hamming", boundary="even"), spectrum scaling
    double sw = 0;
    for (int i = 0; i < s.n; ++i) {
      const double w = 0.54 - 0.46 * std::cos(2.0 * kPi * i / s.n);
      win[i] = (float)w;
      sw += w;
    }
    o->half = s.n / 2;
    o->step = s.n - s.n / 2;
    NMX_REQUIRE(o->half <= W - 1, "STFT nperseg too long for the even extension");
    const int lext = W + 2 * o->half;
    const int nadd = ((-(lext - s.n)) % o->step + o->step) % o->step % s.n;
    o->nseg = (lext + nadd - s.n) / o->step + 1;
    o->scale = (float)(1.0 / sw);
    o->nadd = nadd;
    // share of a constant in a segment's spectrum (NmxOsc::wdc), float64: periodic hamming -> 0.54 n at bin 0,
    // -0.23 n at bin 1 and rounding noise elsewhere for a full segment; every bin for the zero-padded one
    std::vector<float> wdc((size_t)4 * o->nfreq, 0.f);
    for (int sel = 0; sel < 2; ++sel) {
      const int nv = sel ? s.n - nadd : s.n;
      if (nv == s.n && s.n > 4) {   // the closed form (no n x nfreq trigonometric sums at plan time)
        wdc[2 * ((size_t)sel * o->nfreq)] = (float)(0.54 * s.n);
        wdc[2 * ((size_t)sel * o->nfreq + 1)] = (float)(-0.23 * s.n);
        continue;
      }
      if (lng && s.n > 4) {
        // long-window plans (nperseg up to 20 000: the sums below would be 10^8 sincos pairs): the truncated window's
        // transform in closed form, float64 -- the hamming window is three exponentials, each a geometric sum over i < nv:
        //   0.54 G(k) - 0.23 G(k - 1) - 0.23 G(k + 1),  G(m) = (1 - e^(-2 pi i m nv / n)) / (1 - e^(-2 pi i m / n)),  G(0) = nv
        auto G = [&](int m, double* gr, double* gi) {
          const long long mm = ((long long)m % s.n + s.n) % s.n;
          if (mm == 0) { *gr = (double)nv; *gi = 0.0; return; }
          const double a1 = -2.0 * kPi * (double)mm / s.n, an = -2.0 * kPi * (double)((mm * nv) % s.n) / s.n;
          const double pr = 1.0 - std::cos(an), pi = -std::sin(an), qr = 1.0 - std::cos(a1), qi = -std::sin(a1);
          const double q2 = qr * qr + qi * qi;
          *gr = (pr * qr + pi * qi) / q2;
          *gi = (pi * qr - pr * qi) / q2;
        };
        for (int k = 0; k < o->nfreq; ++k) {
          double r0, i0, rm, im1, rp, ip;
          G(k, &r0, &i0); G(k - 1, &rm, &im1); G(k + 1, &rp, &ip);
          double re = 0.54 * r0 - 0.23 * (rm + rp), im = 0.54 * i0 - 0.23 * (im1 + ip);
          if (std::fabs(re) < 1e-9 * s.n) re = 0;
          if (std::fabs(im) < 1e-9 * s.n) im = 0;
          wdc[2 * ((size_t)sel * o->nfreq + k)] = (float)re;
          wdc[2 * ((size_t)sel * o->nfreq + k) + 1] = (float)im;
        }
        continue;
      }
      for (int k = 0; k < o->nfreq; ++k) {
        double re = 0, im = 0;
        for (int i = 0; i < nv; ++i) {
          const double w = 0.54 - 0.46 * std::cos(2.0 * kPi * i / s.n);
          const double ang = -2.0 * kPi * (double)(((long long)i * k) % s.n) / s.n;
          re += w * std::cos(ang);
          im += w * std::sin(ang);
        }
        if (std::fabs(re) < 1e-9 * s.n) re = 0;   // exact zeros of the periodic window's transform
        if (std::fabs(im) < 1e-9 * s.n) im = 0;
        wdc[2 * ((size_t)sel * o->nfreq + k)] = (float)re;
        wdc[2 * ((size_t)sel * o->nfreq + k) + 1] = (float)im;
      }
    }
    o->wdc = (const float2*)upload(P, wdc.data(), wdc.size() * sizeof(float));
    if (!o->wdc) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  o->log10_scale = (float)std::log10((double)o->scale);
  if (kind != 0) {
    o->win = (const float*)upload(P, win.data(), win.size() * sizeof(float));
    if (!o->win) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  *spec_len = (o->k_hi - o->k_lo) * o->nseg;
  return 0;
}

// tables of the wave-level 500-point transform (layout: nmx_k_fft500.h), shared by the Hilbert and the
// time / oscillatory wave kernels of the default window length (1000 samples)
int build_w500_tab(Plan& P) {
  if (P.w500_tab) return 0;
  std::vector<float> t(NMX_W500_TAB_FLOATS);
  auto put = [&](int i, double ang, double scale) {
    t[2 * i] = (float)(scale * std::cos(ang));
    t[2 * i + 1] = (float)(scale * std::sin(ang));
  };
  for (int lane = 0; lane < 64; ++lane) {
    const int l = lane < 50 ? lane : 0, k = l % 10;
    for (int r = 1; r < 10; ++r) put((r - 1) * 64 + lane, -2.0 * kPi * ((5 * k * r) % 500) / 500.0, 1.0);
    for (int r = 1; r < 5; ++r) {
      put((8 + r) * 64 + lane, -2.0 * kPi * ((l * r) % 500) / 500.0, 1.0);
      put((12 + r) * 64 + lane, -2.0 * kPi * (((l + 50) * r) % 500) / 500.0, 1.0);
    }
  }
  for (int k = 0; k < NMX_W500_CS_N; ++k) put(NMX_W500_TW_N + k, 2.0 * kPi * k / 1000.0, k ? 2.0 / 1000.0 : 0.0);
  P.w500_tab = (const float*)upload(P, t.data(), t.size() * sizeof(float));
  if (!P.w500_tab) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  return 0;
}

// the time / oscillatory kernel (be_launch_timeosc), in this order of precedence.  (The logic emulator runs the matrix-pipe
// kernel's arithmetic or the generic item.)
NmxTimeOscKind timeosc_kind(const Plan& P, const NmxTimeOscArgs& A) {
  if (A.long_mode) return NMX_TO_LONG;   // windows / segments beyond the generic LDS layout (build_timeosc)
#ifndef NMX_HOST_EMU
  // no oscillatory feature: the register-resident scan (one wave per window, no LDS)
  if (!A.fft.enabled && !A.welch.enabled && !A.stft.enabled && A.W <= 1024 && A.W >= 3 && env_int("NMX_SCAN_KERNEL", 1)) return NMX_TO_SCAN;
#endif
  // (any batch size, one window included: a result must not depend on how the hops were batched)
  if (A.smm_tab && nmx_specmm_ok(A)) return NMX_TO_SPECMM;
#ifndef NMX_HOST_EMU
  // default shape (W = 1000, band means): one wave per item, wave-level 500-point transforms; the persistent form for the
  // bands below bin 100
  if (A.w500_tab && nmx_timeosc_w1000_ok(A))
    return nmx_timeosc_w1000_low_ok(A) && env_int("NMX_TOW_PERSISTENT", 1) ? NMX_TO_W1000_LOW : NMX_TO_W1000;
  if (A.w500_tab && nmx_timeosc_stft500_ok(A)) return NMX_TO_STFT500;
  // 510-sample FFT / STFT segments (17 ms at 30 kHz): one wave per item, in-place prime-factor transforms
  if (A.w510_tab && nmx_timeosc_w510_ok(A, A.w510_tab)) return NMX_TO_W510;
  if (P.timeosc.nt == 128) return NMX_TO_FIXED128;
#endif
  return NMX_TO_GENERIC;
}

int build_timeosc(Plan& P) {
  const nmx_plan_desc& d = P.d;
  const unsigned mask = NMX_F_HJORTH | NMX_F_RAW | NMX_F_LINELENGTH | NMX_F_FFT | NMX_F_WELCH | NMX_F_STFT;
  if (!(d.features & mask)) return 0;
  TimeOscStage& S = P.timeosc;
  S.nt = d.window <= 1024 ? 128 : 256;
  NmxTimeOscArgs& A = S.a;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.W = d.window;
  A.n_bands = d.n_bands;
  A.features = d.features;
  A.hjorth_cols = cv(d.hjorth_cols);
  A.raw_cols = cv(d.raw_cols);
  A.ll_cols = cv(d.linelength_cols);
  int maxc = 1, maxspec = 1, rc;
  // The long-window kernel (NMX_TO_LONG) takes every plan above 16 384 samples, and below that every plan without STFT whose
  // generic layout -- window + two transform buffers + spectrum -- does not fit LDS (FFT / Welch segments above ~13 650
  // samples).  A plan whose generic layout fits keeps it.
  // With NMX_LONG_STFT=1 (the opt-in of nmx_plan_create) the same holds for plans with STFT; without it such a plan below
  // 16 384 samples is laid out generically, and refused where that does not fit.
  bool lng = d.window > 16384;
  const bool long_stft = env_int("NMX_LONG_STFT", 0) != 0;
  if (!lng && (!(d.features & NMX_F_STFT) || long_stft)) {
    int gc = 1, gs = 1;
    for (int kind = 0; kind < 3; ++kind) {
      const nmx_osc_desc& s = kind == 0 ? d.fft : kind == 1 ? d.welch : d.stft;
      if (!(d.features & (kind == 0 ? NMX_F_FFT : kind == 1 ? NMX_F_WELCH : NMX_F_STFT)) || s.n < 2 || s.n > d.window) continue;
      int lo, hi;
      osc_bin_range(d, s, &lo, &hi);
      const int step = s.n - s.n / 2;
      int nseg = kind ? (d.window - s.n) / step + 1 : 1;
      if (kind == 2) {   // (build_osc: scipy's even extension and padding)
        const int lext = d.window + 2 * (s.n / 2), nadd = ((-(lext - s.n)) % step + step) % step % s.n;
        nseg = (lext + nadd - s.n) / step + 1;
      }
      gc = std::max(gc, (s.n & 1) ? s.n : s.n / 2);
      gs = std::max(gs, (hi - lo) * nseg);
    }
    lng = ((long long)al4(d.window) + 2ll * al4(2 * gc) + al4(gs) + 64) * 4 > 160 * 1024;
  }
  auto add = [&](const nmx_osc_desc& s, int kind, NmxOsc* o) -> int {
    int c = 0, sp = 0;
    int r = build_osc(P, s, kind, o, &c, &sp, lng);
    if (r) return r;
    maxc = std::max(maxc, c);
    maxspec = std::max(maxspec, sp);
    return 0;
  };
  if (d.features & NMX_F_FFT) if ((rc = add(d.fft, 0, &A.fft))) return rc;
  if (d.features & NMX_F_WELCH) if ((rc = add(d.welch, 1, &A.welch))) return rc;
  if (d.features & NMX_F_STFT) if ((rc = add(d.stft, 2, &A.stft))) return rc;
  // per-wave STFT needs room for (threads / 64) transforms of 250 points in each buffer
  A.stft_per_wave = (d.features & NMX_F_STFT) && maxc >= 250 * (S.nt / 64);
  A.long_mode = 0; A.long_nb = 0; A.long_spec_slab = 0; A.slab_floats = 0; A.slab_blocks = 0; A.slab = nullptr;
  A.long_sp_floats = 0; A.long_stft = 0; A.long_stft_acc = 0;
  if (lng) {
    // the window at [0, W) for the time-domain phase; then two transform buffers of one subsequence over it, the
    // accumulators (long_nb complex) and the spectrum (long_nb floats) behind them -- or in the workgroup's slab
    A.long_mode = 1;
    A.long_nb = 0;
    if (d.features & NMX_F_FFT) A.long_nb = std::max(A.long_nb, al4(A.fft.k_hi - A.fft.k_lo));
    if (d.features & NMX_F_WELCH) A.long_nb = std::max(A.long_nb, al4(A.welch.k_hi - A.welch.k_lo));
    A.long_sp_floats = 3 * A.long_nb;
    if (d.features & NMX_F_STFT) {
      // the segment class (nmx_k_timeosc_long.h).  The per-wave class is the device's (as in the generic item) and needs a
      // slice of 250 complex points per wave in each buffer; the split class keeps accumulators in front of the spectrum
      A.long_stft = A.stft.n <= 64 ? NMX_TOL_STFT_DIRECT : A.stft.split_d > 1 ? NMX_TOL_STFT_SPLIT : NMX_TOL_STFT_LDS;
#ifndef NMX_HOST_EMU
      if (A.stft.n == 500 && env_int("NMX_LONG_STFT_PER_WAVE", 1)) {
        A.long_stft = NMX_TOL_STFT_WAVE500;
        maxc = std::max(maxc, 250 * (512 / 64));   // (nmx_timeosc_long.hip: NMX_BLOCK_FIXED = 512)
      }
#endif
      A.long_stft_acc = A.long_stft == NMX_TOL_STFT_SPLIT ? 2 * al4(A.stft.k_hi - A.stft.k_lo) : 0;
      A.long_sp_floats = std::max(A.long_sp_floats, A.long_stft_acc + al4((A.stft.k_hi - A.stft.k_lo) * A.stft.nseg));
    }
    const bool osc = (d.features & (NMX_F_FFT | NMX_F_WELCH | NMX_F_STFT)) != 0;
    A.off_x = 0;
    A.off_a = 0;
    A.off_b = osc ? al4(2 * maxc) : 0;
    A.off_spec = osc ? A.off_b + al4(2 * maxc) : 0;
    int end = A.off_spec + A.long_sp_floats;
    if ((size_t)(std::max(end, al4(A.W)) + 64) * 4 > 160 * 1024) {
      A.long_spec_slab = 1;
      A.slab_floats = A.long_sp_floats;
      end = A.off_spec;
    }
    A.off_red = std::max(end, al4(A.W));
    A.lds_floats = A.off_red + 64;
    NMX_REQUIRE((size_t)A.lds_floats * 4 <= 160 * 1024, "time/oscillatory kernel needs more than 160 KiB LDS");
    // one workgroup per CU (the layout is at least half of its LDS), NMX_TIMEOSC_LONG_BLOCKS caps the grid; the slabs --
    // where a plan needs them: at most 3 x 20 001 floats each -- within 64 MiB of device memory
    A.slab_blocks = 1;
#ifndef NMX_HOST_EMU
    A.slab_blocks = slab_workgroups(P, (size_t)A.lds_floats * 4, (size_t)A.slab_floats, env_int("NMX_TIMEOSC_LONG_BLOCKS", 0));
#endif
    if (A.slab_floats > 0) {
      A.slab = (float*)plan_alloc(P, (size_t)A.slab_blocks * A.slab_floats * sizeof(float));
      if (!A.slab) return nmx_fail(NMX_E_NOMEM, "time/oscillatory slab allocation failed");
    }
  } else {
    A.off_x = 0;
    A.off_a = al4(A.W);
    A.off_b = A.off_a + al4(2 * maxc);
    A.off_spec = A.off_b + al4(2 * maxc);
    A.off_red = A.off_spec + al4(maxspec);
    A.lds_floats = A.off_red + 64;
    NMX_REQUIRE(A.lds_floats * 4 <= 160 * 1024, "time/oscillatory kernel needs more than 160 KiB LDS");
  }
  A.w500_tab = nullptr;
  const bool stft500 = (d.features & NMX_F_STFT) && !(d.features & (NMX_F_FFT | NMX_F_WELCH)) && A.stft.n == 500 && d.window <= 2048;
  if ((d.window == 1000 || stft500) && env_int("NMX_TIMEOSC_W1000", 1)) {
    int rc2 = build_w500_tab(P);
    if (rc2) return rc2;
    A.w500_tab = P.w500_tab;
  }
  A.smm_tab = nullptr;
  A.smm_k0 = 0;
  A.starts_mod4 = 0;
  A.todo = nullptr;
  // the matrix-pipe spectrum kernel (nmx_k_specmm.h; the logic emulator runs its arithmetic: nmx_specmm_item_emu): FFT band means whose bins fit 32 consecutive rows, no Welch / STFT
  if (d.window == 1000 && (d.features & NMX_F_FFT) && !(d.features & (NMX_F_WELCH | NMX_F_STFT)) && A.fft.n == 1000 &&
      !A.fft.complex_full && A.fft.estimators == NMXD_EST_MEAN && !A.fft.return_spectrum && A.fft.k_lo >= 1 &&
      A.fft.k_hi - A.fft.k_lo <= 32 && A.fft.k_hi <= 500 && env_int("NMX_SPECMM", 1)) {
    // [class: cos even k, cos odd k, sin even k, sin odd k][granule G = n / 4][row][n % 4], n = 0 .. 249 of the twice-folded
    // half-sample-phase transform (nmx_k_specmm.h); row r of a class is bin (first even / odd k >= k_lo) + 2 r; rows past
    // k_hi and n = 250, 251 are zero
    std::vector<float> t((size_t)NMX_SMM_TAB_FLOATS, 0.f);
    const int ke0 = A.fft.k_lo + (A.fft.k_lo & 1), ko0 = A.fft.k_lo + 1 - (A.fft.k_lo & 1);
    for (int X = 0; X < 4; ++X)
      for (int r = 0; r < 16; ++r) {
        const int k = ((X & 1) ? ko0 : ke0) + 2 * r;
        if (k >= A.fft.k_hi) continue;
        for (int n = 0; n < 250; ++n) {
          const long long m = ((long long)k * (2 * n + 1)) % 2000;   // phi = pi m / 1000
          const double a = kPi * (double)m / 1000.0;
          t[(((size_t)X * NMX_SMM_NG + (size_t)(n >> 2)) * 16 + (size_t)r) * 4 + (size_t)(n & 3)] = (float)(X < 2 ? std::cos(a) : std::sin(a));
        }
      }
    A.smm_tab = (const float*)upload(P, t.data(), t.size() * sizeof(float));
    if (!A.smm_tab) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
    A.smm_k0 = A.fft.k_lo;
  }
  A.w510_tab = nullptr;
#ifndef NMX_HOST_EMU
  if (env_int("NMX_TIMEOSC_W510", 1) && (((d.features & NMX_F_FFT) && A.fft.n == 510) || ((d.features & NMX_F_STFT) && A.stft.n == 510))) {
    // position tables of the in-place prime-factor 510-point transform (nmx_k_timeosc_w510.h, tools/model_pfa510.py)
    const int N = 510, dims[4] = {2, 3, 5, 17};
    int inv[4];
    for (int i = 0; i < 4; ++i) {
      const int s = N / dims[i];
      inv[i] = 0;
      for (int t = 1; t < dims[i]; ++t) if ((s * t) % dims[i] == 1) inv[i] = t;
    }
    auto coord = [&](int p, int i) { return (p * inv[i]) % dims[i]; };
    std::vector<unsigned short> t(800, 0);
    int n10 = 0, n3 = 0, n17 = 0;
    for (int p = 0; p < N; ++p) {
      if (coord(p, 0) == 0 && coord(p, 2) == 0) t[0 + n10++] = (unsigned short)p;
      if (coord(p, 1) == 0) t[64 + n3++] = (unsigned short)p;
      if (coord(p, 3) == 0) t[256 + n17++] = (unsigned short)p;
      int k = 0;
      for (int i = 0; i < 4; ++i) k += coord(p, i) * (N / dims[i]) * inv[i];
      t[288 + k % N] = (unsigned short)p;
    }
    NMX_REQUIRE(n10 == 51 && n3 == 170 && n17 == 30, "internal: prime-factor tables");
    A.w510_tab = (const unsigned short*)upload(P, t.data(), t.size() * sizeof(unsigned short));
    if (!A.w510_tab) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
#endif
  S.kind = timeosc_kind(P, A);
  S.takes_dc = S.kind != NMX_TO_STFT500 && S.kind != NMX_TO_W510;
  P.have_timeosc = true;
  return 0;
}

// the time / oscillatory features of one chunk (nw hops) from the windows `v`.  (The matrix-pipe kernel's redo launch --
// the windows it flagged: NaN / infinity on load -- stays outside the stage's timer and kernel list.)
static int launch_timeosc_stage(Plan& P, const WinView& v, int nw, float* d_out, be_stream_t s, bool tev, bool& dc_made) {
  if (!P.have_timeosc) return 0;
  TimeOscStage& S = P.timeosc;
  const int C = P.d.n_channels;
  int rc;
  NmxTimeOscArgs A = S.a;
  A.out = d_out;
  A.starts_mod4 = (!v.starts || P.starts_mod4) ? 1 : 0;
  if ((rc = dc_bind(P, A, S.takes_dc, v, nw, s, dc_made))) return rc;
  A.todo = nullptr;
  const bool smm = S.kind == NMX_TO_SPECMM;
  if (smm) {   // flags of the matrix-pipe kernel (nmx_k_specmm.h): a 16-bit mask per tile of 16 windows
    if ((rc = ensure(S.todo, (size_t)((nw + 15) / 16) * C * sizeof(unsigned short)))) return rc;
    A.todo = (unsigned short*)S.todo.p;
  }
  if (tev) be_timer_start(P.timers[ST_TIMEOSC], s);
  be_stage(ST_TIMEOSC);
  be_launch_timeosc(A, S.kind, nw * C, S.nt, (size_t)A.lds_floats * 4, P.n_cu, s);
  if (tev) be_timer_stop(P.timers[ST_TIMEOSC], s);
  if (smm) { be_stage(ST_BATCH); be_launch_timeosc_redo(A, nw * C, s); }
  return 0;
}

// ---- coherence between channel pairs (nmx_k_coh.h) --------------------------------------------------------------------
int build_coh(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!(d.features & NMX_F_COHERENCE) || d.coh_n_pairs <= 0) return 0;
  const int W = d.window, n = d.coh_nperseg, C = d.n_channels;
  NMX_REQUIRE(d.coh_pairs, "coherence: coh_pairs is NULL");
  NMX_REQUIRE(n >= 2 && n <= W && n <= NMX_COH_MAX_N,
              "coherence: nperseg (clamped to the window) must lie in [2, 4096]");
  NMX_REQUIRE(d.coh_methods & 1u, "coherence: method coh must be enabled (the reference fails without it)");
  NMX_REQUIRE(d.coh_n_bands >= 0 && d.coh_n_bands <= NMX_MAX_BANDS_DEV, "coherence: too many bands");
  NmxCohArgs& A = P.coherence.a;
  A = NmxCohArgs{};
  A.n = n;
  A.step = n - n / 2;
  A.nseg = (W - n) / A.step + 1;
  A.nfreq = n / 2 + 1;
  A.W = W;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_pairs = d.coh_n_pairs;
  A.n_bands = d.coh_n_bands;
  for (int b = 0; b < d.coh_n_bands; ++b) {
    NMX_REQUIRE(0 <= d.coh_bin_lo[b] && d.coh_bin_lo[b] <= d.coh_bin_hi[b] && d.coh_bin_hi[b] <= A.nfreq,
                "coherence: band bin range outside the frequency grid");
    A.bin_lo[b] = d.coh_bin_lo[b];
    A.bin_hi[b] = d.coh_bin_hi[b];
  }
  A.feats = d.coh_features & 7u;
  A.methods = d.coh_methods & 3u;
  A.df = d.coh_df;
  A.cols = cv(d.coh_cols);
  // every column the plan writes must lie inside the row
  const int nfb = (int)(A.feats & 1u) + (int)((A.feats >> 1) & 1u);
  const int slots = d.coh_n_bands * nfb + ((A.feats & 4u) ? 1 : 0);
  const int n_meth = (A.methods & 2u) ? 2 : 1;
  if (slots > 0) {
    const long long last = (long long)A.cols.base + (long long)(A.n_pairs - 1) * A.cols.a_stride +
                           (long long)(n_meth - 1) * A.cols.b_stride + (slots - 1);
    NMX_REQUIRE(A.cols.base >= 0 && A.cols.a_stride >= 0 && A.cols.b_stride >= 0 && last < d.n_outputs,
                "coherence: output columns outside the row");
  }
  std::vector<int> pairs(2 * (size_t)A.n_pairs);
  for (int i = 0; i < 2 * A.n_pairs; ++i) {
    NMX_REQUIRE(d.coh_pairs[i] >= 0 && d.coh_pairs[i] < C, "coherence: pair channel index out of range");
    pairs[i] = d.coh_pairs[i];
  }
  int rc = build_fft(P, n, &A.fft);
  if (rc) return rc;
  std::vector<float> win(n);
  for (int i = 0; i < n; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)i / (double)n));   // periodic Hann
  A.win = (const float*)upload(P, win.data(), win.size() * sizeof(float));
  A.pairs = (const int*)upload(P, pairs.data(), pairs.size() * sizeof(int));
  if (!A.win || !A.pairs) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  A.off_a = 0;
  A.off_b = 2 * n;
  A.off_acc = 4 * n;
  A.off_red = A.off_acc + 4 * al4(A.nfreq);
  A.lds_floats = A.off_red + 64 + 2 * 128 + 16;
  P.have_coh = true;
  return 0;
}

// coherence of one chunk from the windows `v`: on the main stream, behind the time / oscillatory kernel
static void launch_coh_stage(Plan& P, const WinView& v, int nw, float* d_out, be_stream_t s, bool tev) {
  if (!P.have_coh) return;
  NmxCohArgs A = P.coherence.a;
  view_into(A, v);
  A.out = d_out;
  if (tev) be_timer_start(P.timers[ST_COH], s);
  be_stage(ST_COH);
  be_launch_coh(A, nw * A.n_pairs, s);
  if (tev) be_timer_stop(P.timers[ST_COH], s);
}

// ---- nolds: sample entropy, Hurst exponent and DFA of the window and of band series of it (nmx_k_nolds.h) ----------------------------------------
int build_nolds_bands(Plan& P);   // the band filters: nmx_engine_plan_fir.inc, beside the other FIR stages
static int launch_nolds_bands(Plan& P, const WinView& v, int nw, be_stream_t s, bool& dc_made);

int build_nolds(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!(d.features & NMX_F_NOLDS)) return 0;
  NMX_REQUIRE(d.nolds_n_bands >= 0 && d.nolds_n_bands <= NMX_MAX_BANDS, "nolds: nolds_n_bands out of range");
  const int n_series = (d.nolds_raw ? 1 : 0) + d.nolds_n_bands;
  if (n_series == 0 || d.nolds_measures == 0) return 0;   // (nothing to compute: the reference emits no key either)
  const bool dfa = (d.nolds_measures & NMX_NOLDS_DFA) && d.nolds_dfa_fit == 1;
  NMX_REQUIRE(d.nolds_dfa_fit == 0 || d.nolds_dfa_fit == 1, "nolds: nolds_dfa_fit must be 0 (off) or 1 (\"poly\")");
  const bool hurst = (d.nolds_measures & NMX_NOLDS_HURST) && d.nolds_hurst_fit == 1;
  NMX_REQUIRE(d.nolds_hurst_fit == 0 || d.nolds_hurst_fit == 1, "nolds: nolds_hurst_fit must be 0 (off) or 1 (\"poly\")");
  if (d.nolds_measures & ~(NMX_NOLDS_SAMPEN | (dfa ? NMX_NOLDS_DFA : 0u) | (hurst ? NMX_NOLDS_HURST : 0u)))
    return nmx_fail(NMX_E_UNSUPPORTED, "nolds: only sample_entropy has a kernel (correlation_dimension, lyapunov_exponent, "
                    "hurst_exponent and detrended_fluctuation_analysis end in the reference's unseeded RANSAC line fit)");
  NMX_REQUIRE(d.window <= NMX_NOLDS_MAX_N, "nolds: a series holds at most 40 000 samples (it has to fit the CU's LDS)");
  NMX_REQUIRE(std::isfinite(d.nolds_tol_factor) && d.nolds_tol_factor >= 0.0 && d.nolds_ddof >= 0, "nolds: tol factor / ddof");
  NmxNoldsArgs& A = P.nolds.a;
  A = NmxNoldsArgs{};
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.W = d.window;
  A.raw = d.nolds_raw ? 1 : 0;
  A.n_band = d.nolds_n_bands;
  A.tol_factor = d.nolds_tol_factor;
  A.ddof = d.nolds_ddof;
  A.cols = cv(d.nolds_cols);
  // every column the stage writes must lie inside the row
  const long long last = (long long)A.cols.base + (long long)(d.n_channels - 1) * A.cols.ch_stride +
                         (long long)(n_series - 1) * A.cols.a_stride;
  NMX_REQUIRE(A.cols.base >= 0 && A.cols.ch_stride >= 0 && A.cols.a_stride >= 0 && last < d.n_outputs,
              "nolds: output columns outside the row");
  A.lds_floats = al4(d.window) + 64;
  P.nolds.have_sampen = (d.nolds_measures & NMX_NOLDS_SAMPEN) != 0;
  if (dfa) {
    const int S = d.nolds_dfa_n_scales;
    NMX_REQUIRE(d.nolds_dfa_scales && S >= 2 && S <= NMX_NOLDS_DFA_MAX_SCALES, "nolds: DFA needs a table of 2 .. 64 scales");
    for (int k = 0; k < S; ++k)
      NMX_REQUIRE(d.nolds_dfa_scales[k] >= 2 && d.nolds_dfa_scales[k] < d.window && (k == 0 || d.nolds_dfa_scales[k] > d.nolds_dfa_scales[k - 1]),
                  "nolds: DFA scales must ascend within [2, window - 1]");
    NmxNoldsDfaArgs& D = P.nolds.dfa;
    D = NmxNoldsDfaArgs{};
    D.s = A;
    D.s.cols = cv(d.nolds_dfa_cols);
    const long long dlast = (long long)D.s.cols.base + (long long)(d.n_channels - 1) * D.s.cols.ch_stride +
                            (long long)(n_series - 1) * D.s.cols.a_stride;
    NMX_REQUIRE(D.s.cols.base >= 0 && D.s.cols.ch_stride >= 0 && D.s.cols.a_stride >= 0 && dlast < d.n_outputs,
                "nolds: DFA output columns outside the row");
    D.n_scales = S;
    D.scales = (const int*)upload(P, d.nolds_dfa_scales, (size_t)S * sizeof(int));
    if (!D.scales) return nmx_fail(NMX_E_NOMEM, "nolds: DFA scale table");
    D.lds_floats = al4(d.window) + 64 + 2 * S;
    P.d.nolds_dfa_scales = nullptr;   // (copied: the caller's array may go)
    P.nolds.have_dfa = true;
  }
  if (hurst) {
    const int S = d.nolds_hurst_n_scales;
    NMX_REQUIRE(d.nolds_hurst_scales && d.nolds_hurst_log_expected && S >= 2 && S <= NMX_NOLDS_HURST_MAX_SCALES,
                "nolds: the Hurst exponent needs tables of 2 .. 15 scales");
    for (int k = 0; k < S; ++k) {
      NMX_REQUIRE(d.nolds_hurst_scales[k] >= 2 && d.nolds_hurst_scales[k] < d.window &&
                  (k == 0 || d.nolds_hurst_scales[k] > d.nolds_hurst_scales[k - 1]),
                  "nolds: Hurst scales must ascend within [2, window - 1]");
      NMX_REQUIRE(std::isfinite(d.nolds_hurst_log_expected[k]), "nolds: Hurst ln E(n) must be finite");
    }
    NmxNoldsHurstArgs& H = P.nolds.hurst;
    H = NmxNoldsHurstArgs{};
    H.s = A;
    H.s.cols = cv(d.nolds_hurst_cols);
    const long long hlast = (long long)H.s.cols.base + (long long)(d.n_channels - 1) * H.s.cols.ch_stride +
                            (long long)(n_series - 1) * H.s.cols.a_stride;
    NMX_REQUIRE(H.s.cols.base >= 0 && H.s.cols.ch_stride >= 0 && H.s.cols.a_stride >= 0 && hlast < d.n_outputs,
                "nolds: Hurst output columns outside the row");
    H.n_scales = S;
    H.lanes = nmx_nolds_hurst_lanes(d.window);
    H.scales = (const int*)upload(P, d.nolds_hurst_scales, (size_t)S * sizeof(int));
    H.log_e = (const double*)upload(P, d.nolds_hurst_log_expected, (size_t)S * sizeof(double));
    if (!H.scales || !H.log_e) return nmx_fail(NMX_E_NOMEM, "nolds: Hurst tables");
    H.lds_floats = al4(d.window) + 64 + 2 * S + al4(S);
    P.d.nolds_hurst_scales = nullptr;   // (copied: the caller's arrays may go)
    P.d.nolds_hurst_log_expected = nullptr;
    P.nolds.have_hurst = true;
  }
  int rc = build_nolds_bands(P);
  if (rc) return rc;
  P.have_nolds = true;
  return 0;
}

// nolds of one chunk from the windows `v`: on the main stream, behind the time / oscillatory kernel
static int launch_nolds_stage(Plan& P, const WinView& v, int nw, float* d_out, be_stream_t s, bool tev, bool& dc_made) {
  if (!P.have_nolds) return 0;
  NmxNoldsArgs A = P.nolds.a;
  view_into(A, v);
  A.dcf = dc_table(P);
  A.out = d_out;
  if (tev) be_timer_start(P.timers[ST_NOLDS], s);
  be_stage(ST_NOLDS);
  int rc = 0;
  if (P.nolds.have_fir && !(rc = launch_nolds_bands(P, v, nw, s, dc_made))) A.yb = (const float*)P.nolds.yb.p;
  const int n_items = nw * (A.raw + A.n_band) * A.n_channels;
  NoldsStage& N = P.nolds;
  if (!rc && N.h_probe) {   // (nmx_nolds_probe)
    if (!(rc = ensure(N.d_probe, (size_t)n_items * 4 * sizeof(unsigned)))) A.probe = (unsigned*)N.d_probe.p;
    if (!rc && N.h_series && !(rc = ensure(N.d_series, (size_t)n_items * A.W * sizeof(float)))) A.series_out = (float*)N.d_series.p;
  }
  if (!rc && N.have_sampen) be_launch_nolds(A, n_items, s);
  if (!rc && N.h_probe) {
    const size_t per_hop = (size_t)(A.raw + A.n_band) * A.n_channels;
    be_d2h_async(N.h_probe + (size_t)N.probe_w0 * per_hop * 4, A.probe, (size_t)n_items * 4 * sizeof(unsigned), s);
    if (A.series_out)
      be_d2h_async(N.h_series + (size_t)N.probe_w0 * per_hop * A.W, A.series_out, (size_t)n_items * A.W * sizeof(float), s);
  }
  if (!rc && N.have_hurst) {   // the same series, the Hurst columns
    NmxNoldsHurstArgs H = N.hurst;
    const NmxCols hcols = H.s.cols;
    H.s = A;
    H.s.cols = hcols;
    H.s.probe = nullptr;
    H.s.series_out = nullptr;
    const size_t per_item = 2 * (size_t)H.n_scales + 3, per_hop = (size_t)(A.raw + A.n_band) * A.n_channels;
    if (N.h_hurst) {   // (nmx_nolds_hurst_probe)
      if (!(rc = ensure(N.d_hurst, (size_t)n_items * per_item * sizeof(double)))) H.probe = (double*)N.d_hurst.p;
      if (!rc && N.h_series && !(rc = ensure(N.d_series, (size_t)n_items * A.W * sizeof(float)))) H.s.series_out = (float*)N.d_series.p;
    }
    if (!rc) be_launch_nolds_hurst(H, n_items, s);
    if (!rc && N.h_hurst) {
      be_d2h_async(N.h_hurst + (size_t)N.probe_w0 * per_hop * per_item, H.probe, (size_t)n_items * per_item * sizeof(double), s);
      if (H.s.series_out)
        be_d2h_async(N.h_series + (size_t)N.probe_w0 * per_hop * A.W, H.s.series_out, (size_t)n_items * A.W * sizeof(float), s);
    }
  }
  if (!rc && N.have_dfa) {   // the same series, the DFA columns
    NmxNoldsDfaArgs D = N.dfa;
    const NmxCols dcols = D.s.cols;
    D.s = A;
    D.s.cols = dcols;
    D.s.probe = nullptr;
    D.s.series_out = nullptr;
    const size_t per_item = (size_t)D.n_scales + 3, per_hop = (size_t)(A.raw + A.n_band) * A.n_channels;
    if (N.h_dfa) {   // (nmx_nolds_dfa_probe)
      if (!(rc = ensure(N.d_dfa, (size_t)n_items * per_item * sizeof(double)))) D.probe = (double*)N.d_dfa.p;
      if (!rc && N.h_series && !(rc = ensure(N.d_series, (size_t)n_items * A.W * sizeof(float)))) D.s.series_out = (float*)N.d_series.p;
    }
    if (!rc) be_launch_nolds_dfa(D, n_items, s);
    if (!rc && N.h_dfa) {
      be_d2h_async(N.h_dfa + (size_t)N.probe_w0 * per_hop * per_item, D.probe, (size_t)n_items * per_item * sizeof(double), s);
      if (D.s.series_out)
        be_d2h_async(N.h_series + (size_t)N.probe_w0 * per_hop * A.W, D.s.series_out, (size_t)n_items * A.W * sizeof(float), s);
    }
  }
  if (tev) be_timer_stop(P.timers[ST_NOLDS], s);
  return rc;
}
