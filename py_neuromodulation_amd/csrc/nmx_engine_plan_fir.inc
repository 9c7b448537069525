// nmx_engine_plan_fir.inc -- plan building, part 2: FIR work -- tap spectra, the one-wave kernels' tables (M = 1024 /
// 1536 / 2048 / 4096), partitioned overlap-save mode, band-pass bank, notch, Hilbert.  Included by nmx_engine.inc.
// real spectrum H[0 .. M / 2] of circularly centred symmetric taps, pre-scaled by 1/M
int host_spectrum(const double* h, int L, int M, std::vector<float>* out) {
  NMX_REQUIRE(L >= 1 && (L & 1), "FIR taps must have odd length (zero-phase)");
  const int half = (L - 1) / 2;
  double amax = 0;
  for (int i = 0; i < L; ++i) amax = std::max(amax, std::fabs(h[i]));
  for (int j = 1; j <= half; ++j)
    NMX_REQUIRE(std::fabs(h[half + j] - h[half - j]) <= 1e-9 * amax + 1e-300,
                "FIR taps must be symmetric (linear phase)");
  const int Mh = M / 2;
  std::vector<float>& H = *out;
  H.assign(Mh + 1, 0.f);
  // cos(2 pi j k / M) via a table of cos(2 pi i / M), index (j * k) mod M
  std::vector<double> ct(M);
  for (int i = 0; i < M; ++i) ct[i] = std::cos(2.0 * kPi * i / M);
  for (int k = 0; k <= Mh; ++k) {
    double acc = h[half];
    long long idx = 0;
    for (int j = 1; j <= half; ++j) {
      idx += k;
      if (idx >= M) idx -= M;
      acc += 2.0 * h[half + j] * ct[idx];
    }
    H[k] = (float)(acc / M);
  }
  return 0;
}
// ... uploaded to `out`; the host copy stays in `H`
int filter_spectrum(Plan& P, const double* h, int L, int M, const float** out, std::vector<float>* H) {
  int rc = host_spectrum(h, L, M, H);
  if (rc) return rc;
  *out = (const float*)upload(P, H->data(), H->size() * sizeof(float));
  if (!*out) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  return 0;
}


// fast path tables A_k, B_k (see nmx_k_bank_w64.h) from the float H tables
int build_w64(Plan& P, const NmxBankArgs& A, const std::vector<std::vector<float>>& Hhost,
              NmxBankW64Args* out) {
  const int n = A.M / 2;
  out->b = A;
  for (int i = 0; i < A.n_filters; ++i) {
    std::vector<float> hs(n), hd(n);
    for (int k = 0; k < n; ++k) {
      const double a = Hhost[i][k], b = Hhost[i][n - k], th = 2.0 * kPi * k / (2.0 * n);
      hs[k] = (float)((a + b) - (a - b) * std::sin(th));
      hd[k] = (float)((a - b) * std::cos(th));
    }
    out->Hs[i] = (const float*)upload(P, hs.data(), n * sizeof(float));
    out->Hd[i] = (const float*)upload(P, hd.data(), n * sizeof(float));
    if (!out->Hs[i] || !out->Hd[i]) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  {  // per-lane twiddles of passes B and C for the persistent kernel (layout: nmx_k_bank_w64.h)
    std::vector<float> tw(NMX_W64_TWL_FLOATS);
    for (int r = 1; r < 16; ++r)
      for (int k = 0; k < 16; ++k) {
        const double a = -2.0 * kPi * r * k / 256.0;
        tw[2 * ((r - 1) * 16 + k)] = (float)std::cos(a);
        tw[2 * ((r - 1) * 16 + k) + 1] = (float)std::sin(a);
      }
    for (int r = 1; r < 4; ++r)
      for (int t = 0; t < 4; ++t)
        for (int l = 0; l < 64; ++l) {
          const double a = -2.0 * kPi * r * (l + 64 * t) / 1024.0;
          const int i = NMX_W64_TWB_N + ((r - 1) * 4 + t) * 64 + l;
          tw[2 * i] = (float)std::cos(a);
          tw[2 * i + 1] = (float)std::sin(a);
        }
    out->twl = (const float*)upload(P, tw.data(), tw.size() * sizeof(float));
    if (!out->twl) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  out->off_Z = 0;
  out->off_X = 0;
  out->off_red = out->off_X + al4(2 * (n + n / 16));
  out->lds_floats = out->off_red + 64;
  return 0;
}

// M = 4096 path (nmx_k_bank_w64x2.h): per filter ONE interleaved table of 2048 (A_k, B_k) pairs (kept in Hs[i]), the
// pass B / C twiddles of the 1024-point transforms and w^k = exp(-2 pi i k / 2048), k < 1024
int build_w64x2(Plan& P, const NmxBankArgs& A, const std::vector<std::vector<float>>& Hhost, NmxBankW64Args* out) {
  int rc = build_w64(P, A, Hhost, out);   // twl (+ split Hs / Hd tables of length n = 2048: replaced below)
  if (rc) return rc;
  const int n = A.M / 2;   // 2048
  for (int i = 0; i < A.n_filters; ++i) {
    std::vector<float> ab(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
      const double a = Hhost[i][k], b = Hhost[i][n - k], th = 2.0 * kPi * k / (2.0 * n);
      ab[2 * k] = (float)((a + b) - (a - b) * std::sin(th));
      ab[2 * k + 1] = (float)((a - b) * std::cos(th));
    }
    out->Hs[i] = (const float*)upload(P, ab.data(), ab.size() * sizeof(float));
    out->Hd[i] = nullptr;
    if (!out->Hs[i]) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  std::vector<float> t2(2048);
  for (int k = 0; k < 1024; ++k) {
    const double a = -2.0 * kPi * k / 2048.0;
    t2[2 * k] = (float)std::cos(a);
    t2[2 * k + 1] = (float)std::sin(a);
  }
  out->tw2 = (const float*)upload(P, t2.data(), t2.size() * sizeof(float));
  if (!out->tw2) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  out->off_Z = 0;
  out->off_X = 0;
  out->off_red = al4(2 * (1024 + 64));   // ONE 1024-point exchange tile per wave
  out->lds_floats = out->off_red + 64;
  return 0;
}

// Channel-pair tables of one launch (nmx_k_bank_w64c.h: M = 1536, nmx_k_bank_w64d.h: M = 1024, nmx_k_bank_w64e.h:
// M = 2048): the REAL spectra H[fi][0 .. M / 2] of the filters of `mask`, in the register order of the transform's output
// (M = 1536 / 2048: k of lane qa + 8 u, register 8 g + qb is u + 8 g + (M / 64) (qa + 8 qb); M = 1024: natural order,
// k = lane + 64 reg), two registers per 8-byte entry.  Twiddles: pass A exp(-2 pi i l ka / M) by [register 8 r + p:
// ka = R p + r][lane] with R = 3 (M = 1024 / 1536: the M = 1024 kernel reads twl instead) or 4, then exp(-2 pi i a b / 64);
// the M = 2048 ones are shared by every use.
int build_pair_tables(Plan& P, NmxFirKernel kind, unsigned mask, const std::vector<std::vector<float>>& H, FirLaunch* L) {
  const int M = kind == NMX_FIR_PAIR_D ? 1024 : kind == NMX_FIR_PAIR_C ? 1536 : 2048;
  std::vector<float> hc;
  int n_sel = 0;
  for (int fi = 0; fi < (int)H.size(); ++fi) {
    if (!((mask >> fi) & 1u)) continue;
    const int i = n_sel++;
    hc.resize((size_t)n_sel * M);
    for (int pr = 0; pr < M / 128; ++pr)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 2; ++e) {
          const int reg = 2 * pr + e, qa = lane & 7, u = lane >> 3, g = reg >> 3, qb = reg & 7;
          const int k = M == 1024 ? lane + 64 * reg : u + 8 * g + M / 64 * (qa + 8 * qb);
          hc[(size_t)i * M + (size_t)(pr * 64 + lane) * 2 + e] = H[fi][k <= M / 2 ? k : M - k];
        }
  }
  L->mask = mask;
  L->kernel = kind;
  L->pipelined = false;
  L->hc = (const float*)upload(P, hc.data(), hc.size() * sizeof(float));
  if (!L->hc) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  if (M == 2048 && P.w64e_tw) {
    L->twc = P.w64e_tw;
    return 0;
  }
  const int n_reg = M == 2048 ? 32 : 24, R = n_reg / 8;
  std::vector<float> tw(2 * n_reg * 64 + 2 * 64);
  for (int reg = 0; reg < n_reg; ++reg)
    for (int l = 0; l < 64; ++l) {
      const int ka = R * (reg & 7) + (reg >> 3);
      const double a = -2.0 * kPi * (double)(l * ka) / (double)M;
      tw[2 * (reg * 64 + l)] = (float)std::cos(a);
      tw[2 * (reg * 64 + l) + 1] = (float)std::sin(a);
    }
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < 8; ++b) {
      const double th = -2.0 * kPi * (double)(a * b) / 64.0;
      tw[2 * n_reg * 64 + 2 * (a * 8 + b)] = (float)std::cos(th);
      tw[2 * n_reg * 64 + 2 * (a * 8 + b) + 1] = (float)std::sin(th);
    }
  L->twc = (const float*)upload(P, tw.data(), tw.size() * sizeof(float));
  if (!L->twc) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  if (M == 2048) P.w64e_tw = L->twc;
  return 0;
}

// the one-wave arguments of launch L: the filters of L.mask (in their order) and L's pair tables
static NmxBankW64Args fir_launch_args(const NmxBankW64Args& W, const FirLaunch& L) {
  NmxBankW64Args B = W;
  int n = 0;
  for (int i = 0; i < W.b.n_filters; ++i) {
    if (!((L.mask >> i) & 1u)) continue;
    B.b.f[n] = W.b.f[i];
    B.Hs[n] = W.Hs[i];
    B.Hd[n] = W.Hd[i];
    ++n;
  }
  B.b.n_filters = n;
  B.hc = L.hc;
  B.twc = L.twc;
  B.kernel = L.kernel;
  B.pipelined = L.pipelined;
  return B;
}

// Do the kernels launch_fir_stage launches take the carried offset on load (NmxBankArgs::dcf)?  The LDS kernels do; of the
// one-wave kernels the channel-pair items of nmx_k_bank_w64c.h and nmx_k_bank_w64e.h (PAD = 0) -- and a launch inside the
// notch kernel, whose condition it is.  Computed once, behind choose_notch_bank_fuse (FirStage::takes_dc).
static bool fir_stage_takes_dc(const FirStage& S) {
  if (!S.w64) return true;
  for (const FirLaunch& L : S.launches)
    if (!L.fused && L.kernel != NMX_FIR_PAIR_C && !(L.kernel == NMX_FIR_PAIR_E && S.a.pad_mode == 0)) return false;
  return true;
}

// Launches FIR stage S over n_items (window, channel) items; A = S.a with the per-call fields patched in (A.yb_out: the
// band series for the stand-alone Hilbert kernel).  The bank's filters may take two launches: the channel-pair kernel over
// those it can take, the M = 2048 kernel over the others (stage 6: with the default settings the two 1651-tap sharp-wave
// filters, whose "same" convolution needs M >= 1825).  `timed`: each launch's stage timer runs around it.  A launch that
// the plan moved into the notch kernel (FirLaunch::fused) is skipped unless `with_fused` (nmx_filter_window: no notch).
static void launch_fir_stage(Plan& P, const FirStage& S, const NmxBankArgs& A, int n_items, be_stream_t s, bool timed = false,
                             bool with_fused = false) {
  const Stage first = S.launches[0].stage;
  Stage cur = first;
  if (timed) be_timer_start(P.timers[cur], s);
  if (!S.w64) {
    be_launch_bank(A, n_items, P.nt_bank, (size_t)A.lds_floats * 4, s);
  } else {
    NmxBankW64Args W = S.w;
    W.b = A;
    W.yb_out = A.yb_out;   // (the one-wave kernels take the band series through their own field)
    W.b.yb_out = nullptr;
    for (const FirLaunch& L : S.launches) {
      if (L.fused && !with_fused) continue;
      if (L.stage != cur) {
        if (timed) { be_timer_stop(P.timers[cur], s); be_timer_start(P.timers[L.stage], s); }
        be_stage(cur = L.stage);
      }
      be_launch_bank_w64(fir_launch_args(W, L), n_items, (size_t)W.lds_floats * 4, P.n_cu, s);
    }
    if (cur != first) be_stage(first);
  }
  if (timed) be_timer_stop(P.timers[cur], s);
}

#ifndef NMX_HOST_EMU
// The notch hand-off that is a register move (nmx_k_bank_w64e.h, FUSE).  The default notch and the bank's second launch
// (stage 6: the 1651-tap sharp-wave pre-filters at the default settings) are two instantiations of one item -- same M,
// tile, twiddles, workgroup shape, one wave per (window, channel pair) -- and the window the notch stores sits in the
// registers the filters load it into.  The plan moves that launch into the notch kernel when
//   * the notch is the M = 2048 pair kernel of the compile-time shape (nmx_w64e_notch_w1000) and the launch the M = 2048
//     PAD = 0 pair kernel over the same windows, its spectra (NMX_NOTCH_SW_FUSE=2: and the notch's) fitting next to the
//     tiles, none of its filters a burst band (their series tensor and the Hilbert kernel belong to the bank stage);
//   * nothing sits between notch and bank (no resampler, no raw normaliser).
// y_notch is still written: the M = 1536 launch, the time / oscillatory kernel, coherence and the tap read it.
// NMX_NOTCH_SW_FUSE: 1 (default) the notch's spectrum from global memory -- the tiles of the two launches, seven waves per
// workgroup with two filters; 2 its spectrum in LDS, one tile fewer (for measurement); 0 two launches.
void choose_notch_bank_fuse(Plan& P) {
  const int want = env_int("NMX_NOTCH_SW_FUSE", 1);
  if (!want || !P.have_notch || !P.have_bank || P.have_resample || P.have_rawnorm) return;
  if (!P.notch.w64 || !P.bank.w64 || P.notch.launches.size() != 1 || P.bank.launches.size() != 2) return;
  FirLaunch& L = P.bank.launches[1];
  if (L.stage != ST_BANK2 || L.kernel != NMX_FIR_PAIR_E) return;
  if (P.notch.launches[0].kernel != NMX_FIR_PAIR_E || !nmx_w64e_notch_w1000(P.notch.a)) return;
  if (P.bank.a.W != P.notch.a.W || P.bank.a.n_channels != P.notch.a.n_channels) return;
  if (!nmx_w64e_fits(__builtin_popcount(L.mask) + (want == 2 ? 1 : 0))) return;
  for (int i = 0; i < P.bank.a.n_filters; ++i)
    if (((L.mask >> i) & 1u) && P.bank.a.f[i].burst_index >= 0) return;
  L.fused = true;
  P.notch_bank_fuse = want == 2 ? 2 : 1;
}
// the fused launch: An / Ab = the notch's and the bank's arguments with the per-call fields patched in
static void launch_notch_bank_fused(Plan& P, const NmxBankArgs& An, const NmxBankArgs& Ab, int n_items, be_stream_t s) {
  NmxBankW64Args N = P.notch.w, F = P.bank.w;
  N.b = An;
  F.b = Ab;
  F.yb_out = nullptr;
  F.b.yb_out = nullptr;
  be_launch_notch_bank_fused(fir_launch_args(F, P.bank.launches[1]), fir_launch_args(N, P.notch.launches[0]),
                             P.notch_bank_fuse == 2, n_items, P.n_cu, s);
}
#endif

int choose_M(int need) {
  int M = need + (need & 1);
  while (!smooth5(M / 2)) M += 2;
  return M;
}

// does the FFT convolution of length M (window W) fit one LDS transform?  If not the bank runs in DIRECT mode
bool bank_fits_lds(int M, int W, bool with_hilbert) {
  const int Mh = M / 2, nb = with_hilbert ? std::max(Mh, W) : Mh;
  return M / 2 <= 32768 && (size_t)(al4(2 * (Mh + 1)) + 2 * al4(2 * nb) + 64) * 4 <= 160 * 1024;
}
// in-place radix-2 transform of n = 2^k complex points (host, float64): the partition spectra below
static void host_fft(std::vector<double>& re, std::vector<double>& im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const double ang = -2.0 * kPi / (double)len;
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const double wr = std::cos(ang * (double)k), wi = std::sin(ang * (double)k);
        const size_t a = i + k, b = i + k + len / 2;
        const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
        re[b] = re[a] - tr; im[b] = im[a] - ti;
        re[a] += tr; im[a] += ti;
      }
  }
}

// Windows x taps whose FFT convolution does not fit one LDS transform (>= 6 kHz recordings with 1 s windows):
// uniformly partitioned overlap-save (nmx_k_bank.h: NmxBankArgs::ups_*), y[W] in LDS for the epilogues.
int bank_partitioned_setup(Plan& P, NmxBankArgs& A, const std::vector<const double*>& taps) {
  A.M = 0;
  A.off_X = 0;
  A.partitioned = 1;
  // (blocks of 128 samples only where 256 do not fit beside the window: from 39 873 samples on)
  int B = 2048;
  while (B > 128 && (size_t)(al4(A.W) + 2 * al4(2 * B) + 64) * 4 > 160 * 1024) B >>= 1;
  A.off_a = al4(A.W);
  A.off_b = A.off_a + al4(2 * B);
  A.off_red = A.off_b + al4(2 * B);
  A.lds_floats = A.off_red + 64;
  NMX_REQUIRE((size_t)A.lds_floats * 4 <= 160 * 1024, "window too long for the partitioned FIR kernel (> 40 384 samples)");
  // (a filter of ups_diff_mask also runs its differenced taps, one tap longer on each side: NmxBankArgs::ups_diff_mask)
  int hm = 0;
  for (int i = 0; i < A.n_filters; ++i) hm = std::max(hm, A.f[i].half + (int)((A.ups_diff_mask >> i) & 1u));
  A.ups_B = B;
  A.ups_hm = hm;
  A.ups_frames = (2 * hm + A.W - 1) / B + 1;   // blocks 0 .. (half_f + hm + W - 1) / B
  int rc;
  if ((rc = build_fft(P, B, &A.fft))) return rc;
  std::vector<double> re(2 * B), im(2 * B);
  // the partition spectra [ceil(n / B)][B + 1] of the taps t[0, n), appended to H
  auto partitions = [&](const double* t, int n, std::vector<float>& H) {
    for (int p = 0; p < (n + B - 1) / B; ++p) {
      std::fill(re.begin(), re.end(), 0.0);
      std::fill(im.begin(), im.end(), 0.0);
      for (int j = 0; j < B && p * B + j < n; ++j) re[j] = t[p * B + j];
      host_fft(re, im);
      for (int k = 0; k <= B; ++k) {
        H.push_back((float)(re[k] / (2.0 * B)));
        H.push_back((float)(im[k] / (2.0 * B)));
      }
    }
  };
  for (int i = 0; i < A.n_filters; ++i) {
    const int L = 2 * A.f[i].half + 1;
    std::vector<float> H;
    partitions(taps[i], L, H);
    if ((A.ups_diff_mask >> i) & 1u) {
      // g1[j] = h[j - 1] - h[j - 2], g2[j] = h[j] - 2 h[j - 1] + h[j - 2], j in [0, L + 2), in float64 from the live taps
      auto h = [&](int j) { return j >= 0 && j < L ? taps[i][j] : 0.0; };
      std::vector<double> g1(L + 2), g2(L + 2);
      for (int j = 0; j < L + 2; ++j) {
        g1[j] = h(j - 1) - h(j - 2);
        g2[j] = (h(j) - h(j - 1)) - (h(j - 1) - h(j - 2));
      }
      if (A.bp_features & 6u) partitions(g1.data(), L + 2, H);   // (only the series the plan's features read)
      if (A.bp_features & 4u) partitions(g2.data(), L + 2, H);
    }
    A.f[i].H = (const float*)upload(P, H.data(), H.size() * sizeof(float));
    if (!A.f[i].H) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
  // one scratch slot per resident workgroup (be_launch_bank launches at most NMX_UPS_SLOTS of them)
  const size_t slot = (size_t)A.ups_frames * (B + 1) * sizeof(float2);
  A.ups_scratch = (float2*)be_alloc(slot * NMX_UPS_SLOTS);
  if (!A.ups_scratch) return nmx_fail(NMX_E_NOMEM, "scratch allocation failed");
  P.tables.push_back(A.ups_scratch);
  return 0;
}

int bank_lds(NmxBankArgs& A, bool with_hilbert) {
  const int Mh = A.M / 2;
  const int nb = with_hilbert ? std::max(Mh, A.W) : Mh;
  A.off_X = 0;
  A.off_a = al4(2 * (Mh + 1));
  A.off_b = A.off_a + al4(2 * nb);
  A.off_red = A.off_b + al4(2 * nb);
  A.lds_floats = A.off_red + 64;
  NMX_REQUIRE(A.lds_floats * 4 <= 160 * 1024, "FIR bank kernel needs more than 160 KiB LDS "
              "(window x filter length too large)");
  return 0;
}

// What the kinds of FIR stage decide differently (build_fir_stage)
struct FirRules {
  int reach;      // the "same" convolution of a window needs M >= W + reach
  int w64_lo;     // the one-wave M = 2048 kernels for W + reach in (w64_lo, 2048]
  bool w64x2;     // the M = 4096 one-wave kernel for W + reach in (2048, 4096] (device only)
  bool hilbert;   // the LDS bank kernel also holds the Hilbert transform's buffers
  Stage stage;    // timer / kernel-name stage of its launches
};

// a launch of the filters of `mask` on the one-channel M = 2048 kernels (NMX_FIR_ONE); S.w is built
static FirLaunch fir_one_launch(const FirStage& S, unsigned mask, Stage stage) {
  FirLaunch L{mask, stage};
  L.pipelined = nmx_w64p_ok(S.a, __builtin_popcount(mask), S.w.lds_floats);
  return L;
}

// The decisions every FIR stage makes: kernel family, convolution length M, tap spectra and the kernels' tables.  The
// caller has filled S->a but for those (W, pad mode, epilogue; per filter all but H, f[i].half = half-length of the live
// taps[i]).  Hhost: the filters' real spectra at M (none in partitioned mode).
int build_fir_stage(Plan& P, const std::vector<const double*>& taps, const FirRules& r, FirStage* S,
                    std::vector<std::vector<float>>* Hhost = nullptr) {
  NmxBankArgs& A = S->a;
  A.n_filters = (int)taps.size();
  NMX_REQUIRE(!A.pad_mode || A.n_filters == 1, "internal: a reflected FIR stage has one filter");
  S->launches = {FirLaunch{(1u << A.n_filters) - 1u, r.stage}};
  const int need = A.W + r.reach;
  const bool on = env_int("NMX_BANK_W64", 1) == 1;
  const bool w64 = on && need > r.w64_lo && need <= 2048;
  bool w64x2 = false;
#ifndef NMX_HOST_EMU   // (device only: unpaired LDS reads and explicit operand modifiers)
  w64x2 = r.w64x2 && on && env_int("NMX_BANK_W64X2", 1) == 1 && need > 2048 && need <= 4096;
#endif
  A.M = w64 ? 2048 : w64x2 ? 4096 : choose_M(need);
  if (!w64 && !w64x2 && (!bank_fits_lds(A.M, A.W, r.hilbert) || env_int("NMX_BANK_PARTITIONED", 0) == 1))
    return bank_partitioned_setup(P, A, taps);
  std::vector<std::vector<float>> local;
  std::vector<std::vector<float>>& H = Hhost ? *Hhost : local;
  H.assign(taps.size(), {});
  int rc;
  if ((rc = build_fft(P, A.M / 2, &A.fft))) return rc;
  for (size_t i = 0; i < taps.size(); ++i)
    if ((rc = filter_spectrum(P, taps[i], 2 * A.f[i].half + 1, A.M, &A.f[i].H, &H[i]))) return rc;
  if ((rc = bank_lds(A, r.hilbert))) return rc;
  S->w64 = w64 || w64x2;
  if (!S->w64) return 0;
  if ((rc = w64x2 ? build_w64x2(P, A, H, &S->w) : build_w64(P, A, H, &S->w))) return rc;
#ifndef NMX_HOST_EMU
  if (w64x2) {
    NMX_REQUIRE(nmx_w64x2_lds_tables(S->w.lds_floats) >= 0, "internal: M = 4096 FIR path: LDS budget");
    S->launches[0].kernel = NMX_FIR_X2;
    return 0;
  }
#endif
  S->launches[0] = fir_one_launch(*S, S->launches[0].mask, r.stage);
  return 0;
}

int build_bank(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (d.n_filters == 0) return 0;
  NMX_REQUIRE(d.n_filters <= NMX_MAX_FILTERS_DEV, "too many filters");
  FirStage& S = P.bank;
  NmxBankArgs& A = S.a;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.W = d.window;
  A.pad_mode = 0;
  int reach = 0;
  bool hil = false;
  std::vector<const double*> live;
  for (int i = 0; i < d.n_filters; ++i) {
    const nmx_filter_desc& f = d.filters[i];
    NMX_REQUIRE(f.n_taps & 1, "FIR taps must have odd length");
    // only taps within W-1 of the centre can touch the window (SURVEY A.4)
    const int half = (f.n_taps - 1) / 2, uh = std::min(half, d.window - 1);
    live.push_back(P.taps[i].data() + (half - uh));
    reach = std::max(reach, uh);
    hil |= f.burst_index >= 0;
    NmxFilterDev& F = A.f[i];
    F.half = uh;
    F.bp_seglen = f.bp_seglen;
    F.bp_band = f.bp_band_index;
    F.burst_index = f.burst_index;
    F.sw_index = f.sw_index;
    F.store_raw = 0;
    NMX_REQUIRE(f.bp_seglen >= 0 && f.bp_seglen <= d.window, "band-pass segment longer than the window");
    NMX_REQUIRE(f.bp_seglen == 0 || f.bp_seglen >= 3 || !(d.bp_features & 6u), "segment too short");
    NMX_REQUIRE(f.burst_index < d.n_burst_bands && f.sw_index < d.n_sw_filters, "filter index out of range");
  }
  A.bp_features = d.bp_features;
  A.bp_log = d.bp_log_transform;
  A.bp_kalman_mask = (d.bp_features & 1u) ? d.bp_kalman_mask : 0u;
  A.bp_cols = cv(d.bp_cols);
  A.n_burst_bands = d.n_burst_bands;
  A.n_sw_filters = d.n_sw_filters;
  // one-wave M = 2048 from W + reach = 513 on (513 .. 1024: the one-wave 1024-point path still beats the multi-wave LDS
  // Stockham of half the length, measured on BASELINE config 5)
  const bool fits_x2 = (d.window & 3) == 0 && !(d.bp_features & 6u);
  // Above 16 384 samples (NMX_LONG_BANDPOWER: nmx_plan_create) mobility and complexity come from differenced taps: the
  // second difference of a stored fp32 band series cancels to rounding noise at those rates (NmxBankArgs::ups_diff_mask).
  // Below, the outputs are pinned and the epilogue stays as it is.  (Activity alone takes the same form with one series: only
  // the output blocks that hold the tail are transformed.)
  A.ups_diff_mask = 0;
  if (d.window > 16384)
    for (int i = 0; i < d.n_filters; ++i)
      if (A.f[i].bp_seglen > 0) A.ups_diff_mask |= 1u << i;
  std::vector<std::vector<float>> H;
  int rc = build_fir_stage(P, live, FirRules{reach, 512, fits_x2, hil, ST_BANK}, &S, &H);
  if (rc) return rc;
  NMX_REQUIRE(!A.ups_diff_mask || A.partitioned, "internal: band-pass power above 16 384 samples runs on the partitioned bank");
  if (hil && !A.partitioned) {
    A.hil_full = d.window & 1;
    if ((rc = build_fft(P, A.hil_full ? d.window : d.window / 2, &A.hil_r))) return rc;
    if ((rc = build_fft(P, d.window, &A.hil_c))) return rc;
  }
  // the one-wave and partitioned kernels leave burst bands as series: the stand-alone Hilbert kernel follows (run_chunk)
  if (hil && (S.w64 || A.partitioned) && (rc = build_hilbert(P))) return rc;
#ifndef NMX_HOST_EMU   // (device only, like the M = 4096 path)
  if (S.w64 && A.M == 2048 && nmx_w64_pair_shape_ok(A)) {
    // M = 1536, two channels per transform, for every filter with W + (L - 1) / 2 <= 1536 (the default band-pass taps:
    // 999), M = 1024 when all of them fit it; longer ones (the default sharp-wave taps: 1651) go to a second launch: the
    // M = 2048 channel-pair kernel (nmx_k_bank_w64e.h), or the one-channel M = 2048 kernels
    const unsigned all = S.launches[0].mask;
    S.launches.clear();
    unsigned mask = 0;
    if (env_int("NMX_BANK_W64C", 1) == 1) {
      int n_sel = 0, need = 0;
      for (int i = 0; i < d.n_filters; ++i)
        if (d.window + A.f[i].half <= NMX_W64C_M) { mask |= 1u << i; ++n_sel; need = std::max(need, d.window + A.f[i].half); }
      // (a second launch repeats the forward transform: not for one filter out of many.  The count the M = 1536 kernel
      // holds in LDS bounds the M = 1024 kernel's too, whose tables are smaller)
      if ((n_sel >= 2 || n_sel == d.n_filters) && nmx_w64c_fits(n_sel)) {
        // short windows (the taps that touch them end at 2 W - 1): the 1024-point channel-pair kernel
        const NmxFirKernel kind = (need <= 1024 && (d.window & 1) == 0 && env_int("NMX_BANK_W64D", 1) == 1) ? NMX_FIR_PAIR_D : NMX_FIR_PAIR_C;
        NMX_REQUIRE(kind != NMX_FIR_PAIR_D || nmx_w64d_fits(n_sel, S.w.lds_floats), "internal: M = 1024 FIR path: LDS budget");
        const int M = kind == NMX_FIR_PAIR_D ? 1024 : NMX_W64C_M;
        std::vector<std::vector<float>> HM(d.n_filters);
        for (int i = 0; i < d.n_filters; ++i)
          if (((mask >> i) & 1u) && (rc = host_spectrum(live[i], 2 * A.f[i].half + 1, M, &HM[i]))) return rc;
        S.launches.emplace_back();
        if ((rc = build_pair_tables(P, kind, mask, HM, &S.launches.back()))) return rc;
      } else {
        mask = 0;
      }
    }
    if (all & ~mask) {
      FirLaunch rest = fir_one_launch(S, all & ~mask, mask ? ST_BANK2 : ST_BANK);
      // (one spectrum's room is left free: the notch's, when the launch moves into the notch kernel with it in LDS --
      // choose_notch_bank_fuse, NMX_NOTCH_SW_FUSE=2)
      if (env_int("NMX_BANK_W64E", 1) == 1 && nmx_w64e_fits(__builtin_popcount(rest.mask) + 1) &&
          (rc = build_pair_tables(P, NMX_FIR_PAIR_E, rest.mask, H, &rest))) return rc;
      S.launches.push_back(rest);
    }
  }
#endif
  P.have_bank = true;
  return 0;
}

int build_notch(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!d.notch_taps) return 0;
  FirStage& S = P.notch;
  NmxBankArgs& A = S.a;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.W = P.w_in;
  const int L = d.n_notch_taps;
  NMX_REQUIRE(L & 1, "notch taps must have odd length");
  if (L == 1) return nmx_fail(NMX_E_INVALID, "single-tap notch is not supported");
  const int half = (L - 1) / 2;
  A.pad_mode = 1;   // odd reflection: every tap reaches into the window
  A.n_edge = std::max(std::min(L, P.w_in) - 1, 0);
  A.pad_half = half;
  // residual form (NmxBankArgs::residual): the kernels convolve with g = delta - h and store x - g * x_ext
  A.residual = env_int("NMX_NOTCH_RESIDUAL", 1) != 0;
  P.notch_taps_used = P.notch_taps;   // (P.notch_taps stays h: the offset split reads its DC gain, nmx_engine_dc.inc)
  if (A.residual) {
    for (double& t : P.notch_taps_used) t = -t;
    P.notch_taps_used[(size_t)half] += 1.0;
  }
  NmxFilterDev& F = A.f[0];
  F.half = half;
  F.bp_seglen = 0;
  F.burst_index = -1;
  F.sw_index = -1;
  F.store_raw = 1;
  std::vector<std::vector<float>> H;
  int rc = build_fir_stage(P, {P.notch_taps_used.data()}, FirRules{2 * half, 1024, false, false, ST_PREP}, &S, &H);
  if (rc) return rc;
#ifndef NMX_HOST_EMU
  // two channels per 2048-point complex transform (nmx_k_bank_w64e.h, PAD = 1)
  if (S.w64 && env_int("NMX_BANK_W64E", 1) == 1 && nmx_w64e_notch_ok(A) &&
      (rc = build_pair_tables(P, NMX_FIR_PAIR_E, 1u, H, &S.launches[0]))) return rc;
#endif
  P.have_notch = true;
  return 0;
}

// ---- the band series of the nolds stage (build_nolds, nmx_engine_plan_spectral.inc) ---------------------------------------
// Zero-padded "same" FIRs over the pre-processed window, series out: the band-pass bank's kernels with the series as their
// only output.  The taps are the host's: those of the bank the reference's Nolds builds (BandPower(use_kf = False): every
// band of frequency_ranges_hz, sfreq - 1 taps), picked by the reference's own index (plan_desc._nolds).
int build_nolds_bands(Plan& P) {
  const nmx_plan_desc& d = P.d;
  NoldsStage& N = P.nolds;
  const int nb = d.nolds_n_bands;
  if (nb == 0) return 0;
  NMX_REQUIRE(nb <= NMX_MAX_FILTERS_DEV, "nolds: too many band series");
  FirStage& S = N.fir;
  NmxBankArgs& A = S.a;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.W = d.window;
  A.pad_mode = 0;
  A.n_sw_filters = nb;
  N.taps.resize(nb);
  std::vector<const double*> live;
  int reach = 0;
  for (int j = 0; j < nb; ++j) {
    NMX_REQUIRE(d.nolds_taps[j] && d.nolds_n_taps[j] >= 1 && (d.nolds_n_taps[j] & 1), "nolds: band filter taps must have odd length");
    N.taps[j].assign(d.nolds_taps[j], d.nolds_taps[j] + d.nolds_n_taps[j]);
    // only taps within W - 1 of the centre can touch the window (as build_bank)
    const int half = (d.nolds_n_taps[j] - 1) / 2, uh = std::min(half, d.window - 1);
    live.push_back(N.taps[j].data() + (half - uh));
    reach = std::max(reach, uh);
    NmxFilterDev& F = A.f[j];
    F.half = uh;
    F.bp_seglen = 0;
    F.bp_band = 0;
    F.burst_index = -1;
    F.sw_index = j;
    F.store_raw = 0;
  }
  int rc = build_fir_stage(P, live, FirRules{reach, 512, false, false, ST_NOLDS}, &S);
  if (rc) return rc;
  S.takes_dc = fir_stage_takes_dc(S);
  N.have_fir = true;
  return 0;
}

// the band series of one chunk into P.nolds.yb, [nw][C][n_band][W]
static int launch_nolds_bands(Plan& P, const WinView& v, int nw, be_stream_t s, bool& dc_made) {
  NoldsStage& N = P.nolds;
  const nmx_plan_desc& d = P.d;
  int rc;
  if ((rc = ensure(N.yb, (size_t)nw * d.n_channels * d.nolds_n_bands * d.window * sizeof(float)))) return rc;
  NmxBankArgs A = N.fir.a;
  if ((rc = dc_bind(P, A, N.fir.takes_dc, v, nw, s, dc_made))) return rc;
  A.out = nullptr;
  A.sw_out = (float*)N.yb.p;
  launch_fir_stage(P, N.fir, A, nw * d.n_channels, s);
  return 0;
}
