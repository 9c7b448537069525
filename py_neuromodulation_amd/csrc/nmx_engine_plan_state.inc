// nmx_engine_plan_state.inc -- plan building, part 3: raw normaliser, preprocessing_filter stages, resampler, Kalman,
// sharp waves, the front end (re-reference or offset shift); the state-blob sections of the raw normaliser and the Kalman
// filters beside their build functions (rawnorm_state_*, kalman_state_*: the table that walks them is in nmx_engine_abi.inc).
// Included by nmx_engine.inc.
// ---- the raw normaliser's section of the state blob: hops seen | ring capacity of the exporting plan | rings | counts | lengths.
// The capacity depends on the window length; a stream with ragged window lengths hands the blob of one plan to the plan
// of the other length, which re-lays the histories into its own rings (rawnorm_state_import).
static size_t rawnorm_state_bytes_cap(const Plan& P, long long cap) {
  return 2 * sizeof(long long) + (size_t)P.d.n_channels * (size_t)cap * sizeof(float) + P.rawnorm.cnt_bytes + P.rawnorm.len_bytes;
}
static size_t rawnorm_state_bytes(const Plan& P) { return P.have_rawnorm ? rawnorm_state_bytes_cap(P, P.rawnorm.a.cap) : 0; }
// the section's size in a blob that holds `left` bytes from its start `q` on: by the exporting plan's capacity
static int rawnorm_state_bytes_in(const Plan& P, const char* q, size_t left, size_t* n) {
  *n = 0;
  if (!P.have_rawnorm) return 0;
  long long src_cap = P.rawnorm.a.cap;
  if (left >= 2 * sizeof(long long)) memcpy(&src_cap, q + sizeof(long long), sizeof(long long));
  NMX_REQUIRE(src_cap > 0 && src_cap < (1ll << 31), "state blob: bad raw-normaliser header");
  *n = rawnorm_state_bytes_cap(P, src_cap);
  return 0;
}
static void rawnorm_state_reset(Plan& P) {
  if (!P.have_rawnorm) return;
  RawNormStage& S = P.rawnorm;
  be_memset_sync(S.a.ring, 0, S.ring_bytes);
  be_memset_sync(S.a.count, 0, S.cnt_bytes);
  be_memset_sync(S.a.len, 0, S.len_bytes);
  S.hops = 0;
  S.sorted_valid = false;
}
static void rawnorm_state_export(const Plan& P, char* q) {
  if (!P.have_rawnorm) return;
  const RawNormStage& S = P.rawnorm;
  const long long cap = S.a.cap;
  memcpy(q, &S.hops, sizeof(long long)); q += sizeof(long long);
  memcpy(q, &cap, sizeof(long long)); q += sizeof(long long);
  be_d2h_sync(q, S.a.ring, S.ring_bytes); q += S.ring_bytes;
  be_d2h_sync(q, S.a.count, S.cnt_bytes); q += S.cnt_bytes;
  be_d2h_sync(q, S.a.len, S.len_bytes);
}
static int rawnorm_state_import(Plan& P, const char* q, size_t n) {   // (n: what rawnorm_state_bytes_in said)
  if (!P.have_rawnorm) return 0;
  RawNormStage& S = P.rawnorm;
  const int C = P.d.n_channels, cap = S.a.cap;
  const long long src_cap = (long long)((n - rawnorm_state_bytes_cap(P, 0)) / ((size_t)C * sizeof(float)));
  memcpy(&S.hops, q, sizeof(long long)); q += 2 * sizeof(long long);
  const float* ring_src = (const float*)q;
  const char* cnt_src = q + (size_t)C * (size_t)src_cap * sizeof(float);
  const char* len_src = cnt_src + S.cnt_bytes;
  if (src_cap == cap) {
    be_h2d_sync(S.a.ring, ring_src, S.ring_bytes);
  } else {   // a plan of another window length exported this: the same histories at the same sample counts, re-laid
    std::vector<float> ring((size_t)C * cap, 0.f);
    for (int c = 0; c < C; ++c) {
      long long cnt;
      int len;
      memcpy(&cnt, cnt_src + (size_t)c * sizeof(long long), sizeof(long long));
      memcpy(&len, len_src + (size_t)c * sizeof(int), sizeof(int));
      NMX_REQUIRE(len >= 0 && len <= cap && len <= src_cap && cnt >= len, "state blob: raw-normaliser history does not fit this plan");
      for (long long i = cnt - len; i < cnt; ++i) ring[(size_t)c * cap + (size_t)(i % cap)] = ring_src[(size_t)c * src_cap + (size_t)(i % src_cap)];
    }
    be_h2d_sync(S.a.ring, ring.data(), S.ring_bytes);
  }
  be_h2d_sync(S.a.count, cnt_src, S.cnt_bytes);
  be_h2d_sync(S.a.len, len_src, S.len_bytes);
  S.sorted_valid = false;   // the sorted copies are rebuilt from the imported rings
  return 0;
}

int build_rawnorm(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (d.raw_norm_method <= 0) return 0;
  NMX_REQUIRE(d.raw_norm_method >= NMX_RAWNORM_MEAN && d.raw_norm_method <= NMX_RAWNORM_POWER,
              "raw normalisation method outside 1..8 (mean, zscore, median, zscore-median, robust, minmax, quantile, power)");
  NMX_REQUIRE(d.raw_norm_n >= 2 && d.raw_norm_add >= 1 && d.raw_norm_add <= d.window,
              "raw normalisation: need N >= 2 and 1 <= int(sfreq / feat_hz) <= window");
  RawNormStage& S = P.rawnorm;
  NmxRawNormArgs& A = S.a;
  A.n_channels = d.n_channels; A.W = d.window;
  A.add = d.raw_norm_add; A.keep = d.raw_norm_n - 1;
  A.cap = std::max(d.window, A.keep) + A.add + 64;
  A.method = d.raw_norm_method; A.clip = d.raw_norm_clip;
  S.ring_bytes = (size_t)d.n_channels * A.cap * sizeof(float);
  S.cnt_bytes = (size_t)d.n_channels * sizeof(long long);
  S.len_bytes = (size_t)d.n_channels * sizeof(int);
  A.ring = (float*)plan_alloc(P, S.ring_bytes);
  A.count = (long long*)plan_alloc(P, S.cnt_bytes);
  A.len = (int*)plan_alloc(P, S.len_bytes);
  if (!A.ring || !A.count || !A.len) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
  if (A.method == NMX_RAWNORM_POWER) {   // sign(x) log1p|x| of every ring sample (rebuilt inside the kernel when stale)
    A.ring_sl = (double*)plan_alloc(P, (size_t)d.n_channels * A.cap * sizeof(double));
    if (!A.ring_sl) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
  } else if (A.method >= NMX_RAWNORM_MEDIAN) {   // the history sorted, double-buffered; rebuilt from the ring when stale
    if (A.method == NMX_RAWNORM_QUANTILE) {
      A.sub = (float*)plan_alloc(P, (size_t)d.n_channels * NMX_RAWNORM_SUBSAMPLE * sizeof(float));
      if (!A.sub) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
      A.seed = (unsigned)env_int("NMX_QUANTILE_SEED", 20250929);
    }
    A.sorted = (float*)plan_alloc(P, (size_t)d.n_channels * 2 * A.cap * sizeof(float));
    A.cur = (int*)plan_alloc(P, (size_t)d.n_channels * sizeof(int));
    if (!A.sorted || !A.cur) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
    be_memset_sync(A.cur, 0, (size_t)d.n_channels * sizeof(int));
    A.max_list = (d.window + A.add + 1) & ~1;
    // six lists of max_list entries + the reduction scratch (be_launch_rawnorm): in LDS up to window + hop = 6484
    // samples, in device memory beyond
    A.lists = nullptr;
    if ((size_t)24 * A.max_list + 8 * 1024 > 160 * 1024 || env_int("NMX_RAWNORM_GLOBAL_LISTS", 0)) {
      A.lists = (float*)plan_alloc(P, (size_t)d.n_channels * 6 * A.max_list * sizeof(float));
      if (!A.lists) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
    }
  }
  P.have_rawnorm = true;
  rawnorm_state_reset(P);
  return 0;
}

// raw_normalization stage of one chunk / one window: statistics walk, then the elementwise map; `v`: in, its windows; out, the
// normalised ones
static int run_rawnorm(Plan& P, WinView& v, int nw, be_stream_t s) {
  const int C = P.d.n_channels, W = P.d.window;
  RawNormStage& S = P.rawnorm;
  int rc;
  if ((rc = ensure(S.x_rn, (size_t)nw * C * W * sizeof(float)))) return rc;
  if ((rc = ensure(S.mean, (size_t)nw * C * sizeof(float)))) return rc;
  if ((rc = ensure(S.scale, (size_t)nw * C * sizeof(float)))) return rc;
  NmxRawNormArgs A = S.a;
  view_into(A, v);
  A.y = (float*)S.x_rn.p; A.n_windows = nw; A.hop0 = S.hops;
  A.mean = (float*)S.mean.p; A.scale = (float*)S.scale.p;
  A.sorted_valid = S.sorted_valid ? 1 : 0;
  if (A.method == NMX_RAWNORM_QUANTILE) {
    if ((rc = ensure(S.qt, (size_t)nw * C * NMX_RAWNORM_NQ * sizeof(double)))) return rc;
    if ((rc = ensure(S.qn, (size_t)nw * C * sizeof(int)))) return rc;
    A.qt = (double*)S.qt.p; A.qn = (int*)S.qn.p;
  } else if (A.method == NMX_RAWNORM_POWER) {
    if ((rc = ensure(S.qt, (size_t)nw * C * 3 * sizeof(double)))) return rc;
    A.pw = (double*)S.qt.p;
  }
  be_launch_rawnorm(A, s);
  S.sorted_valid = true;
  S.hops += nw;
  v = dense_view(S.x_rn.p, C, W);
  return 0;
}

// preprocessing_filter stages: zero-padded "same" FIR on the incoming window, series out
int build_prefilters(Plan& P) {
  const nmx_plan_desc& d = P.d;
  P.pre.assign(d.n_pre_filters, FirStage{});
  for (int i = 0; i < d.n_pre_filters; ++i) {
    NmxBankArgs& A = P.pre[i].a;
    A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
    A.n_channels = d.n_channels;
    A.W = P.w_in;
    A.pad_mode = 0;
    A.n_sw_filters = 1;
    const int L = d.n_pre_taps[i];
    NMX_REQUIRE(L & 1, "pre-filter taps must have odd length");
    const int half = (L - 1) / 2, uh = std::min(half, A.W - 1);
    NmxFilterDev& F = A.f[0];
    F.half = uh;
    F.bp_seglen = 0;
    F.burst_index = -1;
    F.sw_index = 0;
    F.store_raw = 0;
    int rc = build_fir_stage(P, {P.pre_taps[i].data() + (half - uh)}, FirRules{uh, 1024, false, false, ST_PREP}, &P.pre[i]);
    if (rc) return rc;
  }
  return 0;
}

int build_resample(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (d.raw_window <= 0) return 0;
  NMX_REQUIRE(d.resample_ratio > 0 && d.resample_ratio != 1.0, "resample_ratio must be positive and != 1");
  NMX_REQUIRE(d.raw_window >= 4 && d.raw_window <= 65336, "raw_window must be in [4, 65 336] samples");
  const double ratio = d.resample_ratio;
  const int W = d.raw_window;
  // Python round() is round-half-even; so is nearbyint in the default rounding mode
  const int final_len = (int)std::nearbyint(ratio * W);
  NMX_REQUIRE(final_len == d.window, "window must equal round(resample_ratio * raw_window)");
  // the padding mode (include/nmx.h): "auto" -- the next power of two -- or a fixed count per side
  NMX_REQUIRE(d.resample_npad_mode == 0 || d.resample_npad_mode == 1, "resample_npad_mode must be 0 (\"auto\") or 1 (fixed)");
  const bool fixed = d.resample_npad_mode == 1;
  int n_pad = 1, pad_l;
  if (fixed) {
    NMX_REQUIRE(d.resample_npad >= 0, "resample_npad must be >= 0 samples per side");
    NMX_REQUIRE((long long)W + 2ll * d.resample_npad <= 65536,
                "raw_resampling: raw window " + spaced(W) + " + 2 x npad " + spaced(d.resample_npad) + " = " +
                std::to_string((long long)W + 2ll * d.resample_npad) + " samples exceeds the padded limit of 65 536");
    n_pad = W + 2 * d.resample_npad;
    pad_l = d.resample_npad;
  } else {
    const int min_add = std::min(W / 8, 100) * 2;
    while (n_pad < W + min_add) n_pad <<= 1;
    pad_l = (n_pad - W) / 2;
  }
  const int n_new = std::max((int)std::nearbyint(ratio * n_pad), 1);
  const int crop_l = (int)std::nearbyint(ratio * pad_l);
  NMX_REQUIRE(crop_l + final_len <= n_new, "internal: resample crop outside the output");
  NmxResampleArgs& A = P.resample.a;
  A.n_channels = d.n_channels; A.W = W; A.W_new = final_len;
  A.n_pad = n_pad; A.pad_l = pad_l; A.n_new = n_new; A.crop_l = crop_l;
  A.inv_full = n_new & 1;
  A.scale = (float)(ratio / (double)n_new);
  const int use_len = std::min(n_new, n_pad);
  A.nyq_bin = (use_len % 2 == 0) ? use_len / 2 : -1;
  A.nyq_scale = n_new < n_pad ? 2.f : 0.5f;
  int rc;
  const int n_inv = A.inv_full ? n_new : n_new / 2;
  auto layout = [&](int n_fwd, int keep_x) {
    const int cmax = std::max(n_fwd, n_inv);
    A.off_x = 0;
    A.off_a = keep_x ? al4(W) : 0;
    A.off_b = A.off_a + al4(2 * cmax);
    A.off_X = A.off_b + al4(2 * cmax);
    A.lds_floats = A.off_X + al4(2 * (n_new / 2 + 1));
    return A.lds_floats * 4 <= 160 * 1024;
  };
  A.poly_q = A.poly_m = 0;
  A.tab_n = nullptr;
  A.gen = fixed ? 1 : 0;
  A.fwd_full = 0;
  auto roots_of_n_pad = [&]() {
    std::vector<float> tab(2 * (size_t)n_pad);
    for (int j = 0; j < n_pad; ++j) {
      const double a = -2.0 * kPi * (double)j / (double)n_pad;
      tab[2 * j] = (float)std::cos(a);
      tab[2 * j + 1] = (float)std::sin(a);
    }
    A.tab_n = (const float2*)upload(P, tab.data(), tab.size() * sizeof(float));
    return A.tab_n ? 0 : nmx_fail(NMX_E_NOMEM, "table allocation failed");
  };
  auto max_prime = [](int n) {
    int big = 1;
    for (int p = 2; (long long)p * p <= n; ++p) while (n % p == 0) { big = std::max(big, p); n /= p; }
    return std::max(big, n);
  };
  const std::string lens = "raw window " + spaced(W) + ", n_pad " + spaced(n_pad) + ", n_new " + spaced(n_new);
  if (fixed) {
    // fixed pad: n_pad = W + 2 npad is any length.  The one-transform form wherever its LDS layout fits (the 8192 gate
    // below belongs to "auto"); n_pad odd: a full-length complex forward transform
    NMX_REQUIRE(max_prime(n_new) <= 4096, "raw_resampling: the resampled padded length has a prime factor > 4096 (" + lens + ")");
    const int n_fwd = (n_pad & 1) ? n_pad : n_pad / 2;
    if (n_fwd >= 1 && n_fwd <= 32768 && layout(n_fwd, 1) && max_prime(n_fwd) <= 4096 && !env_int("NMX_RESAMPLE_POLY", 0)) {
      A.fwd_full = n_pad & 1;
      if ((rc = build_fft(P, n_fwd, &A.fwd))) return rc;
    } else {
      // long form: the smallest q in [2, 256] that divides n_pad and leaves m = n_pad / q <= 2048 points per component
      // (every prime factor of m is then below 4096); an odd q leaves its last component unpaired
      int q = 0;
      for (int t = 2; t <= 256 && t < n_pad && !q; ++t)
        if (n_pad % t == 0 && n_pad / t <= 2048 && layout(n_pad / t, 0)) q = t;
      NMX_REQUIRE(q > 0, "raw_resampling: no polyphase split of the padded window (" + lens + "): n_pad needs a divisor q "
                  "in [2, 256] with n_pad / q <= 2048 whose transforms and the resampled padded window fit the LDS");
      A.poly_q = q;
      A.poly_m = n_pad / q;
      if ((rc = build_fft(P, A.poly_m, &A.fwd))) return rc;
      if ((rc = roots_of_n_pad())) return rc;
    }
  } else
  if (n_pad <= 8192 && layout(n_pad / 2, 1) && !env_int("NMX_RESAMPLE_POLY", 0)) {
    if ((rc = build_fft(P, n_pad / 2, &A.fwd))) return rc;
  } else {
    // long windows (nmx_k_resample.h): polyphase components of m complex points each, two per transform
    const int m = std::min(2048, n_pad / 2);
    NMX_REQUIRE(layout(m, 0), "raw_resampling: the RESAMPLED padded window does not fit one LDS transform "
                              "(round(ratio x 2^ceil(log2(raw window + 200))) > 8192 samples)");
    A.poly_m = m;
    A.poly_q = n_pad / m;
    if ((rc = build_fft(P, m, &A.fwd))) return rc;
    if ((rc = roots_of_n_pad())) return rc;
  }
  if ((rc = build_fft(P, n_inv, &A.inv))) return rc;
  P.w_in = W;
  P.have_resample = true;
  return 0;
}

// the resampler of one chunk / one window, behind the notch like the reference's (data_preprocessor.py:9-15,68-71);
// `v`: in, the incoming windows; out, the resampled ones
static int launch_resample(Plan& P, WinView& v, int nw, be_stream_t s) {
  ResampleStage& S = P.resample;
  const int C = P.d.n_channels, W = P.d.window;
  int rc;
  if ((rc = ensure(S.y, (size_t)nw * C * W * sizeof(float)))) return rc;
  NmxResampleArgs A = S.a;
  view_into(A, v);
  A.y = (float*)S.y.p;
  be_launch_resample(A, nw * C, S.nt, (size_t)A.lds_floats * 4, s);
  v = dense_view(S.y.p, C, W);
  return 0;
}

// ---- the Kalman section of the state blob: x, P of every (channel, band) filter
static size_t kalman_state_bytes(const Plan& P) { return P.kalman.bytes; }
static void kalman_state_reset(Plan& P) {
  if (!P.have_kalman) return;
  std::vector<double> st(P.kalman.bytes / sizeof(double));
  for (size_t i = 0; i + 5 < st.size(); i += 6) {   // x = [0, 1], P = cov([[1, 0], [0, 1]])
    st[i] = 0.0; st[i + 1] = 1.0; st[i + 2] = 0.5; st[i + 3] = -0.5; st[i + 4] = -0.5; st[i + 5] = 0.5;
  }
  be_h2d_sync(P.kalman.d_state, st.data(), P.kalman.bytes);
}
static void kalman_state_export(const Plan& P, char* q) {
  if (P.have_kalman) be_d2h_sync(q, P.kalman.d_state, P.kalman.bytes);
}
static int kalman_state_import(Plan& P, const char* q, size_t) {
  if (P.have_kalman) be_h2d_sync(P.kalman.d_state, q, P.kalman.bytes);
  return 0;
}

int build_kalman(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!(d.features & NMX_F_BANDPOWER) || !(d.bp_features & 1u) || !d.bp_kalman_mask) return 0;
  NMX_REQUIRE(d.kalman_Tp > 0 && d.kalman_sigma_v > 0, "Kalman Tp and sigma_v must be positive");
  NMX_REQUIRE((d.bp_kalman_mask >> d.n_bands) == 0u, "Kalman band outside frequency_ranges_hz");
  NmxKalmanArgs& K = P.kalman.a;
  K.n_outputs = d.n_outputs + d.n_extra_cols; K.n_channels = d.n_channels; K.n_bands = d.n_bands;
  K.mask = d.bp_kalman_mask; K.cols = cv(d.bp_cols);
  const double T = d.kalman_Tp, sw2 = d.kalman_sigma_w * d.kalman_sigma_w;
  K.Tp = T; K.R = d.kalman_sigma_v;
  K.q00 = sw2 * T * T * T / 3.0; K.q01 = sw2 * T * T / 2.0; K.q11 = sw2 * T;
  const size_t bytes = (size_t)d.n_channels * d.n_bands * 6 * sizeof(double);
  K.state = P.kalman.d_state = (double*)plan_alloc(P, bytes);
  if (!K.state) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
  P.kalman.bytes = bytes;
  P.have_kalman = true;
  kalman_state_reset(P);
  return 0;
}

// behind the bank, on its stream: sequential over the hops of the chunk, and chunks run in order on `s`
static void launch_kalman(Plan& P, int nw, float* d_out, be_stream_t s) {
  if (!P.have_kalman) return;
  NmxKalmanArgs K = P.kalman.a;
  K.out = d_out; K.n_windows = nw;
  be_launch_kalman(K, s);
}

int build_sharp(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!(d.features & NMX_F_SHARPWAVE)) return 0;
  NMX_REQUIRE(d.n_sw_filters > 0, "sharp waves enabled without filters");
  NMX_REQUIRE(d.sw_n_combos <= NMX_MAX_SW_COMBOS_DEV, "too many sharp-wave (feature, estimator) pairs");
  NMX_REQUIRE(d.sw_distance_peaks >= 1 && d.sw_distance_troughs >= 1, "`distance` must be greater or equal to 1");
  NMX_REQUIRE(!(d.sw_between && !(d.sw_estimate_peaks && d.sw_estimate_troughs)),
              "apply_estimator_between_peaks_and_troughs needs both polarities estimated");
  NmxSharpArgs& A = P.sharp.a;
  A.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  A.n_channels = d.n_channels;
  A.n_filters = d.n_sw_filters;
  A.W = d.window;
  A.ms = (float)(1000.0 / d.sfreq);
  A.sharp_off = (int)(5.0 * (1000.0 / d.sfreq));
  A.dist_peaks = (int)std::ceil(d.sw_distance_peaks);
  A.dist_troughs = (int)std::ceil(d.sw_distance_troughs);
  A.est_peaks = d.sw_estimate_peaks;
  A.est_troughs = d.sw_estimate_troughs;
  A.between = d.sw_between;
  A.n_combos = d.sw_n_combos;
  A.feature_mask = 0;
  A.has_num_peaks = 0;
  int slot = 0;
  for (int i = 0; i < d.sw_n_combos; ++i) {
    NMX_REQUIRE(d.sw_combo_feature[i] >= 0 && d.sw_combo_feature[i] < NMX_SW_NFEAT &&
                d.sw_combo_estimator[i] >= 0 && d.sw_combo_estimator[i] < NMX_SWE_N, "bad sharp-wave combo");
    A.combo_feature[i] = d.sw_combo_feature[i];
    A.combo_est[i] = d.sw_combo_estimator[i];
    A.feature_mask |= 1u << d.sw_combo_feature[i];
    if (d.sw_combo_feature[i] == NMX_SW_NUM_PEAKS) {
      A.has_num_peaks = 1;
      // between mode: num_peaks is emitted once per (ch, filter) in its own block
      // (sharpwaves.py:316-321); otherwise the first num_peaks combo keeps its position
      bool first = true;
      for (int j = 0; j < i; ++j) first &= d.sw_combo_feature[j] != NMX_SW_NUM_PEAKS;
      A.combo_slot[i] = (d.sw_between || !first) ? -1 : slot++;
    } else {
      A.combo_slot[i] = slot++;
    }
  }
  A.fast_estimators = 1;
  for (int i = 0; i < d.sw_n_combos; ++i) {
    const int f = d.sw_combo_feature[i], e = d.sw_combo_estimator[i];
    if (f == NMX_SW_NUM_PEAKS) continue;
    if (!(e == NMX_SWE_MEAN || e == NMX_SWE_MAX || e == NMX_SWE_MIN)) A.fast_estimators = 0;
    if (f == NMX_SW_RISE_STEEPNESS || f == NMX_SW_DECAY_STEEPNESS || f == NMX_SW_SLOPE_RATIO) A.fast_estimators = 0;
  }
  A.dense_ok = env_int("NMX_SW_DENSE", 1) && A.fast_estimators && A.dist_peaks <= 10 && A.dist_troughs <= 10;
  A.cols = cv(d.sw_cols);
  A.np_cols = cv(d.sw_numpeaks_cols);
  const int pm = d.window / 2 + 2;      // an extremum needs a lower neighbour on both sides
  // 16-bit positions and two 15-bit counters per packed prefix sum.  The series + six position lists + the value list
  // of one item are 11 bytes per sample: ~14 500 samples fit 160 KiB of LDS; longer windows take the long-window mode
  // below, whose bound is the series alone (the partitioned FIR stage's: about 40 000 samples).
  // Windows beyond 4098 samples take the two-pass extrema walk of nmx_extrema (per-lane chunks > 64 samples).
  NMX_REQUIRE(pm <= 32767, "window too long for the sharp-wave kernel (16-bit positions)");
  A.pm = pm;
  const int lw = al4((pm + 1) / 2);    // floats per 16-bit list
  A.off_z = 0;
  A.off_emax = al4(d.window);
  A.off_emin = A.off_emax + lw;
  A.off_selt = A.off_emin + lw;
  A.off_lf = A.off_selt + lw;
  A.off_rt = A.off_lf + lw;
  A.off_selp = A.off_rt + lw;          // selP and st are dead once the pairs are formed:
  A.off_st = A.off_selp + lw;          // the per-feature value list aliases them
  A.off_vals = A.off_selp;
  const int tail = std::max(lw + al4((2 * pm + 3) / 4), al4(pm));
  A.off_res = A.off_selp + tail;
  A.off_red = A.off_res + al4(2 * d.sw_n_combos + 2);
  A.lds_floats = A.off_red + 64;
  // dense-first launch layout: series + two raw lists (128 entries suffice, longer ones are only
  // counted) + four 128-entry lists
  A.dz_emax = al4(d.window);
  A.dz_emin = A.dz_emax + 64;
  A.dz_selt = A.dz_emin + 64;
  A.dz_lf = A.dz_selt + 64;
  A.dz_rt = A.dz_lf + 64;
  A.dz_selp = A.dz_rt + 64;
  A.dz_res = A.dz_selp + 64;
  A.dz_lds_floats = A.dz_res + al4(2 * d.sw_n_combos + 2);
  // Long-window mode: the carve above does not fit 160 KiB.  The series (with res / red behind it) stays in LDS, the
  // lists [off_emax, off_res) move to one slab of device memory per resident workgroup of the persistent list kernel
  // (nmx_wave_slab.hip) -- about 7 bytes per sample and workgroup, whatever the number of hops in a chunk.  The
  // dense-first launch keeps its compact LDS layout: the number of extrema follows the pre-filter's pass band and the
  // window's duration, not the sampling rate, so most long windows end there.  (The emulator's be_launch_sharp gives
  // nmx_sharp_item the whole carve in host memory.)
  A.slab_mode = 0; A.slab_floats = 0; A.slab_blocks = 0; A.slab = nullptr;
  A.lz_res = al4(d.window);
  A.lz_red = A.lz_res + al4(2 * d.sw_n_combos + 2);
  A.lz_lds_floats = A.lz_red + 64;
  if ((size_t)A.lds_floats * 4 > 160 * 1024) {
    // (a guard: nmx_plan_create's 40 000-sample cap and the pre-filter's partitioned FIR stage, 39 872 samples, refuse first)
    NMX_REQUIRE((size_t)std::max(A.lz_lds_floats, A.dz_lds_floats) * 4 <= 160 * 1024,
                "window too long for the sharp-wave kernel: the series itself must fit 160 KiB of LDS (about 40 000 samples, "
                "the bound of the partitioned FIR stage)");
    A.slab_mode = 1;
    A.slab_floats = A.off_res - A.off_emax;
#ifndef NMX_HOST_EMU
    // one slab per resident workgroup: as many as the LDS copies of the series allow per CU, within 64 MiB of scratch
    A.slab_blocks = slab_workgroups(P, (size_t)A.lz_lds_floats * 4, (size_t)A.slab_floats);
#endif
  }
  int ns = 0;
  for (int i = 0; i < d.n_filters; ++i) ns += d.filters[i].sw_index >= 0;
  NMX_REQUIRE(ns == d.n_sw_filters, "every sharp-wave filter needs exactly one FIR");
  P.have_sharp = true;
  bool dense = A.dense_ok != 0;
#ifdef NMX_HOST_EMU   // (the register-resident path exists on the device only)
  dense = false;
#endif
  P.sharp.kind = A.slab_mode ? (dense ? NMX_SHARP_DENSE_SLAB : NMX_SHARP_SLAB) : (dense ? NMX_SHARP_DENSE_LIST : NMX_SHARP_LIST);
  return 0;
}

// the sharp-wave analysis of one chunk (nw hops, parity `par`: the bank has filled swy[par]) on stream `ss`
static int launch_sharp_stage(Plan& P, int par, int nw, float* d_out, be_stream_t ss, bool tev) {
  if (!P.have_sharp) return 0;
  SharpStage& S = P.sharp;
  const int n_items = nw * P.d.n_channels * P.d.n_sw_filters;
  int rc;
  NmxSharpArgs A = S.a;
  A.y = (const float*)S.swy[par].p; A.out = d_out; A.n_windows = nw;
  if (A.slab_blocks > 0) {   // long-window kinds: the list kernel's slabs, sized by its grid (nmx_wave_slab.hip)
    const double scale = g_ensure_scale;   // (a fixed size: not one to grow with the chunks that follow)
    g_ensure_scale = 1.0;
    rc = ensure(S.slab, (size_t)A.slab_blocks * A.slab_floats * sizeof(float));
    g_ensure_scale = scale;
    if (rc) return rc;
    A.slab = (float*)S.slab.p;
  }
  if (S.kind == NMX_SHARP_DENSE_LIST || S.kind == NMX_SHARP_DENSE_SLAB) {
    if ((rc = ensure(S.todo[par], (size_t)n_items))) return rc;
    A.todo = (unsigned char*)S.todo[par].p;
  }
  be_stage(ST_SHARP);
  if (tev) be_timer_start(P.timers[ST_SHARP], ss);
  be_launch_sharp(A, S.kind, n_items, (size_t)A.lds_floats * 4, ss);
  if (tev) be_timer_stop(P.timers[ST_SHARP], ss);
  return 0;
}

// Structure of a re-reference matrix (see nmx_k_prep.h): row = up to NMX_RS_TAPS explicit taps + b * (sum over
// a group of input rows).  A row with more than NMX_RS_TAPS non-zeros must consist of ONE repeated value o on a
// set G plus at most NMX_RS_TAPS other entries; the group is G joined with those entries (their taps become
// val - o) -- for the reference's "average" rows (1 on the channel itself, -1/(n-1) on every other good
// channel of its type, processing/rereference.py:61-63) that is the type group, shared by all of its rows.
int find_reref_structure(Plan& P) {
  const int C = P.d.n_channels, Cin = P.d.n_channels_in;
  const std::vector<double>& R = P.ref_matrix;
  std::vector<int> row_idx((size_t)C * NMX_RS_TAPS, 0), row_group(C, -1), members;
  std::vector<float> row_coef((size_t)C * NMX_RS_TAPS, 0.f), row_b(C, 0.f);
  std::map<std::vector<int>, int> groups;
  std::vector<std::vector<int>> group_list;
  for (int r = 0; r < C; ++r) {
    const double* row = R.data() + (size_t)r * Cin;
    std::vector<int> nz;
    for (int j = 0; j < Cin; ++j) if (row[j] != 0.0) nz.push_back(j);
    std::vector<std::pair<int, double>> taps;
    if ((int)nz.size() <= NMX_RS_TAPS) {
      for (int j : nz) taps.push_back({j, row[j]});
    } else {
      std::map<double, int> cnt;
      for (int j : nz) ++cnt[row[j]];
      double o = 0.0; int best = 0;
      for (auto& kv : cnt) if (kv.second > best) { best = kv.second; o = kv.first; }
      if ((int)nz.size() - best > NMX_RS_TAPS) return 0;
      for (int j : nz) if (row[j] != o) taps.push_back({j, row[j] - o});
      auto it = groups.find(nz);   // nz is sorted: G joined with the other entries
      int g;
      if (it == groups.end()) {
        if ((int)group_list.size() == NMX_RS_GROUPS) return 0;
        g = (int)group_list.size();
        groups[nz] = g;
        group_list.push_back(nz);
      } else {
        g = it->second;
      }
      row_group[r] = g;
      row_b[r] = (float)o;
    }
    for (size_t k = 0; k < taps.size(); ++k) {
      row_idx[(size_t)r * NMX_RS_TAPS + k] = taps[k].first;
      row_coef[(size_t)r * NMX_RS_TAPS + k] = (float)taps[k].second;
    }
  }
  NmxRerefStructArgs& A = P.front.rst;
  A.C = C; A.C_in = Cin;
  A.n_groups = (int)group_list.size();
  A.group_off[0] = 0;
  for (int g = 0; g < NMX_RS_GROUPS; ++g) {
    if (g < A.n_groups) members.insert(members.end(), group_list[g].begin(), group_list[g].end());
    A.group_off[g + 1] = (int)members.size();
  }
  A.row_idx = (const int*)upload(P, row_idx.data(), row_idx.size() * sizeof(int));
  A.row_coef = (const float*)upload(P, row_coef.data(), row_coef.size() * sizeof(float));
  A.row_group = (const int*)upload(P, row_group.data(), row_group.size() * sizeof(int));
  A.row_b = (const float*)upload(P, row_b.data(), row_b.size() * sizeof(float));
  A.members = (const int*)upload(P, members.data(), members.size() * sizeof(int));
  if (!A.row_idx || !A.row_coef || !A.row_group || !A.row_b || !A.members)
    return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  P.front.structured = true;
  return 0;
}

// The front end's re-reference, from the plan's copy of the matrix: its fp32 upload, the exact common-average test, the
// structure search.  (A plan without a matrix keeps d_R = null: its front end is the offset shift, or nothing.)
int build_front(Plan& P) {
  if (P.ref_matrix.empty()) return 0;
  FrontStage& F = P.front;
  const int C = P.d.n_channels, Cin = P.d.n_channels_in;
  const std::vector<double>& R = P.ref_matrix;
  std::vector<float> Rf(R.begin(), R.end());
  F.d_R = (float*)upload(P, Rf.data(), Rf.size() * sizeof(float));
  if (!F.d_R) return nmx_fail(NMX_E_NOMEM, "ref matrix");
  if (Cin == C && C >= 2 && env_int("NMX_CAR_FAST", 1)) {
    const double dg = R[0], of = R[1];
    bool ok = true;
    for (int i = 0; i < C && ok; ++i)
      for (int j = 0; j < C; ++j)
        if (std::fabs(R[(size_t)i * C + j] - (i == j ? dg : of)) > 1e-12) { ok = false; break; }
    if (ok) { F.car = true; F.car_diag = (float)dg; F.car_off = (float)of; }
  }
  if (!F.car && env_int("NMX_REREF_STRUCT", 1)) return find_reref_structure(P);
  return 0;
}

// y[C][ldy] = R x[C_in][ldx] over T samples (nan_to_num on load): rank-1 kernel for exact common-average
// matrices, taps + group sums when the structure was found, dense product otherwise
void launch_reref(Plan& P, const float* x, long long ldx, float* y, long long ldy, long long T, be_stream_t s) {
  const int C = P.d.n_channels;
  const FrontStage& F = P.front;
  if (F.car) {
    NmxCarArgs R{};
    R.x = x; R.ldx = ldx; R.y = y; R.ldy = ldy; R.C = C; R.T = T;
    R.diag = F.car_diag; R.off = F.car_off;
    R.sub = P.dc_sub_active ? P.d_dc_sub : nullptr; R.nanv = P.dc_active ? P.d_dc_nanv : nullptr;
    be_launch_car(R, s);
  } else if (F.structured) {
    NmxRerefStructArgs R = F.rst;
    R.x = x; R.ldx = ldx; R.y = y; R.ldy = ldy; R.T = T;
    R.sub = P.dc_sub_active ? P.d_dc_sub : nullptr; R.nanv = P.dc_active ? P.d_dc_nanv : nullptr;
    be_launch_reref_struct(R, s);
  } else {
    NmxRerefArgs R{};
    R.x = x; R.ldx = ldx; R.y = y; R.ldy = ldy; R.R = F.d_R;
    R.C = C; R.C_in = P.d.n_channels_in; R.T = T;
    R.sub = P.dc_sub_active ? P.d_dc_sub : nullptr; R.nanv = P.dc_active ? P.d_dc_nanv : nullptr;
    be_launch_reref(R, s);
  }
}

// The front end of a chunk, or of one window (lo = 0).  `x` / `ldx` address the recording with absolute sample indices; the
// samples [lo, lo + n_range) of every row are re-referenced once (windows overlap: per sample, not per window) -- or, in a
// plan without a matrix that carries constants, split: the learned constants are subtracted and a NaN becomes `nanv` -- into
// x_ref, and `v` then addresses x_ref with the same absolute indices.  Neither: `v` stays on the caller's rows.
// shift_if_host_offsets: whether the CALLER's constants alone (nothing learned, sub = 0: it handed over x - d) ask for the
// shift.  A chunk: yes -- a NaN in the caller's split must still become the recording's value 0, i.e. -d in the split
// domain (nanv); the consumers' own clean-on-load would make it 0 + d = d, and the burst history of that channel would part
// from the reference's.  nmx_preprocess_window: no -- it has made a NaN the value 0 on the host before it subtracted d.
static int launch_front(Plan& P, const float* x, long long ldx, long long lo, long long n_range, bool shift_if_host_offsets,
                        be_stream_t s, WinView& v) {
  FrontStage& F = P.front;
  const int C = P.d.n_channels;
  if (!F.d_R && !(shift_if_host_offsets ? P.dc_active : P.dc_sub_active)) return 0;
  int rc = ensure(F.x_ref, (size_t)C * n_range * sizeof(float));
  if (rc) return rc;
  if (F.d_R) {
    launch_reref(P, x + lo, ldx, (float*)F.x_ref.p, n_range, n_range, s);
  } else {
    NmxShiftArgs Sh{};
    Sh.x = x + lo; Sh.ldx = ldx; Sh.y = (float*)F.x_ref.p; Sh.ldy = n_range; Sh.C = C; Sh.T = n_range;
    Sh.sub = P.d_dc_sub; Sh.nanv = P.d_dc_nanv;
    be_launch_shift(Sh, s);
  }
  v = WinView{(const float*)F.x_ref.p - lo, n_range, v.win_stride, v.starts, 0};
  return 0;
}
