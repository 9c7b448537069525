// nmx_engine_dc.inc -- the OFFSET SPLIT of the fp32 path.  Included by nmx_engine.inc (inside its namespace).
//
// The reference computes in float64 from the raw recording (stream/data_processor.py:238-260); a channel's DC offset --
// electrode potentials, amplifier offsets: easily 10^3 .. 10^5 times the signal -- costs it nothing.  In fp32 every
// rounding of a hand-off tensor is relative to the VALUE, i.e. to the offset: the near-null spectral bins of the STFT /
// Welch features then sit on a noise floor that scales with the offset, not with the signal.  The engine therefore
// carries a recording as
//         x[j][t] = u[j][t] + d_j            u: fp32 on the device,  d_j: one float64 constant per input row
// and moves the constants analytically through every LINEAR stage in float64 on the host:
//     re-reference  y = R x          ->  y = R u + R d                      (processing/rereference.py:99-100)
//     notch         odd reflection of a constant is the constant; a FIR maps it to d * sum(h)
//                                                                           (filter/notch_filter.py:78-93)
// so that the pre-processed windows the features read are  w[c][n] = v[c][n] + D_c.  What a feature does with D_c:
//     Hjorth / LineLength / Welch (constant detrend) / sharp waves:  differences and variances -- nothing
//     Raw:   v[-1] + D                    FFT:  bin 0 += N D              STFT:  bins 0, 1 += D * DFT(window)  (NmxOsc::wdc)
//     FIR bank (zero-padded "same" convolution, filter/mne_filter.py:110-116): it DOES see the level of the window (edge
//     transients of size D that the reference's features contain): D is added back on load (NmxBankArgs::dcf), where its
//     rounding is relative to what the filter output is made of.
// Where the constants come from:
//   * host offsets (nmx_plan_set_offsets): the caller hands over u = x - d, d of its choosing -- the float64 callers
//     (engine.py) subtract before they cast, so the cast itself no longer rounds at the offset's magnitude;
//   * learned offsets: fp32 input that passes a re-reference kernel is split THERE (NmxCarArgs::sub ...): sub_j = the mean
//     of row j over the first window the plan ever sees (when that level exceeds four times the row's spread; 0 otherwise),
//     learned once, part of the plan's state (nmx_state_*) -- a result must not depend on how the hops were batched, so
//     the constants may not either.
// Plans with a stage that is not affine in the window (resampler with its limited reflection, raw normaliser,
// preprocessing filter with zero padding, a notch longer than the window) do not split: dc_ok = false, everything
// behaves as before.

static void dc_recompute(Plan& P, be_stream_t s) {
  const int Cin = P.d.n_channels_in, C = P.d.n_channels;
  std::vector<double> din((size_t)Cin, 0.0);
  bool any = false, any_sub = false;
  for (int j = 0; j < Cin; ++j) {
    din[j] = (P.dc_host_set ? P.dc_host[j] : 0.0) + (double)P.dc_sub_h[j];
    any = any || din[j] != 0.0;
    any_sub = any_sub || P.dc_sub_h[j] != 0.f;
  }
  P.dc_pre_h.assign((size_t)C, 0.0);
  std::vector<float> pref((size_t)C, 0.f);
  for (int i = 0; i < C; ++i) {
    double acc = 0.0;
    if (!P.ref_matrix.empty()) {
      const double* r = P.ref_matrix.data() + (size_t)i * Cin;
      for (int j = 0; j < Cin; ++j) acc += r[j] * din[j];
    } else {
      acc = din[i];
    }
    P.dc_pre_h[i] = acc * P.dc_gain;
    pref[i] = (float)P.dc_pre_h[i];
  }
  std::vector<float> nanv((size_t)Cin);
  for (int j = 0; j < Cin; ++j) nanv[j] = -(float)din[j];
  be_h2d_async(P.d_dc_nanv, nanv.data(), (size_t)Cin * sizeof(float), s);
  be_h2d_async(P.d_dc_sub, P.dc_sub_h.data(), (size_t)Cin * sizeof(float), s);
  be_h2d_async(P.d_dc_pref, pref.data(), (size_t)C * sizeof(float), s);
  be_sync(s);   // (pageable sources on the stack / in vectors that may change: once per change of the constants)
  P.dc_active = any;
  P.dc_sub_active = any_sub;
  P.dc_dirty = false;
}

static int dc_build(Plan& P) {
  P.dc_ok = env_int("NMX_DC_SPLIT", 1) != 0 && !P.have_resample && !P.have_rawnorm && P.pre.empty() &&
            (!P.have_notch || P.notch.a.pad_half <= P.notch.a.n_edge);
  P.dc_auto = env_int("NMX_DC_AUTO", 1) != 0;
  P.dc_gain = 1.0;
  if (P.have_notch) {
    double g = 0.0;
    for (double t : P.notch_taps) g += t;
    P.dc_gain = g;
  }
  const int Cin = P.d.n_channels_in, C = P.d.n_channels;
  P.dc_host.assign((size_t)Cin, 0.0);
  P.dc_sub_h.assign((size_t)Cin, 0.f);
  P.dc_pre_h.assign((size_t)C, 0.0);
  if (!P.dc_ok) return 0;
  P.d_dc_sub = (float*)plan_alloc(P, (size_t)Cin * sizeof(float));
  P.d_dc_pref = (float*)plan_alloc(P, (size_t)C * sizeof(float));
  P.d_dc_nanv = (float*)plan_alloc(P, (size_t)Cin * sizeof(float));
  if (!P.d_dc_sub || !P.d_dc_pref || !P.d_dc_nanv) return nmx_fail(NMX_E_NOMEM, "offset tables");
  be_memset_sync(P.d_dc_nanv, 0, (size_t)Cin * sizeof(float));
  be_memset_sync(P.d_dc_sub, 0, (size_t)Cin * sizeof(float));
  be_memset_sync(P.d_dc_pref, 0, (size_t)C * sizeof(float));
  return 0;
}

// Start of a batch: learn the rows' constants from the first window the plan sees (fp32 input in front of a
// re-reference or notch kernel, no host offsets), refresh the device tables when anything changed.
static int dc_prepare(Plan& P, const float* x, long long ldx, long long t0, bool host, be_stream_t s) {
  if (!P.dc_ok) return 0;
  if (P.dc_auto && (P.front.d_R || P.have_notch) && !P.dc_host_set && !P.dc_learned) {
    // the first window the plan sees: a row is split at its mean there when that level exceeds four times the
    // row's spread -- a recording without offsets keeps its samples as they are
    const int Cin = P.d.n_channels_in, Wi = P.w_in;
    std::vector<float> first((size_t)Cin * Wi, 0.f);
    if (host) {
      if (P.pipe_in_ready) {   // the caller stages the recording slice by slice (nmx_plan_set_pipeline): the first window first
        long long spins = 0;
        while (__atomic_load_n(P.pipe_in_ready, __ATOMIC_ACQUIRE) < t0 + Wi) {
          if (++spins > 2000000) return nmx_fail(NMX_E_INVALID, "nmx_plan_set_pipeline: the input never became ready");
          std::this_thread::sleep_for(std::chrono::microseconds(5));
        }
      }
      for (int j = 0; j < Cin; ++j) memcpy(&first[(size_t)j * Wi], x + (size_t)j * ldx + t0, (size_t)Wi * sizeof(float));
    } else {
      be_d2h_2d_async(first.data(), (size_t)Wi * sizeof(float), x + t0, (size_t)ldx * sizeof(float), (size_t)Wi * sizeof(float),
                      (size_t)Cin, s);
      int rc = be_sync(s);
      if (rc) return rc;
    }
    const double ratio = 4.0;
    for (int j = 0; j < Cin; ++j) {
      double sum = 0.0, sq = 0.0;
      long long n = 0;
      for (int i = 0; i < Wi; ++i) {
        const double v = (double)first[(size_t)j * Wi + i];
        if (std::isfinite(v)) { sum += v; ++n; }
      }
      const double m = n ? sum / (double)n : 0.0;
      for (int i = 0; i < Wi; ++i) {
        const double v = (double)first[(size_t)j * Wi + i];
        if (std::isfinite(v)) sq += (v - m) * (v - m);
      }
      const double sd = n ? std::sqrt(sq / (double)n) : 0.0;
      const float mf = (float)m;
      P.dc_sub_h[j] = (std::isfinite(mf) && std::fabs(m) > ratio * sd) ? mf : 0.f;
    }
    P.dc_learned = true;
    P.dc_dirty = true;
  }
  if (P.dc_dirty) dc_recompute(P, s);
  return 0;
}

// ---- consumers of the pre-processed windows `v` of a chunk (nw hops) ----------------------------------------------------
// The windows with the offset added back, dense [nw][C][W], for a kernel that cannot take the offset on load.  `made`
// (run_chunk's, false when the chunk starts): x_dc holds this chunk's windows already -- one copy serves every such reader.
static int dc_windows(Plan& P, const WinView& v, int nw, be_stream_t s, bool& made, WinView* dense) {
  const int C = P.d.n_channels, W = P.d.window;
  if (!made) {
    int rc = ensure(P.x_dc, (size_t)nw * C * W * sizeof(float));
    if (rc) return rc;
    NmxTapArgs T{};
    view_into(T, v);
    T.y = (float*)P.x_dc.p; T.C = C; T.W = W; T.add = P.d_dc_pref;
    be_launch_tap(T, nw * C, s);
    made = true;
  }
  *dense = dense_view(P.x_dc.p, C, W);
  return 0;
}
// the offset table a consumer's kernel adds on load (null: no constant is carried)
static const float* dc_table(const Plan& P) { return P.dc_active ? P.d_dc_pref : nullptr; }
// What a consumer's arguments read (x .. clean_on_load, dcf): `v` and the offset table when its kernel takes the offset on
// load (FirStage::takes_dc, TimeOscStage::takes_dc), else the copy of dc_windows and no table.
template <class Args>
static int dc_bind(Plan& P, Args& A, bool takes_dc, const WinView& v, int nw, be_stream_t s, bool& made) {
  WinView use = v;
  A.dcf = dc_table(P);
  if (A.dcf && !takes_dc) {
    int rc = dc_windows(P, v, nw, s, made, &use);
    if (rc) return rc;
    A.dcf = nullptr;
  }
  view_into(A, use);
  return 0;
}

// ---- the offsets' section of the state blob: learned flag | host-set flag | sub[C_in] (float, padded to 8 bytes) |
// host[C_in] (double).  All of it lives on the host: the device tables follow at the next batch (dc_dirty).  Reset forgets
// the learned constants; the caller's are a setting of the plan (nmx_plan_set_offsets).
static void dc_state_reset(Plan& P) {
  if (!P.dc_ok) return;
  std::fill(P.dc_sub_h.begin(), P.dc_sub_h.end(), 0.f);
  P.dc_learned = false;
  P.dc_dirty = true;
}
static size_t dc_state_bytes(const Plan& P) {
  if (!P.dc_ok) return 0;
  const size_t Cin = (size_t)P.d.n_channels_in;
  return 2 * sizeof(long long) + ((Cin * sizeof(float) + 7) & ~(size_t)7) + Cin * sizeof(double);
}
static void dc_state_export(const Plan& P, char* q) {
  if (!P.dc_ok) return;
  const size_t Cin = (size_t)P.d.n_channels_in;
  const long long a = P.dc_learned ? 1 : 0, b = P.dc_host_set ? 1 : 0;
  memcpy(q, &a, sizeof a); q += sizeof a;
  memcpy(q, &b, sizeof b); q += sizeof b;
  memset(q, 0, (Cin * sizeof(float) + 7) & ~(size_t)7);
  memcpy(q, P.dc_sub_h.data(), Cin * sizeof(float)); q += (Cin * sizeof(float) + 7) & ~(size_t)7;
  memcpy(q, P.dc_host.data(), Cin * sizeof(double));
}
static int dc_state_import(Plan& P, const char* q, size_t) {
  if (!P.dc_ok) return 0;
  const size_t Cin = (size_t)P.d.n_channels_in;
  long long a = 0, b = 0;
  memcpy(&a, q, sizeof a); q += sizeof a;
  memcpy(&b, q, sizeof b); q += sizeof b;
  memcpy(P.dc_sub_h.data(), q, Cin * sizeof(float)); q += (Cin * sizeof(float) + 7) & ~(size_t)7;
  memcpy(P.dc_host.data(), q, Cin * sizeof(double));
  P.dc_learned = a != 0;
  P.dc_host_set = b != 0;
  P.dc_dirty = true;
  return 0;
}
