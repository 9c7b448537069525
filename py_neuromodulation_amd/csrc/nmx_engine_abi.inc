// nmx_engine_abi.inc -- C ABI, part 1: plan create / destroy, state reset / export / import.  Included by nmx_engine.inc.

// =========================================================================================
extern "C" {

int nmx_abi_version(void) { return NMX_ABI_VERSION; }
int nmx_device_count(void) { return be_device_count(); }
const char* nmx_last_error(void) { return g_nmx_err.c_str(); }

int nmx_plan_destroy(nmx_plan* plan) {
  Plan* P = (Plan*)plan;
  if (!P) return 0;
  be_set_device(P->device);
  be_sync(P->stream);
  be_sync(P->stream_b);
  be_sync(P->stream_d);
  be_sync(P->stream_f);
  for (void* t : P->tables) be_free(t);
  for (Buf* b : {&P->tap, &P->rn_qt, &P->rn_qn, &P->bursts.slots, &P->to_todo, &P->x_dc, &P->x_in, &P->x_ref, &P->x_rs, &P->x_rn, &P->rn_mean, &P->rn_scale, &P->x_pf[0], &P->x_pf[1], &P->sharp.todo[0], &P->sharp.todo[1], &P->sharp.slab, &P->y_notch, &P->bursts.env[0], &P->bursts.env[1], &P->bursts.env_full[0], &P->bursts.env_full[1], &P->sharp.swy[0], &P->sharp.swy[1], &P->bursts.yb, &P->bursts.thr[0], &P->bursts.thr[1], &P->out, &P->starts, &P->mask})
    if (b->p) be_free(b->p);
  for (void* p : {(void*)P->bursts.d_top, (void*)P->bursts.d_counts, (void*)P->bursts.d_floor})
    if (p) be_free(p);
  if (P->d_R) be_free(P->d_R);
  if (P->d_dc_sub) be_free(P->d_dc_sub);
  if (P->d_dc_pref) be_free(P->d_dc_pref);
  if (P->d_dc_nanv) be_free(P->d_dc_nanv);
  if (P->d_kf) be_free(P->d_kf);
  if (P->rn.ring) be_free(P->rn.ring);
  if (P->rn.count) be_free(P->rn.count);
  if (P->rn.len) be_free(P->rn.len);
  if (P->win_pin.p) be_host_free(P->win_pin.p);
  for (auto& t : P->timers) be_timer_destroy(t);
  be_event_destroy(P->ev_fork);
  be_event_destroy(P->ev_join[0]);
  be_event_destroy(P->ev_join[1]);
  be_event_destroy(P->ev_main[0]);
  be_event_destroy(P->ev_main[1]);
  be_event_destroy(P->ev_final);
  be_event_destroy(P->ev_fork_d);
  be_event_destroy(P->ev_join_d[0]);
  be_event_destroy(P->ev_join_d[1]);
  be_stream_destroy(P->stream_d);
  be_stream_destroy(P->stream_f);
  be_event_destroy(P->ev_h2d);
  be_event_destroy(P->ev_done[0]);
  be_event_destroy(P->ev_done[1]);
  be_stream_destroy(P->stream_b);
  be_stream_destroy(P->stream_c);
  be_stream_destroy(P->stream_o);
  be_event_destroy(P->ev_in_free[0]);
  be_event_destroy(P->ev_in_free[1]);
  be_stream_destroy(P->stream);
  delete P;
  be_dev_pool_age();
  return 0;
}

int nmx_plan_create(const nmx_plan_desc* desc, nmx_plan** out) {
  if (!desc || !out) return nmx_fail(NMX_E_INVALID, "null argument");
  *out = nullptr;
  NMX_REQUIRE(desc->abi_version == NMX_ABI_VERSION, "nmx_plan_desc.abi_version mismatch");
  NMX_REQUIRE(desc->n_channels >= 1, "n_channels must be >= 1");
  // 16 384 samples for a plan in general; up to 40 000 (the partitioned FIR stage's bound) for a plan whose window-sized
  // stages are all sized for it: the FIR stages (notch, preprocessing_filter, the sharp-wave pre-filters), re-referencing,
  // the sharp-wave analysis (long-window mode of build_sharp) and the long-window time / oscillatory kernel (build_timeosc:
  // Hjorth, raw, line length, FFT, Welch)
  NMX_REQUIRE(desc->window >= 4 && desc->window <= 40000, "window must be in [4, 40 000 samples]");
  const uint32_t long_ok = NMX_F_SHARPWAVE | NMX_F_HJORTH | NMX_F_RAW | NMX_F_LINELENGTH | NMX_F_FFT | NMX_F_WELCH;
  NMX_REQUIRE(desc->window <= 16384 || (!(desc->features & ~long_ok) && desc->raw_norm_method <= 0 && desc->raw_window <= 0),
              "window must be in [4, 16 384] samples for a plan with stft, bandpass_filter, bursts, coherence, raw_normalization or "
              "raw_resampling; only raw_hjorth, return_raw, linelength, fft, welch and sharpwave_analysis run up to 40 000 samples, behind "
              "re-referencing and FIR pre-processing");
  NMX_REQUIRE(desc->sfreq > 0 && desc->feat_hz > 0, "sfreq and feat_hz must be positive");
  NMX_REQUIRE(desc->n_outputs >= 1, "n_outputs must be >= 1");
  NMX_REQUIRE(desc->n_extra_cols >= 0 && (long long)desc->n_outputs + desc->n_extra_cols < (1ll << 30),
              "n_extra_cols must be >= 0 and the row shorter than 2^30 floats");
  NMX_REQUIRE(desc->n_bands >= 0 && desc->n_bands <= NMX_MAX_BANDS, "n_bands out of range");
  NMX_REQUIRE(desc->n_filters >= 0 && desc->n_filters <= NMX_MAX_FILTERS, "n_filters out of range");
  const int ndev = be_device_count();
  if (ndev <= 0)
    return nmx_fail(NMX_E_NODEVICE, "no HIP device found: libnmx has no CPU path (gfx950 required)");
  NMX_REQUIRE(desc->device >= 0 && desc->device < ndev, "device ordinal out of range");
  Plan* P = new Plan();
  P->d = *desc;
  P->device = desc->device;
  for (auto& t : P->timers) t = be_timer_t{};
  int rc = be_set_device(P->device);
  if (rc) { delete P; return rc; }
  P->n_cu = be_cu_count(P->device);
  P->w_in = P->d.raw_window > 0 ? P->d.raw_window : P->d.window;   // samples per incoming window
  P->stream = be_stream_create();
  P->stream_b = be_stream_create_high();
  be_event_create(P->ev_fork);
  be_event_create(P->ev_join[0]);
  be_event_create(P->ev_join[1]);
  be_event_create(P->ev_main[0]);
  be_event_create(P->ev_main[1]);
  be_event_create(P->ev_final);
  P->stream_f = be_stream_create();
  P->stream_d = be_stream_create();
  be_event_create(P->ev_fork_d);
  be_event_create(P->ev_join_d[0]);
  be_event_create(P->ev_join_d[1]);
  P->stream_c = be_stream_create();
  P->stream_o = be_stream_create();
  be_event_create(P->ev_in_free[0]);
  be_event_create(P->ev_in_free[1]);
  be_event_create(P->ev_h2d);
  be_event_create(P->ev_done[0]);
  be_event_create(P->ev_done[1]);
  P->host_chunk_windows = std::max(1, env_int("NMX_HOST_CHUNK_WINDOWS", 512));
  P->host_first_chunk = std::max(1, env_int("NMX_HOST_FIRST_CHUNK", 128));
  P->overlap = env_int("NMX_OVERLAP", 4);
  for (auto& t : P->timers) be_timer_create(t);
  P->taps.resize(desc->n_filters);
  for (int i = 0; i < desc->n_filters; ++i) {
    if (!desc->filters[i].taps || desc->filters[i].n_taps < 1) {
      nmx_plan_destroy((nmx_plan*)P);
      return nmx_fail(NMX_E_INVALID, "filter without taps");
    }
    P->taps[i].assign(desc->filters[i].taps, desc->filters[i].taps + desc->filters[i].n_taps);
    P->d.filters[i].taps = P->taps[i].data();
  }
  if (desc->n_pre_filters < 0 || desc->n_pre_filters > NMX_MAX_PRE_FILTERS) {
    nmx_plan_destroy((nmx_plan*)P);
    return nmx_fail(NMX_E_INVALID, "n_pre_filters out of range");
  }
  P->pre_taps.resize(desc->n_pre_filters);
  for (int i = 0; i < desc->n_pre_filters; ++i) {
    if (!desc->pre_taps[i] || desc->n_pre_taps[i] < 1) {
      nmx_plan_destroy((nmx_plan*)P);
      return nmx_fail(NMX_E_INVALID, "pre-filter without taps");
    }
    P->pre_taps[i].assign(desc->pre_taps[i], desc->pre_taps[i] + desc->n_pre_taps[i]);
    P->d.pre_taps[i] = P->pre_taps[i].data();
  }
  if (desc->notch_taps) {
    P->notch_taps.assign(desc->notch_taps, desc->notch_taps + desc->n_notch_taps);
    P->d.notch_taps = P->notch_taps.data();
  }
  if (desc->ref_matrix) {
    if (desc->n_channels_in < 1) { nmx_plan_destroy((nmx_plan*)P); return nmx_fail(NMX_E_INVALID, "n_channels_in"); }
    const size_t n = (size_t)desc->n_channels * desc->n_channels_in;
    P->ref_matrix.assign(desc->ref_matrix, desc->ref_matrix + n);
    P->d.ref_matrix = P->ref_matrix.data();
    std::vector<float> Rf(n);
    for (size_t i = 0; i < n; ++i) Rf[i] = (float)P->ref_matrix[i];
    P->d_R = (float*)be_alloc(n * sizeof(float));
    if (!P->d_R) { nmx_plan_destroy((nmx_plan*)P); return nmx_fail(NMX_E_NOMEM, "ref matrix"); }
    be_h2d_sync(P->d_R, Rf.data(), n * sizeof(float));
    const int C = desc->n_channels;
    if (desc->n_channels_in == C && C >= 2 && env_int("NMX_CAR_FAST", 1)) {
      const double dg = P->ref_matrix[0], of = P->ref_matrix[1];
      bool ok = true;
      for (int i = 0; i < C && ok; ++i)
        for (int j = 0; j < C; ++j)
          if (std::fabs(P->ref_matrix[(size_t)i * C + j] - (i == j ? dg : of)) > 1e-12) { ok = false; break; }
      if (ok) { P->car = true; P->car_diag = (float)dg; P->car_off = (float)of; }
    }
    if (!P->car && env_int("NMX_REREF_STRUCT", 1) && (rc = find_reref_structure(*P))) {
      nmx_plan_destroy((nmx_plan*)P);
      return rc;
    }
  } else {
    P->d.n_channels_in = desc->n_channels;
  }
  P->nt_timeosc = desc->window <= 1024 ? 128 : 256;
  P->nt_bank = 256;
  P->tiny_inline = env_int("NMX_TINY_INLINE", 1) != 0;
  P->chunk_windows = env_int("NMX_CHUNK_WINDOWS", 1024);
  P->norm_chunk_windows = std::max(1, env_int("NMX_NORM_CHUNK_WINDOWS", P->norm_chunk_windows));
  if ((rc = build_timeosc(*P)) || (rc = build_coh(*P)) || (rc = build_bank(*P)) || (rc = build_notch(*P)) ||
      (rc = build_bursts(*P)) || (rc = build_sharp(*P)) || (rc = build_kalman(*P)) || (rc = build_resample(*P)) ||
      (rc = build_prefilters(*P)) || (rc = build_rawnorm(*P)) || (rc = dc_build(*P))) {
    std::string keep = g_nmx_err;
    nmx_plan_destroy((nmx_plan*)P);
    g_nmx_err = keep;
    return rc;
  }
#ifndef NMX_HOST_EMU
  choose_notch_bank_fuse(*P);   // (behind every stage's own choice: it reads the notch's, the bank's and what sits between them)
#endif
  P->bank.takes_dc = fir_stage_takes_dc(P->bank);   // (behind the fuse choice: a launch inside the notch kernel takes it)
  if ((P->d.features & NMX_F_BANDPOWER) && !P->have_bank) {
    nmx_plan_destroy((nmx_plan*)P);
    return nmx_fail(NMX_E_INVALID, "bandpass_filter enabled without filters");
  }
  *out = (nmx_plan*)P;
  return 0;
}

// ---- offset split (nmx_engine_dc.inc) ---------------------------------------------------------------------------------------
int nmx_plan_carries_offsets(const nmx_plan* plan, int* yes) {
  if (!plan || !yes) return nmx_fail(NMX_E_INVALID, "null argument");
  *yes = ((const Plan*)plan)->dc_ok ? 1 : 0;
  return 0;
}

int nmx_plan_set_offsets(nmx_plan* plan, const double* d_in) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  if (!d_in) {   // back to "no host offsets" (the learned constants are state: nmx_state_reset)
    if (P->dc_host_set) { std::fill(P->dc_host.begin(), P->dc_host.end(), 0.0); P->dc_host_set = false; P->dc_dirty = true; }
    return 0;
  }
  NMX_REQUIRE(P->dc_ok, "this plan has a stage that is not affine in the window (resampler, raw normaliser, preprocessing "
                        "filter, notch longer than the window): it cannot carry offsets");
  for (int j = 0; j < P->d.n_channels_in; ++j) NMX_REQUIRE(std::isfinite(d_in[j]), "offsets must be finite");
  P->dc_host.assign(d_in, d_in + P->d.n_channels_in);
  P->dc_host_set = true;
  if (P->dc_learned) dc_reset(*P);   // (the caller's split replaces the learned one)
  P->dc_dirty = true;
  return 0;
}

int nmx_plan_get_offsets(nmx_plan* plan, double* d_in, double* d_pre, int* state) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  if (P->dc_ok && P->dc_dirty) {
    be_set_device(P->device);
    dc_recompute(*P, P->stream);
  }
  if (d_in)
    for (int j = 0; j < P->d.n_channels_in; ++j)
      d_in[j] = (P->dc_host_set ? P->dc_host[j] : 0.0) + (double)P->dc_sub_h[j];
  if (d_pre)
    for (int i = 0; i < P->d.n_channels; ++i) d_pre[i] = P->dc_pre_h[i];
  if (state) *state = (P->dc_host_set ? 1 : 0) | (P->dc_learned ? 2 : 0);
  return 0;
}

int nmx_plan_set_pipeline(nmx_plan* plan, const volatile int64_t* in_ready_samples, volatile int64_t* out_done_windows) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  P->pipe_in_ready = in_ready_samples;
  P->pipe_out_done = out_done_windows;
  return 0;
}

int nmx_plan_n_outputs(const nmx_plan* plan, int64_t* n) {
  if (!plan || !n) return nmx_fail(NMX_E_INVALID, "null argument");
  *n = ((const Plan*)plan)->d.n_outputs;
  return 0;
}

// raw normaliser: hops seen | ring capacity of the exporting plan | rings | counts | lengths.  The capacity depends on the
// window length; a stream with ragged window lengths hands the blob of one plan to the plan of the other length, which
// re-lays the histories into its own rings (nmx_state_import).
static size_t rn_state_bytes_cap(const Plan& P, long long cap) {
  return 2 * sizeof(long long) + (size_t)P.d.n_channels * (size_t)cap * sizeof(float) + P.rn_cnt_bytes + P.rn_len_bytes;
}
static size_t burst_state_bytes(const Plan& P) { return P.bursts.top_bytes + P.bursts.counts_bytes; }   // burst ring | counts
static size_t rn_state_bytes(const Plan& P) { return P.have_rawnorm ? rn_state_bytes_cap(P, P.rn.cap) : 0; }

int nmx_state_reset(nmx_plan* plan) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  dc_reset(*P);
  if (!P->have_bursts && !P->have_kalman && !P->have_rawnorm) return 0;
  be_set_device(P->device);
  be_sync(P->stream);
  if (P->last_stream && P->last_stream != P->stream) be_sync(P->last_stream);
  be_sync(P->stream_b);
  be_sync(P->stream_d);
  be_sync(P->stream_f);
  if (P->have_rawnorm) rawnorm_reset(*P);
  if (P->have_bursts) {
    BurstStage& B = P->bursts;
    be_memset_sync(B.d_top, 0, B.top_bytes);
    be_memset_sync(B.d_counts, 0, B.counts_bytes);
    burst_floor_reset(*P);
    B.seen = 0;
  }
  if (P->have_kalman) kalman_reset(*P);
  return 0;
}

int nmx_state_size(const nmx_plan* plan, int64_t* n_bytes) {
  const Plan* P = (const Plan*)plan;
  if (!P || !n_bytes) return nmx_fail(NMX_E_INVALID, "null argument");
  *n_bytes = (int64_t)(burst_state_bytes(*P) + P->kf_bytes + dc_state_bytes(*P) + rn_state_bytes(*P));   // burst ring | counts | Kalman | offsets | raw normaliser
  return 0;
}

int nmx_state_export(nmx_plan* plan, void* dst, int64_t n_bytes) {
  Plan* P = (Plan*)plan;
  if (!P || (!dst && n_bytes)) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE((size_t)n_bytes == burst_state_bytes(*P) + P->kf_bytes + dc_state_bytes(*P) + rn_state_bytes(*P), "state size mismatch");
  if (!n_bytes) return 0;
  dc_state_export(*P, (char*)dst + burst_state_bytes(*P) + P->kf_bytes);   // (never next to a raw normaliser)
  be_set_device(P->device);
  be_sync(P->stream);
  if (P->last_stream && P->last_stream != P->stream) be_sync(P->last_stream);   // batch launched on a caller's stream
  be_sync(P->stream_b);
  be_sync(P->stream_f);
  if (P->have_bursts) {
    be_d2h_sync(dst, P->bursts.d_top, P->bursts.top_bytes);
    be_d2h_sync((char*)dst + P->bursts.top_bytes, P->bursts.d_counts, P->bursts.counts_bytes);
  }
  if (P->have_kalman) be_d2h_sync((char*)dst + burst_state_bytes(*P), P->d_kf, P->kf_bytes);
  if (P->have_rawnorm) {
    char* q = (char*)dst + burst_state_bytes(*P) + P->kf_bytes;
    const long long cap = P->rn.cap;
    memcpy(q, &P->rn_hops, sizeof(long long)); q += sizeof(long long);
    memcpy(q, &cap, sizeof(long long)); q += sizeof(long long);
    be_d2h_sync(q, P->rn.ring, P->rn_ring_bytes); q += P->rn_ring_bytes;
    be_d2h_sync(q, P->rn.count, P->rn_cnt_bytes); q += P->rn_cnt_bytes;
    be_d2h_sync(q, P->rn.len, P->rn_len_bytes);
  }
  return 0;
}

int nmx_state_import(nmx_plan* plan, const void* src, int64_t n_bytes) {
  Plan* P = (Plan*)plan;
  if (!P || (!src && n_bytes)) return nmx_fail(NMX_E_INVALID, "null argument");
  const size_t fixed = burst_state_bytes(*P) + P->kf_bytes + dc_state_bytes(*P);
  long long src_cap = P->have_rawnorm ? P->rn.cap : 0;
  if (P->have_rawnorm && (size_t)n_bytes >= fixed + 2 * sizeof(long long))   // the exporting plan's ring capacity
    memcpy(&src_cap, (const char*)src + fixed + sizeof(long long), sizeof(long long));
  NMX_REQUIRE(!P->have_rawnorm || (src_cap > 0 && src_cap < (1ll << 31)), "state blob: bad raw-normaliser header");
  NMX_REQUIRE((size_t)n_bytes == fixed + (P->have_rawnorm ? rn_state_bytes_cap(*P, src_cap) : 0), "state size mismatch");
  if (!n_bytes) return 0;
  dc_state_import(*P, (const char*)src + burst_state_bytes(*P) + P->kf_bytes);
  be_set_device(P->device);
  be_sync(P->stream);
  if (P->last_stream && P->last_stream != P->stream) be_sync(P->last_stream);
  be_sync(P->stream_b);
  be_sync(P->stream_f);
  if (P->have_bursts) {
    BurstStage& B = P->bursts;
    be_h2d_sync(B.d_top, src, B.top_bytes);
    be_h2d_sync(B.d_counts, (const char*)src + B.top_bytes, B.counts_bytes);
    memcpy(&B.seen, (const char*)src + B.top_bytes + sizeof(long long), sizeof(long long));   // counts[0][1]
    burst_floor_reset(*P);   // (a bound of the history this plan had, not of the imported one: the next steady walk writes it anew)
  }
  if (P->have_kalman) be_h2d_sync(P->d_kf, (const char*)src + burst_state_bytes(*P), P->kf_bytes);
  if (P->have_rawnorm) {
    const char* q = (const char*)src + burst_state_bytes(*P) + P->kf_bytes;
    memcpy(&P->rn_hops, q, sizeof(long long)); q += 2 * sizeof(long long);
    const int C = P->d.n_channels, cap = P->rn.cap;
    const float* ring_src = (const float*)q;
    const char* cnt_src = q + (size_t)C * (size_t)src_cap * sizeof(float);
    const char* len_src = cnt_src + P->rn_cnt_bytes;
    if (src_cap == cap) {
      be_h2d_sync(P->rn.ring, ring_src, P->rn_ring_bytes);
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
      be_h2d_sync(P->rn.ring, ring.data(), P->rn_ring_bytes);
    }
    be_h2d_sync(P->rn.count, cnt_src, P->rn_cnt_bytes);
    be_h2d_sync(P->rn.len, len_src, P->rn_len_bytes);
    P->rn_sorted_valid = false;   // the sorted copies are rebuilt from the imported rings
  }
  return 0;
}

