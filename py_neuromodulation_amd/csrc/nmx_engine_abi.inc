// nmx_engine_abi.inc -- C ABI, part 1: plan create / destroy, state reset / export / import.  Included by nmx_engine.inc.

// =========================================================================================
namespace {

// The sections of the state blob, in the blob's order.  bytes: the section's size in this plan (0: the plan has none);
// export_to / import_from get the section's start in the blob, import_from also its size there.  bytes_in (optional): the
// size of the section in a blob another plan wrote, where that may differ (the raw normaliser of a ragged stream).
struct StateSection {
  size_t (*bytes)(const Plan&);
  void (*reset)(Plan&);
  void (*export_to)(const Plan&, char*);
  int (*import_from)(Plan&, const char*, size_t);
  int (*bytes_in)(const Plan&, const char*, size_t left, size_t* n);
};
const StateSection kStateSections[] = {
    {burst_state_bytes, burst_state_reset, burst_state_export, burst_state_import, nullptr},
    {kalman_state_bytes, kalman_state_reset, kalman_state_export, kalman_state_import, nullptr},
    {dc_state_bytes, dc_state_reset, dc_state_export, dc_state_import, nullptr},
    {rawnorm_state_bytes, rawnorm_state_reset, rawnorm_state_export, rawnorm_state_import, rawnorm_state_bytes_in},
};
size_t state_bytes(const Plan& P) {
  size_t n = 0;
  for (const StateSection& S : kStateSections) n += S.bytes(P);
  return n;
}

}  // namespace

extern "C" {

int nmx_abi_version(void) { return NMX_ABI_VERSION; }
int nmx_device_count(void) { return be_device_count(); }
const char* nmx_last_error(void) { return g_nmx_err.c_str(); }

int nmx_plan_destroy(nmx_plan* plan) {
  Plan* P = (Plan*)plan;
  if (!P) return 0;
  be_set_device(P->device);
  P->sched.quiesce();
  for (auto& t : P->timers) be_timer_destroy(t);
  P->sched.each_event([](be_event_t& e) { be_event_destroy(e); });
  P->sched.each_stream([](be_stream_t& s, bool) { be_stream_destroy(s); });
  delete P;   // every device block and the page-locked one: P.tables, the Bufs
  be_dev_pool_age();
  return 0;
}

namespace {
struct PlanGuard {   // a plan that fails to build is destroyed on the way out; the failure's message stays
  Plan* P;
  ~PlanGuard() {
    if (!P) return;
    const std::string keep = g_nmx_err;
    nmx_plan_destroy((nmx_plan*)P);
    g_nmx_err = keep;
  }
};
}  // namespace

int nmx_plan_create(const nmx_plan_desc* desc, nmx_plan** out) {
  if (!desc || !out) return nmx_fail(NMX_E_INVALID, "null argument");
  *out = nullptr;
  NMX_REQUIRE(desc->abi_version == NMX_ABI_VERSION, "nmx_plan_desc.abi_version mismatch");
  NMX_REQUIRE(desc->n_channels >= 1, "n_channels must be >= 1");
  // 16 384 samples for a plan in general; up to 40 000 (the partitioned FIR stage's bound) for a plan whose window-sized
  // stages are all sized for it: the FIR stages (notch, preprocessing_filter, the sharp-wave pre-filters), re-referencing,
  // the sharp-wave analysis (long-window mode of build_sharp), the long-window time / oscillatory kernel (build_timeosc:
  // Hjorth, raw, line length, FFT, Welch, and STFT behind its opt-in), the bursts chain (partitioned bank, long Hilbert kernel,
  // staged walk, scan statistics: build_hilbert, build_bursts) and coherence (nmx_coh_item reads its samples from the window view
  // and keeps one segment of at most 4096 samples on chip)
  // (a plan of nolds alone takes any window from one sample on: the reference's Nolds does -- NaN below four samples)
  NMX_REQUIRE((desc->window >= 4 || (desc->features == NMX_F_NOLDS && desc->window >= 1)) && desc->window <= 40000,
              "window must be in [4, 40 000 samples]");
  // Bursts above 16 384 samples are OPT-IN (NMX_LONG_BURSTS=1).  The chain is sized for them like the stages above, but the
  // refusal of such a plan is behaviour the suite pins (tests/timeosc_long_cases.py: a 20 000-sample plan with fft and bursts
  // raises): a plan that was refused stays refused until the caller asks.  Making it the default is this one test and the
  // default of this variable.
  // Band-pass power above 16 384 samples is OPT-IN the same way (NMX_LONG_BANDPOWER=1): the partitioned bank then takes the
  // derivative series of mobility and complexity from differenced taps (build_bank, nmx_k_bank.h: NmxBankArgs::ups_diff_mask).
  // STFT and coherence above 16 384 samples are OPT-IN the same way (NMX_LONG_STFT=1, NMX_LONG_COHERENCE=1): the STFT phase of
  // the long-window time / oscillatory kernel (nmx_k_timeosc_long.h), and the coherence stage on the long plan's window view.
  struct LongOptIn { const char* name; const char* var; uint32_t feature; bool on; bool always_hinted; };
  const LongOptIn opt_ins[] = {   // (in the order the "runs up to 40 000" list and the hint name them)
      {"bursts", "NMX_LONG_BURSTS", NMX_F_BURSTS, env_int("NMX_LONG_BURSTS", 0) != 0, true},
      {"bandpass_filter", "NMX_LONG_BANDPOWER", NMX_F_BANDPOWER, env_int("NMX_LONG_BANDPOWER", 0) != 0, true},
      {"stft", "NMX_LONG_STFT", NMX_F_STFT, env_int("NMX_LONG_STFT", 0) != 0, false},
      {"coherence", "NMX_LONG_COHERENCE", NMX_F_COHERENCE, env_int("NMX_LONG_COHERENCE", 0) != 0, false},
  };
  uint32_t long_ok = NMX_F_SHARPWAVE | NMX_F_HJORTH | NMX_F_RAW | NMX_F_LINELENGTH | NMX_F_FFT | NMX_F_WELCH | NMX_F_NOLDS;
  for (const LongOptIn& o : opt_ins) if (o.on) long_ok |= o.feature;
  const bool long_fits = desc->window <= 16384 || (!(desc->features & ~long_ok) && desc->raw_norm_method <= 0 && desc->raw_window <= 0);
  if (!long_fits) {
    // one message, its three parts built from the opt-ins: what stays limited in front of the ';', what runs up to 40 000
    // samples behind it, then the variable of every opt-in that is not set.  (The hint names NMX_LONG_STFT / NMX_LONG_COHERENCE
    // only to a plan that asks for that feature: the text a plan without them gets is the one it always got.)
    auto join = [](const std::vector<std::string>& v, const char* last) {
      std::string t;
      for (size_t i = 0; i < v.size(); ++i) t += (i == 0 ? "" : i + 1 == v.size() ? last : ", ") + v[i];
      return t;
    };
    std::vector<std::string> limited, runs = {"raw_hjorth", "return_raw", "linelength", "fft", "welch", "sharpwave_analysis"};
    for (const char* name : {"stft", "bandpass_filter", "bursts", "coherence"})   // (the order the limited list always had)
      for (const LongOptIn& o : opt_ins) if (!o.on && std::string(name) == o.name) limited.push_back(name);
    limited.push_back("raw_normalization or raw_resampling");
    std::string hint;
    for (const LongOptIn& o : opt_ins) {
      if (o.on) { runs.push_back(o.name); continue; }
      if (!o.always_hinted && !(desc->features & o.feature)) continue;
      hint += hint.empty() ? std::string(" (") + o.name + " too with " + o.var + "=1 in the environment"
                           : std::string(", ") + o.name + " with " + o.var + "=1";
    }
    if (!hint.empty()) hint += ")";
    return nmx_fail(NMX_E_INVALID, "window must be in [4, 16 384] samples for a plan with " + join(limited, ", ") + "; only " +
                                       join(runs, " and ") + " run up to 40 000 samples, behind re-referencing and FIR pre-processing" + hint);
  }
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
  PlanGuard guard{P};
  P->d = *desc;
  P->device = desc->device;
  for (auto& t : P->timers) t = be_timer_t{};
  int rc = be_set_device(P->device);
  if (rc) return rc;
  P->n_cu = be_cu_count(P->device);
  P->w_in = P->d.raw_window > 0 ? P->d.raw_window : P->d.window;   // samples per incoming window
  P->sched.each_stream([](be_stream_t& s, bool high) { s = high ? be_stream_create_high() : be_stream_create(); });
  P->sched.each_event([](be_event_t& e) { be_event_create(e); });
  P->host_chunk_windows = std::max(1, env_int("NMX_HOST_CHUNK_WINDOWS", 512));
  P->host_first_chunk = std::max(1, env_int("NMX_HOST_FIRST_CHUNK", 128));
  P->sched.mode = overlap_mode(env_int("NMX_OVERLAP", 4));
  for (auto& t : P->timers) be_timer_create(t);
  P->taps.resize(desc->n_filters);
  for (int i = 0; i < desc->n_filters; ++i) {
    NMX_REQUIRE(desc->filters[i].taps && desc->filters[i].n_taps >= 1, "filter without taps");
    P->taps[i].assign(desc->filters[i].taps, desc->filters[i].taps + desc->filters[i].n_taps);
    P->d.filters[i].taps = P->taps[i].data();
  }
  NMX_REQUIRE(desc->n_pre_filters >= 0 && desc->n_pre_filters <= NMX_MAX_PRE_FILTERS, "n_pre_filters out of range");
  P->pre_taps.resize(desc->n_pre_filters);
  for (int i = 0; i < desc->n_pre_filters; ++i) {
    NMX_REQUIRE(desc->pre_taps[i] && desc->n_pre_taps[i] >= 1, "pre-filter without taps");
    P->pre_taps[i].assign(desc->pre_taps[i], desc->pre_taps[i] + desc->n_pre_taps[i]);
    P->d.pre_taps[i] = P->pre_taps[i].data();
  }
  if (desc->notch_taps) {
    P->notch_taps.assign(desc->notch_taps, desc->notch_taps + desc->n_notch_taps);
    P->d.notch_taps = P->notch_taps.data();
  }
  if (desc->ref_matrix) {
    NMX_REQUIRE(desc->n_channels_in >= 1, "n_channels_in");
    const size_t n = (size_t)desc->n_channels * desc->n_channels_in;
    P->ref_matrix.assign(desc->ref_matrix, desc->ref_matrix + n);
    P->d.ref_matrix = P->ref_matrix.data();
  } else {
    P->d.n_channels_in = desc->n_channels;
  }
  P->nt_bank = 256;
  P->tiny_inline = env_int("NMX_TINY_INLINE", 1) != 0;
  P->chunk_windows = env_int("NMX_CHUNK_WINDOWS", 1024);
  P->burst_handoff_mb = std::max(1, env_int("NMX_BURST_HANDOFF_MB", P->burst_handoff_mb));
  P->norm_chunk_windows = std::max(1, env_int("NMX_NORM_CHUNK_WINDOWS", P->norm_chunk_windows));
  if ((rc = build_front(*P)) || (rc = build_timeosc(*P)) || (rc = build_coh(*P)) || (rc = build_nolds(*P)) || (rc = build_bank(*P)) ||
      (rc = build_notch(*P)) || (rc = build_bursts(*P)) || (rc = build_sharp(*P)) || (rc = build_kalman(*P)) ||
      (rc = build_resample(*P)) || (rc = build_prefilters(*P)) || (rc = build_rawnorm(*P)) || (rc = dc_build(*P)))
    return rc;
#ifndef NMX_HOST_EMU
  choose_notch_bank_fuse(*P);   // (behind every stage's own choice: it reads the notch's, the bank's and what sits between them)
#endif
  P->sched.bursts = P->have_bursts;
  P->sched.sharp = P->have_sharp;
  P->bank.takes_dc = fir_stage_takes_dc(P->bank);   // (behind the fuse choice: a launch inside the notch kernel takes it)
  NMX_REQUIRE(!(P->d.features & NMX_F_BANDPOWER) || P->have_bank, "bandpass_filter enabled without filters");
  *out = (nmx_plan*)P;
  guard.P = nullptr;
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
  if (P->dc_learned) dc_state_reset(*P);   // (the caller's split replaces the learned one)
  P->dc_dirty = true;
  return 0;
}

int nmx_plan_get_offsets(nmx_plan* plan, double* d_in, double* d_pre, int* state) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  if (P->dc_ok && P->dc_dirty) {
    be_set_device(P->device);
    dc_recompute(*P, P->sched.main);
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

// ---- the state blob: the sections of kStateSections one behind the other
//      burst ring | counts | Kalman | offsets | raw normaliser
int nmx_state_reset(nmx_plan* plan) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  be_set_device(P->device);
  P->sched.quiesce();
  for (const StateSection& S : kStateSections) S.reset(*P);
  return 0;
}

int nmx_state_size(const nmx_plan* plan, int64_t* n_bytes) {
  const Plan* P = (const Plan*)plan;
  if (!P || !n_bytes) return nmx_fail(NMX_E_INVALID, "null argument");
  *n_bytes = (int64_t)state_bytes(*P);
  return 0;
}

int nmx_state_export(nmx_plan* plan, void* dst, int64_t n_bytes) {
  Plan* P = (Plan*)plan;
  if (!P || (!dst && n_bytes)) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE((size_t)n_bytes == state_bytes(*P), "state size mismatch");
  if (!n_bytes) return 0;
  be_set_device(P->device);
  P->sched.quiesce();
  size_t at = 0;
  for (const StateSection& S : kStateSections) {
    S.export_to(*P, (char*)dst + at);
    at += S.bytes(*P);
  }
  return 0;
}

int nmx_state_import(nmx_plan* plan, const void* src, int64_t n_bytes) {
  Plan* P = (Plan*)plan;
  if (!P || (!src && n_bytes)) return nmx_fail(NMX_E_INVALID, "null argument");
  // sizes first: nothing is touched unless the whole blob fits
  constexpr int n_sections = (int)(sizeof kStateSections / sizeof *kStateSections);
  size_t size[n_sections], total = 0;
  int rc;
  for (int i = 0; i < n_sections; ++i) {
    const StateSection& S = kStateSections[i];
    size[i] = S.bytes(*P);
    if (S.bytes_in && (rc = S.bytes_in(*P, (const char*)src + total, (size_t)n_bytes >= total ? (size_t)n_bytes - total : 0, &size[i])))
      return rc;
    total += size[i];
  }
  NMX_REQUIRE((size_t)n_bytes == total, "state size mismatch");
  if (!n_bytes) return 0;
  be_set_device(P->device);
  P->sched.quiesce();
  size_t at = 0;
  for (int i = 0; i < n_sections; ++i) {
    if ((rc = kStateSections[i].import_from(*P, (const char*)src + at, size[i]))) return rc;
    at += size[i];
  }
  return 0;
}

