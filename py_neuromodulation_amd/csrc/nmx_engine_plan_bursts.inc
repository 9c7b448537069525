// nmx_engine_plan_bursts.inc -- the bursts chain as a stage: its plan-time choices (build_hilbert, build_bursts) and its launch
// sequence for one chunk (launch_burst_stage).  Included by nmx_engine.inc.

// Long Hilbert kernel (nmx_k_hilbert_long.h): the smallest D <= 64 that divides W and leaves a complex transform of M = W / D
// <= 8192 points (two LDS buffers of 64 KiB) whose factors the FFT engine takes.  0: none (a prime above 8192, ...).
static int hilbert_split(int W) {
  for (int D = 2; D <= 64; ++D) {
    if (W % D) continue;
    int nc = W / D, twos = 0, stages = 0;
    if (nc > 8192) continue;
    if (nc < 2) break;
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

// the threshold history of a plan: ring length and top-K list entries (nmx_k_bursts.h), refused beyond NMX_THR_K_MAX
static int burst_history(const nmx_plan_desc& d, int* n_ring, int* K) {
  const double q = d.burst_threshold / 100.0;
  NMX_REQUIRE(q >= 0.0 && q <= 1.0, "burst threshold must be a percentile in [0, 100]");
  NMX_REQUIRE(d.sfreq * d.burst_time_duration_s < 2147483647.0, "burst ring buffer (sfreq x time_duration_s) too long");
  *n_ring = (int)(d.sfreq * d.burst_time_duration_s);
  NMX_REQUIRE(*n_ring >= 2, "burst ring buffer too short");
  *K = std::min((int)std::floor((1.0 - q) * (double)(*n_ring - 1)) + 2, *n_ring);
  if (*K > NMX_THR_K_MAX)
    return nmx_fail(NMX_E_INVALID, "burst threshold history too long: floor((1 - threshold / 100) x (int(sfreq x time_duration_s) - 1)) + 2 = " +
                    std::to_string(*K) + " top-K list entries, the limit is 1 048 576 (bursts_settings.threshold, "
                    "bursts_settings.time_duration_s and the sampling rate the bursts see)");
  return 0;
}

// ... for a series whose generic layout (3 W + 4 floats) does not fit LDS
static int build_hilbert_long(Plan& P) {
  const nmx_plan_desc& d = P.d;
  NmxHilbertArgs& H = P.bursts.hil;
  int rc, n_ring, K;
  // (a history beyond the limit is refused before the slabs are allocated, as build_bursts refuses it before the state)
  if ((d.features & NMX_F_BURSTS) && (rc = burst_history(d, &n_ring, &K))) return rc;
  const int W = d.window, D = hilbert_split(W);
  NMX_REQUIRE(D > 0, "bursts: no supported split of a " + spaced(W) + "-point Hilbert transform (a window above 13 650 samples "
              "needs a divisor D <= 64 with window / D <= 8192 and prime factors <= 4096)");
  H.long_mode = 1;
  H.split_d = D;
  H.sub_m = W / D;
  if ((rc = build_fft(P, H.sub_m, &H.hil_c))) return rc;
  auto it = P.twn_cache.find(W);
  if (it == P.twn_cache.end()) {
    std::vector<float> t(2 * (size_t)W);
    for (int k = 0; k < W; ++k) {
      const double a = -2.0 * kPi * (double)k / (double)W;
      t[2 * k] = (float)std::cos(a);
      t[2 * k + 1] = (float)std::sin(a);
    }
    const float2* p = (const float2*)upload(P, t.data(), t.size() * sizeof(float));
    if (!p) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
    it = P.twn_cache.emplace(W, p).first;
  }
  H.tw_n = it->second;
  H.off_a = 0;
  H.off_b = al4(2 * H.sub_m);
  H.off_y = 0;
  H.lds_floats = H.off_b + al4(2 * H.sub_m) + 64;
  NMX_REQUIRE((size_t)H.lds_floats * 4 <= 160 * 1024, "internal: long Hilbert kernel: LDS budget");
  // one workgroup per CU (two where the buffers leave room); the slabs -- the one-sided spectrum, (W + 1) / 2 complex each --
  // within 64 MiB of device memory
  H.slab_floats = al4(2 * ((W + 1) / 2));
  H.slab_blocks = 1;
#ifndef NMX_HOST_EMU
  H.slab_blocks = slab_workgroups(P, (size_t)H.lds_floats * 4, (size_t)H.slab_floats);
#endif
  H.slab = (float*)plan_alloc(P, (size_t)H.slab_blocks * H.slab_floats * sizeof(float));
  if (!H.slab) return nmx_fail(NMX_E_NOMEM, "Hilbert slab allocation failed");
  H.w500_tab = nullptr;
  H.w1000_tab = nullptr;
  P.bursts.hil_kind = NMX_HIL_LONG;
  return 0;
}

// the stand-alone Hilbert kernel of a bank that leaves its burst bands as series (build_bank calls this)
int build_hilbert(Plan& P) {
  const nmx_plan_desc& d = P.d;
  NmxHilbertArgs& H = P.bursts.hil;
  H.W = d.window;
  H.hil_full = d.window & 1;
  // (the layouts below: 2 x al4(2 W) floats for an odd window, 2 x al4(W + 2) + al4(W) for an even one)
  if ((size_t)(H.hil_full ? 2 * al4(2 * d.window) : 2 * al4(d.window + 2) + al4(d.window)) * 4 > 160 * 1024)
    return build_hilbert_long(P);
  int rc;
  if ((rc = build_fft(P, H.hil_full ? d.window : d.window / 2, &H.hil_r, true))) return rc;
  if ((rc = build_fft(P, d.window, &H.hil_c, true))) return rc;
  H.off_a = 0;
  if (H.hil_full) {
    H.off_b = al4(2 * d.window);
    H.off_y = H.off_b;
    H.lds_floats = H.off_b + al4(2 * d.window);
  } else {   // even W: two half-length complex buffers (W / 2 + 1 bins) + a copy of the series
    H.off_b = al4(d.window + 2);
    H.off_y = H.off_b + al4(d.window + 2);
    H.lds_floats = H.off_y + al4(d.window);
  }
  NMX_REQUIRE(H.lds_floats * 4 <= 160 * 1024, "window too long for the Hilbert kernel");
  H.w500_tab = nullptr;
  H.w1000_tab = nullptr;
  if (d.window == 1000) {
    if ((rc = build_w500_tab(P))) return rc;
    H.w500_tab = P.w500_tab;
  }
#ifndef NMX_HOST_EMU
  if (d.window == 2000) {   // tables of the 1000-point wave-level transform (layout: nmx_k_fft500.h)
    std::vector<float> t(NMX_W1000_TAB_FLOATS);
    auto put = [&](int i, double ang, double scale) {
      t[2 * i] = (float)(scale * std::cos(ang));
      t[2 * i + 1] = (float)(scale * std::sin(ang));
    };
    for (int lane = 0; lane < 64; ++lane) {
      const int l = lane < 50 ? lane : 0, k = l % 10;
      for (int r = 1; r < 10; ++r) {
        put((r - 1) * 64 + lane, -2.0 * kPi * ((10 * k * r) % 1000) / 1000.0, 1.0);
        put((8 + r) * 64 + lane, -2.0 * kPi * ((l * r) % 1000) / 1000.0, 1.0);
        put((17 + r) * 64 + lane, -2.0 * kPi * (((l + 50) * r) % 1000) / 1000.0, 1.0);
      }
    }
    for (int k = 0; k < NMX_W1000_CS_N; ++k) put(NMX_W1000_TW_N + k, 2.0 * kPi * k / 2000.0, k ? 2.0 / 2000.0 : 0.0);
    H.w1000_tab = (const float*)upload(P, t.data(), t.size() * sizeof(float));
    if (!H.w1000_tab) return nmx_fail(NMX_E_NOMEM, "table allocation failed");
  }
#endif
  // the kernel (be_launch_hilbert): one wave per series at W = 1000 / 2000, else the 128-thread workgroup kernel
  const bool wave = env_int("NMX_HILBERT_W500", 1) != 0;
  P.bursts.hil_kind = wave && d.window == 1000 ? NMX_HIL_W500 : wave && H.w1000_tab ? NMX_HIL_W1000 : NMX_HIL_FIXED128;
  return 0;
}

// no bound for any sequence: plan creation, state reset, state import (the caller has drained the plan's streams)
void burst_floor_reset(Plan& P) {
  const std::vector<float> f((size_t)P.d.n_channels * P.d.n_burst_bands, -INFINITY);
  be_h2d_sync(P.bursts.d_floor, f.data(), f.size() * sizeof(float));
}

// ---- the bursts' section of the state blob: ring (the sorted top-K lists) | counts
static size_t burst_state_bytes(const Plan& P) { return P.bursts.top_bytes + P.bursts.counts_bytes; }
static void burst_state_reset(Plan& P) {
  if (!P.have_bursts) return;
  BurstStage& B = P.bursts;
  be_memset_sync(B.d_top, 0, B.top_bytes);
  be_memset_sync(B.d_counts, 0, B.counts_bytes);
  burst_floor_reset(P);
  B.seen = 0;
}
static void burst_state_export(const Plan& P, char* q) {
  if (!P.have_bursts) return;
  be_d2h_sync(q, P.bursts.d_top, P.bursts.top_bytes);
  be_d2h_sync(q + P.bursts.top_bytes, P.bursts.d_counts, P.bursts.counts_bytes);
}
static int burst_state_import(Plan& P, const char* q, size_t) {
  if (!P.have_bursts) return 0;
  BurstStage& B = P.bursts;
  be_h2d_sync(B.d_top, q, B.top_bytes);
  be_h2d_sync(B.d_counts, q + B.top_bytes, B.counts_bytes);
  memcpy(&B.seen, q + B.top_bytes + sizeof(long long), sizeof(long long));   // counts[0][1]
  burst_floor_reset(P);   // (a bound of the history this plan had, not of the imported one: the next steady walk writes it anew)
  return 0;
}

int build_bursts(Plan& P) {
  const nmx_plan_desc& d = P.d;
  if (!(d.features & NMX_F_BURSTS)) return 0;
  NMX_REQUIRE(d.n_burst_bands > 0, "bursts enabled without burst bands");
  int nb = 0;
  for (int i = 0; i < d.n_filters; ++i) nb += d.filters[i].burst_index >= 0;
  NMX_REQUIRE(nb == d.n_burst_bands, "every burst band needs exactly one filter");
  BurstStage& B = P.bursts;
  NmxBurstThrArgs& T = B.bthr;
  T.n_channels = d.n_channels;
  T.n_bands = d.n_burst_bands;
  T.W = d.window;
  T.q = d.burst_threshold / 100.0;
  // (before anything of the chain is allocated: the state alone is n_channels x n_burst_bands x K floats)
  int rc_hist;
  if ((rc_hist = burst_history(d, &T.n_ring, &T.K))) return rc_hist;
  const double seg_s = d.segment_length_s > 0 ? d.segment_length_s : (double)d.window / d.sfreq;  // segment_length_features_ms / 1000
  T.overlap = (int)(d.sfreq * seg_s / d.feat_hz);
  // samples_overlap = 0 (30 kHz, 17 ms windows at a 1 kHz feature rate: int(0.51)): the reference's slice
  // filtered_data[:, :, -0:] is the WHOLE window -- every hop appends all W envelope samples (features/bursts.py:155-166)
  // samples_overlap > W (a 16 kHz recording resampled to 1000-sample windows with the raw-rate design): the slice
  // filtered_data[:, :, -1600:] of a 1000-sample array is the whole window as well
  if (T.overlap == 0 || T.overlap > d.window) T.overlap = d.window;
  NMX_REQUIRE(T.overlap >= 1 && T.overlap <= d.window, "burst overlap (sfreq * seg_s / feat_hz) out of range");
  int p2 = 1;
  while (p2 < std::max(std::max(d.window, T.overlap) + 4, 1024)) p2 <<= 1;   // >= NMX_THR_P (flush staging)
  // (the three arrays are only indexed, never sorted as a network: a plan of the tiled kernel takes them as long as they have to be --
  // 1 s windows up to 12.9 kHz instead of 8.1 kHz, where the default 30 s history at the 75th percentile keeps 90 001 entries)
  if (nmx_burst_thr_tiled(T.K)) p2 = std::max(al4(std::max(d.window, T.overlap) + 4), 1024);
  T.P2 = p2;
  // NMX_THR_LIST_GLOBAL=1: the sorted top-K list is not copied to LDS (workgroups of ~20 KB instead of
  // ~50 KB leave room for the kernels that run next to the walk); every list access then goes to L2
  // It is also the fallback when the list does not fit (2 kHz x 30 s at the 50th percentile: 30 001 entries).
  T.stage_tile = 0;
  auto walk_layout = [&]() {
    T.list_in_global = env_int("NMX_THR_LIST_GLOBAL", 0);
    for (int pass = 0; pass < 2; ++pass) {
      T.off_l0 = 0;
      T.off_l1 = 0;                          // (single list: the merge is in place)
      T.off_p = T.list_in_global ? 0 : al4(T.K);   // pc[P2], ps[P2], ins[P2]
      T.off_red = T.off_p + 3 * T.P2 + 2 * 512 + 1024 + 8;   // + fringe x2, pending list, counters
      T.lds_floats = T.off_red + 64;
      if ((size_t)T.lds_floats * 4 <= 160 * 1024 || T.list_in_global) break;
      T.list_in_global = 1;
    }
  };
  walk_layout();
  // Staging arrays for a whole hop that do not fit even with the list in global memory (windows above 8 188 samples, 12 900 with
  // the tiled merge): arrays of NMX_THR_STAGE_TILE samples, and a longer hop is absorbed tile by tile (nmx_burst_thr_walk)
  if ((size_t)T.lds_floats * 4 > 160 * 1024) {
    T.P2 = T.stage_tile = NMX_THR_STAGE_TILE;
    walk_layout();
  }
  // the workgroup walk's kernel (be_launch_burst_thr): a thread's share of the list in registers -- 128 entries x 256 threads, 64 x
  // 1024 in nmx_kern_burst_thr_wide --, beyond 65 536 entries the tiled merge of nmx_kern_burst_thr_tiled
  if (nmx_burst_thr_tiled(T.K)) B.nt_thr = NMX_THR_TILE_NT;
  else if ((T.K + B.nt_thr - 1) / B.nt_thr > 128) B.nt_thr = 1024;
  NMX_REQUIRE(T.lds_floats * 4 <= 160 * 1024,
              "burst threshold state does not fit in 160 KiB LDS (ring x (1 - q) too large)");
  NmxBurstStatArgs& S = B.bstat;
  S.n_outputs = d.n_outputs + d.n_extra_cols;   // (the row stride)
  S.n_channels = d.n_channels;
  S.n_bands = d.n_burst_bands;
  S.W = d.window;
  S.sfreq = (float)d.sfreq;
  S.seg_s = (float)seg_s;
  S.out_mask = d.burst_out_mask;
  S.cols = cv(d.burst_cols);
  S.off_e = 0;
  // the series in LDS, padded (NMX_EP) -- beyond 16 384 samples one tile of it: more than 69 KB of LDS per wave leaves a CU two
  // waves, and from ~38 500 samples on the series does not fit at all
  S.scan_tile = d.window > 16384 ? NMX_BSTAT_TILE : 0;
  const int n_lds = S.scan_tile ? S.scan_tile : d.window;
  S.off_red = al4(n_lds + n_lds / 16 + 1);
  S.lds_floats = S.off_red + 64;
  const size_t n_state = (size_t)d.n_channels * d.n_burst_bands;
  B.top_bytes = n_state * T.K * sizeof(float);
  B.counts_bytes = n_state * 2 * sizeof(long long);
  B.d_top = (float*)plan_alloc(P, B.top_bytes);
  B.d_counts = (long long*)plan_alloc(P, B.counts_bytes);
  B.d_floor = (float*)plan_alloc(P, n_state * sizeof(float));
  if (!B.d_top || !B.d_counts || !B.d_floor) return nmx_fail(NMX_E_NOMEM, "burst state allocation failed");
  // ---- the chain's kernels and the walk's schedule (launch_burst_stage only dispatches on them) ----
  B.own_hilbert = P.bank.w64 || P.bank.a.partitioned;   // (build_bank, which ran before, has called build_hilbert for it)
  B.fill_split = env_int("NMX_FILL_SPLIT", 1) != 0;
  bool wave = env_int("NMX_THR_WAVE", 1) != 0;
#ifdef NMX_HOST_EMU   // (the emulator runs the item code of the workgroup walk and the generic Hilbert item, which stores every row)
  wave = false;
#else
  const int sparse = env_int("NMX_BURST_ENV_SPARSE", 1);
  B.sparse = sparse != 0 && B.own_hilbert && (B.hil_kind == NMX_HIL_W500 || B.hil_kind == NMX_HIL_W1000);
  B.sparse_count = sparse == 2;
#endif
  B.walk = nmx_burst_walk_plan(T, env_int("NMX_THR_FILL", 1) != 0, wave, env_int("NMX_THR_LIST_LDS", 1) != 0);
  B.stat_kind = S.scan_tile ? NMX_BSTAT_SCAN : (d.window & 3) || d.window > 2048 ? NMX_BSTAT_GENERIC
                : d.window <= 1024 ? (B.sparse ? NMX_BSTAT_REG16_SPARSE : NMX_BSTAT_REG16)
                                   : (B.sparse ? NMX_BSTAT_REG32_SPARSE : NMX_BSTAT_REG32);
  P.have_bursts = true;
  burst_state_reset(P);
  return 0;
}

// The bursts chain of one chunk (nw hops) of batch `b` behind the bank on its main stream: Hilbert envelope, threshold walk,
// run statistics.  Its sequential, latency-bound part (walk -> run statistics: a few waves) runs on the high-priority side
// stream next to the throughput kernels that follow on the main stream -- from the walk on, or from the Hilbert kernel on,
// or not at all: the batch's schedule says (nmx_engine_sched.inc).
static int launch_burst_stage(Plan& P, const BatchSched& b, int nw, float* d_out, bool tev) {
  BurstStage& B = P.bursts;
  const int par = P.sched.parity();
  const int n_seq = P.d.n_channels * P.d.n_burst_bands, W = P.d.window;
  Buf& B_env = B.env[par];
  Buf& B_thr = B.thr[par];
  int rc;
  if ((rc = ensure(B_thr, (size_t)nw * n_seq * sizeof(float)))) return rc;
  be_stream_t sb = b.s;
  if (P.sched.hilbert_on_side(b)) sb = P.sched.fork_bursts(b);
  if (tev) be_timer_start(P.timers[ST_BURSTS], sb);
  const unsigned char* env_full = nullptr;
  if (B.own_hilbert) {
    NmxHilbertArgs H = B.hil;
    H.y = (const float*)B.yb.p; H.env = (float*)B_env.p;
    // Rows that cannot reach their threshold leave only the tail the walk reads (B.sparse).
    // No event orders this launch behind the previous chunk's walk, which may still run on the side stream: the kernel
    // reads whatever floor is there.  That is safe because EVERY value ever stored there -- -INFINITY, or the s[lo] some
    // finished walk of this state left -- is a lower bound of all thresholds of the hops behind that walk, this chunk's
    // included (NmxBurstThrArgs::floor); a 4-byte store is seen whole or not at all.  State reset / import drain the
    // streams before they put -INFINITY back.
    if (B.sparse) {
      if ((rc = ensure(B.env_full[par], (size_t)nw * n_seq))) return rc;
      H.floor = B.d_floor; H.full = (unsigned char*)B.env_full[par].p;
      H.n_seq = n_seq; H.overlap = B.bthr.overlap;
      env_full = H.full;
    }
    be_launch_hilbert(H, B.hil_kind, (long long)nw * n_seq, (size_t)H.lds_floats * 4, sb);
    if (env_full && B.sparse_count) {   // NMX_BURST_ENV_SPARSE=2 (tests, measurements): read the flags back, at the price of a sync
      std::vector<unsigned char> f((size_t)nw * n_seq);
      if ((rc = be_sync(sb))) return rc;
      be_d2h_sync(f.data(), env_full, f.size());
      for (unsigned char v : f) B.env_tail_rows += v == 0;
      B.env_rows += (long long)f.size();
    }
  }
  if (P.sched.walk_on_side(b)) sb = P.sched.fork_bursts(b);
  NmxBurstThrArgs T = B.bthr;
  T.top = B.d_top; T.counts = B.d_counts; T.floor = B.d_floor;
  NmxBurstWalkSeg seg[3];
  const int n_seg = nmx_burst_walk_schedule(B.walk, T, B.seen, nw, seg);
  for (int i = 0; i < n_seg; ++i) {
    const NmxBurstWalkSeg& g = seg[i];
    T.env = (const float*)B_env.p + (size_t)g.first * n_seq * W;
    T.thr = (float*)B_thr.p + (size_t)g.first * n_seq;
    T.n_windows = g.n;
    if (g.kind == NMX_WALK_FILL) {   // scratch: the 16-bit slot of every sample, per sequence, and (two-launch form) the sorted samples
      const size_t n_slot = (size_t)n_seq * NMX_FILL_MAX;
      if ((rc = ensure(B.slots, n_slot * (sizeof(unsigned short) + sizeof(float))))) return rc;
      float* sorted = (float*)B.slots.p;   // (the floats first: 4-byte aligned whatever n_slot)
      be_launch_burst_fill(T, n_seq, (unsigned short*)(sorted + n_slot), sorted, B.fill_split, sb);
    } else {
      be_launch_burst_thr(T, B.walk, g, n_seq, B.nt_thr, (size_t)T.lds_floats * 4, sb);
    }
  }
  B.seen += nw;
  NmxBurstStatArgs S = B.bstat;
  S.env = (const float*)B_env.p; S.thr = (const float*)B_thr.p; S.out = d_out; S.n_windows = nw;
  S.full = env_full;
  be_launch_burst_stat(S, B.stat_kind, nw * n_seq, (size_t)S.lds_floats * 4, sb);
  if (tev) be_timer_stop(P.timers[ST_BURSTS], sb);
  P.sched.join_bursts(b, sb);
  return 0;
}
