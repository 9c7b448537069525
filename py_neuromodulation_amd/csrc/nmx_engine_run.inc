// nmx_engine_run.inc -- C ABI, part 2: the launch sequence of one chunk (run_chunk), nmx_process_batch / _window,
// nmx_preprocess_window, nmx_filter_window, timers and kernel names.  Included by nmx_engine.inc.
// -----------------------------------------------------------------------------------------
// The pre-processing behind the front end, of a chunk (nw hops) or of one window (nw = 1, win_stride = 0):
// preprocessing_filter stages -> notch -> resampler (after the notch like the reference, data_preprocessor.py:9-15,68-71)
// -> raw normaliser (the last pre-processor; its input already nan_to_num'ed).  `v` follows the output of each stage that
// runs.  `fuse_bank` (run_chunk, a plan with notch_bank_fuse): the bank's arguments of this chunk -- its second launch runs
// inside the notch kernel (choose_notch_bank_fuse).
static int run_prep_stages(Plan& P, WinView& v, int nw, be_stream_t s, const NmxBankArgs* fuse_bank = nullptr) {
  const int C = P.d.n_channels, Wi = P.w_in;
  int rc;
  for (size_t i = 0; i < P.pre.size(); ++i) {   // preprocessing_filter: FIR stages one after the other
    Buf& dst = P.x_pf[i & 1];
    if ((rc = ensure(dst, (size_t)nw * C * Wi * sizeof(float)))) return rc;
    NmxBankArgs A = P.pre[i].a;
    view_into(A, v);
    A.out = nullptr; A.sw_out = (float*)dst.p;
    launch_fir_stage(P, P.pre[i], A, nw * C, s);
    v = dense_view(dst.p, C, Wi);
  }
  if (P.have_notch) {
    if ((rc = ensure(P.y_notch, (size_t)nw * C * Wi * sizeof(float)))) return rc;
    NmxBankArgs A = P.notch.a;
    view_into(A, v);
    A.out = nullptr; A.y_out = (float*)P.y_notch.p;
#ifndef NMX_HOST_EMU
    if (fuse_bank) launch_notch_bank_fused(P, A, *fuse_bank, nw * C, s);
    else
#endif
    launch_fir_stage(P, P.notch, A, nw * C, s);
    v = dense_view(P.y_notch.p, C, Wi);
  }
  if (P.have_resample && (rc = launch_resample(P, v, nw, s))) return rc;
  if (P.have_rawnorm && (rc = run_rawnorm(P, v, nw, s))) return rc;
  return 0;
}

// One chunk of batch `b`: the stage order of DESIGN section 3 (which stream, which event: nmx_engine_sched.inc).
// d_x / ldx address the recording with ABSOLUTE sample indices (the windows' starts); only the samples
// [lo, hi) that the windows of this chunk touch are read (d_x may point lo samples before a buffer that
// holds just that range).
// d_pre (may be null): where the pre-processed windows of this chunk go, [nw][C][W] on the device.
// samples_free (may be null): recorded once nothing more of this chunk reads the caller's samples -- if that point exists
// (*samples_freed says; a plan whose features read the samples themselves has none before the chunk is complete).
static int run_chunk(Plan& P, const BatchSched& b, const float* d_x, long long ldx, long long lo, long long hi,
                     const long long* d_starts, int nw, float* d_out, bool timed, float* d_pre = nullptr,
                     const int64_t* h_starts = nullptr, be_event_t* samples_free = nullptr, bool* samples_freed = nullptr) {
  const nmx_plan_desc& d = P.d;
  const int C = d.n_channels, W = d.window;
  const be_stream_t s = b.s;
  int rc;
  const int par = P.sched.parity();   // selects the hand-off tensors the side streams read (they exist twice)
  P.sched.begin_chunk(b);
  Buf& B_env = P.bursts.env[par];
  Buf& B_swy = P.sharp.swy[par];
  // ---- pre-processing -------------------------------------------------------------------
  WinView v{d_x, ldx, 0, d_starts, 1};   // what the next stage reads: the caller's samples, until a stage has written its own
  // stage timers: two event records per stage -- 14 per call, ~5 us of host time each -- are what the one-window call of a
  // real-time loop would spend a fifth of its 0.45 ms on: batches of fewer than 8 hops keep the whole-call timer only
  const bool tev = timed && nw >= 8;
  if (timed) be_stage_reset();
  if (tev) be_timer_start(P.timers[ST_PREP], s);
  be_stage(ST_PREP);
  if ((rc = launch_front(P, d_x, ldx, lo, hi - lo, true, s, v))) return rc;
  bool raw_live = v.x == d_x;   // `v` still addresses the caller's samples
  // Window starts in arithmetic progression (every stream with an integer hop; h_starts = the host's copy): the kernels
  // address window w as x + w * hop -- no per-item load of starts[w] (in the DMA-fed kernel of nmx_k_specmm.h the wait
  // for that vector load drained the copies in flight once per tile)
  if (h_starts) {
    long long hop = nw > 1 ? (long long)(h_starts[1] - h_starts[0]) : 0;
    for (int i = 2; i < nw && hop >= 0; ++i)
      if ((long long)(h_starts[i] - h_starts[i - 1]) != hop) hop = -1;
    if (hop >= 0) { v.x += h_starts[0]; v.win_stride = hop; v.starts = nullptr; }
  }
  // the bank's second launch inside the notch kernel (choose_notch_bank_fuse): its outputs exist before the notch runs
  // (begin_chunk has freed this parity's sharp-wave series)
  NmxBankArgs fuse_a{};
  if (P.notch_bank_fuse) {
    fuse_a = P.bank.a;
    fuse_a.out = d_out;
    fuse_a.dcf = dc_table(P);
    if (P.have_sharp) {
      if ((rc = ensure(B_swy, (size_t)nw * C * d.n_sw_filters * W * sizeof(float)))) return rc;
      fuse_a.sw_out = (float*)B_swy.p;
    }
  }
  if ((rc = run_prep_stages(P, v, nw, s, P.notch_bank_fuse ? &fuse_a : nullptr))) return rc;
  if (!P.pre.empty() || P.have_notch || P.have_resample || P.have_rawnorm) raw_live = false;
  if (d_pre) {   // user-registered host features read what the device features read
    NmxTapArgs T{};
    view_into(T, v);
    T.y = d_pre; T.C = C; T.W = W;
    be_launch_tap(T, nw * C, s);
  }
  if (tev) be_timer_stop(P.timers[ST_PREP], s);
  // (a host batch recycles its two input buffers: the copy of the chunk after next waits for THIS point of the stream, not
  // for the chunk's threshold walk and normaliser -- stage_host_chunk)
  const bool freed = !raw_live && samples_free;
  if (freed) be_event_record(*samples_free, s);
  if (samples_freed) *samples_freed = freed;
  // ---- the carried offset (nmx_engine_dc.inc): consumers take it on load; one that cannot reads a copy with it added back,
  // made at most once per chunk (dc_bind)
  bool dc_made = false;
  // ---- features --------------------------------------------------------------------------
  // Launch order: FIR bank (it feeds bursts and sharp waves) -> Hilbert -> threshold walk -> run statistics -> time /
  // oscillatory -> coherence -> sharp waves.  The walk and the statistics are sequential and latency bound (a few waves), the
  // sharp-wave analysis scalar list code: the schedule may run them beside the throughput kernels (NMX_OVERLAP).
  be_stage(ST_BANK);
  if (P.have_bank) {
    NmxBankArgs A = P.bank.a;
    A.out = d_out;
    if ((rc = dc_bind(P, A, P.bank.takes_dc, v, nw, s, dc_made))) return rc;
    if (P.have_bursts) {
      if ((rc = ensure(B_env, (size_t)nw * C * d.n_burst_bands * W * sizeof(float)))) return rc;
      A.env_out = (float*)B_env.p;
    }
    if (P.have_sharp) {
      if ((rc = ensure(B_swy, (size_t)nw * C * d.n_sw_filters * W * sizeof(float)))) return rc;
      A.sw_out = (float*)B_swy.p;
    }
    if (P.have_bursts && P.bursts.own_hilbert) {   // band series for the stand-alone Hilbert kernel
      if ((rc = ensure(P.bursts.yb, (size_t)nw * C * d.n_burst_bands * W * sizeof(float)))) return rc;
      A.yb_out = (float*)P.bursts.yb.p;
    }
    launch_fir_stage(P, P.bank, A, nw * C, s, tev);
    launch_kalman(P, nw, d_out, s);
  }
  const bool sharp_side = P.sched.sharp_on_side(b);
  if (sharp_side) {
    if ((rc = launch_sharp_stage(P, par, nw, d_out, P.sched.fork_sharp(b), tev))) return rc;
    P.sched.join_sharp();
  }
  be_stage(ST_BURSTS);
  if (P.have_bursts && (rc = launch_burst_stage(P, b, nw, d_out, tev))) return rc;
  if ((rc = launch_timeosc_stage(P, v, nw, d_out, s, tev, dc_made))) return rc;
  if ((rc = launch_nolds_stage(P, v, nw, d_out, s, tev, dc_made))) return rc;
  launch_coh_stage(P, v, nw, d_out, s, tev);
  if (!sharp_side && (rc = launch_sharp_stage(P, par, nw, d_out, s, tev))) return rc;
  P.sched.end_main(b);
  be_stage(ST_BATCH);
  if (timed) snapshot_kernels(P);
  return be_check_launch();
}

// What follows a chunk's kernels.  With a feature normaliser attached (sequential over hops: chunks in order) it runs on the
// finalize stream, behind the chunk's main stream and both side streams, and the schedule marks the rows complete there.
// Without one nothing is launched: "the rows are there" is the chunk's own events (Schedule::wait_done) -- a detour over a
// third stream costs two cross-stream hand-offs per call, as much as the whole batch of a light plan (BASELINE
// config[1]: 0.27 ms of kernel, 0.70 ms per call with the detour, 0.30 without).
// (a batch of a few hops on ONE stream normalises there too)
// An attached grid projection (nmx_engine_proj.inc) follows the normaliser on the same stream: it reads normalised rows.
// `ld`: the row stride (features + the plan's extra columns); `timed`: the batch's first chunk (projection timer / kernel name).
static int proj_launch(nmx_proj* proj, float* rows, long long ld, int n_rows, be_stream_t s);
static bool plan_finalizes(const Plan& P) { return P.norm || P.proj; }
static int chunk_finalize(Plan& P, const BatchSched& b, float* d_outk, int ld, int nw, bool timed) {
  int rc = 0;
  if (timed) P.kernels[ST_PROJ].clear();
  if (plan_finalizes(P)) {
    be_stream_t sf = P.sched.begin_finalize(b);
    if (P.norm) rc = nmx_norm_process(P.norm, d_outk, ld, nw, 1, (void*)sf);
    if (P.proj && !rc) {
      const bool tev = timed && nw >= 8;
      if (tev) be_timer_start(P.timers[ST_PROJ], sf);
      if (timed) { be_stage_reset(); be_stage(ST_PROJ); }
      rc = proj_launch(P.proj, d_outk, ld, nw, sf);
      if (tev) be_timer_stop(P.timers[ST_PROJ], sf);
      if (timed) { P.kernels[ST_PROJ] = be_stage_kernels(ST_PROJ); be_stage(ST_BATCH); }
    }
    P.sched.end_finalize(sf);
  }
  P.sched.next_chunk();
  return rc;
}

// ---- a batch, in parts ----------------------------------------------------------------------------------------------------
static int check_batch_args(Plan* P, const float* x, int64_t ldx, int64_t n_samples, const int64_t* starts, int64_t n_windows,
                            float* out, int memspace) {
  if (!P || !x || !starts || !out) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(n_windows >= 1, "n_windows must be >= 1");
  NMX_REQUIRE(memspace == 0 || memspace == 1, "memspace must be 0 (host) or 1 (device)");
  NMX_REQUIRE(ldx >= n_samples && n_samples >= P->w_in, "ldx / n_samples too small");
  bool mod4 = true;
  for (int64_t i = 0; i < n_windows; ++i) {
    NMX_REQUIRE(starts[i] >= 0 && starts[i] + P->w_in <= n_samples, "window outside the data");
    mod4 = mod4 && (starts[i] & 3) == 0;
  }
  P->starts_mod4 = mod4;
  return 0;
}

// Hops per chunk of one batch.
// Host buffers move chunk by chunk on a copy stream: while chunk k computes, the host thread is already
// copying the samples of chunk k + 1 (pageable memory: the copy blocks the host, not the GPU) and the
// features of chunk k - 1 travel back.  Device buffers: one chunk = NMX_CHUNK_WINDOWS hops.
struct ChunkSizes {
  bool host;
  int64_t dev_chunk, host_first, host_big;
  int64_t at(int64_t w0) const { return host ? (w0 == 0 ? host_first : host_big) : dev_chunk; }
};
static ChunkSizes batch_chunk_sizes(const Plan& P, bool host) {
  ChunkSizes z{host, 0, 0, 0};
  // (a plan without a hand-off tensor -- time / oscillatory features straight from the recording -- has nothing a chunk
  // would bound: device-resident batches go out as ONE launch of up to 16 chunks' worth of hops)
  const bool no_handoff = !P.have_bank && !(P.have_nolds && P.nolds.have_fir) && !P.have_notch && !P.front.d_R && !P.have_resample && !P.have_rawnorm && P.pre.empty();
  // (an attached normaliser needs a chunk's rows complete, and hop order: it runs on the finalize stream under the NEXT
  // chunk's kernels, so only the last chunk's pass is exposed -- against that, shorter chunks cost the main kernels 0.16 ms
  // per 1024 hops at 256.  Round 6, scans + cells at ~75 us per pass, headline step with / without the z-score:
  // 128 hops 7.30 / 6.60 ms, 256: 6.90 / 6.57, 384: 6.77 / 6.56, 512: 6.85 / 6.53, 1024: 7.02 / 6.60)
  z.dev_chunk = no_handoff ? (int64_t)P.chunk_windows * 16
                           : (P.norm ? std::min<int64_t>(P.chunk_windows, P.norm_chunk_windows) : (int64_t)P.chunk_windows);
  // host buffers: a SHORT first chunk (its copy is the only one nothing hides; the kernels start a quarter of a
  // millisecond after the call), then chunks as long as the device's own -- the sequential, latency-bound members of the
  // path (threshold walk, feature normaliser: ~1 ms per launch whatever the hop count) are paid per chunk, and a chunk's
  // copy runs under the chunk before it
  z.host_big = std::min<int64_t>(P.chunk_windows, P.host_chunk_windows);
  z.host_first = std::min<int64_t>(z.host_big, P.host_first_chunk);
  if (host && P.have_bursts)   // a fresh stream: the whole fill phase of the burst history in ONE sort (nmx_k_burst_fill.h)
    z.host_first = std::max<int64_t>(z.host_first, P.bursts.fill_hops((int)z.host_big));
  // Long windows: the bursts chain's hand-off buffers -- the band series and the envelope of both chunk parities, hops x
  // channels x bands x window floats each -- bound the chunk (256 channels x 3 bands x 40 000 samples are 123 MB per hop and
  // buffer): as many hops as fit NMX_BURST_HANDOFF_MB together, never fewer than one.  Plans up to 16 384 samples keep theirs.
  // (Band-pass power on long windows hands nothing off -- its series live and die in LDS -- and bounds no chunk.)
  if (P.have_bursts && P.d.window > 16384) {
    const double per_hop = 3.0 * P.d.n_channels * P.d.n_burst_bands * (double)P.d.window * sizeof(float);
    const int64_t cap = std::max<int64_t>(1, (int64_t)((double)P.burst_handoff_mb * 1048576.0 / per_hop));
    z.dev_chunk = std::min(z.dev_chunk, cap);
    z.host_big = std::min(z.host_big, cap);
    z.host_first = std::min(z.host_first, cap);
  }
  // ... and so do the band series of the nolds stage (one buffer, hops x channels x bands x window floats)
  if (P.have_nolds && P.nolds.have_fir && P.d.window > 16384) {
    const double per_hop = (double)P.d.n_channels * P.d.nolds_n_bands * (double)P.d.window * sizeof(float);
    const int64_t cap = std::max<int64_t>(1, (int64_t)((double)P.burst_handoff_mb * 1048576.0 / per_hop));
    z.dev_chunk = std::min(z.dev_chunk, cap);
    z.host_big = std::min(z.host_big, cap);
    z.host_first = std::min(z.host_first, cap);
  }
  return z;
}

// The samples [lo, hi) of every row of a host recording -> input buffer k & 1 of the plan, for chunk k of batch `b`;
// *d_xk / *ldxk address them with absolute sample indices.
static int stage_host_chunk(Plan& P, const BatchSched& b, int k, const float* x, int64_t ldx, long long lo, long long hi,
                            const float** d_xk, long long* ldxk) {
  const int Cin = P.d.n_channels_in;
  const be_stream_t sc = P.sched.in_stream(b);
  Buf& xb = P.x_in2[k & 1];
  const long long n_range = hi - lo;
  int rc;
  if ((rc = ensure(xb, (size_t)Cin * n_range * sizeof(float)))) return rc;
  P.sched.wait_input_free(b, k, plan_finalizes(P));
  if (P.pipe_in_ready) {
    // the caller converts the recording slice by slice on its own threads: the chunk's samples are copied piece by
    // piece as they are published (a caller that publishes finer than a chunk gets its copies under its conversion)
    long long pos = lo, spins = 0;
    while (pos < hi) {
      const long long want = std::min<long long>(hi, pos + 4096);
      long long ready = __atomic_load_n(P.pipe_in_ready, __ATOMIC_ACQUIRE);
      if (ready < want) {
        if (++spins > 2000000) return nmx_fail(NMX_E_INVALID, "nmx_plan_set_pipeline: the input never became ready");
        std::this_thread::sleep_for(std::chrono::microseconds(5));
        continue;
      }
      const long long upto = std::min<long long>(hi, ready);
      be_h2d_2d_async((float*)xb.p + (pos - lo), (size_t)n_range * sizeof(float), x + pos, (size_t)ldx * sizeof(float),
                      (size_t)(upto - pos) * sizeof(float), (size_t)Cin, sc);
      pos = upto;
    }
  } else {
    be_h2d_2d_async(xb.p, (size_t)n_range * sizeof(float), x + lo, (size_t)ldx * sizeof(float),
                    (size_t)n_range * sizeof(float), (size_t)Cin, sc);
  }
  P.sched.input_copied(b);
  *d_xk = (const float*)xb.p - lo;
  *ldxk = n_range;
  return 0;
}

// Where a batch's rows and NaN mask are computed (d_*: the caller's buffers, or the plan's for a host batch) and where the
// caller wants them.
struct BatchOut {
  float *out, *d_out;
  uint8_t* nan_mask;
  unsigned char* d_mask;
  int F, Cin;   // row stride; mask bytes per row
};
// features of the finished chunk of parity `par` (rows [w0, w0 + nw)) -> host
// (on its own stream: behind the copy stream's input copies these waits held the copy of chunk k + 1 until chunk
// k - 1 was complete -- on a young stream, whose threshold walks are the long pole, 6 ms after its samples were ready)
static void fetch_back(Plan& P, const BatchSched& b, const BatchOut& o, int64_t w0, int64_t nw, int par) {
  const be_stream_t so = P.sched.out_stream(b);
  if (!b.inline_all) P.sched.wait_done(b, so, par, plan_finalizes(P), false);
  be_d2h_async(o.out + (size_t)w0 * o.F, o.d_out + (size_t)w0 * o.F, (size_t)nw * o.F * sizeof(float), so);
  if (o.nan_mask) be_d2h_async(o.nan_mask + (size_t)w0 * o.Cin, o.d_mask + (size_t)w0 * o.Cin, (size_t)nw * o.Cin, so);
  if (P.pipe_out_done && P.pipe_marks.size() < P.pipe_marks.capacity()) {   // tell the caller's threads: rows [0, w0 + nw) are there
    P.pipe_marks.push_back(Plan::Progress{P.pipe_out_done, w0 + nw});
    be_host_fn(so, [](void* a) { auto* m = (Plan::Progress*)a; __atomic_store_n(m->dst, m->value, __ATOMIC_RELEASE); },
               &P.pipe_marks.back());
  }
}

static int process_batch_impl(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples,
                              const int64_t* starts, int64_t n_windows, float* out, uint8_t* nan_mask,
                              int memspace, void* hip_stream, float* pre) {
  int rc = check_batch_args((Plan*)plan, x, ldx, n_samples, starts, n_windows, out, memspace);
  if (rc) return rc;
  Plan& P = *(Plan*)plan;
  const nmx_plan_desc& d = P.d;
  if ((rc = be_set_device(P.device))) return rc;
  const bool host = memspace == 0;
  // The one-window call of a real-time loop (and any host batch of a few hops): ONE stream for copies, kernels and the
  // normaliser.  Side streams buy such a batch nothing -- its kernels are microseconds -- and every cross-stream hand-off
  // (fork / join of the bursts and sharp-wave chains, finalize stream, copy stream) is an event round trip of 10 - 25 us
  // on a 0.4 ms call.  (NMX_TINY_INLINE=0: the schedule of large batches.)
  const bool tiny = P.tiny_inline && host && n_windows < 8 && !P.pipe_in_ready && !P.pipe_out_done;
  const BatchSched b{hip_stream ? (be_stream_t)hip_stream : P.sched.main, tiny};
  const be_stream_t s = b.s;
  P.sched.last_stream = s;
  BatchOut o{out, out, nan_mask, nan_mask, d.n_outputs + d.n_extra_cols, d.n_channels_in};
  if ((rc = dc_prepare(P, x, ldx, starts[0], host, s))) return rc;
  if ((rc = ensure(P.starts, (size_t)n_windows * sizeof(long long)))) return rc;
  be_h2d_async(P.starts.p, starts, (size_t)n_windows * sizeof(long long), s);
  if (host) {
    if ((rc = ensure(P.out, (size_t)n_windows * o.F * sizeof(float)))) return rc;
    o.d_out = (float*)P.out.p;
    if (nan_mask) {
      if ((rc = ensure(P.mask, (size_t)n_windows * o.Cin))) return rc;
      o.d_mask = (unsigned char*)P.mask.p;
    }
  }
  const ChunkSizes sizes = batch_chunk_sizes(P, host);
  be_timer_start(P.timers[ST_BATCH], s);
  int64_t prev_w0 = -1, prev_nw = 0;
  int k = 0, last_par = -1;
  P.pipe_marks.clear();
  P.pipe_marks.reserve((size_t)(n_windows / std::max<int64_t>(1, std::min<int64_t>({P.host_first_chunk, P.chunk_windows, sizes.dev_chunk,
                                                                                    sizes.host_first, sizes.host_big})) + 8));
  // an error in mid-batch leaves work in flight: host callbacks holding pointers into P.pipe_marks, copies into the caller's
  // out / mask.  Nothing returns to the caller -- who may free those buffers, or start the next batch, whose
  // pipe_marks.clear() + reserve() may move the marks -- before the batch's streams have drained.
  auto bail = [&](int r) {
    P.sched.drain(b);
    return r;
  };
  struct ScaleGuard { ~ScaleGuard() { g_ensure_scale = 1.0; } } scale_guard;
  for (int64_t w0 = 0; w0 < n_windows; ++k) {
    const int nw = (int)std::min<int64_t>(sizes.at(w0), n_windows - w0);
    // (buffers that grow during the short first chunk: sized for the longest chunk behind it -- see ensure())
    g_ensure_scale = (host && w0 == 0 && n_windows > nw) ? (double)std::min<int64_t>(sizes.host_big, n_windows - nw) / (double)nw : 1.0;
    long long lo = starts[w0], hi = starts[w0] + P.w_in;
    for (int64_t i = w0; i < w0 + nw; ++i) {
      lo = std::min<long long>(lo, starts[i]);
      hi = std::max<long long>(hi, starts[i] + P.w_in);
    }
    const float* d_xk = x;
    long long ldxk = ldx;
    if (host && (rc = stage_host_chunk(P, b, k, x, ldx, lo, hi, &d_xk, &ldxk))) return bail(rc);
    float* d_outk = o.d_out + (size_t)w0 * o.F;
    be_memset_async(d_outk, 0xFF, (size_t)nw * o.F * sizeof(float), s);  // unwritten -> NaN
    if (o.d_mask) {
      NmxNanMaskArgs M{};
      M.x = d_xk; M.ldx = ldxk; M.starts = (const long long*)P.starts.p + w0; M.mask = o.d_mask + (size_t)w0 * o.Cin;
      M.C_in = o.Cin; M.W = P.w_in;
      be_launch_nanmask(M, nw * o.Cin, s);
    }
    float* d_prek = nullptr;
    const size_t pre_n = (size_t)nw * d.n_channels * d.window;
    if (pre) {
      if (host) {
        if ((rc = ensure(P.tap, pre_n * sizeof(float)))) return bail(rc);
        d_prek = (float*)P.tap.p;
      } else {
        d_prek = pre + (size_t)w0 * d.n_channels * d.window;
      }
    }
    bool freed = false;
    P.nolds.probe_w0 = w0;
    rc = run_chunk(P, b, d_xk, ldxk, lo, hi, (const long long*)P.starts.p + w0, nw, d_outk, w0 == 0, d_prek, starts + w0,
                   host ? P.sched.input_consumed_event(b, k) : nullptr, &freed);
    if (rc) return bail(rc);
    if (host) P.sched.input_consumed(k, freed);
    if (pre && host)   // same stream as the kernels: the next chunk's gather waits for this copy
      be_d2h_async(pre + (size_t)w0 * d.n_channels * d.window, d_prek, pre_n * sizeof(float), s);
    const int par_k = P.sched.parity();
    if ((rc = chunk_finalize(P, b, d_outk, o.F, nw, w0 == 0))) return bail(rc);   // (normaliser: hop order = chunk order)
    last_par = par_k;
    if (host) {
      if (prev_w0 >= 0) fetch_back(P, b, o, prev_w0, prev_nw, par_k ^ 1);
      prev_w0 = w0;
      prev_nw = nw;
    }
    w0 += nw;
  }
  // the caller's stream completes when the last chunk's rows do
  if (last_par >= 0 && !tiny) P.sched.wait_done(b, s, last_par, plan_finalizes(P), true);
  be_timer_stop(P.timers[ST_BATCH], s);
  if (host) {
    fetch_back(P, b, o, prev_w0, prev_nw, last_par);
    for (be_stream_t st : {P.sched.out_stream(b), P.sched.in_stream(b), s})   // (a watchdog verdict: nothing more is waited for)
      if ((rc = be_sync_watch(st, P.kernels, ST_COUNT))) return rc;
    if (P.pipe_out_done) __atomic_store_n(P.pipe_out_done, (int64_t)n_windows, __ATOMIC_RELEASE);
  }
  return be_check_launch();
}

int nmx_process_batch(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples,
                      const int64_t* starts, int64_t n_windows, float* out, uint8_t* nan_mask,
                      int memspace, void* hip_stream) {
  return process_batch_impl(plan, x, ldx, n_samples, starts, n_windows, out, nan_mask, memspace, hip_stream, nullptr);
}

int nmx_process_batch_tap(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples,
                          const int64_t* starts, int64_t n_windows, float* out, uint8_t* nan_mask,
                          int memspace, void* hip_stream, float* pre) {
  if (!pre) return nmx_fail(NMX_E_INVALID, "null argument");
  return process_batch_impl(plan, x, ldx, n_samples, starts, n_windows, out, nan_mask, memspace, hip_stream, pre);
}

int nmx_process_window(nmx_plan* plan, const double* x, int64_t ldx, float* out, uint8_t* nan_mask) {
  Plan* P = (Plan*)plan;
  if (!P || !x || !out) return nmx_fail(NMX_E_INVALID, "null argument");
  const int Cin = P->d.n_channels_in, W = P->w_in, F = P->d.n_outputs + P->d.n_extra_cols;
  // The reference's real-time loop makes this call once per hop (stream/stream.py:280-296): everything that crosses the
  // bus lives in ONE page-locked staging block of the plan -- the window cast to float32, the feature row, the mask -- so
  // both copies are plain DMA transfers (a pageable source is staged by the runtime, synchronously: ~0.1 ms per MB).
  const size_t xb = (((size_t)Cin * W * sizeof(float)) + 255) & ~(size_t)255, ob = (((size_t)F * sizeof(float)) + 255) & ~(size_t)255;
  const size_t need = xb + ob + (size_t)Cin;
  if (P->win_pin.cap < need) {
    int rc = be_set_device(P->device);
    if (rc) return rc;
    if (!P->win_pin.regrow(need)) return nmx_fail(NMX_E_NOMEM, "page-locked host allocation failed");
  }
  float* xf = (float*)P->win_pin.p;
  float* of = (float*)((char*)P->win_pin.p + xb);
  uint8_t* mf = (uint8_t*)P->win_pin.p + xb + ob;
  for (int c = 0; c < Cin; ++c) {
    const double dh = P->dc_host_set ? P->dc_host[c] : 0.0;   // (the caller's split: subtracted before the cast rounds)
    const double* xr = x + (size_t)c * ldx;
    float* d = xf + (size_t)c * W;
    for (int i = 0; i < W; ++i) d[i] = (float)(xr[i] - dh);
  }
  const int64_t start = 0;
  const int rc = nmx_process_batch(plan, xf, W, W, &start, 1, of, nan_mask ? mf : nullptr, 0, nullptr);
  if (rc) return rc;
  memcpy(out, of, (size_t)F * sizeof(float));
  if (nan_mask) memcpy(nan_mask, mf, (size_t)Cin);
  return 0;
}

int nmx_preprocess_window(nmx_plan* plan, const double* x, int64_t ldx, double* y, int64_t ldy) {
  Plan* Pp = (Plan*)plan;
  if (!Pp || !x || !y) return nmx_fail(NMX_E_INVALID, "null argument");
  Plan& P = *Pp;
  const nmx_plan_desc& d = P.d;
  const int Cin = d.n_channels_in, C = d.n_channels, Wo = d.window;
  const int W = P.w_in;   // incoming samples per window
  int rc = be_set_device(P.device);
  if (rc) return rc;
  be_stream_t s = P.sched.main;
  std::vector<float> xf((size_t)Cin * W), yf((size_t)C * Wo);
  for (int c = 0; c < Cin; ++c) {
    const double dh = P.dc_host_set ? P.dc_host[c] : 0.0;
    for (int i = 0; i < W; ++i) {
      const double v = x[(size_t)c * ldx + i];
      xf[(size_t)c * W + i] = (float)((v != v ? 0.0 : v) - dh);   // (a NaN is the value 0: data_processor.py:255)
    }
  }
  if ((rc = dc_prepare(P, xf.data(), W, 0, true, s))) return rc;
  if ((rc = ensure(P.x_in, xf.size() * sizeof(float)))) return rc;
  be_h2d_async(P.x_in.p, xf.data(), xf.size() * sizeof(float), s);
  NMX_REQUIRE(P.front.d_R || Cin == C, "n_channels_in != n_channels without ref_matrix");
  WinView v{(const float*)P.x_in.p, W, 0, nullptr, 1};
  be_stage_reset();
  be_stage(ST_PREP);
  if ((rc = launch_front(P, v.x, W, 0, W, false, s, v))) return rc;
  if ((rc = run_prep_stages(P, v, 1, s))) return rc;
  be_stage(ST_BATCH);
  snapshot_kernels(P);   // (nmx_last_kernels: what this call launched)
  be_d2h_async(yf.data(), v.x, yf.size() * sizeof(float), s);
  if ((rc = be_sync(s))) return rc;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < Wo; ++i) {
      float f = yf[(size_t)c * Wo + i];
      if (v.clean) f = (f != f) ? 0.f : f;
      y[(size_t)c * ldy + i] = (double)f + (P.dc_active ? P.dc_pre_h[c] : 0.0);
    }
  return be_check_launch();
}

int nmx_filter_window(nmx_plan* plan, const double* x, int64_t ldx, double* y) {
  Plan* Pp = (Plan*)plan;
  if (!Pp || !x || !y) return nmx_fail(NMX_E_INVALID, "null argument");
  Plan& P = *Pp;
  NMX_REQUIRE(P.have_bank, "plan has no FIR bank");
  const nmx_plan_desc& d = P.d;
  const int C = d.n_channels, W = d.window, NF = d.n_filters;
  int rc = be_set_device(P.device);
  if (rc) return rc;
  be_stream_t s = P.sched.main;
  std::vector<float> xf((size_t)C * W), yf((size_t)C * NF * W);
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < W; ++i) xf[(size_t)c * W + i] = (float)x[(size_t)c * ldx + i];
  if ((rc = ensure(P.x_in, xf.size() * sizeof(float)))) return rc;
  if ((rc = ensure(P.sharp.swy[0], yf.size() * sizeof(float)))) return rc;
  be_h2d_async(P.x_in.p, xf.data(), xf.size() * sizeof(float), s);
  NmxBankArgs A = P.bank.a;
  view_into(A, WinView{(const float*)P.x_in.p, W, 0, nullptr, 0});
  A.out = nullptr;
  A.n_sw_filters = NF; A.sw_out = (float*)P.sharp.swy[0].p;
  // (bp_seglen = 0 switches every epilogue off, the differenced-taps one of a long plan included -- A.out is null here: the
  // plan's kernel runs, and every filter goes the whole-series way)
  for (int i = 0; i < NF; ++i) {
    A.f[i].sw_index = i; A.f[i].bp_seglen = 0; A.f[i].burst_index = -1; A.f[i].store_raw = 0;
  }
  be_stage_reset();
  be_stage(P.bank.launches[0].stage);
  launch_fir_stage(P, P.bank, A, C, s, false, true);   // (no notch here: a launch the plan fused into it runs stand-alone)
  be_stage(ST_BATCH);
  snapshot_kernels(P);   // (nmx_last_kernels: what this call launched)
  be_d2h_async(yf.data(), P.sharp.swy[0].p, yf.size() * sizeof(float), s);
  if ((rc = be_sync(s))) return rc;
  for (size_t i = 0; i < yf.size(); ++i) y[i] = (double)yf[i];
  return be_check_launch();
}

int nmx_last_timing_ms(nmx_plan* plan, int which, float* ms) {
  Plan* P = (Plan*)plan;
  if (!P || !ms || which < ST_BATCH || which >= ST_COUNT || which == ST_GEOM) return nmx_fail(NMX_E_INVALID, "bad argument");
  be_set_device(P->device);
  *ms = be_timer_elapsed(P->timers[which]);
  return 0;
}


int nmx_host_alloc(int64_t n_bytes, void** out) {
  if (!out || n_bytes < 0) return nmx_fail(NMX_E_INVALID, "bad argument");
  if (be_device_count() <= 0) return nmx_fail(NMX_E_NODEVICE, "no HIP device");
  *out = be_host_alloc((size_t)n_bytes);
  if (!*out) return nmx_fail(NMX_E_NOMEM, "page-locked host allocation of " + std::to_string(n_bytes) + " bytes failed");
  return 0;
}
int nmx_host_free(void* p) {
  if (p) be_host_free(p);
  return 0;
}
int nmx_device_pool_trim(int64_t keep_bytes, int64_t* freed) {
  if (keep_bytes < 0) return nmx_fail(NMX_E_INVALID, "keep_bytes must be >= 0");
  const long long n = be_dev_pool_trim((long long)keep_bytes);
  if (freed) *freed = (int64_t)n;
  return 0;
}

int nmx_reref_f64(int device, const double* ref_matrix, int n_out, int n_in, const double* x, int64_t ldx,
                  int64_t n_samples, double* y, int64_t ldy) {
  if (!ref_matrix || !x || !y) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(n_out >= 1 && n_in >= 1 && n_samples >= 0 && ldx >= n_samples && ldy >= n_samples,
              "nmx_reref_f64: n_out, n_in >= 1, n_samples >= 0, ldx / ldy >= n_samples");
  if (n_samples == 0) return 0;
  if (be_device_count() <= 0) return nmx_fail(NMX_E_NODEVICE, "no HIP device");
  int rc = be_set_device(device);
  if (rc) return rc;
  const size_t T = (size_t)n_samples, nR = (size_t)n_out * n_in * sizeof(double);
  const size_t nx = (size_t)n_in * T * sizeof(double), ny = (size_t)n_out * T * sizeof(double);
  // one block: R | x | y (dense rows of n_samples); the pool keeps it for the next call
  char* d = (char*)be_alloc(nR + nx + ny);
  if (!d) return nmx_fail(NMX_E_NOMEM, "nmx_reref_f64: device allocation of " + std::to_string(nR + nx + ny) + " bytes failed");
  be_stream_t s = be_stream_create();
  be_h2d_async(d, ref_matrix, nR, s);
  be_h2d_2d_async(d + nR, T * sizeof(double), x, (size_t)ldx * sizeof(double), T * sizeof(double), (size_t)n_in, s);
  NmxReref64Args A{};
  A.R = (const double*)d; A.x = (const double*)(d + nR); A.ldx = (long long)T; A.y = (double*)(d + nR + nx); A.ldy = (long long)T;
  A.C = n_out; A.C_in = n_in; A.T = (long long)T;
  be_launch_reref64(A, s);
  be_d2h_2d_async(y, (size_t)ldy * sizeof(double), d + nR + nx, T * sizeof(double), T * sizeof(double), (size_t)n_out, s);
  rc = be_sync(s);
  be_stream_destroy(s);
  be_free(d);
  return rc ? rc : be_check_launch();
}

int nmx_resample_f64(int device, const double* x, int64_t ldx, int n_channels, int64_t n_samples, double ratio, double* y,
                     int64_t ldy, int64_t n_out) {
  return nmx_resample_f64_npad(device, x, ldx, n_channels, n_samples, ratio, y, ldy, n_out, -1);
}

int nmx_resample_f64_npad(int device, const double* x, int64_t ldx, int n_channels, int64_t n_samples, double ratio, double* y,
                          int64_t ldy, int64_t n_out, int64_t npad) {
  if (!x || !y) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(n_channels >= 1 && n_samples >= 1 && n_samples <= (1ll << 24) && ldx >= n_samples,
              "nmx_resample_f64: n_channels >= 1, 1 <= n_samples <= 2^24, ldx >= n_samples");
  NMX_REQUIRE(ratio > 0 && ratio != 1.0 && ratio <= 1024.0, "nmx_resample_f64: ratio must be in (0, 1024] and != 1");
  // the lengths of mne.filter.resample (Python's round is round-half-even; so is nearbyint in the default rounding mode)
  const long long W = n_samples, final_len = (long long)std::nearbyint(ratio * (double)W);
  NMX_REQUIRE(final_len == n_out && ldy >= n_out, "nmx_resample_f64: n_out must equal round(ratio * n_samples) and ldy >= n_out");
  if (final_len == 0) return 0;
  long long n_pad = 1, pad_l;
  if (npad >= 0) {   // fixed pad: that many samples per side
    NMX_REQUIRE(W + 2 * (long long)npad <= (1ll << 25), "nmx_resample_f64_npad: n_samples + 2 npad beyond 2^25 samples");
    n_pad = W + 2 * (long long)npad;
    pad_l = (long long)npad;
  } else {
    const long long min_add = std::min<long long>(W / 8, 100) * 2;
    while (n_pad < W + min_add) n_pad <<= 1;
    pad_l = (n_pad - W) / 2;
  }
  const long long n_new = std::max<long long>((long long)std::nearbyint(ratio * (double)n_pad), 1);
  const long long crop_l = (long long)std::nearbyint(ratio * (double)pad_l);
  NMX_REQUIRE(crop_l + final_len <= n_new, "internal: resample crop outside the output");
  NMX_REQUIRE(n_new <= (1ll << 28), "nmx_resample_f64: resampled padded length beyond 2^28 samples");
  long long L = 0, Lf = 0;
  if (n_new & (n_new - 1)) { L = 1; while (L < 2 * n_new - 1) L <<= 1; }
  if (n_pad & (n_pad - 1)) { Lf = 1; while (Lf < 2 * n_pad - 1) Lf <<= 1; }
  if (be_device_count() <= 0) return nmx_fail(NMX_E_NODEVICE, "no HIP device");
  int rc = be_set_device(device);
  if (rc) return rc;
  const int C = n_channels;
  const long long ld = std::max(std::max(n_pad, n_new), std::max(L, Lf));
  const size_t nx = (size_t)C * W * sizeof(double), ny = (size_t)C * final_len * sizeof(double);
  const size_t nw = (size_t)C * ld * sizeof(NmxCplx64), nc = (size_t)std::max(L, Lf) * sizeof(NmxCplx64);
  char* d = (char*)be_alloc(nx + ny + 2 * nw + 2 * nc);
  if (!d) return nmx_fail(NMX_E_NOMEM, "nmx_resample_f64: device allocation of " + std::to_string(nx + ny + 2 * nw + 2 * nc) + " bytes failed");
  be_stream_t s = be_stream_create();
  NmxResample64Args A{};
  A.x = (const double*)d; A.ldx = W; A.y = (double*)(d + nx); A.ldy = final_len;
  A.a = (NmxCplx64*)(d + nx + ny); A.b = (NmxCplx64*)(d + nx + ny + nw); A.ld = ld; A.C = C;
  A.W = W; A.W_new = final_len; A.n_pad = n_pad; A.pad_l = pad_l; A.n_new = n_new; A.crop_l = crop_l; A.L = L; A.Lf = Lf;
  const long long use_len = std::min(n_new, n_pad);
  A.nyq_bin = (use_len % 2 == 0) ? use_len / 2 : -1;
  A.nyq_scale = n_new < n_pad ? 2.0 : 0.5;
  A.scale = ratio / (double)n_new / (L ? (double)L : 1.0) / (Lf ? (double)Lf : 1.0);
  be_h2d_2d_async(d, (size_t)W * sizeof(double), x, (size_t)ldx * sizeof(double), (size_t)W * sizeof(double), (size_t)C, s);
  // a power-of-two transform of `rows` rows: log2(n) Stockham stages between `cur` and `oth`; the result is in `cur`
  auto fft = [&](NmxCplx64*& cur, NmxCplx64*& oth, long long ldr, long long n, int sign, int rows) {
    for (long long ns = n, st = 1; ns > 1; ns >>= 1, st <<= 1) {
      be_launch_rs64_pass(cur, oth, ldr, n, ns, st, sign, rows, s);
      std::swap(cur, oth);
    }
  };
  // Bluestein's chirp convolution, either side: `cur` holds the rows times exp(+i pi j^2 / M), zero-extended to Lb points; it
  // leaves Lb x their circular convolution with exp(-i pi j^2 / M) in `cur` -- the unnormalised INVERSE transform of length M
  // once bin j is multiplied by exp(+i pi j^2 / M) (OUT on the inverse side, MAP -- with the conjugate -- on the forward one)
  auto chirp_conv = [&](NmxCplx64*& cur, NmxCplx64*& oth, long long M, long long Lb) {
    NmxCplx64 *cc = (NmxCplx64*)(d + nx + ny + 2 * nw), *co = cc + std::max(L, Lf);
    A.bM = M; A.bL = Lb;
    be_launch_rs64_elem(A, NMX_RS64_CHIRP, nullptr, cc, Lb, 1, s);
    fft(cc, co, Lb, Lb, -1, 1);
    A.chirp = cc;
    fft(cur, oth, ld, Lb, -1, C);
    be_launch_rs64_elem(A, NMX_RS64_MUL, nullptr, cur, Lb, C, s);
    fft(cur, oth, ld, Lb, +1, C);
  };
  NmxCplx64 *cur = A.a, *oth = A.b;
  be_launch_rs64_elem(A, NMX_RS64_PAD, nullptr, cur, Lf ? Lf : n_pad, C, s);
  if (!Lf) fft(cur, oth, ld, n_pad, -1, C);
  else chirp_conv(cur, oth, n_pad, Lf);
  be_launch_rs64_elem(A, NMX_RS64_MAP, cur, oth, L ? L : n_new, C, s);
  std::swap(cur, oth);
  if (!L) fft(cur, oth, ld, n_new, +1, C);
  else chirp_conv(cur, oth, n_new, L);
  be_launch_rs64_elem(A, NMX_RS64_OUT, cur, nullptr, final_len, C, s);
  be_d2h_2d_async(y, (size_t)ldy * sizeof(double), d + nx, (size_t)final_len * sizeof(double), (size_t)final_len * sizeof(double),
                  (size_t)C, s);
  rc = be_sync(s);
  be_stream_destroy(s);
  be_free(d);
  return rc ? rc : be_check_launch();
}

int nmx_last_kernels(nmx_plan* plan, int which, char* buf, int64_t n) {
  Plan* P = (Plan*)plan;
  if (!P || !buf || n < 1 || which < ST_PREP || which >= ST_COUNT) return nmx_fail(NMX_E_INVALID, "bad argument");
  std::string k = which == ST_GEOM ? P->pair_geom : P->kernels[which];   // (9: no stage, the pair kernels' launch geometry)
  if (which == ST_BURSTS && P->bursts.sparse_count)   // (count mode: rows stored as their tail / rows, over the plan's life)
    k += (k.empty() ? "" : ",") + std::string("env_tail_rows=") + std::to_string(P->bursts.env_tail_rows) + "/" + std::to_string(P->bursts.env_rows);
  const size_t m = std::min<size_t>(k.size(), (size_t)n - 1);
  memcpy(buf, k.data(), m);
  buf[m] = 0;
  return 0;
}


// ---- nolds: a batch that also hands back what the sample-entropy kernel counted (include/nmx.h) ----------------------------
int nmx_nolds_probe(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples, const int64_t* starts, int64_t n_windows,
                    float* out, uint32_t* a, uint32_t* b, float* tol, uint8_t* sum_zero, float* series) {
  Plan* Pp = (Plan*)plan;
  if (!Pp) return nmx_fail(NMX_E_INVALID, "null argument");
  Plan& P = *Pp;
  NMX_REQUIRE(P.have_nolds && P.nolds.have_sampen, "nmx_nolds_probe: the plan has no nolds stage with a sample-entropy kernel");
  NMX_REQUIRE(n_windows >= 1 && n_windows <= (1 << 20), "nmx_nolds_probe: 1 <= n_windows <= 2^20");
  const size_t per_hop = (size_t)(P.nolds.a.raw + P.nolds.a.n_band) * P.d.n_channels, n = (size_t)n_windows * per_hop;
  std::vector<unsigned> hp(n * 4);
  std::vector<float> rows;
  if (!out) { rows.resize((size_t)n_windows * (P.d.n_outputs + P.d.n_extra_cols)); out = rows.data(); }
  P.nolds.h_probe = hp.data();
  P.nolds.h_series = series;
  const int rc = process_batch_impl(plan, x, ldx, n_samples, starts, n_windows, out, nullptr, 0, nullptr, nullptr);
  P.nolds.h_probe = nullptr;
  P.nolds.h_series = nullptr;
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    if (a) a[i] = hp[4 * i];
    if (b) b[i] = hp[4 * i + 1];
    if (tol) memcpy(&tol[i], &hp[4 * i + 2], 4);
    if (sum_zero) sum_zero[i] = (uint8_t)hp[4 * i + 3];
  }
  return 0;
}

// ---- nolds: the same for the DFA kernel (include/nmx.h) --------------------------------------------------------------------
int nmx_nolds_dfa_probe(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples, const int64_t* starts, int64_t n_windows,
                        float* out, double* fluct, double* alpha, uint8_t* sum_zero, int32_t* n_kept, float* series) {
  Plan* Pp = (Plan*)plan;
  if (!Pp) return nmx_fail(NMX_E_INVALID, "null argument");
  Plan& P = *Pp;
  NMX_REQUIRE(P.have_nolds && P.nolds.have_dfa, "nmx_nolds_dfa_probe: the plan has no DFA kernel");
  NMX_REQUIRE(n_windows >= 1 && n_windows <= (1 << 20), "nmx_nolds_dfa_probe: 1 <= n_windows <= 2^20");
  const size_t S = (size_t)P.nolds.dfa.n_scales, per_item = S + 3;
  const size_t n = (size_t)n_windows * (size_t)(P.nolds.a.raw + P.nolds.a.n_band) * P.d.n_channels;
  std::vector<double> hp(n * per_item);
  std::vector<float> rows;
  if (!out) { rows.resize((size_t)n_windows * (P.d.n_outputs + P.d.n_extra_cols)); out = rows.data(); }
  P.nolds.h_dfa = hp.data();
  P.nolds.h_series = series;
  const int rc = process_batch_impl(plan, x, ldx, n_samples, starts, n_windows, out, nullptr, 0, nullptr, nullptr);
  P.nolds.h_dfa = nullptr;
  P.nolds.h_series = nullptr;
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    const double* p = hp.data() + i * per_item;
    if (fluct) memcpy(fluct + i * S, p, S * sizeof(double));
    if (alpha) alpha[i] = p[S];
    if (sum_zero) sum_zero[i] = (uint8_t)(p[S + 1] != 0.0);
    if (n_kept) n_kept[i] = (int32_t)p[S + 2];
  }
  return 0;
}

// ---- nolds: the same for the Hurst kernel (include/nmx.h) ------------------------------------------------------------------
int nmx_nolds_hurst_probe(nmx_plan* plan, const float* x, int64_t ldx, int64_t n_samples, const int64_t* starts, int64_t n_windows,
                          float* out, double* rs, int32_t* kept, double* hurst, uint8_t* sum_zero, int32_t* n_kept, float* series) {
  Plan* Pp = (Plan*)plan;
  if (!Pp) return nmx_fail(NMX_E_INVALID, "null argument");
  Plan& P = *Pp;
  NMX_REQUIRE(P.have_nolds && P.nolds.have_hurst, "nmx_nolds_hurst_probe: the plan has no Hurst kernel");
  NMX_REQUIRE(n_windows >= 1 && n_windows <= (1 << 20), "nmx_nolds_hurst_probe: 1 <= n_windows <= 2^20");
  const size_t S = (size_t)P.nolds.hurst.n_scales, per_item = 2 * S + 3;
  const size_t n = (size_t)n_windows * (size_t)(P.nolds.a.raw + P.nolds.a.n_band) * P.d.n_channels;
  std::vector<double> hp(n * per_item);
  std::vector<float> rows;
  if (!out) { rows.resize((size_t)n_windows * (P.d.n_outputs + P.d.n_extra_cols)); out = rows.data(); }
  P.nolds.h_hurst = hp.data();
  P.nolds.h_series = series;
  const int rc = process_batch_impl(plan, x, ldx, n_samples, starts, n_windows, out, nullptr, 0, nullptr, nullptr);
  P.nolds.h_hurst = nullptr;
  P.nolds.h_series = nullptr;
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    const double* p = hp.data() + i * per_item;
    if (rs) memcpy(rs + i * S, p, S * sizeof(double));
    if (kept) for (size_t k = 0; k < S; ++k) kept[i * S + k] = (int32_t)p[S + k];
    if (hurst) hurst[i] = p[2 * S];
    if (sum_zero) sum_zero[i] = (uint8_t)(p[2 * S + 1] != 0.0);
    if (n_kept) n_kept[i] = (int32_t)p[2 * S + 2];
  }
  return 0;
}
