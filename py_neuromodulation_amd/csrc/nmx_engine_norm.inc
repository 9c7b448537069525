// nmx_engine_norm.inc -- C ABI, part 3: the feature normaliser (nmx_norm_*) and its attachment to a plan.
// Included by nmx_engine.inc.
// ---- feature normaliser -------------------------------------------------------------------------
namespace {
struct NmxNormHandle {
  int device = 0, n_cols = 0, method = 0, cap = 0;
  float clip = 0.f;
  bool scan_on = true;         // mean / z-score as scans (NMX_NORM_SCAN, read when the normaliser is created)
  long long seq = 0;
  Buf ring;                    // float [cap][n_cols]: allocated once (nmx_norm_create), like the two below
  Buf sorted;                  // median methods: scratch, same shape as the ring
  Buf mask;                    // unsigned char [n_cols] (empty: every column)
  Buf stage;
  Buf ext, sl;                 // "power": extended history of a batch (raw fp32) and its sign(x) log1p|x| (fp64)
  Buf scan;                    // "mean" / "zscore" as scans (nmx_k_norm.h, NmxNormScan): sums, counts, raw copy of a batch
  be_stream_t stream = nullptr;
};
}  // namespace

int nmx_norm_create(int32_t device, int32_t n_cols, int32_t method, float clip, int32_t n_hist,
                    const uint8_t* colmask, nmx_norm** out) {
  if (!out) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(n_cols > 0, "n_cols must be positive");
  NMX_REQUIRE(method >= NMX_NORM_MEAN && method <= NMX_NORM_POWER,
              "normalisation method outside 0..7 (mean, zscore, median, zscore-median, robust, minmax, quantile, power)");
  NMX_REQUIRE(n_hist >= 2, "normalisation history must hold at least 2 rows");
  if (device < 0 || device >= be_device_count()) return nmx_fail(NMX_E_NODEVICE, "no such device");
  int rc = be_set_device(device);
  if (rc) return rc;
  NmxNormHandle* H = new NmxNormHandle();
  H->device = device; H->n_cols = n_cols; H->method = method; H->cap = n_hist; H->clip = clip;
  H->scan_on = env_int("NMX_NORM_SCAN", 1) != 0;
  const size_t ring_bytes = (size_t)n_hist * n_cols * sizeof(float);
  if (!H->ring.regrow(ring_bytes) || (method >= NMX_NORM_MEDIAN && method != NMX_NORM_POWER && !H->sorted.regrow(ring_bytes)) ||
      (colmask && !H->mask.regrow((size_t)n_cols))) {
    delete H;
    return nmx_fail(NMX_E_NOMEM, "device allocation failed");
  }
  if (colmask) be_h2d_sync(H->mask.p, colmask, (size_t)n_cols);
  H->stream = be_stream_create();
  *out = (nmx_norm*)H;
  return be_check_launch();
}

int nmx_norm_destroy(nmx_norm* norm) {
  NmxNormHandle* H = (NmxNormHandle*)norm;
  if (!H) return 0;
  be_set_device(H->device);
  be_sync(H->stream);
  be_stream_destroy(H->stream);
  delete H;
  return 0;
}

int nmx_norm_process(nmx_norm* norm, float* rows, int64_t ld, int64_t n_rows, int memspace, void* hip_stream) {
  NmxNormHandle* H = (NmxNormHandle*)norm;
  if (!H || (!rows && n_rows > 0)) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(ld >= H->n_cols && n_rows >= 0 && n_rows < (1ll << 31), "bad row layout");
  NMX_REQUIRE(memspace == 0 || memspace == 1, "memspace must be 0 (host) or 1 (device)");
  if (n_rows == 0) return 0;
  int rc = be_set_device(H->device);
  if (rc) return rc;
  be_stream_t s = hip_stream ? (be_stream_t)hip_stream : H->stream;
  NmxNormArgs A;
  A.n_rows = (int)n_rows; A.n_cols = H->n_cols; A.colmask = (unsigned char*)H->mask.p; A.ring = (float*)H->ring.p;
  A.cap = H->cap; A.seq0 = H->seq; A.method = H->method; A.clip = H->clip; A.sorted = (float*)H->sorted.p;
  auto launch = [&](const NmxNormArgs& N) -> int {
    if (H->method != NMX_NORM_POWER) {
      // mean / z-score: scans + independent cells (nmx_k_norm.h) in pieces of at most cap - 1 hops; the column walk for
      // the one-window call shape (a launch sequence of three is no gain there), short histories and the median family
      const bool scan = H->scan_on && (H->method == NMX_NORM_MEAN || H->method == NMX_NORM_ZSCORE) && N.n_rows >= 8 &&
                        H->cap - 1 >= 64 && H->cap < 65536;   // (a short history would cut a batch into many pieces of five launches each)
      if (!scan) { be_launch_norm(N, s); return 0; }
      const int piece = std::min<int>(N.n_rows, H->cap - 1);
      const size_t cells = (size_t)piece * N.n_cols, cells1 = (size_t)(piece + 1) * N.n_cols;
      const size_t segs = (size_t)((H->cap - 1 + NMX_NORM_SEG - 1) / NMX_NORM_SEG + (piece + NMX_NORM_SEG - 1) / NMX_NORM_SEG) * N.n_cols;
      int rc2;
      if ((rc2 = ensure(H->scan, (cells1 + segs) * (2 * sizeof(double) + sizeof(unsigned)) + cells * sizeof(float)))) return rc2;
      NmxNormScan Sc;
      Sc.s1 = (double*)H->scan.p; Sc.s2 = Sc.s1 + cells1; Sc.t1 = Sc.s2 + cells1; Sc.t2 = Sc.t1 + segs;
      Sc.cn = (unsigned*)(Sc.t2 + segs); Sc.tc = Sc.cn + cells1; Sc.xs = (float*)(Sc.tc + segs);
      for (int r0 = 0; r0 < N.n_rows; r0 += piece) {
        NmxNormArgs M = N;
        M.rows = N.rows + (long long)r0 * N.ld;
        M.n_rows = std::min<int>(piece, N.n_rows - r0);
        M.seq0 = N.seq0 + r0;
        nmx_norm_scan_shape(M, Sc);
        be_launch_norm_scan(M, Sc, s);
      }
      return 0;
    }
    // "power" (nmx_k_power.h): every (hop, column) of the batch is an independent fit over the extended history
    NmxPowerPrepArgs Pp;
    Pp.have = (int)(H->seq < (long long)(H->cap - 1) ? H->seq : (long long)(H->cap - 1));
    Pp.ring = (float*)H->ring.p; Pp.rows = N.rows; Pp.ld = N.ld; Pp.n_rows = N.n_rows; Pp.n_cols = N.n_cols;
    Pp.cap = H->cap; Pp.seq0 = H->seq;
    const size_t cells = (size_t)(Pp.have + N.n_rows) * N.n_cols;
    int rc2;
    if ((rc2 = ensure(H->ext, cells * sizeof(float))) || (rc2 = ensure(H->sl, cells * sizeof(double)))) return rc2;
    Pp.ext = (float*)H->ext.p; Pp.sl = (double*)H->sl.p;
    NmxPowerArgs Pa;
    Pa.ext = Pp.ext; Pa.sl = Pp.sl; Pa.rows = N.rows; Pa.ld = N.ld; Pa.n_rows = N.n_rows; Pa.n_cols = N.n_cols;
    Pa.have = Pp.have; Pa.cap = H->cap; Pa.seq0 = H->seq; Pa.colmask = (unsigned char*)H->mask.p; Pa.clip = H->clip;
    be_launch_power(Pp, Pa, s);
    return 0;
  };
  if (memspace == 1) {
    A.rows = rows; A.ld = ld;
    if ((rc = launch(A))) return rc;
  } else {
    const size_t bytes = (size_t)n_rows * H->n_cols * sizeof(float);
    if (H->stage.cap < bytes && !H->stage.regrow(bytes)) return nmx_fail(NMX_E_NOMEM, "device allocation failed");
    be_h2d_2d_async(H->stage.p, (size_t)H->n_cols * sizeof(float), rows, (size_t)ld * sizeof(float),
                    (size_t)H->n_cols * sizeof(float), (size_t)n_rows, s);
    A.rows = (float*)H->stage.p; A.ld = H->n_cols;
    if ((rc = launch(A))) return rc;
    be_d2h_2d_async(rows, (size_t)ld * sizeof(float), H->stage.p, (size_t)H->n_cols * sizeof(float),
                    (size_t)H->n_cols * sizeof(float), (size_t)n_rows, s);
    if ((rc = be_sync(s))) return rc;
  }
  H->seq += n_rows;
  return be_check_launch();
}

int nmx_norm_reset(nmx_norm* norm) {
  NmxNormHandle* H = (NmxNormHandle*)norm;
  if (!H) return nmx_fail(NMX_E_INVALID, "null argument");
  be_set_device(H->device);
  be_sync(H->stream);
  H->seq = 0;
  return 0;
}

// state = { int64 seq, float ring[cap][n_cols] }
int nmx_norm_state_size(const nmx_norm* norm, int64_t* n_bytes) {
  const NmxNormHandle* H = (const NmxNormHandle*)norm;
  if (!H || !n_bytes) return nmx_fail(NMX_E_INVALID, "null argument");
  *n_bytes = (int64_t)sizeof(int64_t) + (int64_t)H->cap * H->n_cols * (int64_t)sizeof(float);
  return 0;
}
int nmx_norm_state_export(nmx_norm* norm, void* dst, int64_t n_bytes) {
  NmxNormHandle* H = (NmxNormHandle*)norm;
  int64_t need = 0;
  if (!H || !dst) return nmx_fail(NMX_E_INVALID, "null argument");
  nmx_norm_state_size(norm, &need);
  NMX_REQUIRE(n_bytes == need, "state size mismatch");
  int rc = be_set_device(H->device);
  if (rc) return rc;
  if ((rc = be_sync(H->stream))) return rc;
  const int64_t seq = H->seq;
  memcpy(dst, &seq, sizeof(seq));
  be_d2h_sync((char*)dst + sizeof(int64_t), H->ring.p, (size_t)(need - (int64_t)sizeof(int64_t)));
  return be_check_launch();
}
int nmx_norm_state_import(nmx_norm* norm, const void* src, int64_t n_bytes) {
  NmxNormHandle* H = (NmxNormHandle*)norm;
  int64_t need = 0;
  if (!H || !src) return nmx_fail(NMX_E_INVALID, "null argument");
  nmx_norm_state_size(norm, &need);
  NMX_REQUIRE(n_bytes == need, "state size mismatch");
  int rc = be_set_device(H->device);
  if (rc) return rc;
  if ((rc = be_sync(H->stream))) return rc;
  int64_t seq;
  memcpy(&seq, src, sizeof(seq));
  NMX_REQUIRE(seq >= 0, "corrupt normaliser state");
  H->seq = seq;
  be_h2d_sync(H->ring.p, (const char*)src + sizeof(int64_t), (size_t)(need - (int64_t)sizeof(int64_t)));
  return be_check_launch();
}

int nmx_plan_attach_norm(nmx_plan* plan, nmx_norm* norm) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  if (norm) {
    const NmxNormHandle* H = (const NmxNormHandle*)norm;
    NMX_REQUIRE(H->device == P->device, "normaliser and plan live on different devices");
    NMX_REQUIRE(H->n_cols == P->d.n_outputs, "normaliser width != the plan's n_outputs");
  }
  P->norm = norm;
  return 0;
}

}  // extern "C"

