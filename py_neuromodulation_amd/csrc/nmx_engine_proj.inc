// nmx_engine_proj.inc -- C ABI, part 4: the grid projection (nmx_proj_*) and its attachment to a plan.
// Included by nmx_engine.inc.
extern "C" {
namespace {
struct NmxProjHandle {
  int device = 0;
  NmxProjArgs a{};          // argument template: device tables, shape, tile (rows / ld / n_rows per call)
  long long min_ld = 0;     // the last column read or written + 1
  long long first_out = 0;  // the first column written (every gathered column lies in front of it)
  Buf tab;                  // w | gather | ptr | idx | out_col | out_stride | point_group (one allocation)
  Buf stage;                // host calls: rows [first gathered column, min_ld) of a batch
  long long first_in = 0;
  be_stream_t stream = nullptr;
};
}  // namespace

int nmx_proj_create(int32_t device, const nmx_proj_desc* desc, nmx_proj** out) {
  if (!desc || !out) return nmx_fail(NMX_E_INVALID, "null argument");
  *out = nullptr;
  const nmx_proj_desc& D = *desc;
  NMX_REQUIRE(D.n_feat >= 1 && D.n_chan >= 1 && D.n_chan <= NMX_PROJ_MAX_CHAN && D.n_points >= 1,
              "nmx_proj: n_feat, n_points >= 1 and 1 <= n_chan <= 12288");
  NMX_REQUIRE((long long)D.n_feat * D.n_chan < (1ll << 31) && (long long)D.n_feat * D.n_points < (1ll << 31),
              "nmx_proj: too many features");
  NMX_REQUIRE(D.gather && D.ptr && D.out_col && D.out_stride && D.group_chan && D.point_group, "null argument");
  NMX_REQUIRE(D.n_groups >= 1 && D.n_groups <= NMX_PROJ_MAX_GROUPS, "nmx_proj: 1 .. 4 groups");
  NMX_REQUIRE(D.group_chan[0] == 0 && D.group_chan[D.n_groups] == D.n_chan, "nmx_proj: group_chan must run from 0 to n_chan");
  for (int g = 0; g < D.n_groups; ++g) NMX_REQUIRE(D.group_chan[g + 1] >= D.group_chan[g], "nmx_proj: group_chan must not decrease");
  const long long nnz = D.ptr[D.n_points];
  NMX_REQUIRE(D.ptr[0] == 0 && nnz >= 0 && nnz < (1ll << 31), "nmx_proj: ptr must start at 0");
  NMX_REQUIRE(nnz == 0 || (D.idx && D.w), "null argument");
  for (int p = 0; p < D.n_points; ++p) NMX_REQUIRE(D.ptr[p + 1] >= D.ptr[p], "nmx_proj: ptr must not decrease");
  for (int p = 0; p < D.n_points; ++p) {
    const int g = D.point_group[p];
    NMX_REQUIRE(g >= 0 && g < D.n_groups, "nmx_proj: point_group outside the groups");
    for (long long e = D.ptr[p]; e < D.ptr[p + 1]; ++e)
      NMX_REQUIRE(D.idx[e] >= D.group_chan[g] && D.idx[e] < D.group_chan[g + 1], "nmx_proj: idx outside the point's group");
  }
  long long in_lo = 1ll << 40, in_hi = -1, out_lo = 1ll << 40, out_hi = -1;
  for (long long i = 0; i < (long long)D.n_feat * D.n_chan; ++i) {
    NMX_REQUIRE(D.gather[i] >= 0, "nmx_proj: negative gather column");
    in_lo = std::min<long long>(in_lo, D.gather[i]);
    in_hi = std::max<long long>(in_hi, D.gather[i]);
  }
  for (int p = 0; p < D.n_points; ++p) {
    const long long a = D.out_col[p], b = a + (long long)(D.n_feat - 1) * D.out_stride[p];
    NMX_REQUIRE(a >= 0 && b >= 0, "nmx_proj: negative output column");
    out_lo = std::min(out_lo, std::min(a, b));
    out_hi = std::max(out_hi, std::max(a, b));
  }
  NMX_REQUIRE(out_lo > in_hi, "nmx_proj: every output column must lie behind every gathered column");
  if (device < 0 || device >= be_device_count()) return nmx_fail(NMX_E_NODEVICE, "no such device");
  int rc = be_set_device(device);
  if (rc) return rc;
  const size_t n_gather = (size_t)D.n_feat * D.n_chan;
  const size_t bytes = (size_t)nnz * sizeof(double) +
                       (n_gather + (size_t)D.n_points + 1 + (size_t)nnz + 3 * (size_t)D.n_points) * sizeof(int32_t);
  NmxProjHandle* H = new NmxProjHandle();
  H->device = device;
  if (!H->tab.regrow(bytes)) { delete H; return nmx_fail(NMX_E_NOMEM, "device allocation failed"); }
  char* p = (char*)H->tab.p;
  auto put = [&](const void* src, size_t n) -> void* {
    void* at = p;
    if (n) be_h2d_sync(at, src, n);
    p += n;
    return at;
  };
  NmxProjArgs& A = H->a;
  A.w = (const double*)put(D.w, (size_t)nnz * sizeof(double));   // (first: 8-byte aligned)
  A.gather = (const int*)put(D.gather, n_gather * sizeof(int32_t));
  A.ptr = (const int*)put(D.ptr, ((size_t)D.n_points + 1) * sizeof(int32_t));
  A.idx = (const int*)put(D.idx, (size_t)nnz * sizeof(int32_t));
  A.out_col = (const int*)put(D.out_col, (size_t)D.n_points * sizeof(int32_t));
  A.out_stride = (const int*)put(D.out_stride, (size_t)D.n_points * sizeof(int32_t));
  A.point_group = (const int*)put(D.point_group, (size_t)D.n_points * sizeof(int32_t));
  A.n_groups = D.n_groups;
  for (int g = 0; g <= D.n_groups; ++g) A.group_chan[g] = D.group_chan[g];
  A.n_feat = D.n_feat; A.n_chan = D.n_chan; A.n_points = D.n_points;
  // the feature tile: as many features as fit NMX_PROJ_LDS_FLOATS staged inputs
  A.tile = std::max(1, std::min(D.n_feat, NMX_PROJ_LDS_FLOATS / D.n_chan));
  A.n_tiles = (D.n_feat + A.tile - 1) / A.tile;
  H->min_ld = out_hi + 1;
  H->first_out = out_lo;
  H->first_in = in_lo;
  H->stream = be_stream_create();
  *out = (nmx_proj*)H;
  return be_check_launch();
}

int nmx_proj_destroy(nmx_proj* proj) {
  NmxProjHandle* H = (NmxProjHandle*)proj;
  if (!H) return 0;
  be_set_device(H->device);
  be_sync(H->stream);
  be_stream_destroy(H->stream);
  delete H;
  return 0;
}

// rows[n_rows][ld] on the device, asynchronous on `s` (the callers have checked that the columns fit: ld >= min_ld, or a
// staged copy of columns [first_in, min_ld) addressed from column 0)
static int proj_launch(nmx_proj* proj, float* rows, long long ld, int n_rows, be_stream_t s) {
  NmxProjHandle* H = (NmxProjHandle*)proj;
  NmxProjArgs A = H->a;
  A.rows = rows; A.ld = ld; A.n_rows = n_rows;
  be_launch_proj(A, s);
  return 0;
}

int nmx_proj_process(nmx_proj* proj, float* rows, int64_t ld, int64_t n_rows, int memspace, void* hip_stream) {
  NmxProjHandle* H = (NmxProjHandle*)proj;
  if (!H || (!rows && n_rows > 0)) return nmx_fail(NMX_E_INVALID, "null argument");
  NMX_REQUIRE(ld >= H->min_ld && n_rows >= 0 && n_rows < (1ll << 31) / std::max(1, H->a.n_tiles), "bad row layout");
  NMX_REQUIRE(memspace == 0 || memspace == 1, "memspace must be 0 (host) or 1 (device)");
  if (n_rows == 0) return 0;
  int rc = be_set_device(H->device);
  if (rc) return rc;
  be_stream_t s = hip_stream ? (be_stream_t)hip_stream : H->stream;
  if (memspace == 1) {
    if ((rc = proj_launch(proj, rows, ld, (int)n_rows, s))) return rc;
    return be_check_launch();
  }
  // host rows: columns [first_in, min_ld) of every row go over and the grid columns [first_out, min_ld) come back
  const long long w = H->min_ld - H->first_in;
  if ((rc = ensure(H->stage, (size_t)n_rows * w * sizeof(float)))) return rc;
  float* d = (float*)H->stage.p;
  be_h2d_2d_async(d, (size_t)w * sizeof(float), rows + H->first_in, (size_t)ld * sizeof(float), (size_t)w * sizeof(float),
                  (size_t)n_rows, s);
  if ((rc = proj_launch(proj, d - H->first_in, w, (int)n_rows, s))) return rc;
  const long long wo = H->min_ld - H->first_out;
  be_d2h_2d_async(rows + H->first_out, (size_t)ld * sizeof(float), d + (H->first_out - H->first_in), (size_t)w * sizeof(float),
                  (size_t)wo * sizeof(float), (size_t)n_rows, s);
  if ((rc = be_sync(s))) return rc;
  return be_check_launch();
}

int nmx_plan_attach_proj(nmx_plan* plan, nmx_proj* proj) {
  Plan* P = (Plan*)plan;
  if (!P) return nmx_fail(NMX_E_INVALID, "null plan");
  if (proj) {
    const NmxProjHandle* H = (const NmxProjHandle*)proj;
    NMX_REQUIRE(H->device == P->device, "projection and plan live on different devices");
    NMX_REQUIRE(H->min_ld <= (long long)P->d.n_outputs + P->d.n_extra_cols,
                "the projection's columns do not fit the plan's rows (n_outputs + n_extra_cols)");
  }
  P->proj = proj;
  return 0;
}

}  // extern "C"
