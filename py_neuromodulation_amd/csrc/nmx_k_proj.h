// nmx_k_proj.h -- grid projection (processing/projection.py): the features of the projected channels onto the active
// points of the cortical and subcortical grids, in place in the feature rows.
//
// Reference arithmetic (Projection.project_features): per hop Y = P @ X, X[channel, feature] the (normalised) values of the
// projected channels, P[point, channel] = (1 / d) / sum(1 / d) over the contacts closer than max_dist_mm.  The host resolves
// the key names (projection.py) into
//   gather[k][f]            the row column of feature f of projected channel k
//   ptr / idx / w           the non-zero weights of every active point (CSR: channels k, float64 weights)
//   out_col / out_stride    the row column of (point p, feature f) = out_col[p] + f * out_stride[p]
// A dense product sums 0 x X[k, f] over the contacts out of reach as well: a NaN or an infinity there makes the point NaN.
// The sparse sum reproduces that with a count per group (a grid and its channels: cortex / ECoG, subcortex / LFP, one
// product each): when feature f of the point's group holds more non-finite inputs than the point's own contacts see, the
// point is NaN (IEEE arithmetic of the contacts' terms does the rest).
//
// One workgroup per (row, tile of features): the tile's gathered inputs are staged in LDS once (every input feeds several
// points); every output is a float64 sum over its point's contacts, rounded once.  Consecutive threads take consecutive
// points of one feature: adjacent columns.  Every output column lies behind every input column (nmx_proj_create checks it),
// so the stores of one workgroup never meet the loads of another.
//
// Included by nmx_engine.inc: the HIP build gets the kernel and its launcher, the host emulator (NMX_HOST_EMU) a launcher
// that loops the same item code.
#pragma once

#include "nmx_device.h"

#define NMX_PROJ_NT 256
#define NMX_PROJ_LDS_FLOATS 8192   // staged inputs per workgroup (32 KiB): the feature tile is sized from it
#define NMX_PROJ_MAX_CHAN 12288    // (one feature of that many channels: 48 KiB of LDS)
#define NMX_PROJ_MAX_GROUPS 4

struct NmxProjArgs {
  float* rows;              // [n_rows][ld], in place
  long long ld;
  int n_rows;
  int n_feat, n_chan, n_points;
  int tile, n_tiles;        // features per workgroup, workgroups per row
  const int* gather;        // [n_chan][n_feat]
  const int* ptr;           // [n_points + 1]
  const int* idx;           // [nnz] projected channel of each weight
  const double* w;          // [nnz]
  const int* out_col;       // [n_points]
  const int* out_stride;    // [n_points]
  const int* point_group;   // [n_points]
  int n_groups;
  int group_chan[NMX_PROJ_MAX_GROUPS + 1];   // group g = channels [group_chan[g], group_chan[g + 1])
};

NMX_DEV void nmx_proj_item(const NmxProjArgs& A, int r, int t, float* smem) {
  const int f0 = t * A.tile;
  const int nf = (A.n_feat - f0) < A.tile ? (A.n_feat - f0) : A.tile;
  float* row = A.rows + (long long)r * A.ld;
  float* x = smem;                                  // [n_chan][nf]
  int* bad = (int*)(smem + (size_t)A.n_chan * A.tile);   // [n_groups][nf] non-finite inputs per group and feature
  for (int j = NMX_TID; j < A.n_groups * nf; j += NMX_NT) bad[j] = 0;
  NMX_SYNC();
  const int n_in = A.n_chan * nf;
  for (int i = NMX_TID; i < n_in; i += NMX_NT) {
    const int k = i / nf, j = i - k * nf;
    const float v = row[A.gather[(long long)k * A.n_feat + f0 + j]];
    x[i] = v;
    if (!isfinite(v)) {
      int g = 0;
      while (g + 1 < A.n_groups && k >= A.group_chan[g + 1]) ++g;
#ifdef NMX_HOST_EMU
      bad[g * nf + j] += 1;
#else
      atomicAdd(&bad[g * nf + j], 1);
#endif
    }
  }
  NMX_SYNC();
  const int n_out = A.n_points * nf;
  for (int i = NMX_TID; i < n_out; i += NMX_NT) {
    const int j = i / A.n_points, p = i - j * A.n_points;
    const int e0 = A.ptr[p], e1 = A.ptr[p + 1];
    double s = 0.0;
    int seen = 0;
    for (int e = e0; e < e1; ++e) {
      const float v = x[A.idx[e] * nf + j];
      s += A.w[e] * (double)v;
      seen += isfinite(v) ? 0 : 1;
    }
    row[A.out_col[p] + (long long)(f0 + j) * A.out_stride[p]] = bad[A.point_group[p] * nf + j] > seen ? NAN : (float)s;
  }
}

static inline size_t nmx_proj_lds_bytes(const NmxProjArgs& A) {
  return ((size_t)A.n_chan * A.tile + (size_t)A.n_groups * A.tile) * 4;
}

#ifdef NMX_HOST_EMU
static void be_launch_proj(const NmxProjArgs& A, be_stream_t) {
  std::vector<float> sm(nmx_proj_lds_bytes(A) / 4 + 16);
  for (int r = 0; r < A.n_rows; ++r)
    for (int t = 0; t < A.n_tiles; ++t) nmx_proj_item(A, r, t, sm.data());
}
#else
extern __shared__ __attribute__((aligned(16))) float nmx_smem[];
__global__ void __launch_bounds__(NMX_PROJ_NT) nmx_kern_proj(const NmxProjArgs A) {
  const int item = (int)blockIdx.x;
  nmx_proj_item(A, item / A.n_tiles, item % A.n_tiles, nmx_smem);
}
// one workgroup of 256 threads per (row, feature tile); at most 48 KiB of LDS, below the default limit
static void be_launch_proj(const NmxProjArgs& A, be_stream_t s) {
  if (A.n_rows <= 0) return;
  NMX_LAUNCH(nmx_kern_proj, dim3((unsigned)((long long)A.n_rows * A.n_tiles)), dim3(NMX_PROJ_NT), nmx_proj_lds_bytes(A), s, A);
}
#endif
