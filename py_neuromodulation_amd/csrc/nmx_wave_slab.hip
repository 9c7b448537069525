// nmx_wave_slab.hip -- the sharp-wave list kernel of the long-window mode (NmxSharpArgs::slab_mode): windows whose
// series plus worst-case extrema lists exceed 160 KiB of LDS.  The series stays in LDS, the
// index / state / value lists of nmx_sharp_body live in one slab of device memory per workgroup.  Compiled with
// -DNMX_NT_FIXED=64 -DNMX_SYNC_GLOBAL=1: same item code as nmx_wave.hip, but NMX_SYNC() also waits for the wave's
// global stores -- a translation unit of its own, so that the LDS kernels keep their LDS-only fence.
#if !defined(NMX_NT_FIXED) || !defined(NMX_SYNC_GLOBAL)
#error "compile with -DNMX_NT_FIXED=64 -DNMX_SYNC_GLOBAL=1"
#endif
#include <hip/hip_runtime.h>

#include "nmx_k_sharpwave.h"

extern __shared__ __attribute__((aligned(16))) float nmx_smem_slab[];

// Persistent one-wave workgroups, one slab each: scratch = gridDim.x slabs, whatever the number of hops in the chunk.
// Items are dealt round-robin (item = k gridDim.x + blockIdx.x: neighbouring flagged items go to different
// workgroups); with a flag array a wave tests 64 of its items per step -- one byte per lane, one ballot.
__global__ void __launch_bounds__(64) nmx_kern_sharp_slab(const NmxSharpArgs A, int n_items, const unsigned char* todo) {
  const int lane = (int)(threadIdx.x & 63);
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  float* slab = A.slab + (size_t)b * (size_t)A.slab_floats;
  for (long long k0 = 0; k0 * G + b < n_items; k0 += 64) {
    const long long i = (k0 + lane) * G + b;
    unsigned long long m = __ballot(i < n_items && (todo == nullptr || todo[i] != 0));
    while (m) {
      const int item = (int)((k0 + __ffsll((long long)m) - 1) * G + b);
      m &= m - 1;
      const int fi = item % A.n_filters, r = item / A.n_filters;
      nmx_sharp_item_slab(A, r / A.n_channels, r % A.n_channels, fi, nmx_smem_slab, slab);
      NMX_SYNC();
    }
  }
}

extern "C" void nmx_wave_launch_sharp_slab(const NmxSharpArgs* A, int n_items, const unsigned char* todo, hipStream_t s) {
  if (n_items <= 0 || A->slab_blocks <= 0 || !A->slab) return;
  const int grid = n_items < A->slab_blocks ? n_items : A->slab_blocks;
  NMX_LAUNCH(nmx_kern_sharp_slab, dim3(grid), dim3(64), (size_t)A->lz_lds_floats * 4, s, *A, n_items, todo);
}
