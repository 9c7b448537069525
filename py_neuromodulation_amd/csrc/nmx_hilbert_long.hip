// nmx_hilbert_long.hip -- the long-series Hilbert envelope kernel (NMX_HIL_LONG, nmx_k_hilbert_long.h): series up to
// 40 000 samples, split into transforms the LDS machinery takes.  Compiled with -DNMX_BLOCK_FIXED=512: eight waves per
// workgroup (one workgroup holds most of a CU's LDS, so the waves of a CU all come from it), NMX_SYNC() = __syncthreads().
#if !defined(NMX_BLOCK_FIXED) || NMX_BLOCK_FIXED <= 64
#error "compile with -DNMX_BLOCK_FIXED=512"
#endif
#include <hip/hip_runtime.h>

#include "nmx_k_bank_w64.h"

extern __shared__ __attribute__((aligned(16))) float nmx_smem_hl[];

// Persistent workgroups, one slab each: item = k gridDim.x + blockIdx.x.  LDS and slab are reused from item to item.
__global__ void __launch_bounds__(NMX_BLOCK_FIXED) nmx_kern_hilbert_long(const NmxHilbertArgs A, long long n_items) {
  float* slab = A.slab + (size_t)blockIdx.x * (size_t)A.slab_floats;
  for (long long item = (long long)blockIdx.x; item < n_items; item += (long long)gridDim.x) {
    nmx_hilbert_long_item(A, item, nmx_smem_hl, slab);
    NMX_SYNC();
  }
}

extern "C" void nmx_hilbert_long_launch(const NmxHilbertArgs* A, long long n_items, hipStream_t s) {
  if (n_items <= 0 || A->slab_blocks <= 0 || !A->slab) return;
  const int grid = (int)(n_items < (long long)A->slab_blocks ? n_items : (long long)A->slab_blocks);
  NMX_LAUNCH(nmx_kern_hilbert_long, dim3(grid), dim3(NMX_BLOCK_FIXED), (size_t)A->lds_floats * 4, s, *A, n_items);
}
