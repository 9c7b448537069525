// nmx_timeosc_long.hip -- the long-window time / oscillatory kernel (NMX_TO_LONG, nmx_k_timeosc_long.h): windows up to
// 40 000 samples, FFT / Welch segments up to the window.  Compiled with -DNMX_BLOCK_FIXED=512: eight waves per workgroup
// (one workgroup fills a CU's LDS, so the waves of a CU all come from it), NMX_SYNC() = __syncthreads(), which also
// orders the workgroup's global stores to its slab.  A plan with STFT launches nmx_kern_timeosc_long_stft<class>: the
// segment class (NMX_TOL_STFT_*) is a compile-time constant, so the kernel of plans without STFT holds none of that code.
#if !defined(NMX_BLOCK_FIXED) || NMX_BLOCK_FIXED <= 64
#error "compile with -DNMX_BLOCK_FIXED=512"
#endif
#include <hip/hip_runtime.h>

#include "nmx_k_timeosc.h"

extern __shared__ __attribute__((aligned(16))) float nmx_smem_tol[];

// Persistent workgroups, one slab each: item = k gridDim.x + blockIdx.x.  LDS and slab are reused from item to item.
__global__ void __launch_bounds__(NMX_BLOCK_FIXED) nmx_kern_timeosc_long(const NmxTimeOscArgs A, int n_items) {
  float* slab = A.slab ? A.slab + (size_t)blockIdx.x * (size_t)A.slab_floats : nullptr;
  for (int item = (int)blockIdx.x; item < n_items; item += (int)gridDim.x) {
    nmx_time_osc_long_item(A, item / A.n_channels, item % A.n_channels, nmx_smem_tol, slab, NMX_TOL_STFT_NONE);
    NMX_SYNC();
  }
}

template <int CLS>
__global__ void __launch_bounds__(NMX_BLOCK_FIXED) nmx_kern_timeosc_long_stft(const NmxTimeOscArgs A, int n_items) {
  float* slab = A.slab ? A.slab + (size_t)blockIdx.x * (size_t)A.slab_floats : nullptr;
  for (int item = (int)blockIdx.x; item < n_items; item += (int)gridDim.x) {
    nmx_time_osc_long_item(A, item / A.n_channels, item % A.n_channels, nmx_smem_tol, slab, CLS);
    NMX_SYNC();
  }
}

extern "C" void nmx_timeosc_long_launch(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  if (n_items <= 0 || A->slab_blocks <= 0 || (A->long_spec_slab && !A->slab)) return;
  const int grid = n_items < A->slab_blocks ? n_items : A->slab_blocks;
  const dim3 g(grid), b(NMX_BLOCK_FIXED);
  const size_t lds = (size_t)A->lds_floats * 4;
  switch (A->long_stft) {
    case NMX_TOL_STFT_NONE: NMX_LAUNCH(nmx_kern_timeosc_long, g, b, lds, s, *A, n_items); return;
    case NMX_TOL_STFT_WAVE500: NMX_LAUNCH(nmx_kern_timeosc_long_stft<NMX_TOL_STFT_WAVE500>, g, b, lds, s, *A, n_items); return;
    case NMX_TOL_STFT_DIRECT: NMX_LAUNCH(nmx_kern_timeosc_long_stft<NMX_TOL_STFT_DIRECT>, g, b, lds, s, *A, n_items); return;
    case NMX_TOL_STFT_LDS: NMX_LAUNCH(nmx_kern_timeosc_long_stft<NMX_TOL_STFT_LDS>, g, b, lds, s, *A, n_items); return;
    case NMX_TOL_STFT_SPLIT: NMX_LAUNCH(nmx_kern_timeosc_long_stft<NMX_TOL_STFT_SPLIT>, g, b, lds, s, *A, n_items); return;
  }
}
