// nmx_wave.hip -- translation unit of the one-item-per-WAVE kernels (burst statistics, sharp-wave
// analysis).  Compiled with -DNMX_NT_FIXED=64: inside an item NMX_TID is the lane, NMX_NT is the
// constant 64, NMX_SYNC() is a wave-local LDS fence and the block reductions are shuffle-only.
// A workgroup carries `k` independent waves (own LDS slice each), so there is no workgroup barrier
// anywhere in these kernels.
#ifndef NMX_NT_FIXED
#error "compile with -DNMX_NT_FIXED=64"
#endif
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#include "nmx_k_bursts.h"
#include "nmx_k_bank_w64.h"
#include "nmx_k_burst_stat_reg.h"
#include "nmx_k_scan.h"
#include "nmx_k_td.h"
#include "nmx_k_timeosc_w1000.h"
#include "nmx_k_timeosc_w510.h"
#include "nmx_k_sharpwave.h"

extern __shared__ __attribute__((aligned(16))) float nmx_smem_wave[];

// One-wave-per-item kernels can be launched with several waves per workgroup (each wave its own item and LDS slice, no
// barrier between them).  Measured on the MI355X (profiles/r04_waves_per_wg.txt): the sharp-wave kernels -- 30+ KB of
// code, waves at unrelated program counters -- gain 13 % (1000-sample windows) to 24 % (BASELINE config 5) with TWO
// waves per workgroup, which start together and fetch the same instructions; four are no better; the transform kernels
// (time / oscillatory, Hilbert) do not gain, and lose when they overlap the bursts chain.  `dflt` is that choice,
// NMX_WAVES_PER_WG = 1 .. 4 overrides it for every kernel.
static int waves_per_wg(size_t lds_one, int dflt = 1) {
  const char* v = getenv("NMX_WAVES_PER_WG");   // (read per launch: the GPU tests switch it inside one process)
  const int k = (v && atoi(v) >= 1 && atoi(v) <= 4) ? atoi(v) : 0;
  int kk = k ? k : dflt;
  while (kk > 1 && lds_one * kk > 64 * 1024) --kk;
  return kk;
}
// (item, LDS slice) of this wave in a launch of `blockDim.x / 64` waves per workgroup; slice in floats
#define NMX_WAVE_ITEM(item, smem, n_items, slice)                                                   \
  const int wave_ = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                        \
  const int item = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave_;                                \
  if (item >= (n_items)) return;                                                                    \
  float* smem = nmx_smem_wave + wave_ * (slice)

__global__ void __launch_bounds__(256) nmx_kern_burst_stat(const NmxBurstStatArgs A, int n_items, int slice) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform -> SGPR
  const int item = blockIdx.x * (blockDim.x >> 6) + wave;
  if (item >= n_items) return;
  const int bi = item % A.n_bands, r = item / A.n_bands;
  nmx_burst_stat_item(A, r / A.n_channels, r % A.n_channels, bi, nmx_smem_wave + wave * slice);
}

// the envelope of one item in the registers of its wave (nmx_k_burst_stat_reg.h): W % 4 == 0, W <= 64 CH; no LDS
// SPARSE: A.full tells which rows the Hilbert kernel stored whole; the others are six zeros without a load of the row
template <int CH, bool SPARSE = false>
__global__ void __launch_bounds__(256) nmx_kern_burst_stat_reg(const NmxBurstStatArgs A, int n_items) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  const int bi = item % A.n_bands, r = item / A.n_bands;
  nmx_burst_stat_item_reg<CH, SPARSE>(A, r / A.n_channels, r % A.n_channels, bi);
}

// the tile scan (NmxBurstStatArgs::scan_tile): the envelope stays in memory, a wave's LDS slice holds one tile of it
__global__ void __launch_bounds__(256) nmx_kern_burst_stat_scan(const NmxBurstStatArgs A, int n_items) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  const int bi = item % A.n_bands, r = item / A.n_bands;
  nmx_burst_stat_scan_item(A, r / A.n_channels, r % A.n_channels, bi, nmx_smem_wave + wave * A.lds_floats);
}

__global__ void __launch_bounds__(256) nmx_kern_sharp(const NmxSharpArgs A, int n_items, int slice) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform -> SGPR
  const int item = blockIdx.x * (blockDim.x >> 6) + wave;
  if (item >= n_items) return;
  const int fi = item % A.n_filters, r = item / A.n_filters;
  nmx_sharp_item(A, r / A.n_channels, r % A.n_channels, fi, nmx_smem_wave + wave * slice);
}

// threshold walk, steady regime: one wave per (channel, band); NR = registers per lane for a hop's new samples, LL = the
// top-K list in LDS for the launch (nmx_k_bursts.h)
template <int NR, bool LL>
__global__ void __launch_bounds__(64) nmx_kern_burst_thr_wave(const NmxBurstThrArgs A) {
  __builtin_amdgcn_s_setprio(3);   // sequential and on the critical path: win issue arbitration
  const int item = blockIdx.x;
  nmx_burst_thr_wave_item<NR, LL>(A, item / A.n_bands, item % A.n_bands, nmx_smem_wave);
}

// nr, list_lds, lds: the plan's constants and the schedule's verdict for this launch (nmx_burst_walk_plan, nmx_burst_walk_schedule)
extern "C" void nmx_wave_launch_burst_thr(const NmxBurstThrArgs* A, int n_items, int nr, bool list_lds, size_t lds, hipStream_t s) {
  // (<2, false>: K / 64 block counters of the flush -- beyond ~639 000 list entries the working set passes 64 KiB.  The arms
  // stand in the order the three instantiations have always been named in: it is the order the compiler emits them in)
  if (nr == 2 && list_lds) NMX_LAUNCH((nmx_kern_burst_thr_wave<2, true>), dim3(n_items), dim3(64), lds, s, *A);
  else if (nr != 2) NMX_LAUNCH((nmx_kern_burst_thr_wave<4, false>), dim3(n_items), dim3(64), lds, s, *A);
  else NMX_LAUNCH((nmx_kern_burst_thr_wave<2, false>), dim3(n_items), dim3(64), lds, s, *A);
}

// Hilbert envelope of length-1000 series, one wave per series (wave-level 500-point transforms)
__global__ void __launch_bounds__(256) nmx_kern_hilbert_w500(const NmxHilbertArgs A, int n_items) {
  NMX_WAVE_ITEM(item, smem, n_items, NMX_W500_LDS_FLOATS);
  nmx_hilbert_w500_item<false>(A, (long long)item, smem);
}
// ... rows below the bursts chain's threshold floor leave only their tail (NmxHilbertArgs::full)
__global__ void __launch_bounds__(256) nmx_kern_hilbert_w500_sparse(const NmxHilbertArgs A, int n_items) {
  NMX_WAVE_ITEM(item, smem, n_items, NMX_W500_LDS_FLOATS);
  nmx_hilbert_w500_item<true>(A, (long long)item, smem);
}

extern "C" void nmx_wave_launch_hilbert_w500(const NmxHilbertArgs* A, long long n_items, hipStream_t s) {
  const int k = waves_per_wg((size_t)NMX_W500_LDS_FLOATS * 4);
  const dim3 grid((unsigned)((n_items + k - 1) / k)), block(64 * k);
  if (A->full) NMX_LAUNCH(nmx_kern_hilbert_w500_sparse, grid, block, (size_t)NMX_W500_LDS_FLOATS * 4 * k, s, *A, (int)n_items);
  else NMX_LAUNCH(nmx_kern_hilbert_w500, grid, block, (size_t)NMX_W500_LDS_FLOATS * 4 * k, s, *A, (int)n_items);
}

// Hilbert envelope of length-2000 series (BASELINE config 3), one wave per series, four per workgroup (16 KB of LDS each)
__global__ void __launch_bounds__(256) nmx_kern_hilbert_w1000(const NmxHilbertArgs A, long long n_items) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  nmx_hilbert_w1000_item<false>(A, item, nmx_smem_wave + wave * NMX_W1000_LDS_FLOATS);
}
__global__ void __launch_bounds__(256) nmx_kern_hilbert_w1000_sparse(const NmxHilbertArgs A, long long n_items) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  nmx_hilbert_w1000_item<true>(A, item, nmx_smem_wave + wave * NMX_W1000_LDS_FLOATS);
}

extern "C" void nmx_wave_launch_hilbert_w1000(const NmxHilbertArgs* A, long long n_items, hipStream_t s) {
  const dim3 grid((unsigned)((n_items + 3) / 4));
  if (A->full) NMX_LAUNCH(nmx_kern_hilbert_w1000_sparse, grid, dim3(256), (size_t)4 * NMX_W1000_LDS_FLOATS * 4, s, *A, n_items);
  else NMX_LAUNCH(nmx_kern_hilbert_w1000, grid, dim3(256), (size_t)4 * NMX_W1000_LDS_FLOATS * 4, s, *A, n_items);
}

// time-domain + FFT / Welch / STFT band means of the default shape, one wave per (window, channel)
template <int NB, unsigned SPEC = 0>
__global__ void __launch_bounds__(256) nmx_kern_timeosc_w1000(const NmxTimeOscArgs A, int n_items, int slice) {
  NMX_WAVE_ITEM(item, smem, n_items, slice);
  const int w = nmx_uniform_i(item / A.n_channels), c = nmx_uniform_i(item % A.n_channels);
  NmxW500TwReg T;
  T.load(A.w500_tab, (int)(threadIdx.x & 63));
  NmxTdRegs R;
  nmx_td_load<1000>(A, w, c, R);
  nmx_timeosc_w1000_body<NB, false, NmxW500TwReg, false, SPEC>(A, w, c, R, T, smem);
}

// The same without an STFT and with low bands only (nmx_timeosc_w1000_low_ok: the default 4 - 35 Hz bands, BASELINE
// config[1]): PERSISTENT waves (one-wave workgroups, grid = what the chip holds at once) walk the items with stride
// gridDim, and the 16-byte loads of a wave's NEXT window are issued before it works on the current one -- the HBM
// latency of a window (4 KB per wave, distinct per item in SURVEY 8d's Mode A) hides behind the arithmetic of the item
// instead of idling the wave (one-item-per-workgroup form: SQ_WAIT_ANY 45 % of the wave cycles).  What it takes:
//   * vmcnt retires IN ORDER, so the item must not wait for ANY vector-memory load issued after the prefetch: the small
//     loads of the current item (successors, row ends) go out before it, the real-transform twiddles of the bins come
//     from a 102-entry LDS copy, nothing is spilled (3 waves per SIMD: 168 VGPRs), and the prefetch is UNCONDITIONAL
//     (a load issued on some paths only forces s_waitcnt vmcnt(0) at the next use of anything loaded earlier);
//   * the plan (band tables, output columns: ~100 dwords) must NOT be hoisted out of the item loop into scalar
//     registers -- it does not fit, and spilled scalars come back as v_readlane VALU instructions (500 of them in a
//     first build): the kernel-argument pointer is laundered once per iteration, so every use re-reads its dwords with
//     s_load from the constant cache, as the one-item-per-workgroup kernel does.
//   * SPEC: the kernel is also built for two fixed feature sets (nmx_k_timeosc_w1000.h: NMX_TOW_SPEC_*): with the
//     feature tests folded away an item is ~120 scalar instructions and branches shorter, and those share the wave's
//     issue slots with everything else.
template <int NB, unsigned SPEC = 0>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 4)))
nmx_kern_timeosc_w1000_low(const NmxTimeOscArgs A0, int n_items) {
  typedef const NmxTimeOscArgs __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  const NmxTimeOscArgs& A = *(const NmxTimeOscArgs*)Ap;
  const int lane = (int)(threadIdx.x & 63);
  NmxW500TwReg T;
  T.load(A.w500_tab, lane);
  {
    const float2* twr = (A.fft.enabled ? A.fft : A.welch).fft.twr;
    float2* twl = (float2*)(nmx_smem_wave + NMX_TOW_LOW_TWL_OFF);
    twl[lane] = twr[lane];
    if (lane < 38) twl[64 + lane] = twr[64 + lane];
  }
  const int C = A.n_channels, step = (int)gridDim.x;
  int item = (int)blockIdx.x;
  if (item >= n_items) return;
  NmxTdRegs R;
  nmx_f4 Xn[4];
  int w = nmx_uniform_i(item / C), c = nmx_uniform_i(item - w * C);
  nmx_td_load_x<1000>(A, w, c, R);
  NMX_WAVE_FENCE();
#pragma nounroll
  for (;;) {
    const int nxt = item + step;
    int wn = 0, cn = 0;
    nmx_td_rest_from_x<1000>(R);
    {
      const int pf = nxt < n_items ? nxt : item;   // (the last iteration re-reads its own item)
      wn = nmx_uniform_i(pf / C); cn = nmx_uniform_i(pf - wn * C);
      NmxTdRegs Rn;
      nmx_td_load_x<1000>(A, wn, cn, Rn);
      Xn[0] = Rn.x[0]; Xn[1] = Rn.x[1]; Xn[2] = Rn.x[2]; Xn[3] = Rn.x[3];
    }
    asm volatile("" : "+s"(Ap));
    nmx_timeosc_w1000_body<NB, true, NmxW500TwReg, false, SPEC>(*(const NmxTimeOscArgs*)Ap, w, c, R, T, nmx_smem_wave);
    NMX_WAVE_FENCE();
    if (nxt >= n_items) break;
    item = nxt; w = wn; c = cn;
    R.x[0] = Xn[0]; R.x[1] = Xn[1]; R.x[2] = Xn[2]; R.x[3] = Xn[3];
  }
}


// the persistent form (nmx_timeosc_w1000_low_ok).  Resident waves per CU: 12, 3 per SIMD (168 VGPRs).  The channel of a
// wave's items stays fixed -- and with it the XCD whose L2 holds the overlapping windows -- when the stride is a multiple
// of the channel count
extern "C" void nmx_wave_launch_timeosc_w1000_low(const NmxTimeOscArgs* A, int n_items, int n_cu, hipStream_t s) {
  int grid = n_cu * 12;
  const int C = A->n_channels;
  if (grid > C && grid % C) grid -= grid % C;
  if (grid > n_items) grid = n_items;
  const size_t lds = (size_t)NMX_TOW_LOW_LDS_FLOATS * 4;
  const unsigned spec = nmx_tow_spec(*A);
  // (the SPEC masks are reported as the numbers the profiler prints, not as the macros' names)
  static_assert(NMX_TOW_SPEC_C2 == 65809u && NMX_TOW_SPEC_DEFAULT == 196915u && NMX_TOW_SPEC_ALL == 196923u, "reported kernel names");
  if (A->n_bands <= 4 && spec == NMX_TOW_SPEC_C2)
    NMX_LAUNCH_AS("nmx_kern_timeosc_w1000_low<4, 65809u>", (nmx_kern_timeosc_w1000_low<4, NMX_TOW_SPEC_C2>), dim3(grid), dim3(64), lds, s, *A, n_items);
  else if (A->n_bands <= 4 && spec == NMX_TOW_SPEC_DEFAULT)
    NMX_LAUNCH_AS("nmx_kern_timeosc_w1000_low<4, 196915u>", (nmx_kern_timeosc_w1000_low<4, NMX_TOW_SPEC_DEFAULT>), dim3(grid), dim3(64), lds, s, *A, n_items);
  else if (A->n_bands <= 4) NMX_LAUNCH(nmx_kern_timeosc_w1000_low<4>, dim3(grid), dim3(64), lds, s, *A, n_items);
  else NMX_LAUNCH(nmx_kern_timeosc_w1000_low<8>, dim3(grid), dim3(64), lds, s, *A, n_items);
}

extern "C" void nmx_wave_launch_timeosc_w1000(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  const size_t lds = (size_t)(A->stft.enabled ? NMX_TOW_LDS_FLOATS : NMX_TOW_LDS_FLOATS_NOSTFT) * 4;
  const int k = waves_per_wg(lds);
  const dim3 grid((unsigned)((n_items + k - 1) / k)), block(64 * k);
  const int slice = (int)(lds / 4);
  if (A->n_bands <= 4 && nmx_tow_spec(*A) == NMX_TOW_SPEC_ALL)   // the headline set: feature tests folded (the mask reported as its number, as above)
    NMX_LAUNCH_AS("nmx_kern_timeosc_w1000<4, 196923u>", (nmx_kern_timeosc_w1000<4, NMX_TOW_SPEC_ALL>), grid, block, lds * k, s, *A, n_items, slice);
  else if (A->n_bands <= 4) NMX_LAUNCH(nmx_kern_timeosc_w1000<4>, grid, block, lds * k, s, *A, n_items, slice);
  else NMX_LAUNCH(nmx_kern_timeosc_w1000<8>, grid, block, lds * k, s, *A, n_items, slice);
}

// The windows the matrix-pipe kernel (nmx_k_specmm.h) flagged -- a NaN or an infinity among the samples: it does not clean
// on load; a single-pass variance that cancels beyond NMX_SMM_CANCEL -- through the wave-level kernel's item code, which
// cleans and sums in two passes.  One 16-bit mask per tile of that kernel (16
// consecutive windows of a channel, tile = group * n_channels + channel); a wave looks at 64 masks at a time; a clean
// recording never sets a bit.
template <int NB>
__global__ void __launch_bounds__(64) nmx_kern_timeosc_w1000_todo(const NmxTimeOscArgs A, int n_items) {
  const int lane = (int)(threadIdx.x & 63);
  const int C = A.n_channels, n_windows = n_items / C, n_tiles = ((n_windows + 15) / 16) * C;
  NmxW500TwReg T;
  bool loaded = false;
  for (int base = (int)blockIdx.x * 64; base < n_tiles; base += (int)gridDim.x * 64) {
    const int i = base + lane;
    const unsigned mine = i < n_tiles ? A.todo[i] : 0u;
    unsigned long long m = __ballot(mine != 0u);
    while (m) {
      const int src = (int)__ffsll((long long)m) - 1;
      m &= m - 1;
      const int tile = base + src;
      unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)mine, src);
      const int g = tile / C, c = nmx_uniform_i(tile - g * C);
      while (bits) {
        const int j = __ffs((int)bits) - 1;
        bits &= bits - 1;
        if (!loaded) { T.load(A.w500_tab, lane); loaded = true; }
        const int w = nmx_uniform_i(16 * g + j);
        NmxTdRegs R;
        nmx_td_load<1000>(A, w, c, R);
        nmx_timeosc_w1000_body<NB, false, NmxW500TwReg, false, 0>(A, w, c, R, T, nmx_smem_wave);
        NMX_WAVE_FENCE();
      }
    }
  }
}
extern "C" void nmx_wave_launch_timeosc_w1000_todo(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  const size_t lds = (size_t)NMX_TOW_LDS_FLOATS_NOSTFT * 4;
  const int n_windows = n_items / A->n_channels, n_tiles = ((n_windows + 15) / 16) * A->n_channels;
  const int blocks = (n_tiles + 63) / 64;
  const int grid = blocks < 256 * 8 ? blocks : 256 * 8;
  // (reported without the band-count argument: one name behind the matrix-pipe kernel's, whatever the plan)
  if (A->n_bands <= 4) NMX_LAUNCH_AS("nmx_kern_timeosc_w1000_todo", nmx_kern_timeosc_w1000_todo<4>, dim3(grid), dim3(64), lds, s, *A, n_items);
  else NMX_LAUNCH_AS("nmx_kern_timeosc_w1000_todo", nmx_kern_timeosc_w1000_todo<8>, dim3(grid), dim3(64), lds, s, *A, n_items);
}

// STFT with 500-sample segments on windows of other lengths (<= 2048), the only time / oscillatory feature
template <int NB>
__global__ void __launch_bounds__(256) nmx_kern_timeosc_stft500(const NmxTimeOscArgs A, int n_items) {
  NMX_WAVE_ITEM(item, smem, n_items, NMX_TOS_LDS_FLOATS);
  nmx_timeosc_stft500_item<NB>(A, item / A.n_channels, item % A.n_channels, smem);
}
extern "C" void nmx_wave_launch_timeosc_stft500(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  const int k = waves_per_wg((size_t)NMX_TOS_LDS_FLOATS * 4);
  const dim3 grid((unsigned)((n_items + k - 1) / k)), block(64 * k);
  if (A->n_bands <= 4) NMX_LAUNCH(nmx_kern_timeosc_stft500<4>, grid, block, (size_t)NMX_TOS_LDS_FLOATS * 4 * k, s, *A, n_items);
  else NMX_LAUNCH(nmx_kern_timeosc_stft500<8>, grid, block, (size_t)NMX_TOS_LDS_FLOATS * 4 * k, s, *A, n_items);
}

// 510-sample transforms (17 ms at 30 kHz): prime-factor transform per wave (nmx_k_timeosc_w510.h)
#ifndef NMX_W510_WAVES   // resident waves per SIMD the kernel is compiled for (4: 127 VGPRs, measured 6 % faster than 3)
#define NMX_W510_WAVES 4
#endif
#if NMX_W510_WAVES
#define NMX_W510_WPE __attribute__((amdgpu_waves_per_eu(NMX_W510_WAVES, NMX_W510_WAVES)))
#else
#define NMX_W510_WPE
#endif
template <int NB>
__global__ void __launch_bounds__(256) NMX_W510_WPE nmx_kern_timeosc_w510(const NmxTimeOscArgs A0, int n_items, int slice) {
  NMX_WAVE_ITEM(item, smem, n_items, slice);
  // (the plan through the kernel-argument segment pointer: the item launders it between its phases)
  typedef const NmxTimeOscArgs __attribute__((address_space(4)))* nmx_karg_p;
  const NmxTimeOscArgs& A = *(const NmxTimeOscArgs*)(nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  nmx_timeosc_w510_item<NB>(A, A.w510_tab, item / A.n_channels, item % A.n_channels, smem);
}
extern "C" void nmx_wave_launch_timeosc_w510(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  const int slice = NMX_TO510_LDS_FLOATS(A->W);
  const int k = waves_per_wg((size_t)slice * 4);
  const dim3 grid((unsigned)((n_items + k - 1) / k)), block(64 * k);
  if (A->n_bands <= 4) NMX_LAUNCH(nmx_kern_timeosc_w510<4>, grid, block, (size_t)slice * 4 * k, s, *A, n_items, slice);
  else NMX_LAUNCH(nmx_kern_timeosc_w510<8>, grid, block, (size_t)slice * 4 * k, s, *A, n_items, slice);
}

// register-resident scan (Hjorth / Raw / LineLength only): four waves per workgroup, no LDS
__global__ void __launch_bounds__(256) nmx_kern_scan(const NmxTimeOscArgs A, int n_items, int n_windows, int order) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  if (order) nmx_td_item(A, item % n_windows, item / n_windows);
  else nmx_td_item(A, item / A.n_channels, item % A.n_channels);
}

extern "C" void nmx_wave_launch_scan(const NmxTimeOscArgs* A, int n_items, hipStream_t s) {
  const int order = 0;
  NMX_LAUNCH(nmx_kern_scan, dim3((n_items + 3) / 4), dim3(256), 0, s, *A, n_items, n_items / A->n_channels, order);
}

// dense-first launch: compact LDS layout (more waves per CU); overflowing items are flagged
__global__ void __launch_bounds__(256) nmx_kern_sharp_dense(const NmxSharpArgs A, int n_items, int slice) {
  NMX_WAVE_ITEM(item, smem, n_items, slice);
  const int fi = item % A.n_filters, r = item / A.n_filters;
  nmx_sharp_item_dense(A, r / A.n_channels, r % A.n_channels, fi, (long long)item, smem);
}

// (the list kernel of the long-window kinds: nmx_wave_slab.hip)
extern "C" void nmx_wave_launch_sharp_dense(const NmxSharpArgs* A, int n_items, hipStream_t s) {
  const int slice = (A->dz_lds_floats + 3) & ~3;   // (NMX_SHARP_DENSE_SLAB: the series alone is beyond 64 KiB)
  const int k = waves_per_wg((size_t)slice * 4, 2);
  NMX_LAUNCH(nmx_kern_sharp_dense, dim3((unsigned)((n_items + k - 1) / k)), dim3(64 * k), (size_t)slice * 4 * k, s, *A, n_items, slice);
}

// items the fused bank kernel could not finish (more than 128 extrema of a kind): generic list code.
// Persistent waves walk the flag array; on the bench workload no flag is ever set.
// (64 flags per wave and step -- one byte per lane, one ballot -- instead of one dependent load per flag: the scan of
// 524 288 clear flags took 0.3 ms of the side stream)
__global__ void __launch_bounds__(64) nmx_kern_sharp_todo(const NmxSharpArgs A, int n_items, const unsigned char* todo) {
  const int lane = (int)(threadIdx.x & 63);
  for (int base = (int)blockIdx.x * 64; base < n_items; base += (int)gridDim.x * 64) {
    const int i = base + lane;
    unsigned long long m = __ballot(i < n_items && todo[i] != 0);
    while (m) {
      const int item = base + (int)__ffsll((long long)m) - 1;
      m &= m - 1;
      const int fi = item % A.n_filters, r = item / A.n_filters;
      nmx_sharp_item(A, r / A.n_channels, r % A.n_channels, fi, nmx_smem_wave);
      NMX_SYNC();
    }
  }
}

extern "C" void nmx_wave_launch_sharp_todo(const NmxSharpArgs* A, int n_items, size_t lds, const unsigned char* todo,
                                           hipStream_t s) {
  const int blocks = (n_items + 63) / 64;
  const int grid = blocks < 256 * 14 ? blocks : 256 * 14;
  NMX_LAUNCH(nmx_kern_sharp_todo, dim3(grid), dim3(64), lds, s, *A, n_items, todo);
}

extern "C" void nmx_wave_launch_burst_stat(const NmxBurstStatArgs* A, NmxBurstStatKind kind, int n_items, size_t lds, hipStream_t s) {
  const dim3 grid4((n_items + 3) / 4);
  switch (kind) {   // (the register forms: no LDS; the sparse ones report `_sparse<CH>`, the name the kernel-choice tests know them by)
    case NMX_BSTAT_REG16_SPARSE: NMX_LAUNCH_AS("nmx_kern_burst_stat_reg_sparse<16>", (nmx_kern_burst_stat_reg<16, true>), grid4, dim3(256), 0, s, *A, n_items); return;
    case NMX_BSTAT_REG16: NMX_LAUNCH(nmx_kern_burst_stat_reg<16>, grid4, dim3(256), 0, s, *A, n_items); return;
    case NMX_BSTAT_REG32_SPARSE: NMX_LAUNCH_AS("nmx_kern_burst_stat_reg_sparse<32>", (nmx_kern_burst_stat_reg<32, true>), grid4, dim3(256), 0, s, *A, n_items); return;
    case NMX_BSTAT_REG32: NMX_LAUNCH(nmx_kern_burst_stat_reg<32>, grid4, dim3(256), 0, s, *A, n_items); return;
    case NMX_BSTAT_SCAN: NMX_LAUNCH(nmx_kern_burst_stat_scan, grid4, dim3(256), (size_t)A->lds_floats * 4 * 4, s, *A, n_items); return;
    case NMX_BSTAT_GENERIC: break;
  }
  const int k = waves_per_wg(lds);
  const int slice = (int)((lds / 4 + 3) & ~(size_t)3);
  NMX_LAUNCH(nmx_kern_burst_stat, dim3((n_items + k - 1) / k), dim3(64 * k), (size_t)slice * 4 * k, s, *A, n_items, slice);
}

extern "C" void nmx_wave_launch_sharp(const NmxSharpArgs* A, int n_items, size_t lds, hipStream_t s) {
  const int k = waves_per_wg(lds, 2);
  const int slice = (int)((lds / 4 + 3) & ~(size_t)3);
  NMX_LAUNCH(nmx_kern_sharp, dim3((n_items + k - 1) / k), dim3(64 * k), (size_t)slice * 4 * k, s, *A, n_items, slice);
}
