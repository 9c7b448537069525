// nmx_w64.hip -- translation unit of the one-wave FIR kernels (nmx_k_bank_w64*.h): notch, band-pass bank
// (M = 1024 / 1536 channel pairs, M = 2048, M = 4096).  Built ONCE by __graft_entry__.build_lib() with
// -fno-slp-vectorize -DNMX_LDS_ASM=1: complex arithmetic is packed explicitly (inline asm with
// operand modifiers, unpaired ds_read_b64); clang's SLP vectoriser on top of that spills.
// Which launcher runs is the plan's choice (NmxBankW64Args::kernel, be_launch_bank_w64 in nmx_api.hip): no launcher here
// tests whether a shape fits -- the plan asked the predicates beside each kernel's constants.  What depends on the batch
// size (waves per workgroup, grid, the form of the one-channel kernels) is decided here.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "nmx_k_bank_w64.h"
#include "nmx_k_bank_w64p.h"
#include "nmx_k_bank_w64x2.h"
#include "nmx_k_bank_w64c.h"
#include "nmx_k_bank_w64d.h"
#include "nmx_k_bank_w64e.h"

#if !defined(NMX_LDS_ASM)
#error "compile with -DNMX_LDS_ASM=1"
#endif

extern __shared__ __attribute__((aligned(16))) float nmx_smem_w64[];

// Launch geometry of the channel-pair kernels (M = 1024 / 1536 / 2048 and the fused notch + filters): `fixed` floats of
// tables and one tile of `tile` floats per wave, at most `cap` waves per workgroup -- two when the batch is a hop or two, to
// spread the few items over many CUs.  One workgroup per CU; a wave walks `chunk` consecutive (channel pair, window) items.
struct NmxW64PairGeom {
  int nw, grid, chunk, n_windows, n_pairs;
  size_t lds;
};
static NmxW64PairGeom nmx_w64_pair_geom(int fixed, int tile, int cap, int n_items, int C, int n_cu) {
  NmxW64PairGeom g;
  g.n_windows = n_items / C;
  g.n_pairs = g.n_windows * ((C + 1) / 2);
  g.nw = nmx_w64_pair_waves(fixed, tile);
  if (g.nw > cap) g.nw = cap;
  if (g.n_pairs < 2048) g.nw = 2;
  g.lds = (size_t)(fixed + g.nw * tile) * 4;
  g.grid = n_cu > 0 ? n_cu : 256;
  if (g.grid * g.nw > g.n_pairs) g.grid = (g.n_pairs + g.nw - 1) / g.nw;
  g.chunk = (g.n_pairs + g.grid * g.nw - 1) / (g.grid * g.nw);
  return g;
}
static void nmx_w64_note_geom(const NmxW64PairGeom& g) { nmxi_note_pair_geom(g.n_pairs, g.grid, g.nw); }

// register budgets: the FIR-bank instantiation fits 168 VGPRs (3 waves/SIMD, 12 per CU, 5 spilled
// dwords); the notch instantiation (odd-reflection staging) needs the 256-VGPR budget.
__global__ void __launch_bounds__(64, 3) nmx_kern_bank_w64_rd64(const NmxBankW64Args A) {
  const int item = blockIdx.x;
  nmx_bank_w64_item<0, 0, 1>(A, item / A.b.n_channels, item % A.b.n_channels, nmx_smem_w64, nullptr);
}
__global__ void __launch_bounds__(64, 2) nmx_kern_notch_w64_rd64(const NmxBankW64Args A) {
  const int item = blockIdx.x;
  nmx_bank_w64_item<1, 0, 0>(A, item / A.b.n_channels, item % A.b.n_channels, nmx_smem_w64, nullptr);
}

// Persistent variant: one workgroup of `nw` waves per CU; the A/B tables of all filters are
// staged in LDS once per workgroup (instead of being re-fetched from L2 for every item: 27 % of
// the kernel's time), then every wave walks its own items with wave-local fences only.
// HALF = 1: windows of at most 1024 samples -- the upper half of each inverse transform's outputs is never formed.
// Pipelined persistent kernel (nmx_k_bank_w64p.h): the A / B tables are staged INTERLEAVED ((A_k, B_k) pairs: one
// 8-byte read per point), everything else as below.
template <int HALF>
__global__ void __launch_bounds__(64 * 8) nmx_kern_bank_w64pp_rd64(const NmxBankW64Args A0, int n_items, int x_floats) {
  // (kernel-argument pointer laundered once per item: the plan is re-read with s_load, not hoisted into scalar
  // registers that spill to lanes of a VGPR)
  typedef const NmxBankW64Args __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  float* tab = nmx_smem_w64;
  const int n = NMX_W64_N, tab_floats = ((const NmxBankW64Args*)Ap)->b.n_filters * 2 * n;
  {
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    for (int i = threadIdx.x; i < tab_floats; i += blockDim.x) {
      const int fi = i / (2 * n), j = i - fi * 2 * n;
      tab[i] = (j & 1) ? A.Hd[fi][j >> 1] : A.Hs[fi][j >> 1];
    }
    for (int i = threadIdx.x; i < NMX_W64_TWL_FLOATS; i += blockDim.x) tab[tab_floats + i] = A.twl[i];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  float* mine = nmx_smem_w64 + tab_floats + NMX_W64_TWL_FLOATS + wave * x_floats;
#pragma nounroll
  for (int item = blockIdx.x * nw + wave; item < n_items; item += gridDim.x * nw) {
    asm volatile("" : "+s"(Ap));
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    nmx_bank_w64_item_pipe<HALF>(A, item / A.b.n_channels, item % A.b.n_channels, mine, tab);
  }
}

// Notch, four items per workgroup: the filter's A / B tables and the twiddles are staged in LDS once per
// FOUR items (the one-wave-per-workgroup kernel fetches ~27 KB of tables from L2 per item); no item loop,
// so none of the scalar-register pressure of the persistent form.
__global__ void __launch_bounds__(256, 3) nmx_kern_notch_w64q_rd64(const NmxBankW64Args A, int n_items, int x_floats) {
  float* tab = nmx_smem_w64;
  const int n = NMX_W64_N, tab_floats = 2 * n;
  for (int i = threadIdx.x; i < tab_floats; i += 256) tab[i] = i < n ? A.Hs[0][i] : A.Hd[0][i - n];
  for (int i = threadIdx.x; i < NMX_W64_TWL_FLOATS; i += 256) tab[tab_floats + i] = A.twl[i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = blockIdx.x * 4 + wave;
  if (item >= n_items) return;
  nmx_bank_w64_item<1, 1, 0>(A, item / A.b.n_channels, item % A.b.n_channels,
                             nmx_smem_w64 + tab_floats + NMX_W64_TWL_FLOATS + wave * x_floats, tab);
}

// waves of the persistent notch workgroup: ONE workgroup of twelve waves per CU (3 waves / SIMD at 168 VGPRs) shares one
// copy of the 20 KB of tables -- measured on one lease with the reflection table: 12 waves 0.96 ms, 6 (two workgroups per
// CU) 1.15 - 1.20, 4 (only two workgroups fit: 8 waves) 1.22
#ifndef NMX_NOTCH_QP_WAVES
#define NMX_NOTCH_QP_WAVES 12
#endif
// Persistent form of the above: one workgroup per CU (filter tables, twiddles and the reflection table: 20 KB, one
// exchange tile per wave) walks the items -- the tables are staged once
// per workgroup instead of once per four items (the staging + its barrier + the workgroup launch were a quarter of
// the four-item kernel's time).  The kernel-argument pointer is laundered once per iteration so that the plan is
// re-read with s_load instead of being hoisted into (spilled) scalar registers (nmx_wave.hip).
__global__ void __launch_bounds__(64 * NMX_NOTCH_QP_WAVES, 3) nmx_kern_notch_w64qp_rd64(const NmxBankW64Args A0, int n_items,
                                                            int x_floats) {
  typedef const NmxBankW64Args __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  float* tab = nmx_smem_w64;
  const int n = NMX_W64_N, tab_floats = 2 * n;
  {
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    for (int i = threadIdx.x; i < tab_floats; i += 64 * NMX_NOTCH_QP_WAVES) tab[i] = i < n ? A.Hs[0][i] : A.Hd[0][i - n];
    for (int i = threadIdx.x; i < NMX_W64_TWL_FLOATS; i += 64 * NMX_NOTCH_QP_WAVES) tab[tab_floats + i] = A.twl[i];
  }
  unsigned* rtab = (unsigned*)(nmx_smem_w64 + tab_floats + NMX_W64_TWL_FLOATS);   // [16][64] (4 KB)
  nmx_w64_reflect_table(((const NmxBankW64Args*)Ap)->b, rtab, (int)threadIdx.x, 64 * NMX_NOTCH_QP_WAVES);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* mine = nmx_smem_w64 + tab_floats + NMX_W64_TWL_FLOATS + 1024 + wave * x_floats;
#pragma nounroll
  for (int item = blockIdx.x * NMX_NOTCH_QP_WAVES + wave; item < n_items; item += (int)gridDim.x * NMX_NOTCH_QP_WAVES) {
    asm volatile("" : "+s"(Ap));
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    nmx_bank_w64_item<1, 1, 0>(A, item / A.b.n_channels, item % A.b.n_channels, mine, tab, rtab);
    NMX_WAVE_FENCE();
  }
}

// M = 4096 (nmx_k_bank_w64x2.h): persistent workgroups of `nw` waves; LDS = tables of the first n_tab filters,
// pass B / C twiddles, w^k, one exchange tile per wave
template <int HALF>
__global__ void __launch_bounds__(64 * 8) nmx_kern_bank_w64x2_rd64(const NmxBankW64Args A0, int n_items, int x_floats, int n_tab) {
  // (the kernel-argument pointer is laundered once per item: the plan -- eight filters' worth of descriptors -- is then
  // re-read with s_load instead of being hoisted into scalar registers that spill to v_writelane / v_readlane, 108 of
  // them in the first form of this loop)
  typedef const NmxBankW64Args __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  float* tab = nmx_smem_w64;
  const int tab_floats = n_tab * 4096;
  {
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    for (int i = threadIdx.x; i < tab_floats; i += blockDim.x) tab[i] = A.Hs[i >> 12][i & 4095];
    for (int i = threadIdx.x; i < NMX_W64_TWL_FLOATS; i += blockDim.x) tab[tab_floats + i] = A.twl[i];
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) tab[tab_floats + NMX_W64_TWL_FLOATS + i] = A.tw2[i];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  float* mine = nmx_smem_w64 + tab_floats + NMX_W64_TWL_FLOATS + 2048 + wave * x_floats;
#pragma nounroll
  for (int item = blockIdx.x * nw + wave; item < n_items; item += gridDim.x * nw) {
    asm volatile("" : "+s"(Ap));
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    nmx_bank_w64x2_item<HALF>(A, item / A.b.n_channels, item % A.b.n_channels, mine, tab, n_tab);
  }
}

extern "C" void nmx_w64x2_launch_rd64(const NmxBankW64Args* A, int n_items, int n_cu, hipStream_t s) {
  const int nw = NMX_W64X2_WAVES, x_floats = A->lds_floats;
  const int n_tab = nmx_w64x2_lds_tables(x_floats) < A->b.n_filters ? nmx_w64x2_lds_tables(x_floats) : A->b.n_filters;
  const size_t lds = (size_t)(n_tab * 4096 + nmx_w64x2_fixed(x_floats)) * 4;
  int grid = n_cu > 0 ? n_cu : 256;
  if (grid * nw > n_items) grid = (n_items + nw - 1) / nw;
  if (A->b.W <= 2048) NMX_LAUNCH(nmx_kern_bank_w64x2_rd64<1>, dim3(grid), dim3(64 * nw), lds, s, *A, n_items, x_floats, n_tab);
  else NMX_LAUNCH(nmx_kern_bank_w64x2_rd64<0>, dim3(grid), dim3(64 * nw), lds, s, *A, n_items, x_floats, n_tab);
}

// M = 1536, one wave per (window, channel pair) (nmx_k_bank_w64c.h): workgroups of `nw` waves (twelve: three per SIMD at
// <= 168 VGPRs); LDS = the real spectra of all filters, the pass-A twiddles, one 4.5 KiB exchange tile per wave.  A wave walks a CONTIGUOUS run of `chunk` items in the
// order (channel pair, window): consecutive items are consecutive hops of the same two channels, whose windows
// overlap by W - hop samples -- after the first item of a run most of the window comes from L2.
__global__ void __launch_bounds__(64 * 12) nmx_kern_bank_w64c_rd64(const NmxBankW64Args A, int n_windows, int n_pairs, int chunk) {
  float* tab = nmx_smem_w64;
  const int hf = A.b.n_filters * NMX_W64C_H_FLOATS;
  for (int i = threadIdx.x; i < hf; i += blockDim.x) tab[i] = A.hc[i];
  for (int i = threadIdx.x; i < NMX_W64C_TWA_FLOATS; i += blockDim.x) tab[hf + i] = A.twc[i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  NmxW64cLane Ln;
  nmx_w64c_lane_setup(Ln, tab + hf + NMX_W64C_TWA_FLOATS + wave * NMX_W64C_TILE_FLOATS, tab + hf,
                      A.twc + NMX_W64C_TWA_FLOATS, (int)(threadIdx.x & 63));
  const int q0 = (blockIdx.x * nw + wave) * chunk;
  const int q1 = q0 + chunk < n_pairs ? q0 + chunk : n_pairs;
#pragma nounroll
  for (int q = q0; q < q1; ++q) {
    const int cp = q / n_windows;
    nmx_bank_w64c_item(A, q - cp * n_windows, 2 * cp, Ln, tab);
  }
}

// M = 1024, one wave per (window, channel pair) (nmx_k_bank_w64d.h): LDS = real spectra of all filters, pass B / C
// twiddles, one exchange tile per wave; the same contiguous runs of hops per wave
template <int HALF>
__global__ void __launch_bounds__(64 * (HALF ? 12 : 8)) nmx_kern_bank_w64d_rd64(const NmxBankW64Args A, int n_windows,
                                                            int n_pairs, int chunk, int x_floats) {
  float* tab = nmx_smem_w64;
  const int hf = A.b.n_filters * NMX_W64D_H_FLOATS;
  for (int i = threadIdx.x; i < hf; i += blockDim.x) tab[i] = A.hc[i];
  for (int i = threadIdx.x; i < NMX_W64_TWL_FLOATS; i += blockDim.x) tab[hf + i] = A.twl[i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  float* mine = tab + hf + NMX_W64_TWL_FLOATS + wave * x_floats;
  const int q0 = (blockIdx.x * nw + wave) * chunk;
  const int q1 = q0 + chunk < n_pairs ? q0 + chunk : n_pairs;
#pragma nounroll
  for (int q = q0; q < q1; ++q) {
    const int cp = q / n_windows;
    nmx_bank_w64d_item<HALF>(A, q - cp * n_windows, 2 * cp, mine, tab);
  }
}

extern "C" void nmx_w64d_launch_rd64(const NmxBankW64Args* A, int n_items, int n_cu, hipStream_t s) {
  const int x_floats = A->lds_floats;
  // W <= 512: 114 VGPRs, three waves per SIMD fit
  const NmxW64PairGeom g = nmx_w64_pair_geom(nmx_w64d_fixed(A->b.n_filters), x_floats, A->b.W <= 512 ? 12 : 8, n_items, A->b.n_channels, n_cu);
  if (A->b.W <= 512) NMX_LAUNCH(nmx_kern_bank_w64d_rd64<1>, dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk, x_floats);
  else NMX_LAUNCH(nmx_kern_bank_w64d_rd64<0>, dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk, x_floats);
  nmx_w64_note_geom(g);
}

// M = 2048, one wave per (window, channel pair) (nmx_k_bank_w64e.h): PAD = 0 the "same" FIR bank of the filters the
// M = 1536 kernel cannot take, PAD = 1 the notch (odd-reflected window, one filter, the window back to HBM).  LDS = the
// real spectra of the filters, the pass-A twiddles, one 4.5 KiB exchange tile per wave; contiguous runs of hops per wave.
// Seven waves per workgroup, as the 18 KiB tiles allowed: the eighth that LDS now has room for (two on every SIMD, the
// register budget's limit) shortens these kernels alone by ~9 % and takes as much from the kernels on the plan's other
// streams -- the step did not move (profiles/fir_group_exchange.md), so the geometry stays what it was.
#define NMX_W64E_WAVES 7
template <int PAD, int WC = 0, int HC = 0>
__global__ void __launch_bounds__(64 * 8) nmx_kern_bank_w64e_rd64(const NmxBankW64Args A0, int n_windows, int n_pairs, int chunk) {
  // (kernel-argument pointer laundered once per item: the plan is re-read with s_load, not hoisted into scalar
  // registers that spill to lanes of a VGPR)
  typedef const NmxBankW64Args __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  float* tab = nmx_smem_w64;
  const int hf = ((const NmxBankW64Args*)Ap)->b.n_filters * NMX_W64E_H_FLOATS;
  NmxW64cLane Ln;
  unsigned rt[16];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  {
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    for (int i = threadIdx.x; i < hf; i += blockDim.x) tab[i] = A.hc[i];
    for (int i = threadIdx.x; i < NMX_W64E_TWA_FLOATS; i += blockDim.x) tab[hf + i] = A.twc[i];
    nmx_w64c_lane_setup(Ln, tab + hf + NMX_W64E_TWA_FLOATS + wave * NMX_W64E_TILE_FLOATS, tab + hf,
                        A.twc + NMX_W64E_TWA_FLOATS, (int)(threadIdx.x & 63));
    if (PAD && !WC) nmx_w64e_reflect_lane(A.b, (int)(threadIdx.x & 63), rt);
  }
  __syncthreads();
  const int q0 = (blockIdx.x * nw + wave) * chunk;
  const int q1 = q0 + chunk < n_pairs ? q0 + chunk : n_pairs;
#pragma nounroll
  for (int q = q0; q < q1; ++q) {
    asm volatile("" : "+s"(Ap));
    const NmxBankW64Args& A = *(const NmxBankW64Args*)Ap;
    const int cp = q / n_windows;
    nmx_bank_w64e_item<PAD, WC, HC>(A, q - cp * n_windows, 2 * cp, Ln, tab, rt);
  }
}

// The notch with the PAD = 0 filters behind it in ONE item (nmx_k_bank_w64e.h, FUSE): the window the notch stores is the
// window those filters load, in the same registers.  LDS = the filters' spectra, (FUSE = 2: the notch's,) the pass-A
// twiddles, one exchange tile per wave; FUSE = 1 reads the notch's spectrum from global memory (the default since the
// tiles were 18 KiB and its 8 KiB cost a wave; with 4.5 KiB tiles both forms run NMX_W64E_WAVES waves).
template <int WC, int HC, int FUSE>
__global__ void __launch_bounds__(64 * 8) nmx_kern_notch_bank_w64e_rd64(const NmxW64eFusedArgs A0, int n_windows,
                                                            int n_pairs, int chunk) {
  typedef const NmxW64eFusedArgs __attribute__((address_space(4)))* nmx_karg_p;
  nmx_karg_p Ap = (nmx_karg_p)__builtin_amdgcn_kernarg_segment_ptr();
  float* tab = nmx_smem_w64;
  const int hff = ((const NmxW64eFusedArgs*)Ap)->f.b.n_filters * NMX_W64E_H_FLOATS;
  const int hf = hff + (FUSE == 2 ? NMX_W64E_H_FLOATS : 0);
  NmxW64cLane Ln;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  {
    const NmxW64eFusedArgs& A = *(const NmxW64eFusedArgs*)Ap;
    for (int i = threadIdx.x; i < hff; i += blockDim.x) tab[i] = A.f.hc[i];
    if (FUSE == 2)
      for (int i = threadIdx.x; i < NMX_W64E_H_FLOATS; i += blockDim.x) tab[hff + i] = A.n.hg[i];
    for (int i = threadIdx.x; i < NMX_W64E_TWA_FLOATS; i += blockDim.x) tab[hf + i] = A.f.twc[i];
    nmx_w64c_lane_setup(Ln, tab + hf + NMX_W64E_TWA_FLOATS + wave * NMX_W64E_TILE_FLOATS, tab + hf,
                        A.f.twc + NMX_W64E_TWA_FLOATS, (int)(threadIdx.x & 63));
  }
  __syncthreads();
  const int q0 = (blockIdx.x * nw + wave) * chunk;
  const int q1 = q0 + chunk < n_pairs ? q0 + chunk : n_pairs;
#pragma nounroll
  for (int q = q0; q < q1; ++q) {
    asm volatile("" : "+s"(Ap));
    const NmxW64eFusedArgs& A = *(const NmxW64eFusedArgs*)Ap;
    const int cp = q / n_windows;
    nmx_bank_w64e_item<1, WC, HC, FUSE>(A.f, q - cp * n_windows, 2 * cp, Ln, tab, nullptr, &A.n);
  }
}

// the fused launch (the plan's choice: choose_notch_bank_fuse): F and Nn as their own launches would get them (per-call
// fields patched in); g_lds: the notch's spectrum in LDS too
extern "C" void nmx_w64e_launch_fused_rd64(const NmxBankW64Args* F, const NmxBankW64Args* Nn, int g_lds, int n_items, int n_cu,
                                           hipStream_t s) {
  NmxW64eFusedArgs A;
  A.f = *F;
  A.n.x = Nn->b.x; A.n.ch_stride = Nn->b.ch_stride; A.n.win_stride = Nn->b.win_stride; A.n.starts = Nn->b.starts;
  A.n.y_out = Nn->b.y_out; A.n.hg = Nn->hc; A.n.clean_on_load = Nn->b.clean_on_load; A.n.residual = Nn->b.residual;
  const NmxW64PairGeom g = nmx_w64_pair_geom(nmx_w64e_fixed(F->b.n_filters + (g_lds ? 1 : 0)), NMX_W64E_TILE_FLOATS, NMX_W64E_WAVES, n_items,
                                             F->b.n_channels, n_cu);
  if (g_lds) NMX_LAUNCH((nmx_kern_notch_bank_w64e_rd64<1000, 499, 2>), dim3(g.grid), dim3(64 * g.nw), g.lds, s, A, g.n_windows, g.n_pairs, g.chunk);
  else NMX_LAUNCH((nmx_kern_notch_bank_w64e_rd64<1000, 499, 1>), dim3(g.grid), dim3(64 * g.nw), g.lds, s, A, g.n_windows, g.n_pairs, g.chunk);
  nmx_w64_note_geom(g);
}

extern "C" void nmx_w64e_launch_rd64(const NmxBankW64Args* A, int n_items, int n_cu, hipStream_t s) {
  const NmxW64PairGeom g = nmx_w64_pair_geom(nmx_w64e_fixed(A->b.n_filters), NMX_W64E_TILE_FLOATS, NMX_W64E_WAVES, n_items, A->b.n_channels, n_cu);
  if (nmx_w64e_notch_w1000(A->b)) NMX_LAUNCH((nmx_kern_bank_w64e_rd64<1, 1000, 499>), dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk);
  else if (A->b.pad_mode != 0) NMX_LAUNCH(nmx_kern_bank_w64e_rd64<1>, dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk);
  else NMX_LAUNCH(nmx_kern_bank_w64e_rd64<0>, dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk);
  nmx_w64_note_geom(g);
}

extern "C" void nmx_w64c_launch_rd64(const NmxBankW64Args* A, int n_items, int n_cu, hipStream_t s) {
  const NmxW64PairGeom g = nmx_w64_pair_geom(nmx_w64c_fixed(A->b.n_filters), NMX_W64C_TILE_FLOATS, 12, n_items, A->b.n_channels, n_cu);
  NMX_LAUNCH(nmx_kern_bank_w64c_rd64, dim3(g.grid), dim3(64 * g.nw), g.lds, s, *A, g.n_windows, g.n_pairs, g.chunk);
  nmx_w64_note_geom(g);
}

// One channel per M = 2048 transform; `lds`: one item's LDS (the one-wave-per-workgroup kernels).  The form follows the
// batch: >= 4096 items the persistent pipelined bank (nmx_k_bank_w64p.h) where the plan allows it; the notch from 1024 items
// four items per workgroup, from eight items per wave of a full device its persistent form; else a workgroup per item.
extern "C" void nmx_w64_launch_rd64(const NmxBankW64Args* A, int n_items, size_t lds, int n_cu, hipStream_t s) {
  const int x_floats = A->lds_floats;   // per-wave exchange tile (+ scratch)
  if (n_items >= 4096 && A->pipelined) {
    const int nw = NMX_W64P_WAVES, tab_floats = A->b.n_filters * 2 * NMX_W64_N;
    const size_t ldsp = (size_t)(tab_floats + NMX_W64_TWL_FLOATS + nw * x_floats) * 4;
    int grid = n_cu > 0 ? n_cu : 256;
    if (grid * nw > n_items) grid = (n_items + nw - 1) / nw;
    // (W <= 1024: the upper half of every inverse transform's outputs is never formed)
    if (A->b.W <= 1024) NMX_LAUNCH(nmx_kern_bank_w64pp_rd64<1>, dim3(grid), dim3(64 * nw), ldsp, s, *A, n_items, x_floats);
    else NMX_LAUNCH(nmx_kern_bank_w64pp_rd64<0>, dim3(grid), dim3(64 * nw), ldsp, s, *A, n_items, x_floats);
  } else if (A->b.pad_mode != 0 && n_items >= 3 * 256 * 4 * 8) {
    const size_t ldsp = (size_t)(2 * NMX_W64_N + NMX_W64_TWL_FLOATS + 1024 + NMX_NOTCH_QP_WAVES * x_floats) * 4;
    NMX_LAUNCH(nmx_kern_notch_w64qp_rd64, dim3((12 / NMX_NOTCH_QP_WAVES) * 256), dim3(64 * NMX_NOTCH_QP_WAVES), ldsp, s, *A, n_items, x_floats);
  } else if (A->b.pad_mode != 0 && n_items >= 1024) {
    const size_t ldsq = (size_t)(2 * NMX_W64_N + NMX_W64_TWL_FLOATS + 4 * x_floats) * 4;
    NMX_LAUNCH(nmx_kern_notch_w64q_rd64, dim3((n_items + 3) / 4), dim3(256), ldsq, s, *A, n_items, x_floats);
  } else if (A->b.pad_mode == 0) {
    NMX_LAUNCH(nmx_kern_bank_w64_rd64, dim3(n_items), dim3(64), lds, s, *A);
  } else {
    NMX_LAUNCH(nmx_kern_notch_w64_rd64, dim3(n_items), dim3(64), lds, s, *A);
  }
}
