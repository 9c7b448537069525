// nmx_common.h -- shared host/device definitions of the nmx engine (gfx950 / CDNA4).
//
// Device code is written in "phase" style: every cooperative step is a loop
//     for (int j = NMX_TID; j < m; j += NMX_NT) { ... }   followed by NMX_SYNC()
// plus block reductions.  One workgroup processes one item ((channel, window) or
// (channel, band)); all staging happens in LDS.  Compiling with -DNMX_HOST_EMU maps
// NMX_TID/NMX_NT to 0/1 and NMX_SYNC to a no-op so the SAME source runs single-threaded
// under g++; that build exists only for tests/ (kernel-logic checks in a container that
// has no GPU) and is never part of libnmx.so -- the product has no CPU path.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef NMX_HOST_EMU
struct float2 {
  float x, y;
};
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
#define NMX_DEV static inline
#define NMX_DEVM inline            /* member functions */
#define NMX_TID 0
#define NMX_NT 1
#define NMX_SYNC() ((void)0)
#define NMX_GLOBAL_FENCE() ((void)0)
#define NMX_RESTRICT
#else
#include <hip/hip_runtime.h>
#include <atomic>
#define NMX_DEV __device__ __forceinline__
#define NMX_DEVM __device__ __forceinline__
#ifdef NMX_NT_FIXED
// translation units of the one-item-per-WAVE kernels (nmx_wave.hip): the workgroup size is a
// compile-time 64, so no blockDim load from the implicit kernel arguments (a dependent global
// load at the top of every item) and every "block" reduction collapses to its wave part
#define NMX_TID ((int)(threadIdx.x & 63))
#define NMX_NT 64
#elif defined(NMX_BLOCK_FIXED)
// translation units whose kernels are always launched with NMX_BLOCK_FIXED threads: grid-stride loops
// over compile-time lengths get compile-time trip counts (less loop control on the scalar unit)
#define NMX_TID ((int)threadIdx.x)
#define NMX_NT NMX_BLOCK_FIXED
#else
#define NMX_TID ((int)threadIdx.x)
#define NMX_NT ((int)blockDim.x)
#endif
// Workgroup barrier.  A single-wave workgroup needs no s_barrier: its LDS operations execute
// in order, so a compiler fence + lgkmcnt(0) is enough -- and, unlike __syncthreads(), it does
// not drain vmcnt, i.e. it does not stall on outstanding global loads/stores (table prefetches,
// result stores) at every phase boundary.
#define NMX_WAVE_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#if defined(NMX_NT_FIXED) && defined(NMX_SYNC_GLOBAL)
// nmx_wave_slab.hip: the wave's working lists live in device memory -- its own global stores must have landed (and be
// visible to its other lanes) before the next phase reads them
#define NMX_SYNC()                                                       \
  do {                                                                   \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");               \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");          \
  } while (0)
#elif defined(NMX_NT_FIXED)
#define NMX_SYNC() NMX_WAVE_FENCE()
#elif defined(NMX_BLOCK_FIXED)
#define NMX_SYNC()                                        \
  do {                                                    \
    if (NMX_BLOCK_FIXED <= 64) { NMX_WAVE_FENCE(); }      \
    else { __syncthreads(); }                             \
  } while (0)
#else
#define NMX_SYNC()                                   \
  do {                                               \
    if (blockDim.x <= 64) { NMX_WAVE_FENCE(); }      \
    else { __syncthreads(); }                        \
  } while (0)
#endif
#define NMX_RESTRICT __restrict__
// global-memory writes of this thread become visible to the other threads of the workgroup (followed by NMX_SYNC)
#define NMX_GLOBAL_FENCE() __threadfence_block()
// host-side helpers shared by the translation units of libnmx.so
// nmxi_note_kernel: every launch records the kernel it launched (name as rocprofv3 prints it) under the current
// stage -- through NMX_LAUNCH below, never by hand; nmx_last_kernels() reports them (bench.py's roofline names the kernel from here).
extern "C" void nmxi_note_kernel(const char* name);
// nmxi_note_pair_geom: behind nmxi_note_kernel, the channel-pair FIR launchers also record what the batch size made of that
// launch (channel pairs, workgroups x waves per workgroup); nmx_last_kernels(plan, 9) reports it
extern "C" void nmxi_note_pair_geom(int n_pairs, int grid, int nw);
// true the first time the calling site runs on the current device (`seen` = a static bitmask of device ordinals owned by
// the call site; atomic: the plans of a multi-device stream run one host thread each)
static inline bool nmx_first_on_device(std::atomic<unsigned long long>& seen) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d > 63) return true;
  return !((seen.fetch_or(1ull << d, std::memory_order_relaxed) >> d) & 1ull);
}
// ---- the one way to launch a kernel ----
//   NMX_LAUNCH(kernel, grid, block, lds_bytes, stream, args...)           launches and reports the kernel's own spelling
//   NMX_LAUNCH_AS("name", kernel, grid, block, lds_bytes, stream, args...) ... reports `name` (say why beside it)
//   NMX_LAUNCH_QUIET(kernel, grid, block, lds_bytes, stream, args...)     ... reports nothing
// A template-id with commas comes parenthesised, `(nmx_kern_x<1, 2>)`; the reported name drops those parentheses.  More than
// 64 KiB of dynamic LDS is a per-device opt-in of the kernel (up to the CU's 160 KiB): a launch that asks for it opts in,
// once per device -- every launch site owns the mask of its kernel instantiation; the others pay one comparison.
static inline void nmx_launch_allow_lds(const void* kern, size_t lds, std::atomic<unsigned long long>& seen) {
  if (lds > 64 * 1024 && nmx_first_on_device(seen))
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
template <size_t N>
struct NmxKernName {
  char s[N];
};
template <size_t N>
constexpr NmxKernName<N> nmx_kern_name(const char (&t)[N]) {
  NmxKernName<N> r{};
  const size_t par = (N >= 3 && t[0] == '(' && t[N - 2] == ')') ? 1 : 0;
  for (size_t i = 0; i + 1 + 2 * par < N; ++i) r.s[i] = t[i + par];
  return r;
}
#define NMX_LAUNCH_QUIET(kern, grid, block, lds, stream, ...)                   \
  do {                                                                          \
    static std::atomic<unsigned long long> nmx_seen_{0};                        \
    const size_t nmx_lds_ = (size_t)(lds);                                      \
    nmx_launch_allow_lds((const void*)kern, nmx_lds_, nmx_seen_);               \
    hipLaunchKernelGGL(kern, grid, block, nmx_lds_, stream, __VA_ARGS__);       \
  } while (0)
#define NMX_LAUNCH_AS(name, kern, grid, block, lds, stream, ...)                \
  do {                                                                          \
    NMX_LAUNCH_QUIET(kern, grid, block, lds, stream, __VA_ARGS__);              \
    nmxi_note_kernel(name);                                                     \
  } while (0)
#define NMX_LAUNCH(kern, grid, block, lds, stream, ...)                         \
  do {                                                                          \
    static constexpr auto nmx_name_ = nmx_kern_name(#kern);                     \
    NMX_LAUNCH_AS(nmx_name_.s, kern, grid, block, lds, stream, __VA_ARGS__);    \
  } while (0)
#endif

// Values that are wave-uniform by construction but that the compiler cannot prove uniform (results
// of vector memory loads, threadIdx >> 6): moving them to SGPRs keeps the derived addresses, buffer
// descriptors and branches on the scalar unit.
#ifdef NMX_HOST_EMU
static inline int nmx_uniform_i(int v) { return v; }
static inline long long nmx_uniform_ll(long long v) { return v; }
#else
__device__ __forceinline__ int nmx_uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long nmx_uniform_ll(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffll));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
#endif

// slot of the per-stage kernel lists (nmx_last_kernels) that holds the pair launches' geometry text, whatever the stage
#define NMX_GEOM_SLOT 15
#define NMX_MAX_STAGES 12
#define NMX_MAX_BANDS_DEV 16
// table of the matrix-pipe spectrum kernel (nmx_k_specmm.h): granules of four n, n < 250 live
#define NMX_SMM_NG 63
#define NMX_SMM_TAB_FLOATS (4 * NMX_SMM_NG * 64)
#define NMX_MAX_FILTERS_DEV 24
#define NMX_MAX_SW_COMBOS_DEV 48

// ---- FFT plan (complex length n, mixed radix Stockham) --------------------------------
struct NmxFftStage {
  int radix;       // 2, 3, 4, 5 or any prime (generic O(p^2) butterfly)
  int ns;          // product of the radices of the previous stages
  int m;           // n / radix  (butterflies in this stage)
  unsigned magic;  // floor(2^32 / ns) + 1 : q = umulhi(j, magic) == j / ns for j < 2^16
  int tw_step;     // n / (ns * radix)
};

struct NmxFft {
  int n;
  int nstages;
  NmxFftStage st[NMX_MAX_STAGES];
  const float2* tw;   // [n]      exp(-2 pi i k / n)
  const float2* twr;  // [n + 1]  exp(-2 pi i k / (2 n)), real <-> half-length complex split
};

struct NmxCols {
  int base, ch_stride, a_stride, b_stride;
};

// One oscillatory family (FFT / Welch / STFT) as the kernel sees it
struct NmxOsc {
  int enabled;
  int n;         // real transform length (FFT: N, Welch/STFT: nperseg)
  int nfreq;     // n / 2 + 1
  int k_lo, k_hi;  // bins actually evaluated: union of the bands (all bins with return_spectrum)
  int nseg;      // segments (FFT: 1)
  int step;      // hop between segments
  int half;      // STFT: even-extension length nperseg / 2
  int complex_full;  // 1: n odd -> full-length complex transform of (x, 0)
  int log_transform;
  unsigned estimators;
  int n_est;
  int return_spectrum;
  float scale;   // Welch: 1 / (fs * sum w^2); STFT: 1 / sum w
  float log10_scale;   // log10(scale), formed on the host (the library log10f of a plan constant was ~40 VALU instructions per item)
  int bin_lo[NMX_MAX_BANDS_DEV], bin_hi[NMX_MAX_BANDS_DEV];
  float inv_bins[NMX_MAX_BANDS_DEV];   // 1 / (bin_hi - bin_lo), NaN for an empty band (the reference's mean of nothing)
  NmxCols cols, psd_cols;
  NmxFft fft;    // complex length n/2 (or n when complex_full)
  const float* win;  // [n] window (Welch: hann, STFT: hamming), NULL for FFT
  // STFT: the segments are transformed CENTRED (x - mean of the window: fp32 rounding relative to the signal, not to
  // its offset) and the constant's share comes back analytically: X_seg[k] += mean * wdc[sel][k], wdc[0][k] = DFT of
  // the window (a full segment: interior or even-extended edge), wdc[1][k] = DFT of its first n - nadd samples (the
  // zero-padded last segment of scipy's padded=True); float64 on the host, [2][nfreq] complex
  const float2* wdc;
  int nadd;          // STFT: zeros appended to the extended signal (the tail of the last segment)
  // long-window kernel (nmx_k_timeosc_long.h; 0 / NULL elsewhere): the segment is split into split_d interleaved
  // subsequences x_r[m] = x[m split_d + r] of sub_m = n / split_d samples each; `fft` and `complex_full` then describe the
  // transform of ONE subsequence (sub_m / 2 complex points, or sub_m when sub_m is odd), and
  // X[k] = sum_r tw_n[(r k) mod n] X_r[k mod sub_m]
  int split_d, sub_m;
  const float2* tw_n;   // [n] exp(-2 pi i j / n), float64 on the host
};

struct NmxTimeOscArgs {
  int stft_per_wave;     // STFT segments distributed over the waves of the workgroup (needs 2 x 250 complex per buffer)
  const float* x;        // input samples
  long long ch_stride;   // elements between channels
  long long win_stride;  // elements between windows (0 for a strided stream view)
  const long long* starts;  // per-window start sample or NULL
  float* out;            // [n_windows][n_outputs]
  int n_outputs;
  int n_channels;
  int W;
  int n_bands;
  int clean_on_load;     // apply nan_to_num while loading
  unsigned features;     // NMX_F_* (HJORTH, RAW, LINELENGTH handled here)
  NmxCols hjorth_cols, raw_cols, ll_cols;
  NmxOsc fft, welch, stft;
  // LDS carve (float offsets)
  int off_x, off_a, off_b, off_spec, off_red, lds_floats;
  const float* w500_tab;   // W = 1000: tables of the wave-level kernel (nmx_k_fft500.h), else NULL
  const unsigned short* w510_tab;   // 510-sample transforms: position tables of the prime-factor wave kernel (nmx_k_timeosc_w510.h)
  const float* smm_tab;    // matrix-pipe spectrum kernel (nmx_k_specmm.h): [cos even k, cos odd k, sin even k, sin odd k][n / 4][row 16][n % 4], else NULL
  int smm_k0;              // first bin of that table
  int starts_mod4;         // every window start of this launch is a multiple of 4 samples (16-byte loads of the lanes' runs)
  const float* dcf;        // [n_channels] offset the windows were split from (nmx_engine_dc.inc), or NULL: the true window is
                           // x + dcf[c].  Differences and variances do not see a constant; Raw, bin 0 of the FFT and the STFT's
                           // window-DFT share (NmxOsc::wdc) do
  unsigned short* todo;    // matrix-pipe kernel: [ceil(n_windows / 16)][n_channels] masks, bit j = window 16 g + j of the channel holds
                           // a NaN / an infinity (the kernel does not clean on load) and is left to nmx_kern_timeosc_w1000_todo;
                           // NULL without that kernel
  // long-window kernel (NMX_TO_LONG, nmx_k_timeosc_long.h): the window is staged in LDS for the time-domain features only,
  // [off_a, off_spec) then holds the transform buffers of one subsequence (NmxOsc::split_d) over it
  int long_mode;
  int long_nb;             // floats per spectrum: max over FFT / Welch of k_hi - k_lo, rounded up to 4
  int long_spec_slab;      // the accumulators + spectrum (long_sp_floats) live in the workgroup's slab, not at off_spec
  int long_sp_floats;      // floats of that region: 3 long_nb, or the STFT's accumulators + (k_hi - k_lo) x nseg spectrum if larger
  int long_stft;           // STFT segment class (NMX_TOL_STFT_*, nmx_k_timeosc_long.h); 0: no STFT in this plan
  int long_stft_acc;       // floats in front of the STFT spectrum: the accumulators of the split class, else 0
  int slab_floats;         // floats per slab (0: none needed)
  int slab_blocks;         // slabs allocated = resident workgroups of the persistent kernel
  float* slab;             // [slab_blocks][slab_floats] device memory owned by the plan (the emulator runs on slab 0)
};

// the time / oscillatory and Hilbert kernels a plan launches, chosen when it is built (build_timeosc, build_hilbert)
enum NmxTimeOscKind { NMX_TO_SCAN, NMX_TO_SPECMM, NMX_TO_W1000_LOW, NMX_TO_W1000, NMX_TO_STFT500, NMX_TO_W510, NMX_TO_FIXED128, NMX_TO_GENERIC, NMX_TO_LONG };
enum NmxHilbertKind { NMX_HIL_W500, NMX_HIL_W1000, NMX_HIL_FIXED128, NMX_HIL_LONG };   // LONG: nmx_k_hilbert_long.h (3 W + 4 floats beyond LDS)
// the run statistics of the bursts chain (build_bursts): the envelope in the registers of a wave, 16 / 32 chunks per lane, all rows
// or only those the Hilbert kernel stored whole (NmxBurstStatArgs::full); or the LDS kernel
// (windows up to 16 384 samples), or the tile scan that reads the envelope from memory (NmxBurstStatArgs::scan_tile)
enum NmxBurstStatKind { NMX_BSTAT_REG16, NMX_BSTAT_REG16_SPARSE, NMX_BSTAT_REG32, NMX_BSTAT_REG32_SPARSE, NMX_BSTAT_GENERIC, NMX_BSTAT_SCAN };
// the sharp-wave launches (build_sharp): the list kernel over every item, or the compact-LDS dense launch + the list kernel over the
// items it flagged; the list kernel's lists in LDS, or (long windows) in slabs of device memory (nmx_wave_slab.hip)
enum NmxSharpKind { NMX_SHARP_LIST, NMX_SHARP_DENSE_LIST, NMX_SHARP_SLAB, NMX_SHARP_DENSE_SLAB };
// the one-wave FIR kernels of one launch of a FIR stage (nmx_w64.hip), chosen where its tables are built (build_fir_stage,
// build_bank, build_notch): M = 4096; channel pairs at M = 1536 / 1024 / 2048 (2048: bank filters, or the notch); one
// channel per M = 2048 transform (nmx_kern_bank_w64 / _w64pp, nmx_kern_notch_w64 / _w64q / _w64qp: by batch size)
enum NmxFirKernel { NMX_FIR_ONE, NMX_FIR_X2, NMX_FIR_PAIR_C, NMX_FIR_PAIR_D, NMX_FIR_PAIR_E };

#define NMXD_F_HJORTH (1u << 0)
#define NMXD_F_RAW (1u << 1)
#define NMXD_F_BANDPOWER (1u << 2)
#define NMXD_F_STFT (1u << 3)
#define NMXD_F_FFT (1u << 4)
#define NMXD_F_WELCH (1u << 5)
#define NMXD_F_SHARPWAVE (1u << 6)
#define NMXD_F_BURSTS (1u << 7)
#define NMXD_F_LINELENGTH (1u << 8)

#define NMXD_EST_MEAN 1u
#define NMXD_EST_MEDIAN 2u
#define NMXD_EST_STD 4u
#define NMXD_EST_MAX 8u
