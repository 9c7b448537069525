// nmx_engine.inc -- host side of the engine: the Plan, scratch management and the parts below (streams and events of a
// chunk and a batch: nmx_engine_sched.inc; plan building and the stages' launchers: nmx_engine_plan_*.inc; C ABI:
// nmx_engine_abi.inc, nmx_engine_run.inc, nmx_engine_norm.inc).
// Included by nmx_api.hip (HIP backend: the product) and by
// tests/emu/nmx_emu.cpp (single-thread logic emulator used by the CPU-only tests).  The
// includer provides the be_* backend (allocation, copies, launches, events).
//
// C ABI documented in include/nmx.h.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <deque>
#include <functional>
#include <mutex>
#include <condition_variable>
#include <pthread.h>
#include <vector>

#include "../../include/nmx.h"
#include "nmx_k_coh.h"   // coherence kernel + its be_launch_coh (HIP launcher, or the emulator's loop)
#include "nmx_k_proj.h"  // grid-projection kernel + its be_launch_proj (likewise)
#include "nmx_k_nolds.h" // sample-entropy, Hurst and DFA kernels of the nolds feature + be_launch_nolds / _hurst / _dfa (likewise)

static thread_local std::string g_nmx_err;
static int nmx_fail(int code, const std::string& msg) {
  g_nmx_err = msg;
  return code;
}
#define NMX_REQUIRE(cond, msg) \
  do { if (!(cond)) return nmx_fail(NMX_E_INVALID, std::string(msg)); } while (0)

#ifdef NMX_HOST_EMU
// The logic emulator (tests/emu) runs the item code of every stage, whatever kernel the plan chose: its launch interface
// carries none of those choices (it runs the matrix-pipe spectrum's arithmetic when launch_timeosc_stage hands it `todo`).
static void be_launch_timeosc(const NmxTimeOscArgs& A, NmxTimeOscKind, int n, int nt, size_t lds, int, be_stream_t s) { be_launch_timeosc(A, n, nt, lds, s); }
static void be_launch_hilbert(const NmxHilbertArgs& A, NmxHilbertKind, long long n, size_t lds, be_stream_t s) { be_launch_hilbert(A, n, 128, lds, s); }
static void be_launch_bank_w64(const NmxBankW64Args& A, int n, size_t lds, int, be_stream_t s) { be_launch_bank_w64(A, n, lds, s); }
static void be_launch_burst_thr(const NmxBurstThrArgs& A, const NmxBurstWalk&, const NmxBurstWalkSeg&, int n, int nt, size_t lds, be_stream_t s) {
  be_launch_burst_thr(A, n, nt, lds, s);
}
static void be_launch_burst_fill(const NmxBurstThrArgs& A, int n, unsigned short* slots, float* sorted, bool, be_stream_t s) {
  be_launch_burst_fill(A, n, slots, sorted, s);
}
static void be_launch_burst_stat(const NmxBurstStatArgs& A, NmxBurstStatKind, int n, size_t lds, be_stream_t s) { be_launch_burst_stat(A, n, lds, s); }
static void be_launch_sharp(const NmxSharpArgs& A, NmxSharpKind, int n, size_t lds, be_stream_t s) { be_launch_sharp(A, n, lds, s); }
static int be_cu_count(int) { return 256; }
#endif

namespace {

constexpr double kPi = 3.14159265358979323846;

// A block that grows on demand and frees itself with its owner.  Whoever deletes the owner has set the device and drained
// the streams that read the block (nmx_plan_destroy, nmx_norm_destroy, nmx_proj_destroy).
template <void* (*Alloc)(size_t), void (*Free)(void*)>
struct Block {
  void* p = nullptr;
  size_t cap = 0;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { if (p) Free(p); }
  bool regrow(size_t bytes) {   // a fresh block of `bytes` (the contents are not kept); false: no memory, and the block is empty
    if (p) Free(p);
    p = Alloc(bytes);
    cap = p ? bytes : 0;
    return p != nullptr;
  }
};
using Buf = Block<be_alloc, be_free>;                 // device memory (ensure)
using HostBuf = Block<be_host_alloc, be_host_free>;   // page-locked host memory

#include "nmx_engine_sched.inc"

// What a launch reports under: the index of its timer (nmx_last_timing_ms) and of its kernel list (nmx_last_kernels,
// be_stage).  The numbers are ABI (include/nmx.h).
enum Stage {
  ST_BATCH = 0,      // the whole batch (timer only)
  ST_PREP = 1,       // front end and pre-processing
  ST_TIMEOSC = 2,
  ST_BANK = 3,
  ST_BURSTS = 4,
  ST_SHARP = 5,
  ST_BANK2 = 6,      // the bank's second launch, when its filters are split over two kernels
  ST_COH = 7,
  ST_PROJ = 8,       // grid projection: launched by chunk_finalize, behind the stages of run_chunk
  ST_GEOM = 9,       // no stage: nmx_last_kernels(9) is the launch geometry of the channel-pair FIR kernels
  ST_NOLDS = 10,     // nolds: its band filters and the sample-entropy, Hurst and DFA kernels
  ST_COUNT
};

// Where the next stage reads its windows: window w of channel c begins at x + c * ch_stride + (starts ? starts[w] :
// w * win_stride).  run_chunk and nmx_preprocess_window keep one and hand it from stage to stage; every stage that writes
// windows sets it to its output.
struct WinView {
  const float* x;
  long long ch_stride, win_stride;
  const long long* starts;
  int clean;           // NaN / infinity are still in the samples: the reader cleans on load
};
template <class Args>
void view_into(Args& A, const WinView& v) {
  A.x = v.x; A.ch_stride = v.ch_stride; A.win_stride = v.win_stride; A.starts = v.starts; A.clean_on_load = v.clean;
}
void view_into(NmxTapArgs& A, const WinView& v) {
  A.x = v.x; A.ch_stride = v.ch_stride; A.win_stride = v.win_stride; A.starts = v.starts; A.clean = v.clean;
}
// the next stage reads y, laid out [nw][C][w] (and clean)
WinView dense_view(const void* y, int C, int w) { return WinView{(const float*)y, w, (long long)C * w, nullptr, 0}; }

// The front end of a chunk or of one window: the re-reference -- or, in a plan without one, the offset shift
// (nmx_engine_plan_state.inc: build_front, launch_front).
struct FrontStage {
  float* d_R = nullptr;      // [C][C_in] re-reference matrix, fp32 (the plan's block: upload); null: the plan has none
  bool car = false;          // R = (d - o) I + o 11^T: column-sum kernel instead of the dense product
  float car_diag = 0.f, car_off = 0.f;
  bool structured = false;   // taps + group-sum structure found in R (nmx_k_prep.h: NmxRerefStructArgs)
  NmxRerefStructArgs rst{};
  Buf x_ref;                 // the re-referenced / shifted sample range of a chunk
};
// The time / oscillatory kernel, chosen at plan time (nmx_engine_plan_spectral.inc: build_timeosc, launch_timeosc_stage).
struct TimeOscStage {
  NmxTimeOscArgs a{};        // argument template
  NmxTimeOscKind kind = NMX_TO_GENERIC;
  bool takes_dc = true;      // the kernel adds the carried offset on load (else: it reads a copy with it added back, dc_windows)
  int nt = 64;               // threads per workgroup of the generic kernels
  Buf todo;                  // flags of the matrix-pipe spectrum kernel (NmxTimeOscArgs::todo)
};
// Coherence between channel pairs (nmx_k_coh.h; nmx_engine_plan_spectral.inc: build_coh, launch_coh_stage): stateless.
struct CohStage {
  NmxCohArgs a{};            // argument template
};
// The resampler, behind the notch (nmx_engine_plan_state.inc: build_resample, launch_resample).
struct ResampleStage {
  NmxResampleArgs a{};       // argument template
  int nt = 256;
  Buf y;                     // resampled windows of a chunk
};

// A FIR stage -- a preprocessing_filter stage, the notch or the band-pass bank -- with its kernels decided at plan time
// (nmx_engine_plan_fir.inc: build_fir_stage, launch_fir_stage).  One launch of its one-wave kernels: the filters of
// `mask` on kernel `kernel`; the channel-pair kinds come with the tables of nmx_k_bank_w64c/d/e.h (build_pair_tables).
struct FirLaunch {
  unsigned mask = 0;
  Stage stage = ST_BANK;   // timer / kernel-name stage it reports under
  NmxFirKernel kernel = NMX_FIR_ONE;
  bool pipelined = false;   // NMX_FIR_ONE: large batches may run the pipelined persistent form (nmx_w64p_ok)
  const float* hc = nullptr;
  const float* twc = nullptr;
  bool fused = false;  // runs inside the notch's kernel (choose_notch_bank_fuse): the stage's own launches skip it
};
struct FirStage {
  NmxBankArgs a{};     // argument template (per-call fields are patched in by the caller)
  bool w64 = false;    // one-wave kernels (M = 2048 / 4096) ...
  NmxBankW64Args w{};  // ... and their template
  std::vector<FirLaunch> launches;   // (the LDS kernels: one entry, for its stage)
  bool takes_dc = true;   // its kernels add the carried offset on load (NmxBankArgs::dcf; else they read a copy of the windows
                          // with the offset added back, dc_windows): set by fir_stage_finish
};

// nolds (nmx_k_nolds.h; nmx_engine_plan_spectral.inc: build_nolds, launch_nolds_stage): stateless.  Its band series come
// from a FIR stage of its own over the pre-processed windows -- the bank's kernels and the bank's taps, but not the bank's
// launch: a band series is the filter's output alone (no band-power, burst or sharp-wave epilogue next to it), which is
// what nmx_filter_window runs through those kernels as well, and a plan without nolds launches what it launched before.
struct NoldsStage {
  NmxNoldsArgs a{};           // argument template
  FirStage fir;               // zero-padded "same" band filters, series out (sw_out)
  bool have_fir = false;
  std::vector<std::vector<double>> taps;   // deep copies
  Buf yb;                     // band series of a chunk, [nw][C][n_band][W]
  // nmx_nolds_probe: while h_probe is set every chunk also leaves its items' counts (and, with h_series, the series the
  // walk read) in the caller's host arrays, rows [probe_w0, probe_w0 + nw) of them
  unsigned* h_probe = nullptr;
  float* h_series = nullptr;
  long long probe_w0 = 0;
  Buf d_probe, d_series;
  // detrended fluctuation analysis (NMX_NOLDS_DFA): its own kernel behind the sample entropy's, on the same series
  bool have_sampen = false, have_dfa = false;
  NmxNoldsDfaArgs dfa{};      // argument template (scales: a plan table)
  double* h_dfa = nullptr;    // nmx_nolds_dfa_probe: [item][n_scales + 3] of the caller, as h_probe
  Buf d_dfa;
  // Hurst exponent by rescaled range (NMX_NOLDS_HURST): its own kernel between the two, on the same series
  bool have_hurst = false;
  NmxNoldsHurstArgs hurst{};  // argument template (scales, log_e: plan tables)
  double* h_hurst = nullptr;  // nmx_nolds_hurst_probe: [item][2 n_scales + 3] of the caller, as h_probe
  Buf d_hurst;
};

// The bursts chain -- Hilbert envelope (where the bank leaves band series), threshold walk, run statistics -- with its kernels
// and its walk schedule decided at plan time (nmx_engine_plan_bursts.inc: build_hilbert, build_bursts, launch_burst_stage).
struct BurstStage {
  NmxHilbertArgs hil{};       // argument templates (per-call fields are patched in by launch_burst_stage)
  NmxBurstThrArgs bthr{};
  NmxBurstStatArgs bstat{};
  NmxHilbertKind hil_kind = NMX_HIL_FIXED128;
  bool own_hilbert = false;   // the bank leaves the band series (one-wave / partitioned kernels): the stand-alone Hilbert kernel runs
  bool sparse = false;        // ... and stores a row below the threshold floor as its tail only (one-wave kernels; NMX_BURST_ENV_SPARSE)
  bool sparse_count = false;  // ... = 2: and every chunk's flags are read back and counted (nmx_last_kernels(4) reports them)
  long long env_tail_rows = 0, env_rows = 0;
  NmxBurstStatKind stat_kind = NMX_BSTAT_GENERIC;
  NmxBurstWalk walk{};        // the walk's schedule constants (nmx_k_bursts.h; NMX_THR_FILL, NMX_THR_WAVE, NMX_THR_LIST_LDS)
  bool fill_split = true;     // the fill phase as two launches (sort, one-wave walk; NMX_FILL_SPLIT)
  int nt_thr = 256;           // threads of the workgroup walk
  // state (the blocks belong to the plan: plan_alloc)
  long long seen = 0;         // host mirror of the per-sequence window counter (all sequences advance together)
  float* d_top = nullptr;
  long long* d_counts = nullptr;
  size_t top_bytes = 0, counts_bytes = 0;
  float* d_floor = nullptr;   // [C][Bb] lower bound of each sequence's future thresholds (NmxBurstThrArgs::floor): derived from the
                              // state, never exported; -INFINITY whenever the state is new to this plan
  // hand-off
  Buf env[2], thr[2];         // read on the side stream: one set per chunk parity
  Buf env_full[2];            // ... and which rows of env[] are whole (NmxHilbertArgs::full), with it
  Buf yb;                     // band series for the stand-alone Hilbert kernel (exists once)
  Buf slots;                  // scratch of the fill phase
  // a fresh stream sorts the whole fill phase at once (nmx_k_burst_fill.h): how many of `nw` hops that takes, else 0
  int fill_hops(int nw) const { return walk.fill && seen == 0 ? nmx_burst_fill_hops(bthr, nw) : 0; }
};
// The sharp-wave analysis, its launches decided at plan time (nmx_engine_plan_state.inc: build_sharp, launch_sharp_stage).
struct SharpStage {
  NmxSharpArgs a{};           // argument template
  NmxSharpKind kind = NMX_SHARP_LIST;
  Buf swy[2], todo[2];        // filtered series and the dense launch's flags: read on a side stream, one set per chunk parity
  Buf slab;                   // list slabs of the long-window kinds (one stream runs every sharp-wave launch of a plan)
};
// The Kalman filters behind the band-pass activity (nmx_engine_plan_state.inc: build_kalman, kalman_state_*).
struct KalmanStage {
  NmxKalmanArgs a{};          // argument template
  double* d_state = nullptr;  // [C][bands][6]: x, P per filter (the plan's block: plan_alloc)
  size_t bytes = 0;
};
// The raw normaliser, the last pre-processing stage (nmx_engine_plan_state.inc: build_rawnorm, run_rawnorm, rawnorm_state_*).
struct RawNormStage {
  NmxRawNormArgs a{};         // argument template; its rings, counts and sorted copies are the plan's blocks (plan_alloc)
  long long hops = 0;         // hops normalised so far (NmxRawNormArgs::hop0)
  bool sorted_valid = false;  // the sorted copies of the order-statistic methods mirror the rings
  size_t ring_bytes = 0, cnt_bytes = 0, len_bytes = 0;
  Buf x_rn, mean, scale;      // scratch of a chunk: normalised windows, statistics per (hop, channel)
  Buf qt, qn;                 // ... "quantile" tables / "power" parameters
};

struct Plan {
  nmx_plan_desc d;
  std::vector<std::vector<double>> taps;   // deep copies
  std::vector<double> notch_taps, ref_matrix;
  std::vector<double> notch_taps_used;     // what the notch kernels convolve with: h, or delta - h (NmxBankArgs::residual)
  int device = 0;
  int n_cu = 256;                          // compute units of that device (the persistent kernels' grids)
  Schedule sched;                          // streams, events and overlap mode (nmx_engine_sched.inc)
  int host_chunk_windows = 512;            // hops per chunk when the caller hands over host memory ...
  int host_first_chunk = 128;              // ... after a short first one (nmx_engine_run.inc)
  int norm_chunk_windows = 384;           // device-resident batches with an attached normaliser (nmx_engine_run.inc; NMX_NORM_CHUNK_WINDOWS)
  std::vector<void*> tables;               // device allocations of a fixed size (plan_alloc, upload): freed with the plan
  ~Plan() { for (void* t : tables) be_free(t); }   // (and every Buf frees itself: nmx_plan_destroy has set the device)
  std::map<int, NmxFft> fft_cache;
  std::map<int, const float2*> twn_cache;   // exp(-2 pi i k / n), k < n, of the long-window kernel's combination step (NmxOsc::tw_n)
  // the stages of a chunk (run_chunk): argument templates and kinds decided when the plan is built, one launcher each
  FrontStage front;                   // re-reference or offset shift
  FirStage bank;                      // band-pass bank: feeds bursts and sharp waves
  bool have_bank = false;
  FirStage notch;
  bool have_notch = false;
  int notch_bank_fuse = 0;            // the bank's second launch runs inside the notch kernel (NMX_NOTCH_SW_FUSE; 2: the notch's
                                      // spectrum in LDS as well, one exchange tile fewer -- kept for measurement)
  std::vector<FirStage> pre;          // preprocessing_filter stages (one filter each)
  const float* w64e_tw = nullptr;     // twiddles of the M = 2048 channel-pair kernel (nmx_k_bank_w64e.h): notch and bank
  const float* w500_tab = nullptr;    // tables of the wave-level 500-point transform: time / oscillatory and Hilbert kernels
  BurstStage bursts;                  // bursts chain: behind the bank
  bool have_bursts = false;
  SharpStage sharp;                   // sharp-wave analysis: likewise
  bool have_sharp = false;
  TimeOscStage timeosc;               // time / oscillatory kernel
  bool have_timeosc = false;
  CohStage coherence;                 // coherence between channel pairs
  bool have_coh = false;
  NoldsStage nolds;                   // sample entropy of the window and of band series of it
  bool have_nolds = false;
  int nt_bank = 256;
  int chunk_windows = 1024;
  int burst_handoff_mb = 2048;   // windows above 16 384 samples: budget of the bursts chain's hand-off buffers (batch_chunk_sizes; NMX_BURST_HANDOFF_MB)
  bool tiny_inline = true;          // host batches of a few hops on ONE stream (nmx_engine_run.inc)
  bool starts_mod4 = false;         // every window start of the current batch is a multiple of 4 samples
  // scratch
  Buf tap;            // pre-processed windows of a chunk on their way to a host caller (nmx_process_batch_tap)
  Buf x_in, x_in2[2], x_pf[2], y_notch, out, starts, mask;
  HostBuf win_pin;    // page-locked HOST staging of the one-window call (nmx_process_window): cast input, feature row, mask
  // state
  KalmanStage kalman;
  bool have_kalman = false;
  ResampleStage resample;             // raw_resampling, behind the notch
  bool have_resample = false;
  RawNormStage rawnorm;
  bool have_rawnorm = false;
  std::vector<std::vector<double>> pre_taps;
  int w_in = 0;           // samples per incoming window (raw_window when resampling, else window)
  be_timer_t timers[ST_COUNT];
  std::string kernels[ST_COUNT];   // kernels of the first chunk of the last batch, per stage (nmx_last_kernels)
  std::string pair_geom;           // ... and the launch geometry of its channel-pair FIR kernels (nmx_last_kernels 9)
  nmx_norm* norm = nullptr; // attached feature normaliser (not owned): applied to every chunk's rows on the device
  nmx_proj* proj = nullptr; // attached grid projection (not owned): behind the normaliser, on the same stream
  // offset split (nmx_engine_dc.inc): x = u + d per input row, the constants carried in float64 on the host
  bool dc_ok = false;            // every pre-processing stage of this plan is affine in the window
  bool dc_auto = true;           // learn the rows' constants in front of a re-reference kernel (fp32 input, no host offsets)
  bool dc_host_set = false, dc_learned = false, dc_dirty = false;
  bool dc_active = false;        // some constant is non-zero: the consumers get the tables
  bool dc_sub_active = false;    // ... and the re-reference kernels subtract on load
  double dc_gain = 1.0;          // what the notch makes of a constant: sum of its taps
  std::vector<double> dc_host;   // [C_in] caller's offsets (nmx_plan_set_offsets)
  std::vector<float> dc_sub_h;   // [C_in] learned constants, subtracted on load by the re-reference kernels
  std::vector<double> dc_pre_h;  // [C] offset of the pre-processed windows: gain * R (host + sub)
  float* d_dc_sub = nullptr;     // device copies: sub, (float) dc_pre
  float* d_dc_pref = nullptr;
  float* d_dc_nanv = nullptr;    // -(float)(host + sub): the recording's value 0 in the split domain (a cleaned NaN)
  Buf x_dc;                      // windows with the offset added back, for a kernel that cannot take it on load
  // hand-shakes of a host-memory batch with the caller's conversion threads (nmx_plan_set_pipeline)
  const volatile int64_t* pipe_in_ready = nullptr;   // samples [0, *in_ready) of every input row are in place
  volatile int64_t* pipe_out_done = nullptr;         // rows [0, *out_done) of `out` (and the NaN mask) have landed
  struct Progress { volatile int64_t* dst; int64_t value; };
  std::vector<Progress> pipe_marks;
};

// A batch from host memory starts with a SHORT chunk (nmx_engine_run.inc): sized for it, the hand-off buffers of a fresh
// plan would be regrown by the first long chunk -- and a regrow frees a block, i.e. waits for the WHOLE device (be_free):
// on a fresh 120 s stream the host stood still behind the 2.1 ms fill sort of the burst history, and the second chunk's
// filters with it.  While g_ensure_scale > 1 (the short chunk of such a batch) a buffer that has to grow is sized for
// the long chunks that follow.
static thread_local double g_ensure_scale = 1.0;
int ensure(Buf& b, size_t bytes) {
  if (bytes <= b.cap) return 0;
  if (g_ensure_scale > 1.0) bytes = (size_t)((double)bytes * g_ensure_scale) + 256;
  const size_t want = bytes + bytes / 8;
  if (!b.regrow(want)) return nmx_fail(NMX_E_NOMEM, "device allocation of " + std::to_string(want) + " bytes failed");
  return 0;
}

// A device block of a fixed size that lives as long as the plan: P.tables is its only owner.
void* plan_alloc(Plan& P, size_t bytes) {
  void* d = be_alloc(bytes ? bytes : 4);
  if (d) P.tables.push_back(d);
  return d;
}
void* upload(Plan& P, const void* src, size_t bytes) {
  void* d = plan_alloc(P, bytes);
  if (d && bytes) be_h2d_sync(d, src, bytes);
  return d;
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && v[0] >= '0' && v[0] <= '9') ? atoi(v) : dflt;
}

// Workgroups of a persistent kernel that owns one slab of device memory each: as many per CU as `lds_bytes` of LDS leave room
// for (two at the most), the slabs of `slab_floats` floats (0: none) within 64 MiB, at most `cap` (0: no cap); at least one.
int slab_workgroups(const Plan& P, size_t lds_bytes, size_t slab_floats, int cap = 0) {
  const int per_cu = std::max(1, std::min(2, (int)((size_t)160 * 1024 / lds_bytes)));
  size_t blocks = (size_t)P.n_cu * per_cu;
  if (slab_floats > 0) blocks = std::min(blocks, ((size_t)64 << 20) / (slab_floats * 4));
  if (cap > 0) blocks = std::min(blocks, (size_t)cap);
  return (int)std::max<size_t>(1, blocks);
}

// nmx_last_kernels: what the launches behind be_stage_reset() reported, per stage (the projection's: chunk_finalize), and the
// geometry of the channel-pair FIR launches among them
void snapshot_kernels(Plan& P) {
  for (int i = 0; i < ST_PROJ; ++i) P.kernels[i] = be_stage_kernels(i);
  P.kernels[ST_NOLDS] = be_stage_kernels(ST_NOLDS);
  P.pair_geom = be_stage_kernels(NMX_GEOM_SLOT);
}

#include "nmx_engine_dc.inc"
#include "nmx_engine_plan_spectral.inc"
#include "nmx_engine_plan_bursts.inc"
#include "nmx_engine_plan_fir.inc"
#include "nmx_engine_plan_state.inc"

}  // namespace

#include "nmx_engine_abi.inc"
#include "nmx_engine_run.inc"
#include "nmx_engine_norm.inc"
#include "nmx_engine_proj.inc"
#include "nmx_engine_host.inc"
