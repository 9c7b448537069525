// nmx_emu.cpp -- TEST-ONLY single-thread logic emulator of the nmx kernels.
//
// Compiles the SAME device source (py_neuromodulation_amd/csrc/nmx_k_*.h) with
// -DNMX_HOST_EMU (one "thread" per workgroup, barriers are no-ops) behind the same C ABI,
// so the CPU-only test suite can check kernel *logic* (index math, FFT staging, epilogues)
// against the oracle in a container without a GPU.  It is NOT part of the product: the
// package loader only ever opens libnmx.so (HIP); nothing under py_neuromodulation_amd/
// references this file, and wave-level behaviour (races, barriers, shuffles) is only
// exercised by the -m gpu tests on the MI355X.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define NMX_HOST_EMU 1
#include "../../py_neuromodulation_amd/csrc/nmx_k_bank.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_bank_w64.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_bursts.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_burst_fill.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_kalman.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_norm.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_power.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_prep.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_rawnorm.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_resample.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_resample64.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_sharpwave.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_timeosc.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_specmm.h"

typedef void* be_stream_t;
struct be_timer_t { bool used = false; };
static int nmx_fail(int code, const std::string& msg);

static int be_device_count() { return 1; }
static int be_set_device(int) { return 0; }
// blocks handed out and not yet given back, "device" and page-locked together (nmx_emu_live_blocks below:
// tests/test_plan_lifetime_cpu.py)
static std::atomic<long long> g_live_blocks{0};
static void* be_alloc(size_t n) { void* p = calloc(1, n ? n : 4); if (p) ++g_live_blocks; return p; }
static void be_free(void* p) { if (p) --g_live_blocks; free(p); }
static void be_dev_pool_age() {}
static long long be_dev_pool_trim(long long) { return 0; }
static void* be_host_alloc(size_t n) { void* p = malloc(n ? n : 4); if (p) ++g_live_blocks; return p; }
static void be_host_free(void* p) { if (p) --g_live_blocks; free(p); }

// The schedule as the engine issues it (tests/chunk_schedule_cases.py): between nmx_emu_trace_begin() and nmx_emu_trace_end()
// every backend call that touches a stream appends one line --
//   "op <name> <stream>"  a launch, asynchronous copy, memset or host function     "record <stream> <event>"
//   "sync <stream>"       the host waits for the stream                           "wait <stream> <event>"
// Streams and events are numbered as they are created (0: the null stream of the blocking copies, which are an operation
// followed by a sync).  The emulator runs everything at once on the calling thread: the lines say what a device would be
// free to reorder.
static bool g_tracing = false;
static std::string g_trace;
static void nmx_trace(const char* kind, const char* name, const void* stream, int event = -1) {
  if (!g_tracing) return;
  g_trace += kind;
  if (name) g_trace += std::string(" ") + name;
  g_trace += " " + std::to_string((long long)(intptr_t)stream);
  if (event >= 0) g_trace += " " + std::to_string(event);
  g_trace += "\n";
}
#define NMX_TR(st) nmx_trace("op", __func__, st)
static void nmx_trace_blocking(const char* name) { nmx_trace("op", name, nullptr); nmx_trace("sync", nullptr, nullptr); }

static void be_h2d_sync(void* d, const void* s, size_t n) { nmx_trace_blocking(__func__); memcpy(d, s, n); }
static void be_d2h_sync(void* d, const void* s, size_t n) { nmx_trace_blocking(__func__); memcpy(d, s, n); }
static void be_memset_sync(void* d, int v, size_t n) { nmx_trace_blocking(__func__); memset(d, v, n); }
static void be_h2d_async(void* d, const void* s, size_t n, be_stream_t st) { NMX_TR(st); memcpy(d, s, n); }
static void be_d2h_async(void* d, const void* s, size_t n, be_stream_t st) { NMX_TR(st); memcpy(d, s, n); }
static void be_h2d_2d_async(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, be_stream_t st) {
  NMX_TR(st);
  for (size_t r = 0; r < h; ++r) memcpy((char*)d + r * dp, (const char*)s + r * sp, w);
}
static void be_d2h_2d_async(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, be_stream_t st) {
  NMX_TR(st);
  for (size_t r = 0; r < h; ++r) memcpy((char*)d + r * dp, (const char*)s + r * sp, w);
}
static void be_memset_async(void* d, int v, size_t n, be_stream_t st) { NMX_TR(st); memset(d, v, n); }
static void be_host_fn(be_stream_t st, void (*fn)(void*), void* arg) { NMX_TR(st); fn(arg); }
static int be_sync(be_stream_t st) { nmx_trace("sync", nullptr, st); return 0; }
static void be_sync_quiet(be_stream_t st) { nmx_trace("sync", nullptr, st); }
static int be_sync_watch(be_stream_t st, const std::string*, int) { nmx_trace("sync", nullptr, st); return 0; }
static intptr_t g_streams = 0;   // handles are 1, 2, ...: distinct, never dereferenced
static be_stream_t be_stream_create() { return (be_stream_t)++g_streams; }
static be_stream_t be_stream_create_high() { return (be_stream_t)++g_streams; }
static void be_stream_destroy(be_stream_t) {}
typedef int be_event_t;
static int g_events = 0;
static void be_event_create(be_event_t& e) { e = ++g_events; }
static void be_event_destroy(be_event_t&) {}
static void be_event_record(be_event_t& e, be_stream_t st) { nmx_trace("record", nullptr, st, e); }
static void be_stream_wait(be_stream_t st, be_event_t& e) { nmx_trace("wait", nullptr, st, e); }
static void be_timer_create(be_timer_t&) {}
static void be_timer_destroy(be_timer_t&) {}
static void be_timer_start(be_timer_t&, be_stream_t) {}
static void be_timer_stop(be_timer_t& t, be_stream_t) { t.used = true; }
static float be_timer_elapsed(be_timer_t&) { return 0.f; }
static int be_check_launch() { return 0; }
static void be_stage(int) {}
static void be_stage_reset() {}
static std::string be_stage_kernels(int) { return "host emulator (tests only)"; }

// the matrix-pipe spectrum kernel's arithmetic and flag protocol (nmx_k_specmm.h): a 16-bit mask per tile of 16 windows of one
// channel (tile = group * n_channels + channel), the flagged windows redone by the generic item code with its cleaning.
// The plan hands over `todo` when it chose that kernel (build_timeosc); every other choice runs the generic item.
static void be_launch_timeosc(const NmxTimeOscArgs& A, int n_items, int, size_t lds, be_stream_t st) { NMX_TR(st);
  if (A.todo) {
    const int C = A.n_channels, n_windows = n_items / C;
    for (int t = 0; t < ((n_windows + 15) / 16) * C; ++t) A.todo[t] = 0;
    for (int w = 0; w < n_windows; ++w)
      for (int c = 0; c < C; ++c)
        if (nmx_specmm_item_emu(A, w, c)) A.todo[(w / 16) * C + c] |= (unsigned short)(1u << (w & 15));
    return;
  }
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) nmx_time_osc_item(A, it / A.n_channels, it % A.n_channels, sm.data());
}
static void be_launch_timeosc_redo(const NmxTimeOscArgs& A, int n_items, be_stream_t st) { NMX_TR(st);
  const int C = A.n_channels, n_windows = n_items / C;
  std::vector<float> sm((size_t)A.lds_floats + 16);
  for (int w = 0; w < n_windows; ++w)
    for (int c = 0; c < C; ++c)
      if (A.todo[(w / 16) * C + c] & (1u << (w & 15))) nmx_time_osc_item(A, w, c, sm.data());
}
static void be_launch_bank(const NmxBankArgs& A, int n_items, int, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) nmx_bank_item(A, it / A.n_channels, it % A.n_channels, sm.data());
}
static void be_launch_bank_w64(const NmxBankW64Args& A, int n_items, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) {
    if (A.b.pad_mode == 0) nmx_bank_w64_item<0, 0, 1>(A, it / A.b.n_channels, it % A.b.n_channels, sm.data(), nullptr);
    else nmx_bank_w64_item<1, 0, 0>(A, it / A.b.n_channels, it % A.b.n_channels, sm.data(), nullptr);
  }
}
static void be_launch_sharp_todo(const NmxSharpArgs&, int, size_t, const unsigned char*, be_stream_t st) { NMX_TR(st); }
static void be_launch_sharp_dense(const NmxSharpArgs&, int, be_stream_t st) { NMX_TR(st); }
static void be_launch_hilbert(const NmxHilbertArgs& A, long long n_items, int, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (long long it = 0; it < n_items; ++it) nmx_hilbert_item(A, it, sm.data());
}
static void be_launch_burst_thr(const NmxBurstThrArgs& A, int n_items, int, size_t lds, be_stream_t st, long long = -1) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) nmx_burst_thr_item<1>(A, it / A.n_bands, it % A.n_bands, sm.data());
}
static void be_launch_burst_fill(const NmxBurstThrArgs& A, int n_items, unsigned short*, float*, be_stream_t st) { NMX_TR(st);
  for (int it = 0; it < n_items; ++it) nmx_burst_fill_item_emu(A, it / A.n_bands, it % A.n_bands);
}
static void be_launch_burst_stat(const NmxBurstStatArgs& A, int n_items, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) {
    const int bi = it % A.n_bands, r = it / A.n_bands;
    nmx_burst_stat_item(A, r / A.n_channels, r % A.n_channels, bi, sm.data());
  }
}
static void be_launch_sharp(const NmxSharpArgs& A, int n_items, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) {
    const int fi = it % A.n_filters, r = it / A.n_filters;
    nmx_sharp_item(A, r / A.n_channels, r % A.n_channels, fi, sm.data());
  }
}
static void be_launch_reref(const NmxRerefArgs& A, be_stream_t st) { NMX_TR(st);
  for (int c0 = 0; c0 < A.C; c0 += NMX_REREF_ROWS)
    for (long long t = 0; t < A.T; ++t) nmx_reref_tile(A, t, c0);
}
static void be_launch_car(const NmxCarArgs& A, be_stream_t st) { NMX_TR(st);
  for (long long t = 0; t < A.T; ++t) nmx_car_sample(A, t);
}
static void be_launch_reref_struct(const NmxRerefStructArgs& A, be_stream_t st) { NMX_TR(st);
  for (long long t = 0; t < A.T; ++t) nmx_reref_struct_sample(A, t);
}
static void be_launch_resample(const NmxResampleArgs& A, int n_items, int, size_t lds, be_stream_t st) { NMX_TR(st);
  std::vector<float> sm(lds / 4 + 16);
  for (int it = 0; it < n_items; ++it) nmx_resample_item(A, it / A.n_channels, it % A.n_channels, sm.data());
}
static void be_launch_rawnorm(const NmxRawNormArgs& A, be_stream_t st) { NMX_TR(st);
  if (A.method >= NMX_RAWNORM_MEDIAN && A.method != NMX_RAWNORM_POWER) {
    std::vector<float> sm(6 * (size_t)A.max_list + 4 * NMX_RAWNORM_ORDER_NT + 288);
    for (int c = 0; c < A.n_channels; ++c) nmx_rawnorm_order_item(A, c, sm.data());
  } else
  for (int c = 0; c < A.n_channels; ++c) nmx_rawnorm_stats_item(A, c);
  const long long n = (long long)A.n_windows * A.n_channels * A.W;
  for (long long i = 0; i < n; ++i) nmx_rawnorm_apply(A, i);
}
static void be_launch_kalman(const NmxKalmanArgs& A, be_stream_t st) { NMX_TR(st);
  for (int c = 0; c < A.n_channels; ++c)
    for (int b = 0; b < A.n_bands; ++b) nmx_kalman_item(A, c, b);
}
static void be_launch_norm(const NmxNormArgs& A, be_stream_t st) { NMX_TR(st);
  for (int j = 0; j < A.n_cols; ++j) nmx_norm_column(A, j);
}
static void be_launch_norm_scan(const NmxNormArgs& A, const NmxNormScan& S, be_stream_t st) { NMX_TR(st);
  for (int g = 0; g < S.n_hseg; ++g)
    for (int j = 0; j < A.n_cols; ++j) nmx_norm_seg_hist(A, S, g, j);
  for (int g = 0; g < S.n_bseg; ++g)
    for (int j = 0; j < A.n_cols; ++j) nmx_norm_seg_batch(A, S, g, j);
  for (int j = 0; j < A.n_cols; ++j) nmx_norm_seg_offsets(A, S, j);
  for (int r = 0; r < A.n_rows; ++r)
    for (int j = 0; j < A.n_cols; ++j) nmx_norm_scan_cell(A, S, r, j);
  for (int r = 0; r < A.n_rows; ++r)
    for (int j = 0; j < A.n_cols; ++j) nmx_norm_scan_ring(A, S, r, j);
}
static void be_launch_power(const NmxPowerPrepArgs& P, const NmxPowerArgs& A, be_stream_t st) { NMX_TR(st);
  for (int e = 0; e < P.have + P.n_rows; ++e)
    for (int j = 0; j < P.n_cols; ++j) nmx_power_prep_at(P, e, j);
  for (int r = 0; r < A.n_rows; ++r)
    for (int j = 0; j < A.n_cols; ++j) nmx_power_cell(A, r, j);
  for (int r = 0; r < P.n_rows; ++r)
    for (int j = 0; j < P.n_cols; ++j) nmx_power_ring_at(P, r, j);
}
static void be_launch_shift(const NmxShiftArgs& A, be_stream_t st) { NMX_TR(st);
  for (int c = 0; c < A.C; ++c)
    for (long long t = 0; t < A.T; ++t) nmx_shift_sample(A, t, c);
}
static void be_launch_reref64(const NmxReref64Args& A, be_stream_t st) { NMX_TR(st);
  for (int c0 = 0; c0 < A.C; c0 += NMX_REREF64_ROWS)
    for (long long t = 0; t < A.T; ++t) nmx_reref64_tile(A, t, c0);
}
static void be_launch_rs64_elem(const NmxResample64Args& A, int mode, const NmxCplx64* src, NmxCplx64* dst, long long n, int rows,
                                be_stream_t st) {
  NMX_TR(st);
  for (int c = 0; c < rows; ++c)
    for (long long i = 0; i < n; ++i) nmx_rs64_elem(A, mode, src, dst, c, i);
}
static void be_launch_rs64_pass(const NmxCplx64* src, NmxCplx64* dst, long long ld, long long n, long long ns, long long st, int sign,
                                int rows, be_stream_t stream) {
  NMX_TR(stream);
  for (int c = 0; c < rows; ++c)
    for (long long t = 0; t < n / 2; ++t) nmx_rs64_pass(src, dst, ld, n, ns, st, sign, c, t);
}
static void be_launch_nanmask(const NmxNanMaskArgs& A, int n_items, be_stream_t st) { NMX_TR(st);
  float sm[64];
  for (int it = 0; it < n_items; ++it) nmx_nanmask_item(A, it / A.C_in, it % A.C_in, sm);
}
static void be_launch_tap(const NmxTapArgs& A, int n_items, be_stream_t st) { NMX_TR(st);
  for (int it = 0; it < n_items; ++it) nmx_tap_item(A, it / A.C, it % A.C);
}

// coherence and the grid projection bring their emulator launchers with them (nmx_k_coh.h, nmx_k_proj.h): traced under
// the launchers' names
#include "../../include/nmx.h"
#define be_launch_coh nmx_emu_coh_items
#define be_launch_proj nmx_emu_proj_items
#include "../../py_neuromodulation_amd/csrc/nmx_k_coh.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_proj.h"
#undef be_launch_coh
#undef be_launch_proj
static void be_launch_coh(const NmxCohArgs& A, int n_items, be_stream_t st) { NMX_TR(st); nmx_emu_coh_items(A, n_items, st); }
static void be_launch_proj(const NmxProjArgs& A, be_stream_t st) { NMX_TR(st); nmx_emu_proj_items(A, st); }

#include "../../py_neuromodulation_amd/csrc/nmx_engine.inc"

// the emulator library's own exports (not part of include/nmx.h)
extern "C" long long nmx_emu_live_blocks(void) { return g_live_blocks.load(); }
extern "C" void nmx_emu_trace_begin(void) { g_trace.clear(); g_tracing = true; }
// stops tracing; -> the length of the trace's text, of which the first min(n, length) bytes go to buf
extern "C" long long nmx_emu_trace_end(char* buf, long long n) {
  g_tracing = false;
  if (buf && n > 0) memcpy(buf, g_trace.data(), std::min<size_t>((size_t)n, g_trace.size()));
  return (long long)g_trace.size();
}
