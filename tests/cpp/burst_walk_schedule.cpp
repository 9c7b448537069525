// burst_walk_schedule.cpp -- the threshold walk's schedule (nmx_burst_walk_plan, nmx_burst_walk_schedule: plan constants and
// one pure function) against the launch-time logic it replaced, over a grid of shapes, selectors, stream ages and chunk
// sizes.  Host only: tests/test_burst_walk_schedule.py builds it with g++ and runs it.
//
// The reference half (ref_*) is a transliteration of that logic and documents the schedule:
//   * ref_wave_ok: "may the one-wave walk take a launch whose sequences have absorbed `windows_seen` hops", as it was
//     evaluated per launch;
//   * ref_schedule: the launch sequence of one chunk -- the fill phase cut short by a linear search for the first hop the
//     one-wave walk may take, a second linear search that splits the rest between the workgroup kernel and the one-wave
//     walk, and the launcher's own re-test (a `windows_seen` of -1 stood for "always the workgroup kernel");
//   * ref_wave_launch: what the one-wave launcher derived at every launch -- registers per lane, the two LDS sizes and the
//     "list in LDS" verdict.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define NMX_HOST_EMU 1
#include "../../py_neuromodulation_amd/csrc/nmx_k_bursts.h"
#include "../../py_neuromodulation_amd/csrc/nmx_k_burst_fill.h"

struct Launch {
  int first, n;
  NmxBurstWalkKind kind;
  int nr;          // WAVE only
  bool list_lds;   // WAVE only
  size_t lds;      // WAVE only
};

static bool ref_wave_ok(const NmxBurstThrArgs& A, long long windows_seen) {
  const int nr = A.overlap <= 128 ? 2 : 4;
  if (windows_seen <= 0 || A.overlap > 256 || A.overlap + 8 >= 192 * nr) return false;
  const long long total = (long long)A.W + (windows_seen - 1) * (long long)A.overlap;
  const long long m_ring = A.n_ring;
  const double pos_ring = A.q * (double)(m_ring - 1);
  const long long lo_ring = (long long)floor(pos_ring);
  const int ia_ring = (int)(m_ring - 1 - lo_ring);
  return A.K > 2 * 256 * nr && total >= m_ring && ia_ring >= A.K - 3 && ia_ring < A.K;
}

static Launch ref_wave_launch(const NmxBurstThrArgs& A, int first, int n, int n_items, long long windows_seen, bool lds_list) {
  const int nr = A.overlap <= 128 ? 2 : 4;
  const size_t base = (size_t)((nr == 2 ? NMX_THRW_LDS_FLOATS_NR(2) : NMX_THRW_LDS_FLOATS_NR(4)) + A.K / 64 + 4) * 4;
  const size_t with_list = (size_t)((nr == 2 ? NMX_THRW_LDS_FLOATS_OF(2, true) : NMX_THRW_LDS_FLOATS_OF(4, true)) + A.K / 64 + 4) * 4 +
                           (size_t)A.K * 4;
  const long long per_round = 256LL * (long long)((160 * 1024) / with_list);
  const bool ll = lds_list && nr == 2 && with_list <= 80 * 1024 && windows_seen < 4096 && (long long)n_items <= 2 * per_round;
  return Launch{first, n, NMX_WALK_WAVE, nr, ll, ll ? with_list : base};
}

// the launcher: windows_seen = -1 -> always the workgroup kernel
static Launch ref_launch_thr(const NmxBurstThrArgs& A, int first, int n, int n_items, long long windows_seen, bool list_lds) {
  if (windows_seen > 0 && ref_wave_ok(A, windows_seen)) return ref_wave_launch(A, first, n, n_items, windows_seen, list_lds);
  return Launch{first, n, NMX_WALK_WORKGROUP, 0, false, 0};
}

static std::vector<Launch> ref_schedule(const NmxBurstThrArgs& T, bool thr_fill, bool thr_wave, bool thr_list_lds,
                                        long long burst_windows_seen, int nw) {
  std::vector<Launch> out;
  const int n_seq = T.n_channels * T.n_bands;
  int done = 0;
  if (thr_fill && burst_windows_seen == 0 && nw >= 2) {
    int n = nmx_burst_fill_hops(T, nw);
    if (thr_wave)
      for (int k = 1; k < n; ++k)
        if (ref_wave_ok(T, k)) { n = k; break; }
    if (n >= 2) {
      out.push_back(Launch{0, n, NMX_WALK_FILL, 0, false, 0});
      done = n;
    }
  }
  if (done < nw) {
    const long long seen = burst_windows_seen + done;
    const int rem = nw - done;
    int k_fill = 0;
    if (thr_wave && !ref_wave_ok(T, seen)) {
      k_fill = rem;
      for (int k = 1; k < rem; ++k)
        if (ref_wave_ok(T, seen + k)) { k_fill = k; break; }
    }
    if (k_fill > 0 && k_fill < rem) {
      out.push_back(ref_launch_thr(T, done, k_fill, n_seq, -1, thr_list_lds));
      out.push_back(ref_launch_thr(T, done + k_fill, rem - k_fill, n_seq, seen + k_fill, thr_list_lds));
    } else {
      out.push_back(ref_launch_thr(T, done, rem, n_seq, thr_wave ? seen : -1, thr_list_lds));
    }
  }
  return out;
}

int main() {
  const int Ws[] = {500, 901, 1000, 2000, 4000};
  const int overlaps[] = {1, 50, 90, 100, 128, 129, 200, 256, 257, 0};   // 0: the window length
  const int rings[] = {2, 3, 100, 499, 500, 501, 900, 1000, 1001, 1999, 2000, 2049, 2500, 4092, 4099, 5000, 8193, 10000, 30000, 59999, 60000};
  const double qs[] = {0.0, 0.5, 0.75, 0.99, 1.0};
  const int channels[] = {2, 520, 800};   // x 2 bands: below and above "two rounds of walks on the chip" for the default history
  const int nws[] = {1, 2, 9, 128, 512, 1024};
  long long n_checked = 0, n_finite = 0, n_wave = 0, n_fill = 0, n_split = 0, n_list = 0, bad = 0;
  for (int W : Ws) for (int ov : overlaps) for (int n_ring : rings) for (double q : qs) for (int C : channels) {
    NmxBurstThrArgs A{};
    A.n_channels = C; A.n_bands = 2; A.W = W; A.q = q; A.n_ring = n_ring;
    A.overlap = ov ? ov : W;
    if (A.overlap > W) continue;   // (build_bursts keeps the overlap within the window)
    A.K = (int)std::floor((1.0 - q) * (double)(n_ring - 1)) + 2;   // (build_bursts)
    if (A.K > n_ring) A.K = n_ring;
    // ---- wave_from against a linear scan of the predicate
    const long long wave_from = nmx_burst_wave_from(A);
    long long scan = NMX_WALK_NEVER;
    for (long long seen = 0; seen <= (long long)n_ring + 2; ++seen)
      if (ref_wave_ok(A, seen)) { scan = seen; break; }
    if (scan != wave_from) {
      if (++bad < 20) printf("wave_from: W %d overlap %d ring %d q %g: %lld, scan %lld\n", W, A.overlap, n_ring, q, wave_from, scan);
      continue;
    }
    if (wave_from != NMX_WALK_NEVER) {
      ++n_finite;
      for (long long seen = wave_from; seen < wave_from + 3; ++seen)   // (and it is a threshold: true from there on)
        if (!ref_wave_ok(A, seen) || !ref_wave_ok(A, seen + 100000)) { ++bad; printf("not a threshold at %lld\n", seen); }
    }
    // ---- the schedule, segment for segment
    for (int sel = 0; sel < 8; ++sel) {
      const bool fill = sel & 1, wave = sel & 2, list_lds = sel & 4;
      const NmxBurstWalk K = nmx_burst_walk_plan(A, fill, wave, list_lds);
      std::vector<long long> seens = {0, 1, 4095, 4096};
      if (wave_from != NMX_WALK_NEVER)
        for (long long s = wave_from - 1; s <= wave_from + 1; ++s) if (s >= 0) seens.push_back(s);
      for (long long seen : seens) for (int nw : nws) {
        const std::vector<Launch> ref = ref_schedule(A, fill, wave, list_lds, seen, nw);
        NmxBurstWalkSeg seg[3];
        const int n_seg = nmx_burst_walk_schedule(K, A, seen, nw, seg);
        bool same = n_seg == (int)ref.size();
        int covered = 0;
        for (int i = 0; same && i < n_seg; ++i) {
          same = seg[i].first == ref[i].first && seg[i].n == ref[i].n && seg[i].kind == ref[i].kind && seg[i].first == covered && seg[i].n > 0;
          covered += seg[i].n;
          if (same && seg[i].kind == NMX_WALK_WAVE) {
            same = K.nr == ref[i].nr && seg[i].list_lds == ref[i].list_lds && (seg[i].list_lds ? K.lds_list : K.lds) == ref[i].lds;
            ++n_wave;
            n_list += seg[i].list_lds;
          } else if (same) {
            same = !seg[i].list_lds;
          }
          n_fill += seg[i].kind == NMX_WALK_FILL;
        }
        same = same && covered == nw;
        n_split += n_seg >= 2;
        ++n_checked;
        if (!same && ++bad < 20)
          printf("schedule: W %d overlap %d ring %d q %g C %d fill %d wave %d list %d seen %lld nw %d: %d segments, reference %d\n", W,
                 A.overlap, n_ring, q, C, fill, wave, list_lds, seen, nw, n_seg, (int)ref.size());
      }
    }
  }
  // every branch was reached
  if (!n_finite || !n_wave || !n_fill || !n_split || !n_list || n_list == n_wave) { printf("the grid misses a branch\n"); ++bad; }
  if (bad) { printf("FAILED: %lld\n", bad); return 1; }
  printf("OK %lld schedules (%lld shapes with a one-wave walk; segments: %lld fill, %lld one-wave, %lld of them with the list in LDS; "
         "%lld chunks of several launches)\n", n_checked, n_finite, n_fill, n_wave, n_list, n_split);
  return 0;
}
