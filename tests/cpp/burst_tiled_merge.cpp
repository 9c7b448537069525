// burst_tiled_merge.cpp -- nmx_merge_into_tiled (nmx_k_bursts.h: the merge of a top-K list beyond 65 536 entries) against
// std::merge + truncate.  Host only: the same source compiled single-threaded (a tile is NMX_NT x NMX_THR_TILE_E = 8 entries
// here), built with -fsanitize=address,undefined by tests/test_burst_tiled_merge.py.  Every vector is sized exactly -- the
// list K floats, the new samples and their insertion indices n_new -- so an access beyond them is the sanitizer's to find.
//
// Semantics under test: descending order; equal values: list entries first; truncation at K; the entries of L beyond the
// returned length are not specified.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#define NMX_HOST_EMU 1
#include "../../py_neuromodulation_amd/csrc/nmx_k_bursts.h"

static const int TILE = NMX_NT * NMX_THR_TILE_E;
static long long n_cases = 0;

// (equal floats are the same float: which of two equal values came from the list does not show in the result -- the tie
// rule decides only WHERE the kernel writes, and the cases with many ties check that those writes stay a bijection)
static bool check(const std::vector<float>& list, int K, const std::vector<float>& fresh, const char* what) {
  const int len = (int)list.size(), n_new = (int)fresh.size();
  std::vector<float> want(len + n_new);
  std::merge(list.begin(), list.end(), fresh.begin(), fresh.end(), want.begin(), std::greater<float>());
  const int keep = std::min(len + n_new, K);
  std::vector<float> L(K);   // exactly K floats
  std::copy(list.begin(), list.end(), L.begin());
  for (int i = len; i < K; ++i) L[i] = -12345.f;   // (stale entries behind the list: never read)
  std::vector<float> ps(fresh);
  std::vector<int> ins(std::max(n_new, 1), -1);
  const int got = nmx_merge_into_tiled(L.data(), len, K, ps.data(), ins.data(), n_new);
  ++n_cases;
  if (got != keep) {
    printf("FAIL %s: len %d K %d n_new %d -> length %d, want %d\n", what, len, K, n_new, got, keep);
    return false;
  }
  for (int i = 0; i < keep; ++i)
    if (L[i] != want[i]) {
      printf("FAIL %s: len %d K %d n_new %d: entry %d is %g, want %g\n", what, len, K, n_new, i, L[i], want[i]);
      return false;
    }
  return true;
}

static std::vector<float> sorted_desc(std::mt19937& g, int n, float lo, float hi, int distinct = 0) {
  std::vector<float> v(n);
  std::uniform_real_distribution<float> u(lo, hi);
  std::uniform_int_distribution<int> d(0, distinct > 0 ? distinct - 1 : 0);
  for (float& x : v) x = distinct > 0 ? lo + (hi - lo) * (float)d(g) / (float)distinct : u(g);
  std::sort(v.begin(), v.end(), std::greater<float>());
  return v;
}

int main() {
  std::mt19937 g(20240607);
  bool ok = true;
  // lengths around tile multiples, K one below / at / one above a tile multiple, len + n_new below / at / across K
  std::vector<int> lens = {0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 5 * TILE - 1, 5 * TILE, 5 * TILE + 1, 37, 100};
  std::vector<int> news = {1, 2, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 64};
  for (int len : lens)
    for (int n_new : news)
      for (int K : {len + n_new + 9, len + n_new + 1, len + n_new, len + n_new - 1, len + 1, len, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1}) {
        if (K < len || K < 1) continue;
        // random, few distinct values (many ties between the list and the new samples), all equal
        ok &= check(sorted_desc(g, len, 0.f, 1.f), K, sorted_desc(g, n_new, 0.f, 1.f), "random");
        ok &= check(sorted_desc(g, len, 0.f, 1.f, 4), K, sorted_desc(g, n_new, 0.f, 1.f, 4), "ties");
        ok &= check(std::vector<float>(len, 0.5f), K, std::vector<float>(n_new, 0.5f), "all equal");
        // every new sample above the head / below the tail / equal to the tail (sorts behind it: "list entries first")
        ok &= check(sorted_desc(g, len, 0.f, 1.f), K, sorted_desc(g, n_new, 2.f, 3.f), "above the head");
        ok &= check(sorted_desc(g, len, 0.f, 1.f), K, sorted_desc(g, n_new, -3.f, -2.f), "below the tail");
        if (len > 0) {
          const std::vector<float> l = sorted_desc(g, len, 0.f, 1.f);
          ok &= check(l, K, std::vector<float>(n_new, l.back()), "equal to the tail");
          ok &= check(l, K, std::vector<float>(n_new, l.front()), "equal to the head");
        }
        // new samples inside one tile only (the second): the tiles above it shift whole, the first stays
        if (len >= 2 * TILE) {
          const std::vector<float> l = sorted_desc(g, len, 0.f, 1.f);
          std::vector<float> f(n_new);
          for (int j = 0; j < n_new; ++j) f[j] = l[TILE + (j % TILE)];
          std::sort(f.begin(), f.end(), std::greater<float>());
          ok &= check(l, K, f, "inside one tile");
        }
        if (!ok) return 1;
      }
  // ties at the cut: a full list whose tail equals the new sample is left as it is (the early return)
  {
    std::vector<float> l = {5.f, 4.f, 3.f, 3.f};
    ok &= check(l, 4, {3.f}, "tie at the cut");   // (returns before any search: nothing changes)
    ok &= check(l, 5, {3.f, 3.f}, "tie across the cut");
  }
  // a long list, random shapes
  for (int rep = 0; rep < 300 && ok; ++rep) {
    const int len = std::uniform_int_distribution<int>(0, 3000)(g), n_new = std::uniform_int_distribution<int>(1, 500)(g);
    const int K = len + std::uniform_int_distribution<int>(0, n_new + 5)(g);
    if (K < 1) continue;
    ok &= check(sorted_desc(g, len, 0.f, 1.f, rep % 3 == 0 ? 50 : 0), K, sorted_desc(g, n_new, -0.2f, 1.2f, rep % 3 == 0 ? 50 : 0), "long random");
  }
  if (!ok) return 1;
  printf("OK %lld merges, tile %d\n", n_cases, TILE);
  return 0;
}
