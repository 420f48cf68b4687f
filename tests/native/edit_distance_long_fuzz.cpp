// edit_distance_long_fuzz.cpp — drives csrc/edit_distance_long.h (the recurrence of the long-sequence distance kernel, the whole host
// twin and the check both entry points make of their host arrays) over garbage tokens and offset arrays under the address and
// undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size, so a read or write one element outside it is
// a report.  Every distance is compared with the textbook dynamic programme under the same rule (a token outside [0, v) equals
// nothing).  usage: edit_distance_long_fuzz [rounds]; prints "rounds <n> checked <pairs>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "edit_distance_long.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }  // inclusive
static int32_t garbage() {
  switch (rnd() % 6) {
    case 0: return INT32_MAX;
    case 1: return INT32_MIN;
    case 2: return -1;
    case 3: return (int32_t)rnd();
    default: return (int32_t)(rnd() % 1200);
  }
}

static int dp(const int32_t* a, int m, const int32_t* b, int n, int v) {
  std::vector<int> prev(n + 1), cur(n + 1);
  for (int j = 0; j <= n; ++j) prev[j] = j;
  for (int i = 1; i <= m; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      const bool eq = a[i - 1] == b[j - 1] && a[i - 1] >= 0 && a[i - 1] < v;
      int d = prev[j - 1] + (eq ? 0 : 1);
      if (prev[j] + 1 < d) d = prev[j] + 1;
      if (cur[j - 1] + 1 < d) d = cur[j - 1] + 1;
      cur[j] = d;
    }
    prev.swap(cur);
  }
  return prev[n];
}

static int check_heads() {  // offset arrays of exact size, good and bad
  for (int it = 0; it < 400; ++it) {
    const int N = rnd_in(0, 6);
    std::unique_ptr<int32_t[]> a(new int32_t[N + 1]), b(new int32_t[N + 1]), v(new int32_t[N > 0 ? N : 1]);
    a[0] = rnd_in(0, 5);
    b[0] = rnd_in(0, 5);
    int64_t want = (int64_t)N * (int64_t)sizeof(edl_pair);
    for (int p = 0; p < N; ++p) {
      a[p + 1] = a[p] + rnd_in(0, 300);
      b[p + 1] = b[p] + rnd_in(0, 300);
      v[p] = rnd_in(0, 40);
      want += (int64_t)v[p] * ((a[p + 1] - a[p] + 63) / 64) * 8;
    }
    if (edl_check_heads(a.get(), b.get(), v.get(), N) != want) { printf("workspace formula\n"); return 1; }
    if (N == 0) continue;
    std::unique_ptr<edl_pair[]> heads(new edl_pair[N]);
    edl_fill_heads(a.get(), b.get(), v.get(), N, heads.get());
    for (int p = 0; p < N; ++p)
      if (heads[p].m != a[p + 1] - a[p] || heads[p].n != b[p + 1] - b[p] || heads[p].nb != edl_nblocks(heads[p].m)) { printf("heads\n"); return 1; }
    const int p = rnd_in(0, N - 1);
    switch (rnd() % 5) {  // one corruption: refused whatever the rest holds
      case 0: a[p + 1] = a[p] - 1 - (int32_t)(rnd() % 9); break;
      case 1: b[p + 1] = b[p] + MSOCR_EDL_MAX_LEN + 1; break;
      case 2: v[p] = rnd() % 2 ? -1 : INT32_MIN; break;
      case 3: a[0] = -1 - (int32_t)(rnd() % 9); break;
      default: b[p] = INT32_MAX; b[p + 1] = INT32_MIN; break;
    }
    if (edl_check_heads(a.get(), b.get(), v.get(), N) >= 0) { printf("corrupt heads accepted\n"); return 1; }
  }
  if (edl_check_heads(nullptr, nullptr, nullptr, -1) >= 0 || edl_check_heads(nullptr, nullptr, nullptr, 3) >= 0) { printf("null heads\n"); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  if (check_heads()) return 1;
  long checked = 0;
  static const int edges[12] = {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 700};
  for (int it = 0; it < rounds; ++it) {
    static const int Vs[5] = {1, 2, 4, 30, 1000};
    const int v = Vs[rnd() % 5];
    const int m = rnd() % 3 ? edges[rnd() % 12] : rnd_in(0, 400);
    const int n = rnd() % 3 ? edges[rnd() % 12] : rnd_in(0, 400);
    const bool wild = rnd() % 3 == 0;
    std::unique_ptr<int32_t[]> a(new int32_t[m]), b(new int32_t[n]);
    for (int j = 0; j < m; ++j) a[j] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (uint32_t)v);
    for (int j = 0; j < n; ++j) b[j] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (uint32_t)(v + 2));
    const int nb = edl_nblocks(m);
    std::unique_ptr<uint64_t[]> tab(new uint64_t[(size_t)edl_table_words(m, v)]), pv(new uint64_t[nb]), mv(new uint64_t[nb]);
    edl_build_table_host(a.get(), m, v, tab.get());
    const int got = edl_distance_host(tab.get(), m, v, b.get(), n, pv.get(), mv.get());
    const int want = dp(a.get(), m, b.get(), n, v);
    if (got != want) { printf("distance %d, dynamic programme %d (m %d n %d v %d)\n", got, want, m, n, v); return 1; }
    ++checked;
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
