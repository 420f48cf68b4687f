// edit_alignment_fuzz.cpp — drives csrc/edit_alignment.h (the step with its trace words, the rule, the whole host twin, and the
// argument check and workspace arithmetic of both entry points) over garbage tokens and offset arrays under the address and
// undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size, so a read or write one element outside it
// is a report.  Every alignment is compared with the full table walked back by the four rules under the same matching rule (a token
// outside [0, v) equals nothing), and the step with edl_advance word for word.
// usage: edit_alignment_fuzz [rounds]; prints "rounds <n> checked <pairs>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "edit_alignment.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static uint64_t rnd64() { return ((uint64_t)rnd() << 40) ^ ((uint64_t)rnd() << 20) ^ rnd(); }
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

// the four rules on the full table
static void table_alignment(const int32_t* a, int m, const int32_t* b, int n, int v, std::vector<int32_t>& a_map,
                            std::vector<int32_t>& b_map, int32_t* counts, int* dist) {
  std::vector<int> D((size_t)(m + 1) * (n + 1));
  const int W = n + 1;
  auto eq = [&](int i, int j) { return a[i - 1] == b[j - 1] && a[i - 1] >= 0 && a[i - 1] < v; };
  for (int j = 0; j <= n; ++j) D[j] = j;
  for (int i = 1; i <= m; ++i) {
    D[(size_t)i * W] = i;
    for (int j = 1; j <= n; ++j) {
      int d = D[(size_t)(i - 1) * W + j - 1] + (eq(i, j) ? 0 : 1);
      if (D[(size_t)(i - 1) * W + j] + 1 < d) d = D[(size_t)(i - 1) * W + j] + 1;
      if (D[(size_t)i * W + j - 1] + 1 < d) d = D[(size_t)i * W + j - 1] + 1;
      D[(size_t)i * W + j] = d;
    }
  }
  *dist = D[(size_t)m * W + n];
  a_map.assign(m, -1);
  b_map.assign(n, -1);
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  int i = m, j = n;
  while (i > 0 && j > 0) {
    const int here = D[(size_t)i * W + j];
    if (eq(i, j) || D[(size_t)(i - 1) * W + j - 1] + 1 == here) {
      ++counts[eq(i, j) ? EAL_HIT : EAL_SUB];
      a_map[i - 1] = j - 1;
      b_map[j - 1] = i - 1;
      --i;
      --j;
    } else if (D[(size_t)(i - 1) * W + j] + 1 == here) {
      ++counts[EAL_DEL];
      --i;
    } else {
      ++counts[EAL_INS];
      --j;
    }
  }
  counts[EAL_DEL] += i;
  counts[EAL_INS] += j;
}

static int check_step() {  // eal_advance is edl_advance plus a word
  for (int it = 0; it < 20000; ++it) {
    uint64_t pv = rnd64(), mv = rnd64() & ~pv, eq = rnd64() & rnd64(), d0;
    uint64_t pv2 = pv, mv2 = mv;
    const int hin = rnd_in(-1, 1), top = rnd_in(0, 63);
    const int h = edl_advance(pv, mv, eq, hin, top), h2 = eal_advance(pv2, mv2, eq, hin, top, d0);
    if (h != h2 || pv != pv2 || mv != mv2) { printf("step\n"); return 1; }
  }
  return 0;
}

static int check_heads() {  // offset arrays of exact size, good and bad
  for (int it = 0; it < 400; ++it) {
    const int N = rnd_in(0, 6);
    std::unique_ptr<int32_t[]> a(new int32_t[N + 1]), b(new int32_t[N + 1]), v(new int32_t[N > 0 ? N : 1]);
    a[0] = rnd_in(0, 5);
    b[0] = rnd_in(0, 5);
    int64_t want = (int64_t)N * 40, cells = 0;
    std::vector<int64_t> starts;
    for (int p = 0; p < N; ++p) {
      a[p + 1] = a[p] + rnd_in(0, 300);
      b[p + 1] = b[p] + rnd_in(0, 300);
      v[p] = rnd_in(0, 40);
      const int64_t nb = (a[p + 1] - a[p] + 63) / 64;
      want += (int64_t)v[p] * nb * 8;
      starts.push_back(cells);
      cells += nb * (b[p + 1] - b[p]);
    }
    want = (want + 15) / 16 * 16 + cells * 16;
    eal_layout lay;
    if (eal_check_heads(a.get(), b.get(), v.get(), N, &lay) != want) { printf("workspace formula\n"); return 1; }
    if (N == 0) continue;
    if (lay.trace_off != 32ll * N || lay.tables != 40ll * N || lay.trace % 16 || lay.trace < lay.tables + lay.table_words * 8 ||
        lay.total != want) { printf("layout\n"); return 1; }
    std::unique_ptr<int64_t[]> off(new int64_t[N]);
    eal_fill_trace_offsets(a.get(), b.get(), N, off.get());
    for (int p = 0; p < N; ++p)
      if (off[p] != starts[p]) { printf("trace offsets\n"); return 1; }
    const int p = rnd_in(0, N - 1);
    switch (rnd() % 5) {  // one corruption: refused whatever the rest holds
      case 0: a[p + 1] = a[p] - 1 - (int32_t)(rnd() % 9); break;
      case 1: b[p + 1] = b[p] + MSOCR_EDL_MAX_LEN + 1; break;
      case 2: v[p] = rnd() % 2 ? -1 : INT32_MIN; break;
      case 3: a[0] = -1 - (int32_t)(rnd() % 9); break;
      default: b[p] = INT32_MAX; b[p + 1] = INT32_MIN; break;
    }
    if (eal_check_heads(a.get(), b.get(), v.get(), N) >= 0) { printf("corrupt heads accepted\n"); return 1; }
  }
  if (eal_check_heads(nullptr, nullptr, nullptr, -1) >= 0 || eal_check_heads(nullptr, nullptr, nullptr, 3) >= 0) { printf("null heads\n"); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  if (check_step() || check_heads()) return 1;
  long checked = 0;
  static const int edges[12] = {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 700};
  for (int it = 0; it < rounds; ++it) {
    static const int Vs[6] = {0, 1, 2, 4, 30, 1000};
    const int v = Vs[rnd() % 6];
    const int m = rnd() % 3 ? edges[rnd() % 12] : rnd_in(0, 400);
    const int n = rnd() % 3 ? edges[rnd() % 12] : rnd_in(0, 400);
    const bool wild = rnd() % 3 == 0, copy = rnd() % 2 == 0;
    std::unique_ptr<int32_t[]> a(new int32_t[m]), b(new int32_t[n]);
    for (int j = 0; j < m; ++j) a[j] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (uint32_t)(v + 1));
    for (int j = 0; j < n; ++j)  // an edited copy of the pattern, or tokens of its own
      b[j] = wild && rnd() % 4 == 0 ? garbage() : (copy && m > 0 && rnd() % 8) ? a[j % m] : (int32_t)(rnd() % (uint32_t)(v + 2));
    const int nb = edl_nblocks(m);
    std::unique_ptr<uint64_t[]> tab(new uint64_t[(size_t)edl_table_words(m, v)]), pv(new uint64_t[nb]), mv(new uint64_t[nb]);
    std::unique_ptr<eal_cell[]> trace(new eal_cell[(size_t)eal_trace_cells(m, n)]);
    std::unique_ptr<int32_t[]> a_map(new int32_t[m]), b_map(new int32_t[n]);
    int32_t counts[4], want_counts[4];
    edl_build_table_host(a.get(), m, v, tab.get());
    int got = m == 0 ? n : m;
    if (m > 0 && n > 0) got = eal_forward_host(tab.get(), m, v, b.get(), n, pv.get(), mv.get(), trace.get());
    eal_traceback_host(tab.get(), m, v, b.get(), n, trace.get(), a_map.get(), b_map.get(), counts);
    std::vector<int32_t> want_a, want_b;
    int want;
    table_alignment(a.get(), m, b.get(), n, v, want_a, want_b, want_counts, &want);
    if (got != want) { printf("distance %d, dynamic programme %d (m %d n %d v %d)\n", got, want, m, n, v); return 1; }
    if (m > 0 && n > 0 && got != edl_distance_host(tab.get(), m, v, b.get(), n, pv.get(), mv.get())) { printf("the two sweeps differ\n"); return 1; }
    for (int k = 0; k < 4; ++k)
      if (counts[k] != want_counts[k]) { printf("counts[%d] %d, table %d (m %d n %d v %d)\n", k, counts[k], want_counts[k], m, n, v); return 1; }
    for (int i = 0; i < m; ++i)
      if (a_map[i] != want_a[i]) { printf("a_map[%d] %d, table %d (m %d n %d v %d)\n", i, a_map[i], want_a[i], m, n, v); return 1; }
    for (int j = 0; j < n; ++j)
      if (b_map[j] != want_b[j]) { printf("b_map[%d] %d, table %d (m %d n %d v %d)\n", j, b_map[j], want_b[j], m, n, v); return 1; }
    ++checked;
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
