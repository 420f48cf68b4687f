// text_search_fuzz.cpp — drives csrc/text_search.h (the forward scan, the segment window the kernel cuts a text by, the backward start
// walk, the whole host twin, the selection and the check every entry point makes of its host arrays) over garbage tokens and offset
// arrays under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size, so a read or
// write one element outside it is a report.  Every hit list is compared with the plain Sellers table and, for the starts, with the
// plain global table of the pattern against every substring that ends at the hit; the scan cut into segments must give the uncut
// scan's hits.  usage: text_search_fuzz [rounds]; prints "rounds <n> checked <n>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "text_search.h"

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
    default: return (int32_t)(rnd() % 2100);
  }
}
static bool same(int32_t x, int32_t y, int v) { return x == y && x >= 0 && x < v; }

// plain global distance between a [m] and b [n]
static int dp(const int32_t* a, int m, const int32_t* b, int n, int v) {
  std::vector<int> prev(n + 1), cur(n + 1);
  for (int j = 0; j <= n; ++j) prev[j] = j;
  for (int i = 1; i <= m; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      int d = prev[j - 1] + (same(a[i - 1], b[j - 1], v) ? 0 : 1);
      if (prev[j] + 1 < d) d = prev[j] + 1;
      if (cur[j - 1] + 1 < d) d = cur[j - 1] + 1;
      cur[j] = d;
    }
    prev.swap(cur);
  }
  return prev[n];
}

// the smallest l with ed(a, b[j - l .. j)) == s: ed(a, x) = ed(reversed a, reversed x), so the bottom row of one plain global table of
// the reversed pattern against b[j-1], b[j-2], .. holds the distance for every l; every 16th hit also asks dp() itself
static int shortest(const int32_t* a, int m, const int32_t* b, int j, int s, int v) {
  std::vector<int> prev(j + 1), cur(j + 1);
  for (int l = 0; l <= j; ++l) prev[l] = l;
  for (int i = 1; i <= m; ++i) {
    cur[0] = i;
    for (int l = 1; l <= j; ++l) {
      int d = prev[l - 1] + (same(a[m - i], b[j - l], v) ? 0 : 1);
      if (prev[l] + 1 < d) d = prev[l] + 1;
      if (cur[l - 1] + 1 < d) d = cur[l - 1] + 1;
      cur[l] = d;
    }
    prev.swap(cur);
  }
  int l = 0;
  while (l <= j && prev[l] != s) ++l;
  static unsigned calls = 0;
  if (l > j || (calls++ % 16 == 0 && (dp(a, m, b + (j - l), l, v) != s || (l > 0 && dp(a, m, b + (j - l + 1), l - 1, v) == s)))) {
    printf("the yardstick disagrees with itself\n");
    exit(1);
  }
  return l;
}

// the hits of a [m] with bound k in b [n] by the plain Sellers table
static void plain_hits(const int32_t* a, int m, int k, const int32_t* b, int n, int v, int32_t q, int32_t t, std::vector<msocr_search_hit>& out) {
  std::vector<int> prev(n + 1, 0), cur(n + 1);
  for (int i = 1; i <= m; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      int d = prev[j - 1] + (same(a[i - 1], b[j - 1], v) ? 0 : 1);
      if (prev[j] + 1 < d) d = prev[j] + 1;
      if (cur[j - 1] + 1 < d) d = cur[j - 1] + 1;
      cur[j] = d;
    }
    prev.swap(cur);
  }
  for (int j = 1; j <= n; ++j) {
    if (prev[j] > k) continue;
    out.push_back(msocr_search_hit{q, t, j - shortest(a, m, b, j, prev[j], v), j, prev[j]});
  }
}

static bool equal_hit(const msocr_search_hit& x, const msocr_search_hit& y) {
  return x.pattern == y.pattern && x.text == y.text && x.start == y.start && x.end == y.end && x.distance == y.distance;
}

static int check_args() {  // offset arrays of exact size, good and bad
  for (int it = 0; it < 400; ++it) {
    const int Q = rnd_in(1, 5), T = rnd_in(1, 5), v = rnd_in(1, MSOCR_SEARCH_MAX_ALPHABET);
    std::unique_ptr<int32_t[]> po(new int32_t[Q + 1]), k(new int32_t[Q]), to(new int32_t[T + 1]);
    po[0] = rnd_in(0, 5);
    to[0] = rnd_in(0, 5);
    for (int q = 0; q < Q; ++q) {
      const int m = rnd() % 4 ? rnd_in(1, 64) : (rnd() % 2 ? 1 : 64);
      po[q + 1] = po[q] + m;
      k[q] = rnd_in(0, m - 1);
    }
    int64_t segs = 0;
    for (int t = 0; t < T; ++t) {
      to[t + 1] = to[t] + (rnd() % 3 ? rnd_in(0, 300) : 0);
      segs += (to[t + 1] - to[t] + MSOCR_SEARCH_SEGMENT - 1) / MSOCR_SEARCH_SEGMENT;
    }
    const int64_t want = ((int64_t)16 * Q * v + 8 * (T + 1) + 4 * (T + 1) + 4 * (Q + 1) + 4 * Q + 7) / 8 * 8;
    ts_layout lay;
    if (ts_check(po.get(), k.get(), Q, to.get(), T, v, &lay) != want || lay.total != want || lay.segments != segs) { printf("workspace formula\n"); return 1; }
    if (ts_check(nullptr, nullptr, 0, to.get(), T, v, nullptr) != 0 || ts_check(po.get(), k.get(), Q, nullptr, 0, v, nullptr) != 0) { printf("empty side\n"); return 1; }
    std::unique_ptr<unsigned char[]> heads(new unsigned char[(size_t)(lay.total - lay.seg_pre)]);
    ts_fill_heads(po.get(), k.get(), Q, to.get(), T, lay, heads.get());
    const int64_t* sp = (const int64_t*)heads.get();
    const int32_t* ho = (const int32_t*)(heads.get() + (lay.txt_off - lay.seg_pre));
    const int32_t* hk = (const int32_t*)(heads.get() + (lay.max_dist - lay.seg_pre));
    if (sp[0] != 0 || sp[T] != segs || ho[T] != to[T] || hk[Q - 1] != k[Q - 1]) { printf("heads\n"); return 1; }
    const int q = rnd_in(0, Q - 1), t = rnd_in(0, T - 1);
    int vv = v;
    switch (rnd() % 8) {  // one corruption: refused whatever the rest holds
      case 0: po[q + 1] = po[q] - (int32_t)(rnd() % 9); break;        // a length below 1
      case 1: po[q + 1] = po[q] + 65 + (int32_t)(rnd() % 9); break;
      case 2: k[q] = po[q + 1] - po[q]; break;                          // k == m
      case 3: k[q] = rnd() % 2 ? -1 : INT32_MIN; break;
      case 4: to[t + 1] = to[t] - 1 - (int32_t)(rnd() % 9); break;
      case 5: to[0] = -1 - (int32_t)(rnd() % 9); break;
      case 6: vv = rnd() % 2 ? 0 : MSOCR_SEARCH_MAX_ALPHABET + 1; break;
      default: to[t] = INT32_MAX; to[t + 1] = INT32_MIN; break;
    }
    if (ts_check(po.get(), k.get(), Q, to.get(), T, vv, nullptr) >= 0) { printf("corrupt arrays accepted\n"); return 1; }
  }
  if (ts_check(nullptr, nullptr, -1, nullptr, 0, 5, nullptr) >= 0 || ts_check(nullptr, nullptr, 0, nullptr, -1, 5, nullptr) >= 0 ||
      ts_check(nullptr, nullptr, 2, nullptr, 0, 5, nullptr) >= 0 || ts_check(nullptr, nullptr, 0, nullptr, 2, 5, nullptr) >= 0) { printf("null arrays\n"); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  if (check_args()) return 1;
  long checked = 0;
  static const int m_edges[8] = {1, 2, 31, 32, 33, 63, 64, 5};
  static const int Vs[5] = {1, 2, 4, 60, MSOCR_SEARCH_MAX_ALPHABET};
  const int L = MSOCR_SEARCH_SEGMENT;
  for (int it = 0; it < rounds; ++it) {
    const int v = Vs[rnd() % 5];
    const bool wild = rnd() % 3 == 0;
    const int Q = rnd_in(1, 3), T = rnd_in(1, 4);
    // patterns and texts in heap blocks of their exact size
    std::vector<int> ms(Q), ns(T);
    std::unique_ptr<int32_t[]> po(new int32_t[Q + 1]), ks(new int32_t[Q]), to(new int32_t[T + 1]);
    po[0] = 0;
    to[0] = 0;
    for (int q = 0; q < Q; ++q) {
      ms[q] = rnd() % 2 ? m_edges[rnd() % 8] : rnd_in(1, 64);
      ks[q] = rnd() % 4 == 0 ? ms[q] - 1 : rnd_in(0, ms[q] - 1 < 3 ? ms[q] - 1 : 3);
      po[q + 1] = po[q] + ms[q];
    }
    static const int n_edges[10] = {0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 3 * L + 7, 0, 5};
    for (int t = 0; t < T; ++t) {
      ns[t] = rnd() % 2 ? n_edges[rnd() % 10] : rnd_in(0, 260);
      to[t + 1] = to[t] + ns[t];
    }
    std::unique_ptr<int32_t[]> pat(new int32_t[po[Q]]), txt(new int32_t[to[T]]);
    for (int i = 0; i < po[Q]; ++i) pat[i] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (uint32_t)(v < 5 ? v : 5));
    for (int i = 0; i < to[T]; ++i) txt[i] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (uint32_t)((v < 5 ? v : 5) + 1));
    for (int t = 0; t < T; ++t)  // plant the first pattern, whole or without its first token, at the end of every text that has room
      for (int i = 0; i < ms[0] && ms[0] <= ns[t]; ++i) txt[to[t] + ns[t] - ms[0] + i] = i == 0 && rnd() % 2 ? -1 : pat[i];
    if (ts_check(po.get(), ks.get(), Q, to.get(), T, v, nullptr) <= 0) { printf("good arrays refused\n"); return 1; }

    std::vector<msocr_search_hit> want;
    for (int q = 0; q < Q; ++q)
      for (int t = 0; t < T; ++t) plain_hits(pat.get() + po[q], ms[q], ks[q], txt.get() + to[t], ns[t], v, q, t, want);

    // the host twin at a capacity below, at and above the count: exact count, canonical prefix, nothing behind the capacity
    std::unique_ptr<uint64_t[]> rows(new uint64_t[2 * (size_t)v]);
    const int64_t total = (int64_t)want.size();
    const int64_t caps[3] = {total, total > 0 ? (int64_t)(rnd() % (uint32_t)total) : 0, total + 3};
    for (int64_t cap : caps) {
      std::unique_ptr<msocr_search_hit[]> got(new msocr_search_hit[(size_t)cap]);
      const int64_t count = ts_search_host(pat.get(), po.get(), ks.get(), Q, txt.get(), to.get(), T, v, got.get(), cap, rows.get());
      if (count != total) { printf("count %lld, plain table %lld\n", (long long)count, (long long)total); return 1; }
      for (int64_t i = 0; i < (cap < total ? cap : total); ++i)
        if (!equal_hit(got[(size_t)i], want[(size_t)i])) {
          printf("hit %lld: (%d %d %d %d %d), plain table (%d %d %d %d %d)\n", (long long)i, got[i].pattern, got[i].text, got[i].start, got[i].end,
                 got[i].distance, want[i].pattern, want[i].text, want[i].start, want[i].end, want[i].distance);
          return 1;
        }
    }

    // the scan cut into segments as the kernel cuts it: the same hits
    std::vector<msocr_search_hit> cut((size_t)total + 1);
    int64_t found = 0;
    for (int q = 0; q < Q; ++q) {
      ts_build_rows_host(pat.get() + po[q], ms[q], v, rows.get());
      for (int t = 0; t < T; ++t)
        for (int64_t s = 0; s < ts_segments(ns[t]); ++s) {
          int first, lo, hi;
          ts_window(ns[t], s, ms[q] + ks[q], first, lo, hi);
          if (first < 0 || first > lo || lo >= hi || hi > ns[t] || hi - lo > L) { printf("window\n"); return 1; }
          found += ts_scan_host(rows.get(), v, ms[q], ks[q], txt.get() + to[t], first, lo, hi, q, t, cut.data(), total, found < total ? found : total);
        }
    }
    if (found != total) { printf("cut scan: %lld hits, uncut %lld\n", (long long)found, (long long)total); return 1; }
    for (int64_t i = 0; i < total; ++i)
      if (!equal_hit(cut[(size_t)i], want[(size_t)i])) { printf("cut scan: hit %lld differs\n", (long long)i); return 1; }

    // the selection on a shuffled copy: canonical, disjoint within a (pattern, text), and nothing left out that fits
    std::unique_ptr<msocr_search_hit[]> sel(new msocr_search_hit[(size_t)total]);
    for (int64_t i = 0; i < total; ++i) sel[(size_t)i] = want[(size_t)i];
    for (int64_t i = total - 1; i > 0; --i) std::swap(sel[(size_t)i], sel[(size_t)(rnd() % (uint32_t)(i + 1))]);
    const int64_t kept = ts_select(sel.get(), total);
    if (kept < 0 || kept > total || (total > 0 && kept == 0)) { printf("selection count\n"); return 1; }
    for (int64_t i = 0; i + 1 < kept; ++i) {
      const msocr_search_hit &x = sel[(size_t)i], &y = sel[(size_t)i + 1];
      if (!ts_canonical_less(x, y)) { printf("selection order\n"); return 1; }
      if (x.pattern == y.pattern && x.text == y.text && x.end > y.start) { printf("selection overlap\n"); return 1; }
    }
    for (const msocr_search_hit& w : want) {  // a hit that was dropped intersects a kept hit that comes no later in (distance, end)
      bool is_kept = false, blocked = false;
      for (int64_t i = 0; i < kept; ++i) {
        const msocr_search_hit& x = sel[(size_t)i];
        if (equal_hit(x, w)) is_kept = true;
        if (x.pattern == w.pattern && x.text == w.text && x.start < w.end && w.start < x.end &&
            (x.distance < w.distance || (x.distance == w.distance && x.end < w.end)))
          blocked = true;
      }
      if (is_kept == blocked) { printf("selection rule\n"); return 1; }
    }
    ++checked;
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
