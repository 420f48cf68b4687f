// text_search_weighted_fuzz.cpp — drives csrc/text_search_weighted.h (the cost functions, the host twin with its backward start walk,
// the profile entries and the packed-key column step the kernel runs, the argument check) over garbage tokens, classes, offsets and
// cost tables under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size, so a read or
// write one element outside it is a report.  Every hit list is compared with a plain table written here: the semi-global weighted
// table for ends and distances, and for the start the plain global table of the pattern against every substring that ends at the
// hit.  Where no delete costs 0 (what msocr_edit_costs_check_host demands), the kernel's form, run on the host segment by segment
// from profiles built as the kernel builds them, must give the same records.
// usage: text_search_weighted_fuzz [rounds]; prints "rounds <n> checked <n>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "text_search_weighted.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
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
    default: return (int32_t)(rnd() % 800);
  }
}

// ---- the yardstick: the contract of include/msocr.h restated without the header's functions
struct plain {
  const uint8_t *sub, *del, *ins;
  const int32_t* cls;
  int V, unknown, v;
  int klass(int32_t t) const {
    if (t < 0 || t >= v) return -1;
    return cls[t] >= 0 && cls[t] < V ? cls[t] : -1;
  }
  int w_sub(int32_t t, int32_t p) const {
    if (t == p && t >= 0 && t < v) return 0;
    const int ct = klass(t), cp = klass(p);
    return ct >= 0 && cp >= 0 ? sub[(size_t)ct * V + cp] : unknown;
  }
  int w_del(int32_t t) const { return klass(t) >= 0 ? del[klass(t)] : unknown; }
  int w_ins(int32_t p) const { return klass(p) >= 0 ? ins[klass(p)] : unknown; }
  // weighted global distance between a [m] and b [n]
  int global(const int32_t* a, int m, const int32_t* b, int n) const {
    std::vector<int> prev(m + 1), cur(m + 1);
    prev[0] = 0;
    for (int i = 1; i <= m; ++i) prev[i] = prev[i - 1] + w_ins(a[i - 1]);
    for (int j = 1; j <= n; ++j) {
      cur[0] = prev[0] + w_del(b[j - 1]);
      for (int i = 1; i <= m; ++i) {
        int d = prev[i - 1] + w_sub(b[j - 1], a[i - 1]);
        if (prev[i] + w_del(b[j - 1]) < d) d = prev[i] + w_del(b[j - 1]);
        if (cur[i - 1] + w_ins(a[i - 1]) < d) d = cur[i - 1] + w_ins(a[i - 1]);
        cur[i] = d;
      }
      prev.swap(cur);
    }
    return prev[m];
  }
  // the largest s with global(a, b[s .. j)) == score: one global table of the reversed pattern over b[j-1], b[j-2], .. holds every
  // length in its last row; every 16th hit also asks global() itself, for s and for every start behind it
  int start(const int32_t* a, int m, const int32_t* b, int j, int score) const {
    std::vector<int> prev(m + 1), cur(m + 1);
    prev[0] = 0;
    for (int i = 1; i <= m; ++i) prev[i] = prev[i - 1] + w_ins(a[m - i]);
    int l = 0;
    while (prev[m] != score && l < j) {
      ++l;
      const int32_t t = b[j - l];
      cur[0] = prev[0] + w_del(t);
      for (int i = 1; i <= m; ++i) {
        int d = prev[i - 1] + w_sub(t, a[m - i]);
        if (prev[i] + w_del(t) < d) d = prev[i] + w_del(t);
        if (cur[i - 1] + w_ins(a[m - i]) < d) d = cur[i - 1] + w_ins(a[m - i]);
        cur[i] = d;
      }
      prev.swap(cur);
    }
    static unsigned calls = 0;
    bool bad = prev[m] != score;
    if (!bad && calls++ % 16 == 0) {
      bad = global(a, m, b + (j - l), l) != score;
      for (int s = j - l + 1; s <= j && !bad; ++s) bad = global(a, m, b + s, j - s) == score;
    }
    if (bad) {
      printf("the yardstick disagrees with itself\n");
      exit(1);
    }
    return j - l;
  }
  void hits(const int32_t* a, int m, int k, const int32_t* b, int n, int32_t q, int32_t t, std::vector<msocr_search_hit>& out) const {
    std::vector<int> prev(m + 1), cur(m + 1);
    prev[0] = 0;
    for (int i = 1; i <= m; ++i) prev[i] = prev[i - 1] + w_ins(a[i - 1]);
    if (k > prev[m] - 1) k = prev[m] - 1;
    for (int j = 1; j <= n; ++j) {
      cur[0] = 0;
      for (int i = 1; i <= m; ++i) {
        int d = prev[i - 1] + w_sub(b[j - 1], a[i - 1]);
        if (prev[i] + w_del(b[j - 1]) < d) d = prev[i] + w_del(b[j - 1]);
        if (cur[i - 1] + w_ins(a[i - 1]) < d) d = cur[i - 1] + w_ins(a[i - 1]);
        cur[i] = d;
      }
      prev.swap(cur);
      if (prev[m] <= k) out.push_back(msocr_search_hit{q, t, start(a, m, b, j, prev[m]), j, prev[m]});
    }
  }
};

static bool equal_hit(const msocr_search_hit& x, const msocr_search_hit& y) {
  return x.pattern == y.pattern && x.text == y.text && x.start == y.start && x.end == y.end && x.distance == y.distance;
}

static int check_args() {
  uint8_t one = 1;
  for (int it = 0; it < 400; ++it) {
    const int Q = rnd_in(1, 5), T = rnd_in(1, 5), v = rnd_in(1, MSOCR_SEARCH_W_MAX_ALPHABET);
    msocr_edit_costs ec = {&one, &one, &one, rnd_in(1, 512), rnd_in(1, 255), rnd_in(1, 255), rnd_in(1, 255)};
    const int dmin = ec.min_del < ec.unknown ? ec.min_del : ec.unknown;
    std::unique_ptr<int32_t[]> po(new int32_t[Q + 1]), k(new int32_t[Q]), to(new int32_t[T + 1]);
    po[0] = rnd_in(0, 5);
    to[0] = rnd_in(0, 5);
    for (int q = 0; q < Q; ++q) {
      const int m = rnd() % 4 ? rnd_in(1, 64) : (rnd() % 2 ? 1 : 64);
      po[q + 1] = po[q] + m;
      k[q] = rnd() % 3 ? rnd_in(0, (MSOCR_SEARCH_W_MAX_WINDOW - m) * dmin + dmin - 1) : (MSOCR_SEARCH_W_MAX_WINDOW - m) * dmin + dmin - 1;
    }
    int64_t segs = 0;
    for (int t = 0; t < T; ++t) {
      to[t + 1] = to[t] + (rnd() % 3 ? rnd_in(0, 300) : 0);
      segs += (to[t + 1] - to[t] + MSOCR_SEARCH_SEGMENT - 1) / MSOCR_SEARCH_SEGMENT;
    }
    const int64_t want = ((int64_t)8 * (T + 1) + 4 * (T + 1) + 4 * (Q + 1) + 4 * Q + 7) / 8 * 8;
    ts_layout lay;
    if (tsw_check(po.get(), k.get(), Q, to.get(), T, v, &ec, &lay) != want || lay.total != want || lay.segments != segs || lay.seg_pre != 0) {
      printf("workspace formula\n");
      return 1;
    }
    if (tsw_check(nullptr, nullptr, 0, to.get(), T, v, &ec, nullptr) != 0 || tsw_check(po.get(), k.get(), Q, nullptr, 0, v, &ec, nullptr) != 0) {
      printf("empty side\n");
      return 1;
    }
    std::unique_ptr<unsigned char[]> heads(new unsigned char[(size_t)lay.total]);
    ts_fill_heads(po.get(), k.get(), Q, to.get(), T, lay, heads.get());
    const int64_t* sp = (const int64_t*)heads.get();
    const int32_t* ho = (const int32_t*)(heads.get() + lay.txt_off);
    const int32_t* hk = (const int32_t*)(heads.get() + lay.max_dist);
    if (sp[0] != 0 || sp[T] != segs || ho[T] != to[T] || hk[Q - 1] != k[Q - 1]) { printf("heads\n"); return 1; }
    const int q = rnd_in(0, Q - 1), t = rnd_in(0, T - 1);
    int vv = v;
    const msocr_edit_costs* pe = &ec;
    switch (rnd() % 14) {  // one corruption: refused whatever the rest holds
      case 0: po[q + 1] = po[q] - (int32_t)(rnd() % 9); break;  // a length below 1
      case 1: po[q + 1] = po[q] + 65 + (int32_t)(rnd() % 9); break;
      case 2: k[q] = (MSOCR_SEARCH_W_MAX_WINDOW - (po[q + 1] - po[q]) + 1) * dmin; break;  // the window one past the cap
      case 3: k[q] = rnd() % 2 ? -1 : INT32_MIN; break;
      case 4: to[t + 1] = to[t] - 1 - (int32_t)(rnd() % 9); break;
      case 5: to[0] = -1 - (int32_t)(rnd() % 9); break;
      case 6: vv = rnd() % 2 ? 0 : MSOCR_SEARCH_W_MAX_ALPHABET + 1; break;
      case 7: pe = nullptr; break;
      case 8: (rnd() % 3 == 0 ? ec.sub : rnd() % 2 ? ec.del : ec.ins) = nullptr; break;
      case 9: ec.unknown = rnd() % 2 ? 0 : 256; break;
      case 10: ec.min_del = rnd() % 2 ? 0 : 256; break;
      case 11: ec.min_ins = rnd() % 2 ? 0 : 256; break;
      case 12: ec.V = rnd() % 2 ? 0 : 513; break;
      default: to[t] = INT32_MAX; to[t + 1] = INT32_MIN; break;
    }
    if (tsw_check(po.get(), k.get(), Q, to.get(), T, vv, pe, nullptr) >= 0) { printf("corrupt arguments accepted\n"); return 1; }
  }
  msocr_edit_costs ok = {&one, &one, &one, 1, 1, 1, 1};
  if (tsw_check(nullptr, nullptr, -1, nullptr, 0, 5, &ok, nullptr) >= 0 || tsw_check(nullptr, nullptr, 0, nullptr, -1, 5, &ok, nullptr) >= 0 ||
      tsw_check(nullptr, nullptr, 2, nullptr, 0, 5, &ok, nullptr) >= 0 || tsw_check(nullptr, nullptr, 0, nullptr, 2, 5, &ok, nullptr) >= 0) {
    printf("null arrays\n");
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  if (check_args()) return 1;
  long checked = 0;
  static const int m_edges[8] = {1, 5, 8, 9, 63, 64, 2, 33};
  static const int vs[6] = {1, 2, 5, 60, 300, MSOCR_SEARCH_W_MAX_ALPHABET};
  static const int Vs[5] = {1, 2, 7, 194, 512};
  const int L = MSOCR_SEARCH_SEGMENT;
  for (int it = 0; it < rounds; ++it) {
    const int v = vs[rnd() % 6], V = Vs[rnd() % 5];
    const bool wild = rnd() % 3 == 0;         // garbage tokens and classes
    const bool wild_tables = rnd() % 4 == 0;  // any byte anywhere in the tables, zeros included: the twin alone is checked then
    const int top = rnd() % 2 ? 3 : 255;      // cheap tables make many hits, dear ones few
    const int unknown = rnd_in(1, top);
    // tables and the class map, each in a heap block of its exact size
    std::unique_ptr<uint8_t[]> sub(new uint8_t[(size_t)V * V]), del(new uint8_t[V]), ins(new uint8_t[V]);
    std::unique_ptr<int32_t[]> cls(new int32_t[v]);
    for (int x = 0; x < V; ++x) {
      for (int y = 0; y < V; ++y) sub[(size_t)x * V + y] = wild_tables ? (uint8_t)rnd() : (x == y ? 0 : (uint8_t)rnd_in(1, top));
      del[x] = wild_tables ? (uint8_t)rnd() : (uint8_t)rnd_in(1, top);
      ins[x] = wild_tables ? (uint8_t)rnd() : (uint8_t)rnd_in(1, top);
    }
    int min_del = unknown;
    for (int x = 0; x < V; ++x) min_del = del[x] < min_del ? del[x] : min_del;
    for (int x = 0; x < v; ++x) cls[x] = wild && rnd() % 4 == 0 ? garbage() : (rnd() % 5 == 0 ? -1 : (int32_t)(rnd() % (uint32_t)V));  // not injective
    const int Q = rnd_in(1, 3), T = rnd_in(1, 4);
    std::vector<int> ms(Q), ns(T);
    std::unique_ptr<int32_t[]> po(new int32_t[Q + 1]), ks(new int32_t[Q]), to(new int32_t[T + 1]);
    po[0] = 0;
    to[0] = 0;
    const int dmin = min_del > 0 ? min_del : 1;
    for (int q = 0; q < Q; ++q) {
      ms[q] = rnd() % 2 ? m_edges[rnd() % 8] : rnd_in(1, 64);
      const int cap = (MSOCR_SEARCH_W_MAX_WINDOW - ms[q]) * dmin + dmin - 1;  // the largest bound the window allows
      const int want_k = rnd() % 4 == 0 ? 255 * ms[q] : rnd_in(0, 3 * top);   // sometimes above what the pattern costs: clamped
      ks[q] = want_k < cap ? want_k : cap;
      po[q + 1] = po[q] + ms[q];
    }
    static const int n_edges[10] = {0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 3 * L + 7, 0, 5};
    for (int t = 0; t < T; ++t) {
      ns[t] = rnd() % 2 ? n_edges[rnd() % 10] : rnd_in(0, 200);
      to[t + 1] = to[t] + ns[t];
    }
    const uint32_t span = (uint32_t)(v < 5 ? v : 5);
    std::unique_ptr<int32_t[]> pat(new int32_t[po[Q]]), txt(new int32_t[to[T]]);
    for (int i = 0; i < po[Q]; ++i) pat[i] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % span);
    for (int i = 0; i < to[T]; ++i) txt[i] = wild && rnd() % 4 == 0 ? garbage() : (int32_t)(rnd() % (span + 1));
    for (int t = 0; t < T; ++t)  // plant the first pattern, whole or without its first token, at the end of every text that has room
      for (int i = 0; i < ms[0] && ms[0] <= ns[t]; ++i) txt[to[t] + ns[t] - ms[0] + i] = i == 0 && rnd() % 2 ? -1 : pat[i];
    msocr_edit_costs ec = {sub.get(), del.get(), ins.get(), V, unknown, 1, dmin};
    if (tsw_check(po.get(), ks.get(), Q, to.get(), T, v, &ec, nullptr) <= 0) { printf("good arrays refused\n"); return 1; }

    const plain P = {sub.get(), del.get(), ins.get(), cls.get(), V, unknown, v};
    std::vector<msocr_search_hit> want;
    for (int q = 0; q < Q; ++q)
      for (int t = 0; t < T; ++t) P.hits(pat.get() + po[q], ms[q], ks[q], txt.get() + to[t], ns[t], q, t, want);
    for (const msocr_search_hit& h : want)
      if (h.start >= h.end && !wild_tables) { printf("the empty substring matched\n"); return 1; }

    // the host twin at a capacity below, at and above the count: exact count, canonical prefix, nothing behind the capacity
    const tsw_costs C = {sub.get(), del.get(), ins.get(), cls.get(), V, unknown, v};
    const int64_t total = (int64_t)want.size();
    const int64_t caps[3] = {total, total > 0 ? (int64_t)(rnd() % (uint32_t)total) : 0, total + 3};
    for (int64_t cap : caps) {
      std::unique_ptr<msocr_search_hit[]> got(new msocr_search_hit[(size_t)cap]);
      const int64_t count = tsw_search_host(pat.get(), po.get(), ks.get(), Q, txt.get(), to.get(), T, C, got.get(), cap);
      if (count != total) { printf("count %lld, plain table %lld\n", (long long)count, (long long)total); return 1; }
      for (int64_t i = 0; i < (cap < total ? cap : total); ++i)
        if (!equal_hit(got[(size_t)i], want[(size_t)i])) {
          printf("hit %lld: (%d %d %d %d %d), plain table (%d %d %d %d %d)\n", (long long)i, got[i].pattern, got[i].text, got[i].start, got[i].end,
                 got[i].distance, want[i].pattern, want[i].text, want[i].start, want[i].end, want[i].distance);
          return 1;
        }
    }
    ++checked;
    if (wild_tables) continue;

    // the kernel's form, segment by segment: the profile in a block of the kernel's LDS size, the packed-key column
    std::unique_ptr<uint8_t[]> lds(new uint8_t[(size_t)tsw_lds_tail_at(v)]);
    std::vector<msocr_search_hit> cut;
    for (int q = 0; q < Q; ++q) {
      const int m = ms[q], g0 = tsw_first_group(m);
      const int32_t* a = pat.get() + po[q];
      std::unique_ptr<int32_t[]> ca(new int32_t[m]);
      int sum = 0;
      for (int i = 0; i < m; ++i) {
        ca[i] = tsw_class(C, a[i]);
        sum += tsw_one(C, C.ins, ca[i]);
      }
      for (int tok = 0; tok <= v; ++tok) {
        for (int p = g0 * 8; p < 64; ++p) lds[(size_t)tok * MSOCR_TSW_STRIDE + p] = tsw_profile_entry(C, a, ca.get(), m, p, tok);
        lds[(size_t)tsw_lds_hdel(v) + tok] = tsw_profile_delete(C, tok);
      }
      uint32_t pins[16];
      for (int w = 0; w < 16; ++w) {
        pins[w] = 0;
        for (int e = 0; e < 4; ++e) pins[w] |= (uint32_t)tsw_profile_insert(C, ca.get(), m, w * 4 + e) << (8 * e);
      }
      const int k = tsw_clamp(ks[q], sum), W = tsw_warmup(m, k, tsw_dmin(dmin, unknown));
      if (W > MSOCR_SEARCH_W_MAX_WINDOW) { printf("window above the cap\n"); return 1; }
      for (int t = 0; t < T; ++t)
        for (int64_t s = 0; s < ts_segments(ns[t]); ++s) {
          int first, lo, hi;
          ts_window(ns[t], s, W, first, lo, hi);
          int32_t col[64];
          tsw_begin(col, pins, g0);
          for (int p = first; p < hi; ++p) {
            const int32_t c = txt[to[t] + p];
            const int cc = (c >= 0 && c < v) ? c : v;
            const int32_t key = tsw_step(col, lds.get() + (size_t)cc * MSOCR_TSW_STRIDE, lds[(size_t)tsw_lds_hdel(v) + cc], pins, g0, p - first);
            if (p >= lo && tsw_key_cost(key) <= k) cut.push_back(msocr_search_hit{q, t, tsw_key_start(key, first), p + 1, tsw_key_cost(key)});
          }
        }
    }
    if ((int64_t)cut.size() != total) { printf("kernel form: %lld hits, plain table %lld\n", (long long)cut.size(), (long long)total); return 1; }
    for (int64_t i = 0; i < total; ++i)
      if (!equal_hit(cut[(size_t)i], want[(size_t)i])) {
        printf("kernel form: hit %lld: (%d %d %d %d %d), plain table (%d %d %d %d %d)\n", (long long)i, cut[i].pattern, cut[i].text, cut[i].start,
               cut[i].end, cut[i].distance, want[i].pattern, want[i].text, want[i].start, want[i].end, want[i].distance);
        return 1;
      }
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
