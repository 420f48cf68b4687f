// text_search.h — approximate text search (Sellers' semi-global form of the Levenshtein table) of Q short patterns over T texts of int32
// tokens (include/msocr.h, "approximate text search").  Host and device: the kernels of text_search.hip call
// these functions, the host twin msocr_text_search_host is ts_search_host below, msocr_text_search_select_host is ts_select, and a
// plain C++ program feeds them garbage tokens and offset arrays under the address and undefined-behaviour sanitizers
// (tests/native/text_search_fuzz.cpp).  Whatever the token and offset arrays hold, every index formed here lies inside them and
// inside the mask table.
//
// The recurrence is edl_advance of edit_distance_long.h, unchanged, on ONE block (m <= 64):
//   forward scan   hin = 0 (the top row of the table is 0, a match may begin anywhere); the score of the bottom row, m before any
//                  text symbol, takes hout at bit m - 1 after every symbol and is read at every column.
//   backward walk  hin = +1 (the global distance) of the REVERSED pattern over the text read backwards from a hit's end: the first
//                  length at which it equals the hit's score is the shortest substring that attains it.
// Match masks: a table [Q][2][v] of 64-bit words, word [q][0][c] = the positions of token c in pattern q, word [q][1][c] = the
// positions of c in the reversed pattern.  A token outside [0, v), on either side, matches nothing and is never an index.
#ifndef MSOCR_TEXT_SEARCH_H
#define MSOCR_TEXT_SEARCH_H
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "edit_distance_long.h"
#include "msocr.h"

// where the parts of the device workspace lie (bytes from its start) and how many segments the texts are cut into
struct ts_layout {
  int64_t seg_pre;   // int64 [T + 1]: segments before text t; [T] = all of them
  int64_t txt_off;   // int32 [T + 1]
  int64_t pat_off;   // int32 [Q + 1]
  int64_t max_dist;  // int32 [Q]
  int64_t total;     // bytes, a multiple of 8; the tables [Q][2][v] come first, from byte 0 to seg_pre
  int64_t segments;
};

MSOCR_EDL_HD uint64_t ts_eq(const uint64_t* row, int v, int32_t c) { return (c >= 0 && c < v) ? row[c] : 0ull; }

// the forward scan by one text symbol: returns the change of the bottom row's score
MSOCR_EDL_HD int ts_scan_step(uint64_t& pv, uint64_t& mv, uint64_t eq, int m) { return edl_advance(pv, mv, eq, 0, m - 1); }

// segments of a text of n tokens
MSOCR_EDL_HD int64_t ts_segments(int64_t n) { return (n + MSOCR_SEARCH_SEGMENT - 1) / MSOCR_SEARCH_SEGMENT; }

// The window of segment s of a text of n tokens under a warm-up of W = m + k tokens, all inside the text: the scan starts fresh
// (pv = all ones up to m, mv = 0, score m) at token `first` and reports the ends j = p + 1 of tokens p in [lo, hi).  An alignment
// with at most k errors spans at most m + k text tokens, and a restricted start can only raise a score: every s_j <= k is
// reproduced and nothing above k falls to k or below.
MSOCR_EDL_HD void ts_window(int n, int64_t s, int W, int& first, int& lo, int& hi) {
  const int64_t l = s * MSOCR_SEARCH_SEGMENT;
  lo = (int)l;  // s < ts_segments(n): l < n
  hi = (int)(l + MSOCR_SEARCH_SEGMENT < n ? l + MSOCR_SEARCH_SEGMENT : n);
  first = l > W ? (int)(l - W) : 0;
}

// start of the hit (end j, score s) of a pattern of m tokens whose REVERSED mask row is rrow [v], in the text b [>= j]:
// j - l* for the smallest l* with ed(pattern, b[j - l* .. j)) == s.  At most min(j, m + s) steps, all of them reads of b[0 .. j).
MSOCR_EDL_HD int ts_start(const uint64_t* rrow, int v, int m, const int32_t* b, int j, int s) {
  uint64_t pv = edl_begin_pv(m, 0), mv = 0ull;
  const int bound = j < m + s ? j : m + s;
  int score = m;
  for (int l = 1; l <= bound; ++l) {
    score += edl_advance(pv, mv, ts_eq(rrow, v, b[j - l]), 1, m - 1);
    if (score == s) return j - l;
  }
  return j - bound;  // not reached for a true hit: l* exists within the bound
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The argument check every entry point makes of the HOST arrays, and the workspace the device route needs.  Returns the bytes,
// 0 for Q == 0 or T == 0 (a call that finds nothing), or -1 for what is refused.  An array without elements is not read.
inline int64_t ts_check(const int32_t* pat_off, const int32_t* max_dist, int Q, const int32_t* txt_off, int T, int v, ts_layout* lay) {
  if (Q < 0 || T < 0 || v < 1 || v > MSOCR_SEARCH_MAX_ALPHABET) return -1;
  if (Q > 0) {
    if (!pat_off || !max_dist || pat_off[0] < 0) return -1;
    for (int q = 0; q < Q; ++q) {
      const int64_t m = (int64_t)pat_off[q + 1] - pat_off[q];
      if (m < 1 || m > MSOCR_SEARCH_MAX_PATTERN || max_dist[q] < 0 || max_dist[q] >= m) return -1;
    }
  }
  int64_t segs = 0;
  if (T > 0) {
    if (!txt_off || txt_off[0] < 0) return -1;
    for (int t = 0; t < T; ++t) {
      const int64_t n = (int64_t)txt_off[t + 1] - txt_off[t];
      if (n < 0) return -1;
      segs += ts_segments(n);
    }
  }
  ts_layout l;
  l.seg_pre = (int64_t)Q * 2 * v * 8;
  l.txt_off = l.seg_pre + 8 * ((int64_t)T + 1);
  l.pat_off = l.txt_off + 4 * ((int64_t)T + 1);
  l.max_dist = l.pat_off + 4 * ((int64_t)Q + 1);
  l.total = (l.max_dist + 4 * (int64_t)Q + 7) & ~7ll;
  l.segments = segs;
  if (lay) *lay = l;
  return (Q == 0 || T == 0) ? 0 : l.total;
}

// the uploaded heads as the kernels read them: heads = the workspace's bytes from lay.seg_pre to lay.total, in a host buffer of
// that size whose byte 0 stands for lay.seg_pre; the arrays have passed ts_check with Q > 0 and T > 0
inline void ts_fill_heads(const int32_t* pat_off, const int32_t* max_dist, int Q, const int32_t* txt_off, int T, const ts_layout& lay,
                          unsigned char* heads) {
  int64_t* seg_pre = (int64_t*)heads;
  int32_t* to = (int32_t*)(heads + (lay.txt_off - lay.seg_pre));
  int32_t* po = (int32_t*)(heads + (lay.pat_off - lay.seg_pre));
  int32_t* md = (int32_t*)(heads + (lay.max_dist - lay.seg_pre));
  int64_t segs = 0;
  for (int t = 0; t < T; ++t) {
    seg_pre[t] = segs;
    to[t] = txt_off[t];
    segs += ts_segments((int64_t)txt_off[t + 1] - txt_off[t]);
  }
  seg_pre[T] = segs;
  to[T] = txt_off[T];
  for (int q = 0; q < Q; ++q) {
    po[q] = pat_off[q];
    md[q] = max_dist[q];
  }
  po[Q] = pat_off[Q];
}

// rows [2][v] <- the match masks of a [m] (1 <= m <= 64) and of its reversal; a token outside [0, v) sets no bit
inline void ts_build_rows_host(const int32_t* a, int m, int v, uint64_t* rows) {
  for (int i = 0; i < 2 * v; ++i) rows[i] = 0ull;
  for (int i = 0; i < m; ++i)
    if (a[i] >= 0 && a[i] < v) {
      rows[a[i]] |= 1ull << i;
      rows[v + a[i]] |= 1ull << (m - 1 - i);
    }
}

// The hits of pattern q (rows [2][v], m tokens, bound k) in text t (b [n]), ends ascending: appended while fewer than `capacity`
// are written; returns how many there are.  `from` / `lo` / `hi`: the scan starts fresh at token `from` and reports tokens
// [lo, hi) only (the whole text: 0, 0, n), which is how the kernel runs a segment.
inline int64_t ts_scan_host(const uint64_t* rows, int v, int m, int k, const int32_t* b, int from, int lo, int hi, int32_t q, int32_t t,
                            msocr_search_hit* hits, int64_t capacity, int64_t written) {
  uint64_t pv = edl_begin_pv(m, 0), mv = 0ull;
  int score = m;
  int64_t found = 0;
  for (int p = from; p < hi; ++p) {
    score += ts_scan_step(pv, mv, ts_eq(rows, v, b[p]), m);
    if (p >= lo && score <= k) {
      if (written + found < capacity) {
        msocr_search_hit& h = hits[written + found];
        h.pattern = q;
        h.text = t;
        h.end = p + 1;
        h.distance = score;
        h.start = ts_start(rows + v, v, m, b, p + 1, score);
      }
      ++found;
    }
  }
  return found;
}

// the host twin: the first `capacity` hits in canonical order (pattern, text, end ascending) -> the exact number of hits; rows [2 v]
// is scratch.  The arrays have passed ts_check.
inline int64_t ts_search_host(const int32_t* pat_tok, const int32_t* pat_off, const int32_t* max_dist, int Q, const int32_t* txt_tok,
                              const int32_t* txt_off, int T, int v, msocr_search_hit* hits, int64_t capacity, uint64_t* rows) {
  int64_t count = 0;
  for (int q = 0; q < Q; ++q) {
    const int m = pat_off[q + 1] - pat_off[q];
    ts_build_rows_host(pat_tok + pat_off[q], m, v, rows);
    for (int t = 0; t < T; ++t) {
      const int n = txt_off[t + 1] - txt_off[t];
      const int64_t written = count < capacity ? count : capacity;
      count += ts_scan_host(rows, v, m, max_dist[q], txt_tok + txt_off[t], 0, 0, n, q, t, hits, capacity, written);
    }
  }
  return count;
}

inline bool ts_canonical_less(const msocr_search_hit& a, const msocr_search_hit& b) {
  if (a.pattern != b.pattern) return a.pattern < b.pattern;
  if (a.text != b.text) return a.text < b.text;
  return a.end < b.end;
}

// Selection: h [n] sorted into canonical order; per (pattern, text) the hits are walked by (distance, end) ascending and one is kept
// iff [start, end) intersects no kept hit of the same (pattern, text); the kept hits are compacted to the front in canonical order
// -> how many.  A record with start >= end (no output of the search) intersects nothing and is kept.
inline int64_t ts_select(msocr_search_hit* h, int64_t n) {
  std::sort(h, h + n, ts_canonical_less);
  std::vector<char> keep((size_t)n, 0);
  std::vector<int64_t> idx;
  std::map<int32_t, int32_t> kept;  // start -> end of the kept hits of this group, disjoint
  for (int64_t g0 = 0; g0 < n;) {
    int64_t g1 = g0 + 1;
    while (g1 < n && h[g1].pattern == h[g0].pattern && h[g1].text == h[g0].text) ++g1;
    idx.resize((size_t)(g1 - g0));
    for (int64_t i = g0; i < g1; ++i) idx[(size_t)(i - g0)] = i;
    std::sort(idx.begin(), idx.end(), [h](int64_t a, int64_t b) {
      if (h[a].distance != h[b].distance) return h[a].distance < h[b].distance;
      if (h[a].end != h[b].end) return h[a].end < h[b].end;
      return a < b;
    });
    kept.clear();
    for (int64_t i : idx) {
      const int32_t s = h[i].start, e = h[i].end;
      bool free_ = true;
      if (s < e) {
        auto it = kept.lower_bound(s);  // the first kept hit that starts at or behind s
        if (it != kept.end() && it->first < e) free_ = false;
        if (free_ && it != kept.begin()) {
          --it;
          if (it->second > s) free_ = false;
        }
        if (free_) kept[s] = e;
      }
      keep[(size_t)i] = free_;
    }
    g0 = g1;
  }
  int64_t out = 0;
  for (int64_t i = 0; i < n; ++i)
    if (keep[(size_t)i]) h[out++] = h[i];
  return out;
}
#endif
