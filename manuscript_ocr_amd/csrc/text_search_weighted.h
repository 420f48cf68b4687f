// text_search_weighted.h — approximate text search under confusion-weighted costs (include/msocr.h, "The same search under
// confusion-weighted costs"): the semi-global form of the weighted table of edit_distance_weighted.h.  The
// TEXT is the recognised side, the PATTERN the true word.  Host and device: the kernel of text_search_weighted.hip calls the cost
// functions, the profile builder and the column step; the host twin msocr_text_search_weighted_host is tsw_search_host below, and a
// plain C++ program feeds all of it garbage tokens, classes, offsets and tables under the address and undefined-behaviour
// sanitizers (tests/native/text_search_weighted_fuzz.cpp).  Whatever the arrays hold, every index formed here lies inside them.
//
// Two forms of one recurrence:
//   the host twin  the plain table, one column of m + 1 costs per text token, no segments; the start of a hit by a backward walk:
//                  the global table of the pattern against b[j-1], b[j-2], .., the first length whose distance equals the score.
//                  It is the definition.
//   the kernel     the pattern laid against the END of 64 positions (edw_build_profile's layout), the column in 64 registers,
//                  each cell ONE int32 key = cost << 16 | (65535 - (start - first)): the minimum over the three candidates takes
//                  the least cost and, among equals, the largest start.  Row 0 at column j is (0, start j).  The optimal paths into
//                  a cell are the union of those through its minimal predecessors, and none runs along row 0, since a delete costs
//                  at least 1: the bottom cell's start is the largest s whose global distance equals the score, the walk's answer.
#ifndef MSOCR_TEXT_SEARCH_WEIGHTED_H
#define MSOCR_TEXT_SEARCH_WEIGHTED_H
#include "edit_distance_weighted.h"
#include "text_search.h"

// the tables as the cost functions read them; tok_class [v]
struct tsw_costs {
  const uint8_t *sub, *del, *ins;
  const int32_t* tok_class;
  int V, unknown, v;
};

// the cost class of token t, or -1
MSOCR_EDL_HD int tsw_class(const tsw_costs& c, int32_t t) {
  if (t < 0 || t >= c.v) return -1;
  const int32_t k = c.tok_class[t];
  return (k >= 0 && k < c.V) ? (int)k : -1;
}
// reading text token t (class ct) as pattern token p (class cp)
MSOCR_EDL_HD int tsw_sub(const tsw_costs& c, int32_t t, int ct, int32_t p, int cp) {
  if (t == p && t >= 0 && t < c.v) return 0;
  return (ct >= 0 && cp >= 0) ? (int)c.sub[(size_t)ct * c.V + cp] : c.unknown;
}
// dropping a text token of class k (vec = del), supplying a pattern token of class k (vec = ins)
MSOCR_EDL_HD int tsw_one(const tsw_costs& c, const uint8_t* vec, int k) { return k >= 0 ? (int)vec[k] : c.unknown; }

// what a delete costs at the least: a token without a class costs `unknown`
MSOCR_EDL_HD int tsw_dmin(int min_del, int unknown) { return min_del < unknown ? min_del : unknown; }
// the bound that keeps the empty substring out, and the warm-up of a pattern of m tokens under it
MSOCR_EDL_HD int tsw_clamp(int k, int ins_sum) { return k < ins_sum - 1 ? k : ins_sum - 1; }
MSOCR_EDL_HD int tsw_warmup(int m, int k, int dmin) { return m + k / dmin; }

// ---- the kernel's form ---------------------------------------------------------------------------------------------------------
#define MSOCR_TSW_STRIDE MSOCR_EDW_PROFILE_STRIDE  // bytes of a profile row
#define MSOCR_TSW_KEY_START 65535                  // low half of a key whose start is `first`

// first group of 8 positions that holds a pattern token
MSOCR_EDL_HD int tsw_first_group(int m) { return (MSOCR_SEARCH_MAX_PATTERN - m) >> 3; }

// profile entry: position p (>= 8 * tsw_first_group(m)) of the pattern a [m] (classes ca [m]) against text token c in [0, v]; row v
// stands for every token outside [0, v).  In front of the pattern: 255, no substitution is taken there.
MSOCR_EDL_HD uint8_t tsw_profile_entry(const tsw_costs& c, const int32_t* a, const int32_t* ca, int m, int p, int tok) {
  const int i = p - (MSOCR_SEARCH_MAX_PATTERN - m);
  if (i < 0) return (uint8_t)MSOCR_EDW_MAX_COST;
  if (tok >= c.v) return (uint8_t)c.unknown;
  return (uint8_t)tsw_sub(c, tok, tsw_class(c, tok), a[i], ca[i]);
}
// what text token c in [0, v] costs to drop
MSOCR_EDL_HD uint8_t tsw_profile_delete(const tsw_costs& c, int tok) {
  return (uint8_t)(tok >= c.v ? c.unknown : tsw_one(c, c.del, tsw_class(c, tok)));
}
// what position p costs to supply: 0 in front of the pattern, so that such a position hands row 0 down unchanged
MSOCR_EDL_HD uint8_t tsw_profile_insert(const tsw_costs& c, const int32_t* ca, int m, int p) {
  const int i = p - (MSOCR_SEARCH_MAX_PATTERN - m);
  return (uint8_t)(i < 0 ? 0 : tsw_one(c, c.ins, ca[i]));
}

// the fresh column at token `first`: position p holds (the inserts of the positions up to it, start = first)
MSOCR_EDL_HD void tsw_begin(int32_t* col, const uint32_t* pins, int g0) {
  int32_t acc = MSOCR_TSW_KEY_START;
#pragma unroll
  for (int g = 0; g < MSOCR_SEARCH_MAX_PATTERN / 8; ++g) {
    if (g < g0) continue;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = g * 8 + e;
      acc += (int32_t)((pins[i >> 2] >> (8 * (i & 3))) & 255u) << 16;
      col[i] = acc;
    }
  }
}

// One column step: the text token whose profile row is `row` (8-byte aligned) and whose delete cost is del_c, the `rel`-th token from
// `first` (rel >= 0).  pins [16]: the positions' insert costs, four to a word.  -> the key of the bottom cell.
MSOCR_EDL_HD int32_t tsw_step(int32_t* col, const uint8_t* row, int del_c, const uint32_t* pins, int g0, int rel) {
  int32_t diag = MSOCR_TSW_KEY_START - rel;     // row 0 before this token: (0, start = its index)
  int32_t up = MSOCR_TSW_KEY_START - (rel + 1);  // row 0 behind it
  const int32_t dk = (int32_t)del_c << 16;
  const uint8_t* r8 = (const uint8_t*)__builtin_assume_aligned(row, 8);
#pragma unroll
  for (int g = 0; g < MSOCR_SEARCH_MAX_PATTERN / 8; ++g) {
    if (g < g0) continue;
    uint64_t pk;
    __builtin_memcpy(&pk, r8 + g * 8, 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = g * 8 + e;
      const int32_t left = col[i];
      const int32_t a = diag + ((int32_t)((pk >> (8 * e)) & 255u) << 16);
      const int32_t b = left + dk;
      const int32_t c = up + ((int32_t)((pins[i >> 2] >> (8 * (i & 3))) & 255u) << 16);
      const int32_t ab = a < b ? a : b;
      up = ab < c ? ab : c;
      col[i] = up;
      diag = left;
    }
  }
  return up;
}
MSOCR_EDL_HD int tsw_key_cost(int32_t key) { return key >> 16; }
MSOCR_EDL_HD int tsw_key_start(int32_t key, int first) { return first + (MSOCR_TSW_KEY_START - (key & 0xffff)); }

// bytes of the kernel's dynamic LDS: the profile, the delete costs, then tsw_lds_tail bytes of per-pattern state
MSOCR_EDL_HD int tsw_lds_hdel(int v) { return (v + 1) * MSOCR_TSW_STRIDE; }
MSOCR_EDL_HD int tsw_lds_tail_at(int v) { return tsw_lds_hdel(v) + ((v + 1 + 7) & ~7); }

// ---- host side -----------------------------------------------------------------------------------------------------------------
// The argument check every entry point makes of the HOST arrays and of the struct's own fields (the tables it points at are not
// read), and the workspace of the device route: the heads of ts_layout without the mask tables.  Returns the bytes, 0 for Q == 0 or
// T == 0, -1 for what is refused.
inline int64_t tsw_check(const int32_t* pat_off, const int32_t* max_dist, int Q, const int32_t* txt_off, int T, int v,
                         const msocr_edit_costs* costs, ts_layout* lay) {
  if (Q < 0 || T < 0 || v < 1 || v > MSOCR_SEARCH_W_MAX_ALPHABET) return -1;
  if (!costs || !costs->sub || !costs->del || !costs->ins || costs->V < 1 || costs->V > 512) return -1;
  if (costs->unknown < 1 || costs->unknown > MSOCR_EDW_MAX_COST || costs->min_ins < 1 || costs->min_ins > MSOCR_EDW_MAX_COST ||
      costs->min_del < 1 || costs->min_del > MSOCR_EDW_MAX_COST)
    return -1;
  const int dmin = tsw_dmin(costs->min_del, costs->unknown);
  if (Q > 0) {
    if (!pat_off || !max_dist || pat_off[0] < 0) return -1;
    for (int q = 0; q < Q; ++q) {
      const int64_t m = (int64_t)pat_off[q + 1] - pat_off[q];
      if (m < 1 || m > MSOCR_SEARCH_MAX_PATTERN || max_dist[q] < 0) return -1;
      if (m + (int64_t)max_dist[q] / dmin > MSOCR_SEARCH_W_MAX_WINDOW) return -1;
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
  l.seg_pre = 0;
  l.txt_off = 8 * ((int64_t)T + 1);
  l.pat_off = l.txt_off + 4 * ((int64_t)T + 1);
  l.max_dist = l.pat_off + 4 * ((int64_t)Q + 1);
  l.total = (l.max_dist + 4 * (int64_t)Q + 7) & ~7ll;
  l.segments = segs;
  if (lay) *lay = l;
  return (Q == 0 || T == 0) ? 0 : l.total;
}

// start of the hit (end j, score s) of the pattern a [m] (classes ca, insert costs wi) in the text b: j - l* for the smallest l* whose
// weighted global distance between a and b[j - l* .. j) is s.  col [m + 1] is scratch: col[i] = the distance between the LAST i
// pattern tokens and the l text tokens read so far.  The least value of a column never falls from one l to the next, so the walk
// stops where it exceeds s (not before l* for a true hit).
inline int tsw_start_host(const tsw_costs& c, const int32_t* a, const int32_t* ca, const int* wi, int m, const int32_t* b, int j, int s,
                          int* col) {
  col[0] = 0;
  for (int i = 1; i <= m; ++i) col[i] = col[i - 1] + wi[m - i];
  if (col[m] == s) return j;
  for (int l = 1; l <= j; ++l) {
    const int32_t t = b[j - l];
    const int ct = tsw_class(c, t), wd = tsw_one(c, c.del, ct);
    int diag = col[0], least;
    col[0] += wd;
    least = col[0];
    for (int i = 1; i <= m; ++i) {
      const int left = col[i];
      col[i] = edw_cell(diag, left, col[i - 1], tsw_sub(c, t, ct, a[m - i], ca[m - i]), wd, wi[m - i]);
      if (col[i] < least) least = col[i];
      diag = left;
    }
    if (col[m] == s) return j - l;
    if (least > s) break;
  }
  return 0;  // not reached for a true hit
}

// the host twin: the first `capacity` hits in canonical order -> the exact number of hits.  The arrays have passed tsw_check.
inline int64_t tsw_search_host(const int32_t* pat_tok, const int32_t* pat_off, const int32_t* max_dist, int Q, const int32_t* txt_tok,
                               const int32_t* txt_off, int T, const tsw_costs& c, msocr_search_hit* hits, int64_t capacity) {
  int32_t ca[MSOCR_SEARCH_MAX_PATTERN];
  int wi[MSOCR_SEARCH_MAX_PATTERN], col[MSOCR_SEARCH_MAX_PATTERN + 1], walk[MSOCR_SEARCH_MAX_PATTERN + 1];
  int64_t count = 0;
  for (int q = 0; q < Q; ++q) {
    const int m = pat_off[q + 1] - pat_off[q];
    const int32_t* a = pat_tok + pat_off[q];
    int ins_sum = 0;
    for (int i = 0; i < m; ++i) {
      ca[i] = tsw_class(c, a[i]);
      wi[i] = tsw_one(c, c.ins, ca[i]);
      ins_sum += wi[i];
    }
    const int k = tsw_clamp(max_dist[q], ins_sum);
    for (int t = 0; t < T; ++t) {
      const int32_t* b = txt_tok + txt_off[t];
      const int n = txt_off[t + 1] - txt_off[t];
      col[0] = 0;
      for (int i = 0; i < m; ++i) col[i + 1] = col[i] + wi[i];
      for (int j = 1; j <= n; ++j) {
        const int32_t tk = b[j - 1];
        const int ct = tsw_class(c, tk), wd = tsw_one(c, c.del, ct);
        int diag = 0;  // D[0][j - 1]; col[0] stays D[0][j] = 0
        for (int i = 1; i <= m; ++i) {
          const int left = col[i];
          col[i] = edw_cell(diag, left, col[i - 1], tsw_sub(c, tk, ct, a[i - 1], ca[i - 1]), wd, wi[i - 1]);
          diag = left;
        }
        if (col[m] > k) continue;
        if (count < capacity) {
          msocr_search_hit& h = hits[count];
          h.pattern = q;
          h.text = t;
          h.end = j;
          h.distance = col[m];
          h.start = tsw_start_host(c, a, ca, wi, m, b, j, col[m], walk);
        }
        ++count;
      }
    }
  }
  return count;
}
#endif
