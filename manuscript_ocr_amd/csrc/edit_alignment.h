// edit_alignment.h — one optimal alignment behind the Levenshtein distance of edit_distance_long.h: which pattern token pairs with
// which text token, and the counts of hits, substitutions, deletions and insertions (include/msocr.h, "alignment behind the error
// rates").  Host and device: the kernels of edit_alignment.hip call eal_advance and eal_decide, the host
// twin msocr_edit_alignment_host is eal_forward_host + eal_traceback_host below, and a plain C++ program feeds them garbage tokens
// and offset arrays under the address and undefined-behaviour sanitizers (tests/native/edit_alignment_fuzz.cpp).  Whatever the token
// arrays hold, every index formed here lies inside them, inside the mask table, inside the trace and inside the two maps.
//
// The rule.  Pattern a [m], text b [n], D the Levenshtein table.  From (i, j) = (m, n), while i > 0 and j > 0, the first that applies:
//   1. a[i-1] equals b[j-1]           hit           pair them, go to (i-1, j-1)
//   2. D[i-1][j-1] + 1 == D[i][j]     substitution  pair them, go to (i-1, j-1)
//   3. D[i-1][j] + 1 == D[i][j]       deletion      a[i-1] has no partner, go to (i-1, j)
//   4. otherwise                      insertion     b[j-1] has no partner, go to (i, j-1)
// and when one index reaches 0 the rest of the other side is deletions (i left) or insertions (j left).
//
// The trace.  The block recurrence needs no table for this: per text column and pattern block two 64-bit words, both by-products of
// the step, decide every cell of the block in that column (eal_cell):
//   d0 = xh | mv, mv taken BEFORE the step   bit r set iff D[i][j] == D[i-1][j-1]      (xh alone misses the cells mv covers)
//   pv after the step                        bit r set iff D[i][j] == D[i-1][j] + 1
// for row i = 64 blk + r + 1 and column j = t + 1.  Layout [block][column]: cell (blk, t) of a pair at blk * n + t, so the 64
// columns a traceback window reads are contiguous.  16 bytes a cell: 16 * ceil(m / 64) * n bytes a pair, 64 MiB at the cap.
#ifndef MSOCR_EDIT_ALIGNMENT_H
#define MSOCR_EDIT_ALIGNMENT_H
#include "edit_distance_long.h"

enum { EAL_HIT = 0, EAL_SUB = 1, EAL_DEL = 2, EAL_INS = 3 };  // the order of counts_out [N][4]

struct alignas(16) eal_cell {
  uint64_t d0, pv;
};

// edl_advance with the two trace words: the same pv, mv and hout, and d0 as above (pv after the call is the other word)
MSOCR_EDL_HD int eal_advance(uint64_t& pv, uint64_t& mv, uint64_t eq, int hin, int top_bit, uint64_t& d0) {
  const uint64_t hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
  const uint64_t xv = eq | mv;
  eq |= hneg;
  const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
  d0 = xh | mv;
  uint64_t ph = mv | ~(xh | pv);
  uint64_t mh = pv & xh;
  const int hout = (int)((ph >> top_bit) & 1) - (int)((mh >> top_bit) & 1);
  ph = (ph << 1) | hpos;
  mh = (mh << 1) | hneg;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
  return hout;
}

// the rule for the 64 rows of a block in one column at once (eq, d0, pv = the match mask and the trace words of the block and
// column): bit r of diag = the step at that cell is a hit (its eq bit set) or a substitution, of del = a deletion; a bit set in
// neither = an insertion.  The one copy of the rule: eal_decide reads a cell of these words, the traceback kernel whole runs.
MSOCR_EDL_HD void eal_moves(uint64_t eq, uint64_t d0, uint64_t pv, uint64_t& diag, uint64_t& del) {
  diag = eq | ~d0;
  del = ~diag & pv;
}

// the rule at one cell: bit = its row in the block
MSOCR_EDL_HD int eal_decide(uint64_t eq, uint64_t d0, uint64_t pv, int bit) {
  uint64_t diag, del;
  eal_moves(eq, d0, pv, diag, del);
  if ((diag >> bit) & 1) return ((eq >> bit) & 1) ? EAL_HIT : EAL_SUB;
  return ((del >> bit) & 1) ? EAL_DEL : EAL_INS;
}

MSOCR_EDL_HD int64_t eal_trace_cells(int m, int n) { return (int64_t)edl_nblocks(m) * n; }

// ---- host side -------------------------------------------------------------------------------------------------------------
// The workspace of the device route, in bytes from its start: the heads of edit_distance_long.h [N], one int64 per pair (where its
// trace starts, in cells), the mask tables, and, from the next multiple of 16, the traces.
struct eal_layout {
  int64_t trace_off, tables, table_words, trace, total;
};

// edl_check_heads for the alignment: the same refusals; returns the bytes (heads + trace offsets + tables + traces), or -1
inline int64_t eal_check_heads(const int32_t* a_off, const int32_t* b_off, const int32_t* v, int N, eal_layout* lay = nullptr) {
  const int64_t dist_bytes = edl_check_heads(a_off, b_off, v, N);
  if (dist_bytes < 0) return -1;
  int64_t cells = 0;
  for (int p = 0; p < N; ++p) cells += eal_trace_cells(a_off[p + 1] - a_off[p], b_off[p + 1] - b_off[p]);  // <= N * 2^22
  eal_layout l;
  l.trace_off = (int64_t)N * (int64_t)sizeof(edl_pair);
  l.tables = l.trace_off + (int64_t)N * 8;
  l.table_words = (dist_bytes - l.trace_off) / 8;
  l.trace = (dist_bytes + (int64_t)N * 8 + 15) & ~15ll;
  l.total = l.trace + cells * (int64_t)sizeof(eal_cell);
  if (lay) *lay = l;
  return l.total;
}

// where each pair's trace starts, in cells (off [N]); the arrays have passed eal_check_heads
inline void eal_fill_trace_offsets(const int32_t* a_off, const int32_t* b_off, int N, int64_t* off) {
  int64_t cells = 0;
  for (int p = 0; p < N; ++p) {
    off[p] = cells;
    cells += eal_trace_cells(a_off[p + 1] - a_off[p], b_off[p + 1] - b_off[p]);
  }
}

// edl_distance_host that keeps the trace (trace [nb][n]); m > 0
inline int eal_forward_host(const uint64_t* tab, int m, int v, const int32_t* b, int n, uint64_t* pv, uint64_t* mv, eal_cell* trace) {
  const int nb = edl_nblocks(m);
  for (int blk = 0; blk < nb; ++blk) {
    pv[blk] = edl_begin_pv(m, blk);
    mv[blk] = 0;
  }
  int score = m;
  for (int t = 0; t < n; ++t) {
    const int32_t c = b[t];
    int h = 1;
    for (int blk = 0; blk < nb; ++blk) {
      eal_cell& cell = trace[(int64_t)blk * n + t];
      h = eal_advance(pv[blk], mv[blk], edl_eq(tab, v, nb, c, blk), h, edl_top_bit(m, blk), cell.d0);
      cell.pv = pv[blk];
    }
    score += h;
  }
  return score;
}

// the walk back from (m, n): a_map [m], b_map [n] <- the partner's index or -1, counts [4] <- {hits, substitutions, deletions,
// insertions}.  Every i and every j is left exactly once, so every element of both maps is written exactly once.  tab and trace
// are not read where m or n is 0.
inline void eal_traceback_host(const uint64_t* tab, int m, int v, const int32_t* b, int n, const eal_cell* trace, int32_t* a_map,
                               int32_t* b_map, int32_t* counts) {
  const int nb = edl_nblocks(m);
  int i = m, j = n;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  while (i > 0 && j > 0) {
    const int blk = (i - 1) >> 6;
    const eal_cell& cell = trace[(int64_t)blk * n + (j - 1)];
    const int op = eal_decide(edl_eq(tab, v, nb, b[j - 1], blk), cell.d0, cell.pv, (i - 1) & 63);
    ++counts[op];
    if (op == EAL_HIT || op == EAL_SUB) {
      a_map[i - 1] = j - 1;
      b_map[j - 1] = i - 1;
      --i;
      --j;
    } else if (op == EAL_DEL) {
      a_map[--i] = -1;
    } else {
      b_map[--j] = -1;
    }
  }
  counts[EAL_DEL] += i;
  counts[EAL_INS] += j;
  while (i > 0) a_map[--i] = -1;
  while (j > 0) b_map[--j] = -1;
}
#endif
