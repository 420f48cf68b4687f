// edit_distance_long.h — the exact Levenshtein distance (unit costs) between two int32 token sequences of 0..MSOCR_EDL_MAX_LEN tokens
// each: the running text of a page against its transcription, as characters or as words (include/msocr.h, "page-level error rates";
// DESIGN.md section 4.22).  Host and device: the kernels of edit_distance_long.hip call these functions, the host twin
// msocr_edit_distance_long_host is edl_distance_host below, and a plain C++ program feeds them garbage tokens and offset arrays under
// the address and undefined-behaviour sanitizers (tests/native/edit_distance_long_fuzz.cpp).  Whatever the token arrays hold, every
// index formed here lies inside them and inside the mask table.
//
// The recurrence is ed_step of edit_distance.h in its block form (Hyyrö's advance_block): the pattern (m tokens) is cut into
// nb = ceil(m / 64) words of vertical deltas, block 0 at the top.  For one text symbol a block takes a horizontal carry
// hin in {-1, 0, +1} (block 0: always +1, the first row of the table; any other block: the hout of the block above it for the same
// symbol) and gives hout, the horizontal delta of its bottom row: bit 63, or bit (m - 1) % 64 in the last block, where it is added
// to the score.  The last block's bits above that one hold garbage that never reaches a lower bit (additions and shifts carry upwards
// only), exactly as in ed_begin / ed_step at m < 64.
// Match masks: a table [v][nb] of 64-bit words, word [c][blk] = the positions of token c in pattern block blk.  A token outside
// [0, v), on either side, matches nothing and is never an index: the rule of edit_distance.h.
#ifndef MSOCR_EDIT_DISTANCE_LONG_H
#define MSOCR_EDIT_DISTANCE_LONG_H
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MSOCR_EDL_HD __host__ __device__ __forceinline__
#else
#define MSOCR_EDL_HD inline
#endif

#define MSOCR_EDL_MAX_LEN 16384                       // tokens of either side
#define MSOCR_EDL_MAX_BLOCKS (MSOCR_EDL_MAX_LEN / 64)  // 256 = 64 lanes x 4 blocks

// what the kernels know of a pair: uploaded to the head of the workspace, one record per pair
struct edl_pair {
  int64_t tab;         // where the pair's mask table starts, in 64-bit words behind the heads
  int32_t a0, m;       // pattern: tokens a_tok[a0 .. a0 + m)
  int32_t b0, n;       // text:    tokens b_tok[b0 .. b0 + n)
  int32_t v, nb;       // alphabet of the table, blocks of the pattern
};

MSOCR_EDL_HD int edl_nblocks(int m) { return (m + 63) >> 6; }

// vertical deltas of block blk before any text symbol (D[i][0] = i: all +1 up to row m)
MSOCR_EDL_HD uint64_t edl_begin_pv(int m, int blk) {
  const int rows = m - blk * 64;
  return rows >= 64 ? ~0ull : (rows > 0 ? (1ull << rows) - 1 : 0ull);
}

// the bit of block blk at which hout is read
MSOCR_EDL_HD int edl_top_bit(int m, int blk) { return blk == edl_nblocks(m) - 1 ? (m - 1) & 63 : 63; }

// one text symbol in one block: eq = its match mask against the block's 64 pattern tokens; returns hout
MSOCR_EDL_HD int edl_advance(uint64_t& pv, uint64_t& mv, uint64_t eq, int hin, int top_bit) {
  const uint64_t hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
  const uint64_t xv = eq | mv;
  eq |= hneg;
  const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
  uint64_t ph = mv | ~(xh | pv);
  uint64_t mh = pv & xh;
  const int hout = (int)((ph >> top_bit) & 1) - (int)((mh >> top_bit) & 1);
  ph = (ph << 1) | hpos;
  mh = (mh << 1) | hneg;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
  return hout;
}

// match mask of token c in block blk of a table [v][nb]; c outside [0, v) matches nothing
MSOCR_EDL_HD uint64_t edl_eq(const uint64_t* tab, int v, int nb, int32_t c, int blk) {
  return (c >= 0 && c < v) ? tab[(int64_t)c * nb + blk] : 0ull;
}

// words of a pair's table
MSOCR_EDL_HD int64_t edl_table_words(int m, int v) { return (int64_t)v * edl_nblocks(m); }

// ---- host side -------------------------------------------------------------------------------------------------------------
// The argument check both entry points make of the HOST arrays, and the workspace the device route needs:
// offsets monotone from a value >= 0, every length <= MSOCR_EDL_MAX_LEN, every v >= 0.  Returns the bytes (heads + tables), or -1.
inline int64_t edl_check_heads(const int32_t* a_off, const int32_t* b_off, const int32_t* v, int N) {
  if (N < 0) return -1;
  if (N == 0) return 0;
  if (!a_off || !b_off || !v) return -1;
  if (a_off[0] < 0 || b_off[0] < 0) return -1;
  int64_t words = 0;
  for (int p = 0; p < N; ++p) {
    const int64_t m = (int64_t)a_off[p + 1] - a_off[p], n = (int64_t)b_off[p + 1] - b_off[p];
    if (m < 0 || n < 0 || m > MSOCR_EDL_MAX_LEN || n > MSOCR_EDL_MAX_LEN || v[p] < 0) return -1;
    words += edl_table_words((int)m, v[p]);
    if (words > (1ll << 58)) return -1;
  }
  return (int64_t)N * (int64_t)sizeof(edl_pair) + words * 8;
}

// the heads as the kernels read them (heads [N]); the arrays have passed edl_check_heads
inline void edl_fill_heads(const int32_t* a_off, const int32_t* b_off, const int32_t* v, int N, edl_pair* heads) {
  int64_t words = 0;
  for (int p = 0; p < N; ++p) {
    edl_pair& h = heads[p];
    h.tab = words;
    h.a0 = a_off[p];
    h.m = a_off[p + 1] - a_off[p];
    h.b0 = b_off[p];
    h.n = b_off[p + 1] - b_off[p];
    h.v = v[p];
    h.nb = edl_nblocks(h.m);
    words += edl_table_words(h.m, h.v);
  }
}

// tab [v][nb] <- the match masks of a [m]; a token outside [0, v) sets no bit
inline void edl_build_table_host(const int32_t* a, int m, int v, uint64_t* tab) {
  const int nb = edl_nblocks(m);
  const int64_t words = edl_table_words(m, v);
  for (int64_t i = 0; i < words; ++i) tab[i] = 0;
  for (int j = 0; j < m; ++j)
    if (a[j] >= 0 && a[j] < v) tab[(int64_t)a[j] * nb + (j >> 6)] |= 1ull << (j & 63);
}

// distance between a [m] (whose table is tab [v][nb]) and b [n], block by block in plain order; pv / mv [nb] are scratch
inline int edl_distance_host(const uint64_t* tab, int m, int v, const int32_t* b, int n, uint64_t* pv, uint64_t* mv) {
  if (m <= 0) return n;
  const int nb = edl_nblocks(m);
  for (int blk = 0; blk < nb; ++blk) {
    pv[blk] = edl_begin_pv(m, blk);
    mv[blk] = 0;
  }
  int score = m;
  for (int t = 0; t < n; ++t) {
    const int32_t c = b[t];
    int h = 1;
    for (int blk = 0; blk < nb; ++blk) h = edl_advance(pv[blk], mv[blk], edl_eq(tab, v, nb, c, blk), h, edl_top_bit(m, blk));
    score += h;
  }
  return score;
}
#endif
