// edit_distance_weighted.h — the edit distance between a recognised row and a lexicon word under per-symbol costs (DESIGN.md section
// 4.26): what it costs to turn the ROW into the WORD.  sub [V][V] u8, sub[a * V + b] = reading recognised symbol a as lexicon symbol b
// (not symmetric); del [V] u8 = dropping recognised symbol a; ins [V] u8 = supplying lexicon symbol b; any edit that involves a symbol
// outside [0, V), on either side, costs `unknown` (such a symbol matches nothing, itself included: edit_distance.h's rule).
// Host and device: the kernel of lexicon_nearest.hip calls these functions, and so do its host twin and a plain C++ program that feeds
// them corrupted word lists, garbage rows, t_run values and cost tables under the address and undefined-behaviour sanitizers
// (tests/native/edit_distance_weighted_fuzz.cpp).  Whatever the arrays hold, every index formed here lies inside them: a malformed
// list, row or table can give a wrong distance, not an out-of-bounds read.  The row's text is ed_row_text's (0..64 symbols), a
// word's range ed_word_range's (0..63 tokens), both of edit_distance.h.
//
// The distance is the textbook dynamic programme, one column of m + 1 values over the row's symbols per word token:
//   D[i][0] = sum of del over the first i row symbols      D[0][j] = sum of ins over the first j word tokens
//   D[i][j] = min(D[i-1][j-1] + sub, D[i-1][j] + del, D[i][j-1] + ins)
// in int32: every cost is at most 255 and a path has at most 64 + 63 edits, so no value exceeds 127 * 255 = 32 385.
#ifndef MSOCR_EDIT_DISTANCE_WEIGHTED_H
#define MSOCR_EDIT_DISTANCE_WEIGHTED_H
#include "edit_distance.h"

#define MSOCR_EDW_MAX_COST 255

// cost of reading recognised symbol a as lexicon symbol b
MSOCR_ED_HD int edw_sub(const uint8_t* sub, int V, int unknown, int32_t a, int32_t b) {
  return (a < 0 || a >= V || b < 0 || b >= V) ? unknown : (int)sub[(size_t)a * V + b];
}
// cost of dropping recognised symbol a (vec = del), or of supplying lexicon symbol b (vec = ins)
MSOCR_ED_HD int edw_one(const uint8_t* vec, int V, int unknown, int32_t s) { return (s < 0 || s >= V) ? unknown : (int)vec[s]; }

// one cell: diag = D[i-1][j-1], left = D[i][j-1] (the same row symbol, one word token less), up = D[i-1][j]
MSOCR_ED_HD int edw_cell(int diag, int left, int up, int sub_c, int ins_c, int del_c) {
  const int a = diag + sub_c, b = left + ins_c, c = up + del_c;
  const int ab = a < b ? a : b;
  return ab < c ? ab : c;
}

// what a word of n tokens costs a row of m symbols at the least: the tokens it has too many are supplied, those it lacks dropped.
// min_ins / min_del must be lower bounds over EVERY symbol that can occur, so min(the vector's minimum, unknown) where rows or words
// may hold symbols outside [0, V).
MSOCR_ED_HD int edw_length_bound(int m, int n, int min_ins, int min_del) { return n > m ? (n - m) * min_ins : (m - n) * min_del; }

// distance between sym [m] (m <= 64) and tok [n] (n <= 63)
MSOCR_ED_HD int edw_distance(const uint8_t* sub, const uint8_t* del, const uint8_t* ins, int V, int unknown, const int32_t* sym, int m,
                             const int32_t* tok, int n) {
  int col[MSOCR_ED_MAX_PATTERN + 1], dl[MSOCR_ED_MAX_PATTERN];
  if (m < 0) m = 0;
  if (m > MSOCR_ED_MAX_PATTERN) m = MSOCR_ED_MAX_PATTERN;
  col[0] = 0;
  for (int i = 0; i < m; ++i) {
    dl[i] = edw_one(del, V, unknown, sym[i]);
    col[i + 1] = col[i] + dl[i];
  }
  for (int t = 0; t < n; ++t) {
    const int32_t c = tok[t];
    const int ins_c = edw_one(ins, V, unknown, c);
    int diag = col[0];
    col[0] += ins_c;
    for (int i = 0; i < m; ++i) {
      const int left = col[i + 1];
      col[i + 1] = edw_cell(diag, left, col[i], edw_sub(sub, V, unknown, sym[i], c), ins_c, dl[i]);
      diag = left;
    }
  }
  return col[m];
}

// ---- the same distance from a query profile: the form the kernel runs, one row against many words.
// The row is laid against the END of a 64-position column: symbol j sits at position 64 - m + j, so that the distance is always the
// column's last entry and no loop depends on where the row ends, only on where it starts: the first group of 8 positions that holds a
// symbol, g0 = (64 - m) / 8.  Positions of that group in front of the row are padding that costs nothing to drop (del 0) and 255 to
// read as any token: since no insert costs more than 255, such a position hands the value above it down unchanged.
// prof: V + 1 rows of `stride` bytes (stride >= 64, a multiple of 8; prof 8-byte aligned), row c = what each position costs to be read
// as token c, prof[c * stride + 64 - m + j] = edw_sub(sym[j], c); row V stands for every token outside [0, V).  insl [V + 1]: the
// insert cost of token c, insl[V] = unknown.  dpk [16]: the positions' delete costs, four to a word, position p in byte p & 3 of
// dpk[p >> 2].  Positions in front of group g0 are never read.
#define MSOCR_EDW_PROFILE_STRIDE 72  // 18 banks of 4 bytes: the rows of neighbouring tokens start in different LDS banks

MSOCR_ED_HD int edw_first_group(int m) { return (MSOCR_ED_MAX_PATTERN - (m < 0 ? 0 : (m > MSOCR_ED_MAX_PATTERN ? MSOCR_ED_MAX_PATTERN : m))) >> 3; }

// one profile entry: position p (>= 8 * edw_first_group(m)) of the row sym [m] against token c in [0, V]
MSOCR_ED_HD uint8_t edw_profile_entry(const uint8_t* sub, int V, int unknown, const int32_t* sym, int m, int p, int c) {
  const int j = p - (MSOCR_ED_MAX_PATTERN - m);
  return j < 0 ? (uint8_t)MSOCR_EDW_MAX_COST : (uint8_t)edw_sub(sub, V, unknown, sym[j], c);
}
// delete costs of positions 4 q .. 4 q + 3, packed
MSOCR_ED_HD uint32_t edw_profile_deletes(const uint8_t* del, int V, int unknown, const int32_t* sym, int m, int q) {
  uint32_t w = 0;
  for (int e = 0; e < 4; ++e) {
    const int j = q * 4 + e - (MSOCR_ED_MAX_PATTERN - m);
    if (j >= 0) w |= (uint32_t)edw_one(del, V, unknown, sym[j]) << (8 * e);
  }
  return w;
}

MSOCR_ED_HD void edw_build_profile(const uint8_t* sub, const uint8_t* del, const uint8_t* ins, int V, int unknown, const int32_t* sym,
                                   int m, uint8_t* prof, int stride, uint8_t* insl, uint32_t* dpk) {
  const int p0 = edw_first_group(m) * 8;
  for (int c = 0; c <= V; ++c) {
    insl[c] = (uint8_t)edw_one(ins, V, unknown, c);
    for (int p = p0; p < MSOCR_ED_MAX_PATTERN; ++p) prof[(size_t)c * stride + p] = edw_profile_entry(sub, V, unknown, sym, m, p, c);
  }
  for (int q = 0; q < MSOCR_ED_MAX_PATTERN / 4; ++q) dpk[q] = edw_profile_deletes(del, V, unknown, sym, m, q);
}

// The column lives in registers: every loop over it is unrolled with constant indices and skips the groups in front of g0, which is
// the same for all lanes of a workgroup.  0 <= m <= 64, n <= 63.
MSOCR_ED_HD int edw_distance_profile(const uint8_t* prof, int stride, const uint8_t* insl, const uint32_t* dpk, int V, int m,
                                     const int32_t* tok, int n) {
  const int g0 = edw_first_group(m);
  int col[MSOCR_ED_MAX_PATTERN];
  int top = 0;  // the value above the column: the inserts of the tokens so far
  {
    int acc = 0;
#pragma unroll
    for (int g = 0; g < MSOCR_ED_MAX_PATTERN / 8; ++g) {
      if (g < g0) continue;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = g * 8 + e;
        acc += (int)((dpk[i >> 2] >> (8 * (i & 3))) & 255u);
        col[i] = acc;
      }
    }
  }
  for (int t = 0; t < n; ++t) {
    const int32_t c = tok[t];
    const int cc = (c >= 0 && c < V) ? c : V;
    const int ins_c = insl[cc];
    const uint8_t* p = (const uint8_t*)__builtin_assume_aligned(prof + (size_t)cc * stride, 8);
    int diag = top;
    top += ins_c;
    int up = top;
#pragma unroll
    for (int g = 0; g < MSOCR_ED_MAX_PATTERN / 8; ++g) {
      if (g < g0) continue;
      uint64_t pk;
      __builtin_memcpy(&pk, p + g * 8, 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = g * 8 + e;
        const int left = col[i];
        up = edw_cell(diag, left, up, (int)((pk >> (8 * e)) & 255u), ins_c, (int)((dpk[i >> 2] >> (8 * (i & 3))) & 255u));
        col[i] = up;
        diag = left;
      }
    }
  }
  return g0 < MSOCR_ED_MAX_PATTERN / 8 ? col[MSOCR_ED_MAX_PATTERN - 1] : top;
}
#endif
