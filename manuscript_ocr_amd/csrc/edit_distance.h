// edit_distance.h — the exact Levenshtein distance (unit costs) between a recognised row and a lexicon word, or between two rows, and
// the reads the nearest-word lookup makes of a word list (CSR arrays of msocr_wordlist: word_begin [n_words + 1], word_tok [n_tok]).
// Host and device: the kernels of lexicon_nearest.hip call these functions, and so do their host twins and a plain C++ program that
// feeds them corrupted word lists and garbage rows under the address and undefined-behaviour sanitizers
// (tests/native/edit_distance_fuzz.cpp).  Whatever the arrays hold, every index formed here lies inside them: a malformed list can
// give a wrong distance, not an out-of-bounds read.
//
// The distance is Myers' bit-parallel dynamic programme in Hyyrö's global-distance form: the pattern (a row's text, 0..64 symbols) is
// one 64-bit column of vertical deltas (pv / mv), a text symbol costs one ed_step.  With m == 64 the carry out of bit 63 is dropped,
// which is what the recurrence wants (there is no row 65).
#ifndef MSOCR_EDIT_DISTANCE_H
#define MSOCR_EDIT_DISTANCE_H
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MSOCR_ED_HD __host__ __device__ __forceinline__
#else
#define MSOCR_ED_HD inline
#endif

#define MSOCR_ED_MAX_PATTERN 64  // symbols of a row's text: one DP column per 64-bit word
#define MSOCR_ED_MAX_WORD 63     // tokens of a lexicon word (Lexicon: max_len - 1 <= 63); a longer one is read up to here
#define MSOCR_ED_MAX_V 512       // match masks per pattern

// A row's text, the rule of TRBA.texts: the ids before the first eos_id among the first min(max(trun, 0), steps, 64) steps, pad_id and
// blank_id (-1 = none) removed.  sym [64] receives them as they are (an id outside [0, V) stays a symbol that matches nothing);
// returns their number.
MSOCR_ED_HD int ed_row_text(const int32_t* ids, int steps, int trun, int eos_id, int pad_id, int blank_id, int32_t* sym) {
  int e = trun < 0 ? 0 : (trun > steps ? steps : trun);
  if (e > MSOCR_ED_MAX_PATTERN) e = MSOCR_ED_MAX_PATTERN;
  int m = 0;
  for (int t = 0; t < e; ++t) {
    const int32_t v = ids[t];
    if (v == eos_id) break;
    if (v == pad_id || (blank_id >= 0 && v == blank_id)) continue;
    sym[m++] = v;
  }
  return m;
}

// peq [V] <- for every token its positions in sym [m] as a bit mask; a symbol outside [0, V) sets no bit and is never an index
MSOCR_ED_HD void ed_build_masks(const int32_t* sym, int m, int V, uint64_t* peq) {
  for (int v = 0; v < V; ++v) peq[v] = 0;
  for (int j = 0; j < m; ++j)
    if (sym[j] >= 0 && sym[j] < V) peq[sym[j]] |= 1ull << j;
}

struct ed_state {
  uint64_t pv, mv, top;
  int score;
};

// the DP column before any text symbol: D[i][0] = i
MSOCR_ED_HD ed_state ed_begin(int m) {
  ed_state s;
  s.pv = m >= 64 ? ~0ull : (1ull << m) - 1;
  s.mv = 0;
  s.top = m > 0 ? 1ull << (m - 1) : 0;
  s.score = m;
  return s;
}

// one text symbol whose match mask against the pattern is eq
MSOCR_ED_HD void ed_step(ed_state& s, uint64_t eq) {
  const uint64_t xv = eq | s.mv;
  const uint64_t xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
  uint64_t ph = s.mv | ~(xh | s.pv);
  uint64_t mh = s.pv & xh;
  s.score += (ph & s.top) != 0;
  s.score -= (mh & s.top) != 0;
  ph = (ph << 1) | 1;
  mh <<= 1;
  s.pv = mh | ~(xv | ph);
  s.mv = ph & xv;
}

// the token range of word i, [lo, lo + n): the begins clamped into [0, n_tok] with lo <= hi, and n at most MSOCR_ED_MAX_WORD; empty
// for i outside [0, n_words)
MSOCR_ED_HD void ed_word_range(const int32_t* word_begin, int n_words, int n_tok, int i, int& lo, int& n) {
  lo = n = 0;
  if (i < 0 || i >= n_words) return;
  const int b0 = word_begin[i], b1 = word_begin[i + 1];
  lo = b0 < 0 ? 0 : (b0 > n_tok ? n_tok : b0);
  const int hi = b1 < lo ? lo : (b1 > n_tok ? n_tok : b1);
  n = hi - lo > MSOCR_ED_MAX_WORD ? MSOCR_ED_MAX_WORD : hi - lo;
}

// distance between the pattern whose masks are peq [V] (m symbols) and tok [n]; a token outside [0, V) matches nothing
MSOCR_ED_HD int ed_distance_masks(const uint64_t* peq, int V, int m, const int32_t* tok, int n) {
  if (m <= 0) return n;
  ed_state s = ed_begin(m);
  for (int t = 0; t < n; ++t) {
    const int32_t c = tok[t];
    ed_step(s, (c >= 0 && c < V) ? peq[c] : 0ull);
  }
  return s.score;
}

// match mask of token c against a [m] without a table; c or a symbol outside [0, V) matches nothing
MSOCR_ED_HD uint64_t ed_eq_scan(const int32_t* a, int m, int V, int32_t c) {
  uint64_t eq = 0;
  if (c < 0 || c >= V) return 0;
  for (int j = 0; j < m; ++j) eq |= (uint64_t)(a[j] == c) << j;
  return eq;
}

// distance between two symbol sequences of at most 64 symbols each, no table (the pair form)
MSOCR_ED_HD int ed_distance_scan(const int32_t* a, int m, const int32_t* b, int n, int V) {
  if (m <= 0) return n;
  ed_state s = ed_begin(m);
  for (int t = 0; t < n; ++t) ed_step(s, ed_eq_scan(a, m, V, b[t]));
  return s.score;
}

// top-k keys: (distance << 32) | index, so that ascending keys are ascending (distance, index); ED_NO_KEY marks an unfilled rank
#define MSOCR_ED_NO_KEY (~0ull)
MSOCR_ED_HD uint64_t ed_key(int dist, int index) { return ((uint64_t)(uint32_t)dist << 32) | (uint32_t)index; }

// insert key into the ascending list best [k] if it is smaller than the last entry
MSOCR_ED_HD void ed_topk_insert(uint64_t* best, int k, uint64_t key) {
  if (key >= best[k - 1]) return;
  int r = k - 1;
  while (r > 0 && best[r - 1] > key) {
    best[r] = best[r - 1];
    --r;
  }
  best[r] = key;
}
#endif
