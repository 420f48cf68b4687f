// edit_distance_fuzz.cpp — drives csrc/edit_distance.h (the arithmetic of the nearest-word kernels and their host twins) over corrupted
// word lists and garbage rows under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its exact
// size, so a read one element outside it is a report.  On valid inputs the bit-parallel distance is also compared with the textbook
// dynamic programme.  usage: edit_distance_fuzz [iterations]; prints "rounds <n> checked <pairs>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "edit_distance.h"

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
    default: return (int32_t)(rnd() % 600);
  }
}

static int dp(const int32_t* a, int m, const int32_t* b, int n, int V) {
  std::vector<int> prev(n + 1), cur(n + 1);
  for (int j = 0; j <= n; ++j) prev[j] = j;
  for (int i = 1; i <= m; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      const bool eq = a[i - 1] == b[j - 1] && a[i - 1] >= 0 && a[i - 1] < V;
      int v = prev[j - 1] + (eq ? 0 : 1);
      if (prev[j] + 1 < v) v = prev[j] + 1;
      if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
      cur[j] = v;
    }
    prev.swap(cur);
  }
  return prev[n];
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
  long checked = 0;
  for (int it = 0; it < rounds; ++it) {
    static const int Vs[5] = {2, 4, 58, 194, 512};
    const int V = Vs[rnd() % 5];
    // a row of exactly `steps` ids, possibly garbage, with t_run anywhere
    const int steps = rnd_in(1, 64);
    std::unique_ptr<int32_t[]> row(new int32_t[steps]);
    const bool wild_row = rnd() % 3 == 0;
    for (int t = 0; t < steps; ++t) row[t] = wild_row ? garbage() : (int32_t)(rnd() % (uint32_t)V);
    const int eos = rnd_in(0, V - 1), pad = rnd_in(0, V - 1), blank = rnd() % 2 ? -1 : rnd_in(0, V - 1);
    const int truns[7] = {-5, 0, steps / 2, steps, steps + 7, INT32_MAX, INT32_MIN};
    const int trun = truns[rnd() % 7];
    std::unique_ptr<int32_t[]> sym(new int32_t[MSOCR_ED_MAX_PATTERN]);
    const int m = ed_row_text(row.get(), steps, trun, eos, pad, blank, sym.get());
    if (m < 0 || m > steps) { printf("bad text length %d\n", m); return 1; }
    std::unique_ptr<uint64_t[]> peq(new uint64_t[V]);
    ed_build_masks(sym.get(), m, V, peq.get());

    // a word list of exact size, then corrupted
    const int n_words = rnd_in(1, 40);
    std::vector<int> lens(n_words);
    int n_tok = 0;
    for (int& l : lens) { l = rnd_in(1, rnd() % 4 ? 12 : 63); n_tok += l; }
    std::unique_ptr<int32_t[]> begin(new int32_t[n_words + 1]);
    std::unique_ptr<int32_t[]> tok(new int32_t[n_tok]);
    begin[0] = 0;
    for (int i = 0; i < n_words; ++i) begin[i + 1] = begin[i] + lens[i];
    for (int t = 0; t < n_tok; ++t) tok[t] = (int32_t)(rnd() % (uint32_t)V);
    const bool corrupt = rnd() % 2 == 0;
    if (corrupt) {
      for (int c = rnd_in(1, 4); c > 0; --c) {
        if (rnd() % 2) begin[rnd_in(0, n_words)] = rnd() % 3 ? garbage() : rnd_in(-3, n_tok + 3);
        else tok[rnd_in(0, n_tok - 1)] = garbage();
      }
    }
    uint64_t best[16];
    const int k = rnd_in(1, 16);
    for (int r = 0; r < k; ++r) best[r] = MSOCR_ED_NO_KEY;
    for (int w = -2; w < n_words + 2; ++w) {  // indices outside the list too: an empty range
      int lo, n;
      ed_word_range(begin.get(), n_words, n_tok, w, lo, n);
      if (lo < 0 || n < 0 || n > MSOCR_ED_MAX_WORD || lo + n > n_tok) { printf("range outside the list\n"); return 1; }
      const int d = ed_distance_masks(peq.get(), V, m, tok.get() + lo, n);
      const int want = dp(sym.get(), m, tok.get() + lo, n, V);
      if (d != want) { printf("distance %d, dynamic programme %d (m %d n %d V %d)\n", d, want, m, n, V); return 1; }
      if (ed_distance_scan(sym.get(), m, tok.get() + lo, n, V) != want) { printf("scan form differs\n"); return 1; }
      if (w >= 0 && w < n_words) ed_topk_insert(best, k, ed_key(d, w));
      ++checked;
    }
    for (int r = 1; r < k; ++r)
      if (best[r - 1] > best[r] || (best[r] != MSOCR_ED_NO_KEY && best[r - 1] == best[r])) { printf("top-k not ascending\n"); return 1; }
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
