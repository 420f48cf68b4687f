// edit_distance_weighted_fuzz.cpp — drives csrc/edit_distance_weighted.h (the arithmetic of the weighted nearest-word kernel and its host
// twin) over corrupted word lists, garbage rows and t_run values and arbitrary cost tables under the address and undefined-behaviour
// sanitizers.  Every array lives in a heap block of its exact size, so a read one element outside it is a report.  Both forms of the
// distance, the plain column DP and the query-profile form the kernel runs, are compared with a full-table dynamic programme written
// here, on well-formed and on corrupted inputs alike (a symbol outside [0, V) costs `unknown` in all three).
// usage: edit_distance_weighted_fuzz [iterations]; prints "rounds <n> checked <pairs>" and exits 0, or 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "edit_distance_weighted.h"

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

struct Costs {
  const uint8_t *sub, *del, *ins;
  int V, unknown;
  bool in(int32_t s) const { return s >= 0 && s < V; }
  int s(int32_t a, int32_t b) const { return in(a) && in(b) ? sub[(size_t)a * V + b] : unknown; }
  int d(int32_t a) const { return in(a) ? del[a] : unknown; }
  int i(int32_t b) const { return in(b) ? ins[b] : unknown; }
};

// the full table, rows = row symbols a [m], columns = word tokens b [n]
static int dp(const Costs& c, const int32_t* a, int m, const int32_t* b, int n) {
  std::vector<std::vector<int>> D(m + 1, std::vector<int>(n + 1, 0));
  for (int i = 1; i <= m; ++i) D[i][0] = D[i - 1][0] + c.d(a[i - 1]);
  for (int j = 1; j <= n; ++j) D[0][j] = D[0][j - 1] + c.i(b[j - 1]);
  for (int i = 1; i <= m; ++i)
    for (int j = 1; j <= n; ++j) {
      int v = D[i - 1][j - 1] + c.s(a[i - 1], b[j - 1]);
      if (D[i - 1][j] + c.d(a[i - 1]) < v) v = D[i - 1][j] + c.d(a[i - 1]);
      if (D[i][j - 1] + c.i(b[j - 1]) < v) v = D[i][j - 1] + c.i(b[j - 1]);
      D[i][j] = v;
    }
  return D[m][n];
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
  long checked = 0;
  for (int it = 0; it < rounds; ++it) {
    static const int Vs[5] = {1, 4, 58, 194, 512};
    const int V = Vs[rnd() % 5];
    // cost tables of exact size: well-formed (zero diagonal, the rest 1..255) or anything at all
    std::unique_ptr<uint8_t[]> sub(new uint8_t[(size_t)V * V]), del(new uint8_t[V]), ins(new uint8_t[V]);
    const bool wild_costs = rnd() % 4 == 0;
    for (int a = 0; a < V; ++a) {
      del[a] = (uint8_t)(wild_costs ? rnd() : rnd_in(1, 255));
      ins[a] = (uint8_t)(wild_costs ? rnd() : rnd_in(1, 255));
      for (int b = 0; b < V; ++b) sub[(size_t)a * V + b] = (uint8_t)(wild_costs ? rnd() : (a == b ? 0 : rnd_in(1, 255)));
    }
    const int unknown = rnd_in(1, 255);
    const Costs costs{sub.get(), del.get(), ins.get(), V, unknown};
    int min_ins = 255, min_del = 255;
    for (int a = 0; a < V; ++a) {
      if (ins[a] < min_ins) min_ins = ins[a];
      if (del[a] < min_del) min_del = del[a];
    }
    if (unknown < min_ins) min_ins = unknown;  // this program's rows and words hold symbols outside [0, V) too
    if (unknown < min_del) min_del = unknown;

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

    // the query profile in blocks of exact size
    const int stride = MSOCR_EDW_PROFILE_STRIDE;
    std::unique_ptr<uint64_t[]> prof_block(new uint64_t[(size_t)(V + 1) * stride / 8]);  // 8-byte aligned, (V + 1) * stride bytes
    uint8_t* prof = (uint8_t*)prof_block.get();
    memset(prof, 0xa5, (size_t)(V + 1) * stride);
    std::unique_ptr<uint8_t[]> insl(new uint8_t[V + 1]);
    std::unique_ptr<uint32_t[]> dpk(new uint32_t[MSOCR_ED_MAX_PATTERN / 4]);
    edw_build_profile(sub.get(), del.get(), ins.get(), V, unknown, sym.get(), m, prof, stride, insl.get(), dpk.get());

    // a word list of exact size, then corrupted
    const int n_words = rnd_in(1, 24);
    std::vector<int> lens(n_words);
    int n_tok = 0;
    for (int& l : lens) { l = rnd_in(1, rnd() % 4 ? 12 : 63); n_tok += l; }
    std::unique_ptr<int32_t[]> begin(new int32_t[n_words + 1]);
    std::unique_ptr<int32_t[]> tok(new int32_t[n_tok]);
    begin[0] = 0;
    for (int i = 0; i < n_words; ++i) begin[i + 1] = begin[i] + lens[i];
    for (int t = 0; t < n_tok; ++t) tok[t] = (int32_t)(rnd() % (uint32_t)V);
    if (rnd() % 2 == 0) {
      for (int c = rnd_in(1, 4); c > 0; --c) {
        if (rnd() % 2) begin[rnd_in(0, n_words)] = rnd() % 3 ? garbage() : rnd_in(-3, n_tok + 3);
        else tok[rnd_in(0, n_tok - 1)] = garbage();
      }
    }
    for (int w = -2; w < n_words + 2; ++w) {  // indices outside the list too: an empty range
      int lo, n;
      ed_word_range(begin.get(), n_words, n_tok, w, lo, n);
      if (lo < 0 || n < 0 || n > MSOCR_ED_MAX_WORD || lo + n > n_tok) { printf("range outside the list\n"); return 1; }
      const int want = dp(costs, sym.get(), m, tok.get() + lo, n);
      const int d = edw_distance(sub.get(), del.get(), ins.get(), V, unknown, sym.get(), m, tok.get() + lo, n);
      if (d != want) { printf("distance %d, dynamic programme %d (m %d n %d V %d)\n", d, want, m, n, V); return 1; }
      const int dq = edw_distance_profile(prof, stride, insl.get(), dpk.get(), V, m, tok.get() + lo, n);
      if (dq != want) { printf("profile form %d, dynamic programme %d (m %d n %d V %d)\n", dq, want, m, n, V); return 1; }
      if (want > (MSOCR_ED_MAX_PATTERN + MSOCR_ED_MAX_WORD) * MSOCR_EDW_MAX_COST) { printf("distance beyond the largest\n"); return 1; }
      if (!wild_costs && edw_length_bound(m, n, min_ins, min_del) > want) { printf("the length bound exceeds the distance\n"); return 1; }
      ++checked;
    }
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
