// word_spotting_partial_fuzz.cpp — drives the subsequence part of csrc/word_spotting.h (the argument check, the f64 table with the
// start column every cell carries, the tie rules, the smallest end, the length gate) over garbage lengths and non-finite features
// under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size, so a read or write one
// element outside it is a report.  Lengths are garbage on the way into the checks and into the normalisation (which clamps them);
// the distance runs only on what its entry point's check admits.  Every distance and span is compared with a plain full table.
// usage: word_spotting_partial_fuzz [rounds]; prints "rounds <n> checked <n>" and exits 0, or 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "word_spotting.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }  // inclusive
static float rnd_unit() { return (float)((int)(rnd() % 2001) - 1000) / 1000.f; }
static float garbage_float() {
  switch (rnd() % 12) {
    case 0: return std::numeric_limits<float>::infinity();
    case 1: return -std::numeric_limits<float>::infinity();
    case 2: return std::numeric_limits<float>::quiet_NaN();
    case 3: return 3e38f;
    case 4: return 1e-30f;
    case 5: return 0.f;
    case 6: return -0.f;
    default: return rnd_unit();
  }
}
static int32_t garbage_len(int T) {
  switch (rnd() % 8) {
    case 0: return INT32_MAX;
    case 1: return INT32_MIN;
    case 2: return -1;
    case 3: return 0;
    case 4: return T + 1;
    default: return rnd_in(1, T);
  }
}

template <class X>
static std::unique_ptr<X[]> block(size_t n) { return std::unique_ptr<X[]>(new X[n ? n : 1]); }

static int fail(const char* what, int round) {
  printf("MISMATCH %s in round %d\n", what, round);
  return 1;
}

// the definition over a full table: S, and the column at which every cell's path left row 0
static float plain_sub(const float* a, int La, const float* b, int Lb, int H, int32_t* span) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> S((size_t)La * Lb, inf);
  std::vector<int> st((size_t)La * Lb, -1);
  for (int i = 0; i < La; ++i)
    for (int j = 0; j < Lb; ++j) {
      double dot = 0.0;
      for (int k = 0; k < H; ++k) dot += (double)a[(size_t)i * H + k] * (double)b[(size_t)j * H + k];
      const size_t at = (size_t)i * Lb + j;
      if (i == 0) {
        S[at] = 1.0 - dot;
        st[at] = j;
        continue;
      }
      double best = inf;
      int from = -1;
      if (j) best = S[at - Lb - 1], from = st[at - Lb - 1];
      if (S[at - Lb] < best) best = S[at - Lb], from = st[at - Lb];
      if (j && S[at - 1] < best) best = S[at - 1], from = st[at - 1];
      S[at] = (1.0 - dot) + best;
      st[at] = from;
    }
  const size_t last = (size_t)(La - 1) * Lb;
  int e = 0;
  for (int j = 1; j < Lb; ++j)
    if (S[last + j] < S[last + e]) e = j;
  span[0] = st[last + e];
  span[1] = e + 1;
  return (float)(S[last + e] / (double)La);
}

static bool same_float(float x, float y) { return memcmp(&x, &y, 4) == 0; }

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 100;
  int checked = 0;
  for (int round = 0; round < rounds; ++round) {
    const int T = rnd_in(1, round % 10 == 0 ? 64 : 12), H = 64 * rnd_in(1, round % 7 == 0 ? 8 : 2);
    const int Q = rnd_in(0, 4), N = rnd_in(0, 9);
    auto qf = block<float>((size_t)Q * T * H), cf = block<float>((size_t)N * T * H);
    auto qu = block<float>((size_t)Q * T * H), cu = block<float>((size_t)N * T * H);
    auto ql = block<int32_t>(Q), cl = block<int32_t>(N), lo = block<int32_t>(Q), hi = block<int32_t>(Q);
    auto dist = block<float>((size_t)Q * N);
    auto span = block<int32_t>((size_t)Q * N * 2);
    // ---- the argument check: the envelope on either side, every pointer
    {
      const int t = rnd_in(-1, 66), h = 32 * rnd_in(-1, 18);
      const int n = rnd() % 4 ? rnd_in(-2, 40) : (int)(rnd() & 0x7fffffffu);
      const bool want = n >= 0 && t >= 1 && t <= 64 && h >= 64 && h <= 512 && h % 64 == 0 && (int64_t)n * t * h < ((int64_t)1 << 31);
      const void* ptr[8] = {qu.get(), ql.get(), lo.get(), hi.get(), cu.get(), cl.get(), dist.get(), span.get()};
      if (ws_sub_args_ok(ptr[0], ptr[1], ptr[2], ptr[3], n, ptr[4], ptr[5], 1, t, h, ptr[6], ptr[7]) != want)
        return fail("ws_sub_args_ok, the query side", round);
      if (ws_sub_args_ok(ptr[0], ptr[1], ptr[2], ptr[3], 1, ptr[4], ptr[5], n, t, h, ptr[6], ptr[7]) != want)
        return fail("ws_sub_args_ok, the word side", round);
      const int hole = rnd_in(0, 7);
      ptr[hole] = nullptr;
      if (ws_sub_args_ok(ptr[0], ptr[1], ptr[2], ptr[3], 1, ptr[4], ptr[5], 1, 4, 64, ptr[6], ptr[7])) return fail("a null pointer", round);
    }
    // ---- garbage lengths, garbage features, exact-size blocks
    const bool dirty = round % 3 == 0;
    for (size_t i = 0; i < (size_t)Q * T * H; ++i) qf[i] = dirty ? garbage_float() : rnd_unit();
    for (size_t i = 0; i < (size_t)N * T * H; ++i) cf[i] = dirty ? garbage_float() : rnd_unit();
    for (int q = 0; q < Q; ++q) ql[q] = round % 4 == 0 ? garbage_len(T) : rnd_in(1, T);
    for (int n = 0; n < N; ++n) cl[n] = round % 4 == 0 ? garbage_len(T) : rnd_in(1, T);
    for (int q = 0; q < Q; ++q) {
      lo[q] = round % 5 == 0 ? garbage_len(T) : rnd_in(1, T);
      hi[q] = round % 5 == 0 ? garbage_len(T) : rnd_in(lo[q], T);
    }
    if (round % 6 == 1)  // exact costs: one-hot frames over few symbols, so that ties are everywhere and the tie rules decide
      for (int side = 0; side < 2; ++side) {
        float* f = side ? cf.get() : qf.get();
        for (size_t fr = 0; fr < (size_t)(side ? N : Q) * T; ++fr) {
          for (int e = 0; e < H; ++e) f[fr * H + e] = 0.f;
          f[fr * H + rnd() % 3] = 2.f;
        }
      }
    ws_normalize_host(qf.get(), ql.get(), Q, T, H, qu.get());
    ws_normalize_host(cf.get(), cl.get(), N, T, H, cu.get());
    // ---- the distance and the span, where the entry point's check admits the lengths
    bool ok = ws_sub_args_ok(qu.get(), ql.get(), lo.get(), hi.get(), Q, cu.get(), cl.get(), N, T, H, dist.get(), span.get());
    if (!ok) return fail("ws_sub_args_ok on a legal call", round);
    ok = ws_lens_ok(ql.get(), Q, T) && ws_lens_ok(cl.get(), N, T);
    for (int q = 0; q < Q; ++q) ok = ok && lo[q] <= hi[q];
    if (ok) {
      ws_dtw_sub_host(qu.get(), ql.get(), lo.get(), hi.get(), Q, cu.get(), cl.get(), N, T, H, dist.get(), span.get());
      for (int q = 0; q < Q; ++q)
        for (int n = 0; n < N; ++n) {
          const size_t at = (size_t)q * N + n;
          const float got = dist[at];
          if (cl[n] < lo[q] || cl[n] > hi[q]) {
            if (!(got == std::numeric_limits<float>::infinity()) || span[2 * at] != -1 || span[2 * at + 1] != -1) return fail("the gate", round);
            continue;
          }
          int32_t want_span[2];
          const float want = plain_sub(qu.get() + (size_t)q * T * H, ql[q], cu.get() + (size_t)n * T * H, cl[n], H, want_span);
          if (!same_float(got, want)) return fail("a distance", round);
          if (!std::isfinite(got)) return fail("a non-finite distance of unit frames", round);
          if (span[2 * at] != want_span[0] || span[2 * at + 1] != want_span[1]) return fail("a span", round);
          if (span[2 * at] < 0 || span[2 * at] >= span[2 * at + 1] || span[2 * at + 1] > cl[n]) return fail("a span outside its word", round);
        }
    }
    ++checked;
  }
  printf("rounds %d checked %d\n", rounds, checked);
  return checked == rounds ? 0 : 1;
}
