// word_spotting_fuzz.cpp — drives csrc/word_spotting.h (the frame rule and the order of its f32 sum, the f64 table of the distance, the
// length gate, the ordering key and the selection, with the checks every entry point makes before them) over garbage lengths and
// non-finite features under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its exact size,
// so a read or write one element outside it is a report.  Lengths are garbage on the way into the checks and into the normalisation
// (which clamps them); the distance runs only on what its check admits, as the entry point does.  Every distance is compared with a
// plain full table, every selection with a plain stable sort.  usage: word_spotting_fuzz [rounds]; prints "rounds <n> checked <n>"
// and exits 0, or 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "word_spotting.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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

// the definition over a full table
static float plain_dtw(const float* a, int La, const float* b, int Lb, int H) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> D((size_t)La * Lb, inf);
  for (int i = 0; i < La; ++i)
    for (int j = 0; j < Lb; ++j) {
      double dot = 0.0;
      for (int k = 0; k < H; ++k) dot += (double)a[(size_t)i * H + k] * (double)b[(size_t)j * H + k];
      double best = inf;
      if (i == 0 && j == 0) best = 0.0;
      if (i && j) best = std::min(best, D[(size_t)(i - 1) * Lb + j - 1]);
      if (i) best = std::min(best, D[(size_t)(i - 1) * Lb + j]);
      if (j) best = std::min(best, D[(size_t)i * Lb + j - 1]);
      D[(size_t)i * Lb + j] = (1.0 - dot) + best;
    }
  return (float)(D[(size_t)La * Lb - 1] / (double)(La + Lb));
}

static bool same_float(float x, float y) { return memcmp(&x, &y, 4) == 0; }

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 100;
  int checked = 0;
  for (int round = 0; round < rounds; ++round) {
    // ---- shapes: the check admits exactly the envelope
    {
      const int T = rnd_in(-1, 66), H = 32 * rnd_in(-1, 18);
      const int64_t n = rnd() % 4 ? rnd_in(-2, 40) : ((int64_t)rnd() << 8);
      const bool want = n >= 0 && T >= 1 && T <= 64 && H >= 64 && H <= 512 && H % 64 == 0 && n * T * H < ((int64_t)1 << 31);
      if (ws_shape_ok(n, T, H) != want) return fail("ws_shape_ok", round);
    }
    const int T = rnd_in(1, round % 10 == 0 ? 64 : 12), H = 64 * rnd_in(1, round % 7 == 0 ? 8 : 2);
    const int Q = rnd_in(0, 4), N = rnd_in(0, 9);
    // ---- normalisation: garbage lengths, garbage features, exact-size blocks
    auto qf = block<float>((size_t)Q * T * H), cf = block<float>((size_t)N * T * H);
    auto qu = block<float>((size_t)Q * T * H), cu = block<float>((size_t)N * T * H);
    auto ql = block<int32_t>(Q), cl = block<int32_t>(N), lo = block<int32_t>(Q), hi = block<int32_t>(Q);
    const bool dirty = round % 3 == 0;
    for (size_t i = 0; i < (size_t)Q * T * H; ++i) qf[i] = dirty ? garbage_float() : rnd_unit();
    for (size_t i = 0; i < (size_t)N * T * H; ++i) cf[i] = dirty ? garbage_float() : rnd_unit();
    for (int q = 0; q < Q; ++q) ql[q] = round % 4 == 0 ? garbage_len(T) : rnd_in(1, T);
    for (int n = 0; n < N; ++n) cl[n] = round % 4 == 0 ? garbage_len(T) : rnd_in(1, T);
    for (int q = 0; q < Q; ++q) {
      lo[q] = round % 5 == 0 ? garbage_len(T) : rnd_in(1, T);
      hi[q] = round % 5 == 0 ? garbage_len(T) : rnd_in(lo[q], T);
    }
    ws_normalize_host(qf.get(), ql.get(), Q, T, H, qu.get());
    ws_normalize_host(cf.get(), cl.get(), N, T, H, cu.get());
    for (int side = 0; side < 2; ++side) {
      const int cnt = side ? N : Q;
      const float *f = side ? cf.get() : qf.get(), *u = side ? cu.get() : qu.get();
      const int32_t* len = side ? cl.get() : ql.get();
      for (int n = 0; n < cnt; ++n)
        for (int t = 0; t < T; ++t) {
          const float *x = f + ((size_t)n * T + t) * H, *y = u + ((size_t)n * T + t) * H;
          double ss = 0.0, uu = 0.0;
          bool fin = true;
          for (int e = 0; e < H; ++e) {
            ss += (double)x[e] * x[e];
            uu += (double)y[e] * y[e];
            fin = fin && std::isfinite(x[e]);
            if (!std::isfinite(y[e])) return fail("a non-finite unit element", round);
          }
          const int L = len[n] < 0 ? 0 : len[n] > T ? T : len[n];
          if (t >= L || !fin || ss < 0.5 * FLT_MIN || ss > 2.0 * FLT_MAX) {  // clearly no direction: the zero frame
            if (uu != 0.0) return fail("a frame that must be zero", round);
          } else if (ss > 2.0 * FLT_MIN && ss < 0.5 * FLT_MAX) {            // clearly one: unit length
            if (std::fabs(std::sqrt(uu) - 1.0) > (H + 4) * 0x1p-24) return fail("a unit frame's length", round);
          }
        }
    }
    // ---- the distance, where the entry point's check admits the lengths
    bool ok = ws_lens_ok(ql.get(), Q, T) && ws_lens_ok(cl.get(), N, T);
    for (int q = 0; q < Q; ++q) ok = ok && lo[q] <= hi[q];
    auto dist = block<float>((size_t)Q * N);
    if (ok) {
      ws_dtw_host(qu.get(), ql.get(), lo.get(), hi.get(), Q, cu.get(), cl.get(), N, T, H, dist.get());
      for (int q = 0; q < Q; ++q)
        for (int n = 0; n < N; ++n) {
          const float got = dist[(size_t)q * N + n];
          if (cl[n] < lo[q] || cl[n] > hi[q]) {
            if (!(got == std::numeric_limits<float>::infinity())) return fail("the gate", round);
            continue;
          }
          const float want = plain_dtw(qu.get() + (size_t)q * T * H, ql[q], cu.get() + (size_t)n * T * H, cl[n], H);
          if (!same_float(got, want)) return fail("a distance", round);
          if (!std::isfinite(got)) return fail("a non-finite distance of unit frames", round);
        }
    } else {
      for (size_t i = 0; i < (size_t)Q * N; ++i) dist[i] = garbage_float();
    }
    // ---- the selection on what the distance left, and on garbage
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1)
        for (size_t i = 0; i < (size_t)Q * N; ++i) dist[i] = rnd() % 3 ? (float)(int)(rnd() % 5) - 2.f : garbage_float();
      const int k = rnd() % 3 ? rnd_in(1, 12) : rnd_in(200, 256);
      auto idx = block<int32_t>((size_t)Q * k);
      auto val = block<float>((size_t)Q * k);
      ws_topk_host(dist.get(), Q, N, k, idx.get(), val.get());
      for (int q = 0; q < Q; ++q) {
        const float* row = dist.get() + (size_t)q * N;
        std::vector<int> order;
        for (int i = 0; i < N; ++i)
          if (std::isfinite(row[i])) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return row[a] < row[b]; });
        for (int s = 0; s < k; ++s) {
          const int32_t gi = idx[(size_t)q * k + s];
          const float gv = val[(size_t)q * k + s];
          if ((size_t)s < order.size()) {
            if (gi != order[s] || !same_float(gv, row[order[s]])) return fail("a selected entry", round);
          } else if (gi != -1 || !(gv == std::numeric_limits<float>::infinity())) {
            return fail("an unused slot", round);
          }
        }
      }
    }
    ++checked;
  }
  printf("rounds %d checked %d\n", rounds, checked);
  return checked == rounds ? 0 : 1;
}
