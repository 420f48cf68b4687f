// quad_match_fuzz.cpp — drives csrc/quad_iou.h (the geometry of the quad-matching kernels and the whole host twin) over garbage
// coordinates and counts at the bounds under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of its
// exact size, so a read or write one element outside it is a report.  The results are checked for what must hold whatever the
// input: match indices inside the page's ground truth, a ground truth taken at most once per threshold, tp + fp = n_pred,
// fn = n_gt - tp, no NaN and no negative IoU, entries behind n_pred untouched, and the clip functions agreeing with each other.
// usage: quad_match_fuzz [rounds]; prints "rounds <n> checked <quads>" and exits 0, or 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "quad_iou.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }  // inclusive
static float unit() { return (float)(rnd() % 100001) / 100000.0f; }
static float garbage() {
  switch (rnd() % 10) {
    case 0: return std::numeric_limits<float>::quiet_NaN();
    case 1: return std::numeric_limits<float>::infinity();
    case 2: return -std::numeric_limits<float>::infinity();
    case 3: return std::numeric_limits<float>::max();
    case 4: return -std::numeric_limits<float>::max();
    case 5: return std::numeric_limits<float>::denorm_min();
    case 6: return 0.0f;
    case 7: {  // any bit pattern
      const uint32_t b = rnd() ^ (rnd() << 16);
      float f;
      memcpy(&f, &b, 4);
      return f;
    }
    default: return (unit() - 0.5f) * 1e4f;
  }
}
// a word-like quad on a small page, so that quads overlap, or eight garbage values
static void fill_quad(float* q, bool wild) {
  if (wild) {
    for (int k = 0; k < 8; ++k) q[k] = rnd() % 3 ? garbage() : unit() * 300.0f;
    return;
  }
  const float cx = unit() * 300.0f, cy = unit() * 200.0f, w = 5.0f + unit() * 80.0f, h = 5.0f + unit() * 30.0f;
  const float a = (unit() - 0.5f) * 1.0f, c = cosf(a), s = sinf(a);
  const float dx[4] = {-w / 2, w / 2, w / 2, -w / 2}, dy[4] = {-h / 2, -h / 2, h / 2, h / 2};
  const bool flip = rnd() % 2;
  for (int k = 0; k < 4; ++k) {
    const int v = flip ? (4 - k) & 3 : k;
    q[2 * k] = cx + c * dx[v] - s * dy[v] + (unit() - 0.5f) * 2.0f;
    q[2 * k + 1] = cy + s * dx[v] + c * dy[v] + (unit() - 0.5f) * 2.0f;
  }
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 200;
  long checked = 0;
  for (int it = 0; it < rounds; ++it) {
    // ---- the geometry alone, on quads that need not be valid
    for (int r = 0; r < 50; ++r) {
      std::unique_ptr<float[]> qa(new float[8]), qb(new float[8]);
      fill_quad(qa.get(), rnd() % 2);
      fill_quad(qb.get(), rnd() % 2);
      std::unique_ptr<double[]> va(new double[8]), vb(new double[8]);
      const bool oka = qi_canonical(qa.get(), va.get()), okb = qi_canonical(qb.get(), vb.get());
      for (int k = 0; k < 8; ++k) {  // the plain conversion stands in for garbage that is not finite: the clip must stay in bounds
        if (!(fabs(va[k]) <= 1e300)) va[k] = 1e300;
        if (!(fabs(vb[k]) <= 1e300)) vb[k] = -1e300;
      }
      const double g = qi_polygon_iou_general(va.get(), vb.get());
      double f = 0.0;
      const bool fits = qi_polygon_iou_fast(va.get(), vb.get(), &f);
      if (fits && !(f != f && g != g) && memcmp(&f, &g, 8) != 0) FAIL("register clip %.17g, general clip %.17g", f, g);
      if (oka && okb) {
        const QiBox ba = qi_box(va.get()), bb = qi_box(vb.get());
        const double v = qi_iou(va.get(), ba, vb.get(), bb);
        if (memcmp(&v, &g, 8) != 0) FAIL("qi_iou %.17g, general clip %.17g", v, g);
        if (!(v >= 0.0)) FAIL("IoU %.17g of two valid quads", v);
      }
      ++checked;
    }
    // ---- the host twin: counts at the bounds, arrays of exact size
    const int N = rnd_in(0, 3), T = rnd() % 4 ? rnd_in(1, 4) : MSOCR_QM_MAX_T;
    const int max_pred = rnd() % 8 ? rnd_in(0, 40) : 0, max_gt = rnd() % 8 ? rnd_in(0, 40) : 0;
    std::unique_ptr<int32_t[]> n_pred(new int32_t[N]), n_gt(new int32_t[N]);
    for (int p = 0; p < N; ++p) {
      n_pred[p] = rnd() % 3 ? rnd_in(0, max_pred) : (rnd() % 2 ? max_pred : 0);
      n_gt[p] = rnd() % 3 ? rnd_in(0, max_gt) : (rnd() % 2 ? max_gt : 0);
    }
    const size_t np_all = (size_t)N * max_pred, ng_all = (size_t)N * max_gt;
    std::unique_ptr<float[]> pred(new float[np_all * 8]), gt(new float[ng_all * 8]);
    const bool wild = rnd() % 2;
    for (size_t i = 0; i < np_all; ++i) fill_quad(pred.get() + 8 * i, wild && rnd() % 3 == 0);
    for (size_t i = 0; i < ng_all; ++i) fill_quad(gt.get() + 8 * i, wild && rnd() % 3 == 0);
    std::unique_ptr<double[]> th(new double[T]);
    for (int t = 0; t < T; ++t) th[t] = t == 0 ? 1.0 : 0.05 + 0.9 * unit();
    if (!qm_shape_ok(N, max_pred, max_gt, th.get(), T)) FAIL("a shape inside the envelope was refused");
    if (qm_shape_ok(N, MSOCR_QM_MAX_QUADS + 1, max_gt, th.get(), T) || qm_shape_ok(N, max_pred, max_gt, th.get(), 0) ||
        qm_shape_ok(N, max_pred, max_gt, th.get(), MSOCR_QM_MAX_T + 1) || qm_shape_ok(N, max_pred, max_gt, nullptr, T))
      FAIL("a shape outside the envelope was accepted");
    const size_t rows = (size_t)N * T * max_pred;
    std::unique_ptr<int32_t[]> match(new int32_t[rows]), counts(new int32_t[(size_t)N * T * 3]);
    std::unique_ptr<double[]> iou(new double[rows]);
    for (size_t i = 0; i < rows; ++i) {
      match[i] = -77;
      iou[i] = -77.0;
    }
    qm_match_host(pred.get(), n_pred.get(), max_pred, gt.get(), n_gt.get(), max_gt, N, th.get(), T, match.get(), iou.get(), counts.get());
    for (int p = 0; p < N; ++p)
      for (int t = 0; t < T; ++t) {
        const int32_t* m = match.get() + ((size_t)p * T + t) * max_pred;
        const double* v = iou.get() + ((size_t)p * T + t) * max_pred;
        const int32_t* c = counts.get() + ((size_t)p * T + t) * 3;
        std::vector<int> taken(n_gt[p], 0);
        int tp = 0, fp = 0;
        for (int i = 0; i < max_pred; ++i) {
          if (i >= n_pred[p]) {
            if (m[i] != -77 || v[i] != -77.0) FAIL("an entry behind n_pred was written");
            continue;
          }
          if (m[i] < -2 || m[i] >= n_gt[p]) FAIL("match %d outside the page's %d ground truths", m[i], n_gt[p]);
          if (!(v[i] >= 0.0)) FAIL("IoU %.17g", v[i]);
          if (m[i] >= 0) {
            if (taken[m[i]]++) FAIL("ground truth %d taken twice", m[i]);
            if (!(v[i] >= th[t])) FAIL("a match below its threshold");
            ++tp;
          } else {
            if (m[i] == -1 && v[i] >= th[t]) FAIL("a false positive at or above its threshold");
            ++fp;
          }
        }
        if (c[0] != tp || c[1] != fp || c[2] != n_gt[p] - tp) FAIL("counts %d %d %d, counted %d %d of %d", c[0], c[1], c[2], tp, fp, n_gt[p]);
        checked += n_pred[p];
      }
  }
  printf("rounds %d checked %ld\n", rounds, checked);
  return 0;
}
