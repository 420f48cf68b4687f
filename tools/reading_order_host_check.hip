// dev: stand-alone sanitizer run of the reading-order host twin and of the host form of the box / fit helpers (CPU only).
//
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/reading_order_host_check.hip -o /tmp/reading_order_host_check && /tmp/reading_order_host_check
//
// Random pages plus hostile ones: duplicates, zero and negative extents, nested cliques that never stop intersecting (all 50
// sweeps), coordinates at +-(2^31 - 1).  Prints "ok" and returns 0 when every order is a list of valid word indices, the text lines
// of msocr_reading_lines_host tile that order with the right boxes, and the helpers agree with their plain restatements; a
// sanitizer report aborts the run.
#include <stdio.h>

#include <random>
#include <vector>

#include "../manuscript_ocr_amd/csrc/host_glue.hip"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const int32_t BIG_ = 2147483647;

static void run_page(const std::vector<int32_t>& b, double tol, double gap) {
  const int n = (int)b.size() / 4;
  std::vector<int32_t> order(n, -1);
  EXPECT(msocr_reading_order_host(b.data(), n, tol, gap, order.data()) == MSOCR_OK);
  for (int v : order) EXPECT(v >= 0 && v < n);
  // the same page through msocr_reading_lines_host: the same order, line indices that start at 0 and step by 0 or 1, records
  // whose spans tile [0, n) and whose boxes are the unions of the words at their positions; one guard word behind every output
  const int32_t G = -777;
  std::vector<int32_t> order2(n + 1, G), line(n + 1, G), recs(6 * (size_t)n + 1, G);
  int32_t nlines = G;
  EXPECT(msocr_reading_lines_host(b.data(), n, tol, gap, order2.data(), line.data(), recs.data(), &nlines) == MSOCR_OK);
  EXPECT(order2[n] == G && line[n] == G && recs[6 * (size_t)n] == G);
  EXPECT(nlines >= (n > 0 ? 1 : 0) && nlines <= n);
  int pos = 0;
  for (int l = 0; l < nlines && l < n; ++l) {
    const int32_t* r = &recs[6 * (size_t)l];
    EXPECT(r[0] == pos && r[1] >= 1 && r[0] + (long long)r[1] <= n);
    if (r[0] != pos || r[1] < 1 || r[0] + (long long)r[1] > n) break;
    int32_t u[4] = {BIG_, BIG_, -BIG_, -BIG_};
    for (int k = 0; k < r[1]; ++k, ++pos) {
      EXPECT(order2[pos] == order[pos] && line[pos] == l);
      const int32_t* w = &b[4 * (size_t)order[pos]];
      u[0] = std::min(u[0], w[0]); u[1] = std::min(u[1], w[1]); u[2] = std::max(u[2], w[2]); u[3] = std::max(u[3], w[3]);
    }
    EXPECT(r[2] == u[0] && r[3] == u[1] && r[4] == u[2] && r[5] == u[3]);
  }
  EXPECT(pos == n);
  for (size_t k = 6 * (size_t)std::max(nlines, 0); k < 6 * (size_t)n; ++k) EXPECT(recs[k] == G);  // rows past the line count
}

int main() {
  const int32_t BIG = BIG_;
  {  // no boxes: no lines, nothing else touched or needed
    int32_t nlines = -5;
    EXPECT(msocr_reading_lines_host(nullptr, 0, 0.6, INFINITY, nullptr, nullptr, nullptr, &nlines) == MSOCR_OK && nlines == 0);
    EXPECT(msocr_reading_lines_host(nullptr, 0, 0.6, INFINITY, nullptr, nullptr, nullptr, nullptr) == MSOCR_E_ARG);
    run_page({}, 0.6, INFINITY);
  }
  std::mt19937 rng(20260101);
  auto uni = [&](int lo, int hi) { return (int32_t)std::uniform_int_distribution<int>(lo, hi)(rng); };
  for (int rep = 0; rep < 40; ++rep) {  // random pages, some words doubled
    const int n = uni(1, 300);
    std::vector<int32_t> b;
    for (int i = 0; i < n; ++i) {
      const int x = uni(-20, 2000), y = uni(-20, 1500);
      const int32_t box[4] = {x, y, x + uni(0, 120), y + uni(0, 40)};
      for (int k = 0; k < (i % 7 == 3 ? 2 : 1); ++k) b.insert(b.end(), box, box + 4);
    }
    run_page(b, 0.6, rep % 2 ? 1.5 : INFINITY);
  }
  {  // zero and negative extents, duplicates of them
    std::vector<int32_t> b = {5, 5, 5, 5, 5, 5, 5, 5, 10, 10, 2, 3, 10, 10, 2, 3, 0, 0, 0, 9, 7, 7, -7, -7, 1, 1, 30, 30};
    run_page(b, 0.6, INFINITY);
    run_page(b, 0.0, 0.0);
  }
  {  // a nested clique left of / above the origin: truncation toward zero undoes the shrink, so all 50 sweeps find every pair
    std::vector<int32_t> b;
    for (int i = 0; i < 60; ++i) { const int32_t box[4] = {-40 - i, -30 - i, -3, -2}; b.insert(b.end(), box, box + 4); }
    run_page(b, 0.6, INFINITY);
    b.clear();  // and one that shrinks to nothing
    for (int i = 0; i < 60; ++i) { const int32_t box[4] = {0, 0, 1000000 + i, 900000 - i}; b.insert(b.end(), box, box + 4); }
    run_page(b, 0.6, INFINITY);
  }
  {  // coordinates at the ends of int32, in every combination over a few boxes
    const int32_t ends[4] = {-BIG, BIG, 0, -1};
    std::vector<int32_t> b;
    for (int m = 0; m < 256; ++m) { const int32_t box[4] = {ends[m & 3], ends[(m >> 2) & 3], ends[(m >> 4) & 3], ends[(m >> 6) & 3]}; b.insert(b.end(), box, box + 4); }
    run_page(b, 0.6, INFINITY);
    run_page(b, 1e300, -1e300);
    for (int m = 0; m < 256; ++m) {
      const Box4 x{b[4 * m], b[4 * m + 1], b[4 * m + 2], b[4 * m + 3]};
      int win[4] = {0, 0, 0, 0};
      const bool keep = box_crop_window(x, 1536, 2048, 5, win);
      if (keep) EXPECT(win[0] >= 0 && win[1] >= 0 && win[2] <= 2048 && win[3] <= 1536 && win[2] > win[0] && win[3] > win[1]);
      Box4 s = x;
      box_shrink(s);
      EXPECT(s.x0 == x.x0 && s.y0 == x.y0);
      EXPECT(x.x0 <= x.x1 ? (s.x1 >= x.x0 && s.x1 <= x.x1) : (s.x1 <= x.x0 && s.x1 >= x.x1));
      EXPECT(box_same(x, x) && box_hit(x, x) == (x.x1 > x.x0 && x.y1 > x.y0));
    }
  }
  {  // the helpers against their plain restatements
    const float q[8] = {10.9f, -3.7f, 99.2f, -0.4f, 98.5f, 20.99f, 9.1f, 21.5f};
    const Box4 a = box_from_quad(q);
    EXPECT(a.x0 == 9 && a.y0 == -3 && a.x1 == 99 && a.y1 == 21);
    EXPECT(box_shrink(0, 100) == 90 && box_shrink(-10, -3) == -3 && box_shrink(3, 12) == 11);
    int win[4];
    EXPECT(box_crop_window(Box4{-4, -6, 30, 20}, 100, 200, 5, win) && win[0] == 0 && win[1] == 0 && win[2] == 30 && win[3] == 20);
    EXPECT(!box_crop_window(Box4{0, 0, 4, 20}, 100, 200, 5, win));
    EXPECT(box_crop_window(Box4{-90, 0, -10, 20}, 100, 200, 5, win) && win[2] == 190);  // negative stop: from the end
    const int canvases[3][2] = {{32, 100}, {32, 128}, {64, 256}};
    for (const auto& c : canvases)
      for (int w = 1; w <= 2200; w += (w < 300 ? 1 : 37))
        for (int h = 1; h <= 1700; h += (h < 200 ? 1 : 41)) {
          const CanvasFit f = canvas_fit((double)w, (double)h, c[0], c[1]);
          const double scale = fmin((double)c[0] / h, (double)c[1] / w);  // the unguarded form of the AABB path
          const int nw = std::max(1, (int)rint(w * scale)), nh = std::max(1, (int)rint(h * scale));
          EXPECT(f.new_w == nw && f.new_h == nh && f.y0 == std::max(0, std::min((c[0] - nh) / 2, c[0] - nh)));
          EXPECT(nw <= c[1] && nh <= c[0]);
        }
    const CanvasFit huge = canvas_fit(1e300, 1.0, 32, 100), tiny = canvas_fit(1.0, 1e300, 32, 100);
    EXPECT(huge.new_w == 100 && huge.new_h == 1 && tiny.new_w == 1 && tiny.new_h == 32);
  }
  if (fails == 0) printf("ok\n");
  return fails ? 1 : 0;
}
