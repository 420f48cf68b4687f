// page_skew.h — the per-word arithmetic of the page-skew estimate and of the deskewed ordering boxes (Pipeline.deskew; DESIGN.md
// section 4.19), written once for reading_order_kernel<.., DESKEW = true> and its host twins msocr_page_skew_host /
// msocr_deskew_boxes_host.  Integer arithmetic, or correctly rounded f64 in one written order (compile with -ffp-contract=off); no
// transcendental function.  The sums over a page are int64 and therefore exact in any order.
#pragma once
#include "word_boxes.h"

constexpr long long SKEW_QMAX = 1LL << 23;  // qx below this: with at most 16384 words every product of a sum and a word stays below 2^61
constexpr int SKEW_MIN_WORDS = 8;           // a placeholder, not a tuned value (no trained checkpoint to tune on)

// The direction of one word in 1/16 px of its mean horizontal edge: d = (P1 - P0) + (P2 - P3) of the canonical corners, quantised
// as (int64)rint(8 d).  False when the word does not vote: a non-finite corner, a quad that is not strictly convex, a direction
// outside (0, 2^23) x [-qx, qx], or a word that is taller than wide (r = (P3 - P0) + (P2 - P1) longer than d: a single letter or
// vertical marginalia, which the canonical order presents by the short side).
WB_HD bool skew_word(const float* q, long long* qx, long long* qy) {
  float c[8];
  if (!quad_canonical(q, c)) return false;
  const double x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5], x3 = c[6], y3 = c[7];
  const double dx = (x1 - x0) + (x2 - x3), dy = (y1 - y0) + (y2 - y3);
  const double rx = (x3 - x0) + (x2 - x1), ry = (y3 - y0) + (y2 - y1);
  const double a = rint(8.0 * dx), b = rint(8.0 * dy), e = rint(8.0 * rx), f = rint(8.0 * ry);
  // beyond 2^24 nothing can pass (px^2 <= qx^2 + qy^2 < 2^47), and the doubles are not converted unchecked
  const double lim = 16777216.0;
  if (!(fabs(a) < lim && fabs(b) < lim && fabs(e) < lim && fabs(f) < lim)) return false;
  const long long x = (long long)a, y = (long long)b, px = (long long)e, py = (long long)f;
  if (!(x > 0 && x < SKEW_QMAX) || (y < 0 ? -y : y) > x) return false;
  if (x * x + y * y < px * px + py * py) return false;
  *qx = x;
  *qy = y;
  return true;
}

// Second pass: the word lies within atan(1/4) = 14 degrees of the first estimate S1 (a placeholder, not a tuned value):
// 4 |S1 x q| <= S1 . q, written without the factor 4 on the left so that nothing leaves int64 (the cross product is >= 0 and the
// quotient truncates toward zero, which equals the floor wherever the test can hold).
WB_HD bool skew_near(long long s1x, long long s1y, long long qx, long long qy) {
  const long long cr = s1x * qy - s1y * qx, dot = s1x * qx + s1y * qy;
  return dot >= 0 && (cr < 0 ? -cr : cr) <= dot / 4;
}

// The rotation is applied: enough words, a direction within 45 degrees, and outside the dead zone of atan(1/256) = 0.22 degrees
// that keeps an upright page's order as it is.
WB_HD bool skew_applied(long long s2x, long long s2y, long long m) {
  const long long ay = s2y < 0 ? -s2y : s2y;
  return m >= SKEW_MIN_WORDS && s2x > 0 && ay <= s2x && 256 * ay > s2x;
}

// cs = {c, s} of the rotation by -atan2(S2y, S2x); the identity {1, 0} when it is not applied.
WB_HD void skew_cos_sin(long long s2x, long long s2y, bool applied, double* cs) {
  cs[0] = 1.0;
  cs[1] = 0.0;
  if (!applied) return;
  const double nrm = sqrt((double)s2x * (double)s2x + (double)s2y * (double)s2y);
  cs[0] = (double)s2x / nrm;
  cs[1] = (double)s2y / nrm;
}

WB_HD int floor_i32(double v) {  // floor, clipped to int32 (a NaN gives the lower end)
  const double f = floor(v);
  return f >= 2147483647.0 ? 2147483647 : (f >= -2147483648.0 ? (int)f : (-2147483647 - 1));
}

// The ordering box of a word: its corners rotated about the page centre, floor of the extremes.  A word with a non-finite corner,
// and every word of a page whose rotation is not applied, keeps box_from_quad's box (floor and truncation differ below zero, so the
// identity is not sent through the formula).
WB_HD Box4 deskew_box(const float* q, bool applied, double c, double s, int page_h, int page_w) {
  bool finite = true;
  for (int k = 0; k < 8; ++k) finite = finite && finite_f32(q[k]);
  if (!applied || !finite) return box_from_quad(q);
  const double hx = 0.5 * (double)page_w, hy = 0.5 * (double)page_h;
  double xa = 0.0, xb = 0.0, ya = 0.0, yb = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double u = (double)q[2 * k] - hx, v = (double)q[2 * k + 1] - hy;
    const double x = (c * u + s * v) + hx, y = (c * v - s * u) + hy;
    xa = (k == 0 || x < xa) ? x : xa; xb = (k == 0 || x > xb) ? x : xb;
    ya = (k == 0 || y < ya) ? y : ya; yb = (k == 0 || y > yb) ? y : yb;
  }
  return Box4{floor_i32(xa), floor_i32(ya), floor_i32(xb), floor_i32(yb)};
}
