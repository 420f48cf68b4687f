// word_boxes.h — the integer word boxes of the Pipeline glue and the recogniser canvas fit, written once for the kernels and
// their host twins (reading_order_kernel, msocr_reading_order_host, quad_descriptor), and the canonical corner order of a stored
// quad, which the rectified crops (quad_crop.hip) and the page-skew estimate (page_skew.h) share.  Integer or correctly rounded f64
// arithmetic in one written order (compile with -ffp-contract=off), so host and device give the same values.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#define WB_HD __host__ __device__ __forceinline__

struct Box4 { int x0, y0, x1, y1; };

WB_HD bool box_hit(const Box4& a, const Box4& b) {  // utils.py:515-523
  return !(a.x1 <= b.x0 || b.x1 <= a.x0 || a.y1 <= b.y0 || b.y1 <= a.y0);
}
WB_HD bool box_same(const Box4& a, const Box4& b) { return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1; }
// int(hi - (hi - lo) * 0.1): f64, truncation toward zero (utils.py:525-528).  hi - lo is formed in 64 bits: the same value for
// every box a kernel sees (decode drops |x| >= 1e7), and defined for any int32 pair; the result lies between lo and hi.
WB_HD int box_shrink(int lo, int hi) { return (int)((double)hi - (double)((long long)hi - (long long)lo) * 0.1); }
WB_HD void box_shrink(Box4& b) { b.x1 = box_shrink(b.x0, b.x1); b.y1 = box_shrink(b.y0, b.y1); }  // 10 % towards the top-left

// Word AABB of a stored quad q[8]: np.array(polygon, dtype=np.int32) truncates toward zero, then min / max over the 4 points
// (_pipeline.py:106-109).  Coordinates must convert to int32 (decode keeps them below 1e7).
WB_HD Box4 box_from_quad(const float* q) {
  Box4 b{(int)q[0], (int)q[1], (int)q[0], (int)q[1]};
  for (int k = 1; k < 4; ++k) {
    const int x = (int)q[2 * k], y = (int)q[2 * k + 1];
    b.x0 = x < b.x0 ? x : b.x0; b.x1 = x > b.x1 ? x : b.x1;
    b.y0 = y < b.y0 ? y : b.y0; b.y1 = y > b.y1 ? y : b.y1;
  }
  return b;
}

// Crop window win = {x1, y1, x2, y2} of image[y1:y2, x1:x2] (_pipeline.py:204-221): clamped to the page, a negative stop counted
// from the end as a Python slice does.  False when the word is under min_text on a side (_pipeline.py:110) or the window is empty.
WB_HD bool box_crop_window(const Box4& bx, int page_h, int page_w, int min_text, int* win) {
  if ((long long)bx.x1 - bx.x0 < min_text || (long long)bx.y1 - bx.y0 < min_text) return false;
  int c = bx.x1 < page_w ? bx.x1 : page_w, d = bx.y1 < page_h ? bx.y1 : page_h;
  if (c < 0) c = page_w + c > 0 ? page_w + c : 0;
  if (d < 0) d = page_h + d > 0 ? page_h + d : 0;
  win[0] = bx.x0 > 0 ? bx.x0 : 0; win[1] = bx.y0 > 0 ? bx.y0 : 0; win[2] = c; win[3] = d;
  return c > win[0] && d > win[1];
}

WB_HD int rint_clip(double v, int hi) {  // max(1, rint(v)) clipped to hi, without converting an out-of-range double
  const double r = rint(v);
  return r >= (double)hi ? hi : (r >= 1.0 ? (int)r : 1);
}

// ResizeAndPadA's size arithmetic (transforms.py:91-95,114-117; Python round = rint) for a w x h region, w, h >= 1, on an
// img_h x img_w canvas.  The reference writes max(1, int(round(w * scale))) with no upper clip; the clip of rint_clip never
// binds: scale = min(img_h / h, img_w / w) <= (img_w / w)(1 + 2^-53), so w * scale <= img_w (1 + 2^-53)^2, whose rint is at
// most img_w (and likewise for h), so both forms give the same integers, here without ever converting an unchecked double.
struct CanvasFit { int new_w, new_h, y0; };
WB_HD CanvasFit canvas_fit(double w, double h, int img_h, int img_w) {
  const double sh = (double)img_h / h, sw = (double)img_w / w, scale = sh < sw ? sh : sw;
  CanvasFit f{rint_clip(w * scale, img_w), rint_clip(h * scale, img_h), 0};
  const int t = (img_h - f.new_h) / 2, room = img_h - f.new_h;  // floor division: new_h <= img_h
  f.y0 = t < room ? t : room;  // max(0, min(t, room))
  f.y0 = f.y0 > 0 ? f.y0 : 0;
  return f;
}

// ---- stored quads: bit patterns, finiteness and the canonical corner order (quad_crop.hip, page_skew.h)
WB_HD float bits_f32(int32_t v) {
  float f;
  memcpy(&f, &v, 4);
  return f;
}
WB_HD int32_t f32_bits(float f) {
  int32_t v;
  memcpy(&v, &f, 4);
  return v;
}
WB_HD bool finite_f32(float f) { return (f32_bits(f) & 0x7f800000) != 0x7f800000; }

// Canonical corner order of the quad q[8] (x, y pairs as stored) -> c[8]; false when the quad is not usable (a non-finite corner,
// a zero edge cross product, or cross products of both signs).
WB_HD bool quad_canonical(const float* q, float* c) {
  for (int k = 0; k < 8; ++k)
    if (!finite_f32(q[k])) return false;
  int pos = 0, neg = 0;
  for (int i = 0; i < 4; ++i) {  // cross product of the edges P[i] -> P[i+1] and P[i+1] -> P[i+2]
    const int j = (i + 1) & 3, k = (i + 2) & 3;
    const double ax = (double)q[2 * j] - (double)q[2 * i], ay = (double)q[2 * j + 1] - (double)q[2 * i + 1];
    const double bx = (double)q[2 * k] - (double)q[2 * j], by = (double)q[2 * k + 1] - (double)q[2 * j + 1];
    const double cr = ax * by - ay * bx;
    pos += cr > 0.0 ? 1 : 0;
    neg += cr < 0.0 ? 1 : 0;
  }
  if (pos != 4 && neg != 4) return false;
  // y points down: positive cross products = clockwise on screen; otherwise walk the stored corners backwards (3, 2, 1, 0)
  int idx[4];
  for (int k = 0; k < 4; ++k) idx[k] = pos == 4 ? k : 3 - k;
  // the rotation whose first edge has the largest x1 - x0; on equality the start corner with the smallest stored index
  int best = 0;
  double best_dx = 0.0;
  for (int r = 0; r < 4; ++r) {
    const double dx = (double)q[2 * idx[(r + 1) & 3]] - (double)q[2 * idx[r]];
    if (r == 0 || dx > best_dx || (dx == best_dx && idx[r] < idx[best])) {
      best = r;
      best_dx = dx;
    }
  }
  for (int k = 0; k < 4; ++k) {
    c[2 * k] = q[2 * idx[(best + k) & 3]];
    c[2 * k + 1] = q[2 * idx[(best + k) & 3] + 1];
  }
  return true;
}
