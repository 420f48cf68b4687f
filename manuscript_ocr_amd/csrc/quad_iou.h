// quad_iou.h — the geometry and the matching rule of msocr_quad_match (include/msocr.h, "detection quality"): which quads are valid,
// how a valid quad is wound, the fp64 IoU of two quads, and the greedy one-to-one matching of a page's predictions to its ground
// truth.  Host and device: the kernels of quad_match.hip call the geometry, msocr_quad_match_host is qm_match_host below, and a plain
// C++ program drives both over garbage coordinates under the address and undefined-behaviour sanitizers
// (tests/native/quad_match_fuzz.cpp).
//
// The IoU performs the operations of the reference's lanms.py:7-91 (polygon_area, compute_intersection, clip_polygon,
// polygon_intersection, polygon_iou) in their written order on f64 values; built with -ffp-contract=off it returns the reference's
// value bit for bit.  east_post.hip keeps its own copy of the same code for LANMS.
#ifndef MSOCR_QUAD_IOU_H
#define MSOCR_QUAD_IOU_H
#include <math.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MSOCR_QI_HD __host__ __device__ __forceinline__
#define MSOCR_QI_HD_NOINLINE __host__ __device__ __noinline__
#else
#define MSOCR_QI_HD inline
#define MSOCR_QI_HD_NOINLINE inline
#endif

#define MSOCR_QM_MAX_QUADS 16384  // quads of one page on either side (the box tail's bound per page)
#define MSOCR_QM_MAX_T 16         // thresholds of one call
#define MSOCR_QI_MAXV 20          // lanms.py:34, the clip buffer of the general path

// ---- validity and winding ------------------------------------------------------------------------------------------------------
// q [4][2] f32 -> v [8] f64, the quad as the IoU reads it.  Valid: all eight coordinates finite and the four turn cross products
// (v[i+1]-v[i]) x (v[i+2]-v[i+1]) all > 0 or all < 0 (strictly convex).  A valid quad with negative turns is stored as
// [v0, v3, v2, v1], so that every valid quad comes out with positive turns: polygon_iou takes the left of the clip polygon's edges
// as inside.  Returns false (v then holds the plain conversion) for an invalid quad.
MSOCR_QI_HD bool qi_canonical(const float* q, double* v) {
  bool finite = true;
  for (int k = 0; k < 8; ++k) {
    v[k] = (double)q[k];
    finite = finite && (fabs(v[k]) <= 3.4028234663852886e38);  // false for NaN and for +-inf
  }
  if (!finite) return false;
  int pos = 0, neg = 0;
  for (int i = 0; i < 4; ++i) {
    const int i1 = (i + 1) & 3, i2 = (i + 2) & 3;
    const double ax = v[2 * i1] - v[2 * i], ay = v[2 * i1 + 1] - v[2 * i + 1];
    const double bx = v[2 * i2] - v[2 * i1], by = v[2 * i2 + 1] - v[2 * i1 + 1];
    const double c = ax * by - ay * bx;
    pos += c > 0 ? 1 : 0;
    neg += c < 0 ? 1 : 0;
  }
  if (neg == 4) {
    const double x1 = v[2], y1 = v[3];
    v[2] = v[6];
    v[3] = v[7];
    v[6] = x1;
    v[7] = y1;
    return true;
  }
  return pos == 4;
}

// ---- the exact far-apart shortcut ----------------------------------------------------------------------------------------------
// When the clip quad is strictly convex by a margin (every turn above 1e-9) and the two axis-aligned bounding boxes are separated by
// a margin far above rounding error, Sutherland-Hodgman returns an empty polygon (a surviving vertex would have to lie within
// rounding distance of both hulls), so the reference's IoU is exactly 0.0.  Anything else takes the clip.
struct QiBox {
  double l, r, t, b, ext;  // bounds and the largest |coordinate|
  int firm;                // every turn of the (canonical) quad above 1e-9: may stand as the clip quad of the shortcut
};
MSOCR_QI_HD QiBox qi_box(const double* v) {
  QiBox o;
  o.l = o.r = v[0];
  o.t = o.b = v[1];
  for (int i = 1; i < 4; ++i) {
    o.l = fmin(o.l, v[2 * i]);
    o.r = fmax(o.r, v[2 * i]);
    o.t = fmin(o.t, v[2 * i + 1]);
    o.b = fmax(o.b, v[2 * i + 1]);
  }
  o.ext = fmax(fmax(fabs(o.l), fabs(o.r)), fmax(fabs(o.t), fabs(o.b)));
  o.firm = 1;
  for (int i = 0; i < 4; ++i) {
    const int i1 = (i + 1) & 3, i2 = (i + 2) & 3;
    const double ax = v[2 * i1] - v[2 * i], ay = v[2 * i1 + 1] - v[2 * i + 1];
    const double bx = v[2 * i2] - v[2 * i1], by = v[2 * i2 + 1] - v[2 * i1 + 1];
    if (!(ax * by - ay * bx > 1e-9)) o.firm = 0;
  }
  return o;
}
// subject box a, clip box b
MSOCR_QI_HD bool qi_far_apart(const QiBox& a, const QiBox& b) {
  const double ext = fmax(a.ext, b.ext);
  if (!b.firm || !(ext < 1e12)) return false;
  const double margin = 1e-6 * (1.0 + ext);
  return (a.l > b.r + margin) || (b.l > a.r + margin) || (a.t > b.b + margin) || (b.t > a.b + margin);
}

// ---- polygon_iou ---------------------------------------------------------------------------------------------------------------
MSOCR_QI_HD double qi_polygon_area(const double* poly, int n) {  // lanms.py:7-14
  double area = 0.0;
  for (int i = 0; i < n; i++) {
    const int j = (i + 1) % n;
    area += poly[2 * i] * poly[2 * j + 1] - poly[2 * j] * poly[2 * i + 1];
  }
  return fabs(area) / 2.0;
}

// Register-resident clip: a quad clipped by the four half-planes of a convex quad holds at most 8 vertices, so the polygon lives in
// 8 + 8 values with statically indexed, predicated loops and a select chain for "append at position count".  A stage that would hold a
// ninth vertex (rounding can make a clipped polygon cross a line more than twice) reports it, and the caller runs the general path.
struct QiPoly8 {
  double x[8], y[8];
  int n;
};
MSOCR_QI_HD void qi_p8_push(QiPoly8& o, double px, double py, bool& over) {
  if (o.n >= 8) {
    over = true;
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    o.x[k] = (o.n == k) ? px : o.x[k];
    o.y[k] = (o.n == k) ? py : o.y[k];
  }
  ++o.n;
}
MSOCR_QI_HD void qi_p8_clip(const QiPoly8& s, double Ax, double Ay, double Bx, double By, QiPoly8& o, bool& over) {  // lanms.py:32-57
  o.n = 0;
  double px = s.x[0], py = s.y[0];  // prev of vertex 0 is vertex n-1
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    px = (s.n - 1 == k) ? s.x[k] : px;
    py = (s.n - 1 == k) ? s.y[k] : py;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < s.n) {
      const double cx = s.x[i], cy = s.y[i];
      const bool curr_in = (Bx - Ax) * (cy - Ay) - (By - Ay) * (cx - Ax) >= 0;
      const bool prev_in = (Bx - Ax) * (py - Ay) - (By - Ay) * (px - Ax) >= 0;
      if (curr_in != prev_in) {  // compute_intersection(prev, curr, A, B)  (lanms.py:17-29)
        const double BAx = cx - px, BAy = cy - py;
        const double DCx = Bx - Ax, DCy = By - Ay;
        const double denom = BAx * DCy - BAy * DCx;
        const double CAx = Ax - px, CAy = Ay - py;
        double ix = px, iy = py;
        if (denom != 0) {
          const double t = (CAx * DCy - CAy * DCx) / denom;
          ix = px + t * BAx;
          iy = py + t * BAy;
        }
        qi_p8_push(o, ix, iy, over);
      }
      if (curr_in) qi_p8_push(o, cx, cy, over);
      px = cx;
      py = cy;
    }
  }
}
MSOCR_QI_HD double qi_p8_area(const QiPoly8& p) {  // polygon_area (lanms.py:7-14)
  double area = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < p.n) {
      const double xj = (i + 1 < p.n && i + 1 < 8) ? p.x[(i + 1) & 7] : p.x[0];
      const double yj = (i + 1 < p.n && i + 1 < 8) ? p.y[(i + 1) & 7] : p.y[0];
      area += p.x[i] * yj - xj * p.y[i];
    }
  }
  return fabs(area) / 2.0;
}
// false (result unspecified) when a clip stage needs more than 8 vertices
MSOCR_QI_HD bool qi_polygon_iou_fast(const double* poly1, const double* poly2, double* iou) {
  QiPoly8 a, b;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a.x[k] = 0.0;
    a.y[k] = 0.0;
    b.x[k] = 0.0;
    b.y[k] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.x[k] = poly1[2 * k];
    a.y[k] = poly1[2 * k + 1];
  }
  a.n = 4;
  b.n = 0;
  bool over = false;
  // the four clip stages of polygon_intersection (lanms.py:60-77); the live polygon alternates between b and a
  qi_p8_clip(a, poly2[0], poly2[1], poly2[2], poly2[3], b, over);
  int cnt = b.n;
  bool in_a = false;
  if (cnt != 0) {
    qi_p8_clip(b, poly2[2], poly2[3], poly2[4], poly2[5], a, over);
    cnt = a.n;
    in_a = true;
    if (cnt != 0) {
      qi_p8_clip(a, poly2[4], poly2[5], poly2[6], poly2[7], b, over);
      cnt = b.n;
      in_a = false;
      if (cnt != 0) {
        qi_p8_clip(b, poly2[6], poly2[7], poly2[0], poly2[1], a, over);
        cnt = a.n;
        in_a = true;
      }
    }
  }
  if (over) return false;
  double inter_area = 0.0;
  if (cnt > 2) inter_area = in_a ? qi_p8_area(a) : qi_p8_area(b);
  const double area1 = qi_polygon_area(poly1, 4), area2 = qi_polygon_area(poly2, 4);
  const double union_area = area1 + area2 - inter_area;
  *iou = union_area <= 0 ? 0.0 : inter_area / union_area;
  return true;
}

// The general path, with the reference's 20-vertex buffers (a vertex past the twentieth, where the reference would fail, is dropped).
MSOCR_QI_HD_NOINLINE double qi_polygon_iou_general(const double* poly1, const double* poly2) {
  double bufa[2 * MSOCR_QI_MAXV], bufb[2 * MSOCR_QI_MAXV];
  double *cur = bufa, *nxt = bufb;
  for (int k = 0; k < 8; ++k) cur[k] = poly1[k];
  int cnt = 4;
  for (int e = 0; e < 4; e++) {
    const double Ax = poly2[2 * e], Ay = poly2[2 * e + 1], Bx = poly2[2 * ((e + 1) & 3)], By = poly2[2 * ((e + 1) & 3) + 1];
    int count = 0;
    for (int i = 0; i < cnt; i++) {
      const double cx = cur[2 * i], cy = cur[2 * i + 1];
      const int ip = (i - 1 + cnt) % cnt;
      const double px = cur[2 * ip], py = cur[2 * ip + 1];
      const bool curr_in = (Bx - Ax) * (cy - Ay) - (By - Ay) * (cx - Ax) >= 0;
      const bool prev_in = (Bx - Ax) * (py - Ay) - (By - Ay) * (px - Ax) >= 0;
      if (curr_in != prev_in && count < MSOCR_QI_MAXV) {
        const double BAx = cx - px, BAy = cy - py;
        const double DCx = Bx - Ax, DCy = By - Ay;
        const double denom = BAx * DCy - BAy * DCx;
        const double CAx = Ax - px, CAy = Ay - py;
        double ix = px, iy = py;
        if (denom != 0) {
          const double t = (CAx * DCy - CAy * DCx) / denom;
          ix = px + t * BAx;
          iy = py + t * BAy;
        }
        nxt[2 * count] = ix;
        nxt[2 * count + 1] = iy;
        count++;
      }
      if (curr_in && count < MSOCR_QI_MAXV) {
        nxt[2 * count] = cx;
        nxt[2 * count + 1] = cy;
        count++;
      }
    }
    cnt = count;
    double* t = cur;
    cur = nxt;
    nxt = t;
    if (cnt == 0) break;
  }
  double inter_area = 0.0;
  if (cnt > 2) inter_area = qi_polygon_area(cur, cnt);
  const double area1 = qi_polygon_area(poly1, 4), area2 = qi_polygon_area(poly2, 4);
  const double union_area = area1 + area2 - inter_area;
  if (union_area <= 0) return 0.0;
  return inter_area / union_area;
}

// polygon_iou(subject, clip) of two canonical valid quads with their boxes
MSOCR_QI_HD double qi_iou(const double* subject, const QiBox& sbox, const double* clip, const QiBox& cbox) {
  if (qi_far_apart(sbox, cbox)) return 0.0;
  double r;
  if (qi_polygon_iou_fast(subject, clip, &r)) return r;
  return qi_polygon_iou_general(subject, clip);
}

// The total order under which a prediction picks its ground truth: IoU descending, then index ascending.  With best_iou starting at
// 0 and bj at -1 it restates "take j when iou > best_iou, scanning j ascending" for any order of the offers.
MSOCR_QI_HD bool qi_better(double iou, int j, double best_iou, int bj) { return iou > best_iou || (iou == best_iou && bj >= 0 && j < bj); }

// ---- the host twin -------------------------------------------------------------------------------------------------------------
// the argument rules shared by both entry points; counts are checked where they are host memory
inline bool qm_shape_ok(int N, int max_pred, int max_gt, const double* thresholds, int T) {
  if (N < 0 || max_pred < 0 || max_pred > MSOCR_QM_MAX_QUADS || max_gt < 0 || max_gt > MSOCR_QM_MAX_QUADS) return false;
  if (T < 1 || T > MSOCR_QM_MAX_T || !thresholds) return false;
  for (int t = 0; t < T; ++t)
    if (!(thresholds[t] > 0.0 && thresholds[t] <= 1.0)) return false;  // NaN fails both
  return true;
}

// msocr_quad_match_host without its argument checks.  Per page: canonical ground truth once; per prediction the non-zero IoUs once,
// in ascending j; per threshold the scan of the rule over them.
inline void qm_match_host(const float* pred, const int32_t* n_pred, int max_pred, const float* gt, const int32_t* n_gt, int max_gt, int N,
                          const double* thresholds, int T, int32_t* match_out, double* iou_out, int32_t* counts_out) {
  std::vector<double> G;
  std::vector<QiBox> gbox;
  std::vector<uint8_t> gvalid, used;
  std::vector<double> ciou;
  std::vector<int32_t> cj;
  for (int p = 0; p < N; ++p) {
    const int np = n_pred[p], ng = n_gt[p];
    const float* P = pred + (size_t)p * max_pred * 8;
    const float* Q = gt + (size_t)p * max_gt * 8;
    G.assign((size_t)ng * 8, 0.0);
    gbox.resize(ng);
    gvalid.assign(ng, 0);
    for (int j = 0; j < ng; ++j) {
      gvalid[j] = qi_canonical(Q + (size_t)j * 8, &G[(size_t)j * 8]) ? 1 : 0;
      if (gvalid[j]) gbox[j] = qi_box(&G[(size_t)j * 8]);
    }
    used.assign((size_t)T * ng, 0);
    std::vector<int32_t> tp(T, 0), fp(T, 0);
    for (int i = 0; i < np; ++i) {
      double v[8];
      const bool valid = qi_canonical(P + (size_t)i * 8, v);
      ciou.clear();
      cj.clear();
      if (valid) {
        const QiBox vb = qi_box(v);
        for (int j = 0; j < ng; ++j) {
          if (!gvalid[j]) continue;
          const double iou = qi_iou(v, vb, &G[(size_t)j * 8], gbox[j]);
          if (iou > 0) {
            ciou.push_back(iou);
            cj.push_back(j);
          }
        }
      }
      for (int t = 0; t < T; ++t) {
        const size_t o = ((size_t)p * T + t) * max_pred + i;
        if (!valid) {
          match_out[o] = -2;
          iou_out[o] = 0.0;
          fp[t]++;
          continue;
        }
        double best_iou = 0.0;
        int bj = -1;
        for (size_t c = 0; c < cj.size(); ++c)
          if (!used[(size_t)t * ng + cj[c]] && ciou[c] > best_iou) {
            best_iou = ciou[c];
            bj = cj[c];
          }
        iou_out[o] = best_iou;
        if (best_iou >= thresholds[t]) {
          tp[t]++;
          used[(size_t)t * ng + bj] = 1;
          match_out[o] = bj;
        } else {
          fp[t]++;
          match_out[o] = -1;
        }
      }
    }
    for (int t = 0; t < T; ++t) {
      int32_t* c = counts_out + ((size_t)p * T + t) * 3;
      c[0] = tp[t];
      c[1] = fp[t];
      c[2] = ng - tp[t];
    }
  }
}
#endif
