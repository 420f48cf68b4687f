// quad_crop.hip — rectified word crops: the recogniser's canvas is cut ALONG the detected quadrilateral instead of from its
// axis-aligned window (an extension beyond the reference, off by default: Pipeline.rectify_crops).
//
//   quad_descriptor   corners as stored -> canonical (tl, tr, br, bl) order, side lengths, ResizeAndPadA's size arithmetic
//   quad_pixel        one canvas pixel: mean of Sx x Sy sub-samples of the page, each mapped through the bilinear patch of the
//                     four corners and read with 4 clamped taps
//
// Both are __host__ __device__ and all their arithmetic is f64 in one written order (compile with -ffp-contract=off, the Makefile
// does; +, -, *, /, sqrt, floor, ceil and rint are correctly rounded on both sides), so the kernels and their host twins
// (msocr_quad_crop_descriptors_host, msocr_quad_crop_host) give the same bytes.  No transcendental is used anywhere.
//
// Descriptor = 12 x int32 {page, x0, y0, x1, y1, x2, y2, x3, y3 (f32 bit patterns, canonical order), new_w, new_h, y0}.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "block_prims.h"
#include "internal.h"
#include "msocr.h"
#include "word_boxes.h"

namespace {
#define HD __host__ __device__ __forceinline__

constexpr int QD = 12;        // words per quad descriptor
constexpr int QDESC_T = 1024; // threads per page of the descriptor kernel
constexpr int QCROP_T = 256;  // threads per crop

HD double dmax(double a, double b) { return a > b ? a : b; }

// Side lengths of canonical corners: w = max(|P1-P0|, |P2-P3|), h = max(|P3-P0|, |P2-P1|).
HD void quad_size(const float* c, double* w, double* h) {
  const double x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5], x3 = c[6], y3 = c[7];
  const double top = sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
  const double bot = sqrt((x2 - x3) * (x2 - x3) + (y2 - y3) * (y2 - y3));
  const double lft = sqrt((x3 - x0) * (x3 - x0) + (y3 - y0) * (y3 - y0));
  const double rgt = sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1));
  *w = dmax(top, bot);
  *h = dmax(lft, rgt);
}

// One quad descriptor from the stored corners q[8] and the word's AABB descriptor aabb[8] (msocr_crop_resize_pad's format).
// natural != 0: the region at its own size (new_w = rint(w), new_h = rint(h), y0 = 0) instead of ResizeAndPadA's fit.
HD void quad_descriptor(const float* q, const int32_t* aabb, int img_h, int img_w, int natural, int32_t* out) {
  float c[8];
  double w = 0.0, h = 0.0;
  bool ok = quad_canonical(q, c);
  if (ok) {
    quad_size(c, &w, &h);
    ok = w >= 1.0 && h >= 1.0;  // false for NaN too
  }
  if (!ok) {  // fallback: the corners of the clamped AABB window
    const float a = (float)aabb[1], b = (float)aabb[2], cc = (float)aabb[3], d = (float)aabb[4];
    c[0] = a; c[1] = b; c[2] = cc; c[3] = b; c[4] = cc; c[5] = d; c[6] = a; c[7] = d;
    quad_size(c, &w, &h);
    w = dmax(w, 1.0);  // windows written by msocr_reading_order_crops / ops.crop_descriptors are at least 1 x 1
    h = dmax(h, 1.0);
  }
  int nw, nh, yy = 0;
  if (natural) {
    nw = rint_clip(w, 1 << 30);
    nh = rint_clip(h, 1 << 30);
  } else {
    const CanvasFit f = canvas_fit(w, h, img_h, img_w);
    nw = f.new_w; nh = f.new_h; yy = f.y0;
  }
  out[0] = aabb[0];
  for (int k = 0; k < 8; ++k) out[1 + k] = f32_bits(c[k]);
  out[9] = nw; out[10] = nh; out[11] = yy;
}

// What the crop kernel and the wrapper refuse: page out of range, a non-finite corner, new_w / new_h / y0 outside the canvas.
HD bool quad_desc_valid(const int32_t* d, int N, int img_h, int img_w) {
  if (d[0] < 0 || d[0] >= N) return false;
  for (int k = 0; k < 8; ++k)
    if (!finite_f32(bits_f32(d[1 + k]))) return false;
  const int nw = d[9], nh = d[10], y0 = d[11];
  return nw >= 1 && nw <= img_w && nh >= 1 && nh <= img_h && y0 >= 0 && y0 <= img_h - nh;
}

struct QuadCrop {  // per-crop constants of the sampling
  double px[4], py[4];
  double dnw, dnh, inv_n;  // new_w, new_h as doubles; Sx * Sy
  int nw, nh, y0, sx, sy;
  const uint8_t* page;
};

HD int sub_samples(double side, int n) {  // clamp(ceil(side / n), 1, 4)
  const double r = ceil(side / (double)n);
  return r >= 4.0 ? 4 : (r >= 1.0 ? (int)r : 1);
}

HD QuadCrop quad_crop_setup(const int32_t* d, const uint8_t* pages, int H, int W) {
  QuadCrop q;
  float c[8];
  for (int k = 0; k < 8; ++k) c[k] = bits_f32(d[1 + k]);
  for (int k = 0; k < 4; ++k) { q.px[k] = c[2 * k]; q.py[k] = c[2 * k + 1]; }
  double w, h;
  quad_size(c, &w, &h);
  q.nw = d[9]; q.nh = d[10]; q.y0 = d[11];
  q.dnw = (double)q.nw; q.dnh = (double)q.nh;
  q.sx = sub_samples(w, q.nw);
  q.sy = sub_samples(h, q.nh);
  q.inv_n = (double)(q.sx * q.sy);
  q.page = pages + (long)d[0] * H * W * 3;
  return q;
}

HD int clamp_index(double v, int n) {  // an integral double -> [0, n - 1]
  return v <= 0.0 ? 0 : (v >= (double)(n - 1) ? n - 1 : (int)v);
}

// Canvas pixel (dx, dy) of the resized region, 0 <= dx < new_w, 0 <= dy < new_h -> rgb[3].
HD void quad_pixel(const QuadCrop& q, int H, int W, int dx, int dy, uint8_t* rgb) {
  double sum[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < q.sy; ++j) {
    const double v = ((double)dy + ((double)j + 0.5) / (double)q.sy) / q.dnh;
    for (int i = 0; i < q.sx; ++i) {
      const double u = ((double)dx + ((double)i + 0.5) / (double)q.sx) / q.dnw;
      const double w0 = (1.0 - u) * (1.0 - v), w1 = u * (1.0 - v), w2 = u * v, w3 = (1.0 - u) * v;
      const double x = w0 * q.px[0] + w1 * q.px[1] + w2 * q.px[2] + w3 * q.px[3] - 0.5;
      const double y = w0 * q.py[0] + w1 * q.py[1] + w2 * q.py[2] + w3 * q.py[3] - 0.5;
      const double xf = floor(x), yf = floor(y);
      const double fx = x - xf, fy = y - yf;
      const int xa = clamp_index(xf, W), xb = clamp_index(xf + 1.0, W);
      const int ya = clamp_index(yf, H), yb = clamp_index(yf + 1.0, H);
      const uint8_t* ra = q.page + (long)ya * W * 3;
      const uint8_t* rb = q.page + (long)yb * W * 3;
      const uint8_t *ta = ra + xa * 3, *tb = ra + xb * 3, *tc = rb + xa * 3, *td = rb + xb * 3;
      for (int ch = 0; ch < 3; ++ch)
        sum[ch] += (1.0 - fy) * ((1.0 - fx) * (double)ta[ch] + fx * (double)tb[ch]) +
                   fy * ((1.0 - fx) * (double)tc[ch] + fx * (double)td[ch]);
    }
  }
  for (int ch = 0; ch < 3; ++ch) {
    const double r = rint(sum[ch] / q.inv_n);
    rgb[ch] = (uint8_t)(r <= 0.0 ? 0.0 : (r >= 255.0 ? 255.0 : r));
  }
}

// One workgroup per page: quad descriptors of the page's kept words, compacted in the order of desc (the rank of a kept position
// is the prefix sum of keep).  Nothing is written for a page with ncrop < 0.
__global__ __launch_bounds__(QDESC_T) void quad_descriptors_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ nbox,
                                                                    int max_cand, int img_h, int img_w,
                                                                    const int32_t* __restrict__ order, const int32_t* __restrict__ keep,
                                                                    const int32_t* __restrict__ desc, const int32_t* __restrict__ ncrop,
                                                                    int32_t* __restrict__ qdesc) {
  const int pg = blockIdx.x, tid = threadIdx.x;
  const int nc = ncrop[pg];
  int n = nbox[pg];
  if (nc <= 0 || n <= 0) return;  // uniform per workgroup
  n = n < max_cand ? n : max_cand;
  const int32_t* oo = order + (long)pg * max_cand;
  const int32_t* ko = keep + (long)pg * max_cand;
  const int32_t* din = desc + (long)pg * max_cand * 8;
  const float* ib = boxes + (long)pg * max_cand * 9;
  int32_t* dout = qdesc + (long)pg * max_cand * QD;
  __shared__ int wave_tot[QDESC_T / 64];
  const int per = (n + QDESC_T - 1) / QDESC_T;
  const int a0 = min(n, tid * per), a1 = min(n, a0 + per);
  int sum = 0;
  for (int k = a0; k < a1; ++k) sum += ko[k] != 0 ? 1 : 0;
  int total, rank = block_exclusive_scan<QDESC_T>(sum, wave_tot, &total);
  for (int pos = a0; pos < a1; ++pos) {
    if (ko[pos] == 0) continue;
    if (rank < nc && rank < max_cand) {  // always, for the outputs of msocr_reading_order_crops
      const int wi = oo[pos];
      float q[8];
      for (int k = 0; k < 8; ++k) q[k] = (wi >= 0 && wi < n) ? ib[9 * (long)wi + k] : NAN;  // a bad index takes the fallback
      quad_descriptor(q, din + 8 * (long)rank, img_h, img_w, 0, dout + QD * (long)rank);
    }
    ++rank;
  }
}

// One workgroup per crop, one canvas pixel per thread iteration.
__global__ __launch_bounds__(QCROP_T) void quad_crop_kernel(const uint8_t* __restrict__ pages, int N, int H, int W,
                                                             const int32_t* __restrict__ qdesc, int img_h, int img_w,
                                                             uint8_t* __restrict__ out) {
  const int m = blockIdx.x;
  const int32_t* d = qdesc + (long)m * QD;
  uint8_t* o = out + (long)m * img_h * img_w * 3;
  if (!quad_desc_valid(d, N, img_h, img_w)) {
    for (int p = threadIdx.x; p < img_h * img_w * 3; p += QCROP_T) o[p] = 255;
    return;
  }
  __shared__ QuadCrop qs;  // the crop's constants, computed once
  if (threadIdx.x == 0) qs = quad_crop_setup(d, pages, H, W);
  __syncthreads();
  const int nw = qs.nw, nh = qs.nh, y0 = qs.y0;
  for (int p = threadIdx.x; p < img_h * img_w; p += QCROP_T) {
    const int cy = p / img_w, cx = p - cy * img_w;
    const int dy = cy - y0;
    uint8_t r[3] = {255, 255, 255};
    if (dy >= 0 && dy < nh && cx < nw) quad_pixel(qs, H, W, cx, dy, r);
    o[(long)p * 3] = r[0];
    o[(long)p * 3 + 1] = r[1];
    o[(long)p * 3 + 2] = r[2];
  }
}
}  // namespace

extern "C" int msocr_quad_crop_descriptors_host(const float* quads_host, const int32_t* desc_host, int M, int img_h, int img_w,
                                                int natural, int32_t* qdesc_out_host) {
  if (M < 0 || (M > 0 && (!quads_host || !desc_host || !qdesc_out_host))) return MSOCR_E_ARG;
  if (!natural && (img_h <= 0 || img_w <= 0)) return MSOCR_E_ARG;
  for (int m = 0; m < M; ++m)
    quad_descriptor(quads_host + 8 * (size_t)m, desc_host + 8 * (size_t)m, img_h, img_w, natural, qdesc_out_host + QD * (size_t)m);
  return MSOCR_OK;
}

extern "C" int msocr_quad_crop_descriptors(const float* boxes, const int32_t* nbox, int N, int max_cand, int img_h, int img_w,
                                           const int32_t* order, const int32_t* keep, const int32_t* desc, const int32_t* ncrop,
                                           int32_t* qdesc_out, void* stream) {
  if (!boxes || !nbox || !order || !keep || !desc || !ncrop || !qdesc_out) return MSOCR_E_ARG;
  if (N <= 0 || max_cand <= 0 || img_h <= 0 || img_w <= 0) return MSOCR_E_ARG;
  MSOCR_LAUNCH(quad_descriptors_kernel, dim3(N), dim3(QDESC_T), 0, (hipStream_t)stream, boxes, nbox, max_cand, img_h, img_w, order,
               keep, desc, ncrop, qdesc_out);
  return LAUNCH_OK();
}

static bool quad_crop_args_ok(const void* pages, const void* qdesc, const void* canvases, int N, int H, int W, int M, int img_h,
                              int img_w) {
  return pages && qdesc && canvases && N > 0 && H > 0 && W > 0 && M > 0 && img_h > 0 && img_w > 0;
}

extern "C" int msocr_quad_crop(const uint8_t* pages, int N, int H, int W, const int32_t* qdesc_dev, const int32_t* qdesc_host, int M,
                               int img_h, int img_w, uint8_t* canvases, void* stream) {
  if (!quad_crop_args_ok(pages, qdesc_dev, canvases, N, H, W, M, img_h, img_w)) return MSOCR_E_ARG;
  for (int m = 0; qdesc_host && m < M; ++m)
    if (!quad_desc_valid(qdesc_host + QD * (size_t)m, N, img_h, img_w)) return MSOCR_E_ARG;
  MSOCR_LAUNCH(quad_crop_kernel, dim3(M), dim3(QCROP_T), 0, (hipStream_t)stream, pages, N, H, W, qdesc_dev, img_h, img_w, canvases);
  return LAUNCH_OK();
}

extern "C" int msocr_quad_crop_host(const uint8_t* pages_host, int N, int H, int W, const int32_t* qdesc_host, int M, int img_h,
                                    int img_w, uint8_t* canvases_host) {
  if (!quad_crop_args_ok(pages_host, qdesc_host, canvases_host, N, H, W, M, img_h, img_w)) return MSOCR_E_ARG;
  for (int m = 0; m < M; ++m) {
    const int32_t* d = qdesc_host + QD * (size_t)m;
    uint8_t* o = canvases_host + (size_t)m * img_h * img_w * 3;
    memset(o, 255, (size_t)img_h * img_w * 3);
    if (!quad_desc_valid(d, N, img_h, img_w)) continue;  // a white canvas, as the kernel writes
    const QuadCrop q = quad_crop_setup(d, pages_host, H, W);
    for (int dy = 0; dy < q.nh; ++dy)
      for (int dx = 0; dx < q.nw; ++dx) quad_pixel(q, H, W, dx, dy, o + ((size_t)(dy + q.y0) * img_w + dx) * 3);
  }
  return MSOCR_OK;
}
