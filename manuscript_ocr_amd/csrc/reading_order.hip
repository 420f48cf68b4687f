// reading_order.hip — the Pipeline glue between detector and recogniser ON THE DEVICE, one workgroup per page:
// final detector boxes -> word AABBs -> reading order -> crop descriptors for msocr_crop_resize_pad.
//
//   Pipeline.predict sort + crop section              _pipeline.py:100-137  (np.array(polygon, int32) truncation, min_text_size)
//   Pipeline._extract_word_image                      _pipeline.py:204-221  (clamped AABB)
//   resolve_intersections                             detectors/_east/utils.py:500-547
//   sort_boxes_reading_order                          detectors/_east/utils.py:550-607
//   sort_boxes_reading_order_with_resolutions         detectors/_east/utils.py:610-644 (dict(zip(shrunk, boxes)): later duplicate wins)
//   first-equal-word re-match                         _pipeline.py:113-121
//   ResizeAndPadA size arithmetic                     recognizers/_trba/data/transforms.py:91-95,114-117 (Python round = rint)
//
// Everything is integer or f64 arithmetic in the reference's order, so the result is bit-identical to the host helper
// msocr_reading_order_host (host_glue.hip) + ops.crop_descriptors, which stay as the fallback for pages this kernel flags
// (ncrop = -1: more boxes than the capacity, more than RO_MAXLINES text lines, or more intersecting pairs than the pair buffer).
// msocr_reading_order_lines launches the same body with LINES = true: the text lines the order is built from leave as well (the
// line of every position, one record per line, the line count), bit-identical to msocr_reading_lines_host.
// msocr_reading_order_deskew launches it with DESKEW = true (Pipeline.deskew): the page's skew is estimated
// from the quads (page_skew.h, two exact int64 reductions over the workgroup) and the boxes that are shrunk, grouped and ordered are
// those of the rotated corners; windows, descriptors and line unions stay those of the original boxes.  Bit-identical to
// msocr_page_skew_host + msocr_deskew_boxes_host + msocr_reading_lines_host.
//
// resolve_intersections is a SEQUENTIAL sweep over all pairs (i < j): an intersecting pair shrinks both boxes at once, which
// changes what later pairs of the same sweep see.  It is parallelised exactly: boxes only ever shrink during a sweep, so the
// pairs that intersect at the START of a sweep are a superset of the pairs the sequential sweep will find; those candidates are
// found by all threads, ordered lexicographically by a prefix sum, and replayed in order by one thread with the live boxes.
// Compile with -ffp-contract=off (the Makefile does): int(x1 - (x1 - x0) * 0.1) must round like Python.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_prims.h"
#include "internal.h"
#include "msocr.h"
#include "page_skew.h"
#include "word_boxes.h"

namespace {
constexpr int RO_T = 1024;         // threads per page
constexpr int RO_CAP = 16384;      // boxes per page
constexpr int RO_MAXLINES = 4096;  // text lines per page (line state lives in LDS)

__host__ __device__ inline int ro_cap(int max_cand) { return max_cand < RO_CAP ? max_cand : RO_CAP; }
__host__ __device__ inline long ro_pair_cap(int cap) { return 8L * cap + 4096; }
// per-page workspace in 4-byte words: ob[4c] sb[4c] cnt[c+4] pairs[2P] sorted[c] lineof[c] seq[c] emitted[c] keepf[c]
__host__ __device__ inline long ro_ws_words(int cap) { return (4L * cap + 4L * cap + (cap + 4) + 2 * ro_pair_cap(cap) + 5L * cap + 3) / 4 * 4; }

// in-place exclusive prefix sum of arr[0..n) by the whole workgroup (contiguous chunk per thread); returns the total
__device__ int ro_block_scan(int* arr, int n, int* wave_tot /* LDS [RO_T/64] */) {
  const int tid = threadIdx.x;
  const int per = (n + RO_T - 1) / RO_T;
  const int a0 = min(n, tid * per), a1 = min(n, a0 + per);
  int sum = 0;
  for (int k = a0; k < a1; ++k) sum += arr[k];
  int total, run = block_exclusive_scan<RO_T>(sum, wave_tot, &total);
  for (int k = a0; k < a1; ++k) {
    const int v = arr[k];
    arr[k] = run;
    run += v;
  }
  __threadfence();
  __syncthreads();
  return total;
}

// the text lines of the reading order as a result (msocr_reading_order_lines); unused and compiled out with LINES = false
struct RoLineOut {
  int32_t* line;    // [N][max_cand]
  int32_t* lines;   // [N][rows][6]
  int32_t* nlines;  // [N]
  int rows;
};

// the page's skew estimate as a result (msocr_reading_order_deskew); unused and compiled out with DESKEW = false
struct RoSkewOut {
  int64_t* skew;  // [N][4] {S2x, S2y, m, applied}
  double* cs;     // [N][2] {c, s}
};

template <bool LINES, bool DESKEW>
__global__ __launch_bounds__(RO_T) void reading_order_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ nbox,
                                                              int max_cand, int cap, int page_h, int page_w, int min_text,
                                                              int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                                              int page_base, int32_t* __restrict__ order_out,
                                                              int32_t* __restrict__ keep_out, int32_t* __restrict__ desc_out,
                                                              int32_t* __restrict__ ncrop_out, int32_t* __restrict__ ws, RoLineOut lo,
                                                              RoSkewOut so) {
  const int pg = blockIdx.x, tid = threadIdx.x;
  const int n = nbox[pg];
  __shared__ long long skew_s[4];  // DESKEW: {S2x, S2y, m, applied}, written out with the verdict of a page that is not flagged
  __shared__ double cs_s[2];
  // the page's verdict: crops (and lines) of the page, 0 for an empty page, -1 = the host path takes it
  auto verdict = [&](int ncrop, int nlines) {
    if (tid == 0) {
      ncrop_out[pg] = ncrop;
      if constexpr (LINES) lo.nlines[pg] = nlines;
      if constexpr (DESKEW)
        if (ncrop >= 0) {
          for (int k = 0; k < 4; ++k) so.skew[4 * (long)pg + k] = (n > 0 ? skew_s[k] : 0LL);
          so.cs[2 * (long)pg] = n > 0 ? cs_s[0] : 1.0;
          so.cs[2 * (long)pg + 1] = n > 0 ? cs_s[1] : 0.0;
        }
    }
  };
  if (n < 0 || n > cap) {
    verdict(-1, -1);
    return;
  }
  if (n == 0) {
    verdict(0, 0);
    return;
  }
  int32_t* w = ws + (long)pg * (ro_ws_words(cap) + (DESKEW ? 4L * cap : 0L));
  Box4* ob = reinterpret_cast<Box4*>(w);
  // DESKEW: the boxes of the rotated corners, unshrunk (the dictionary and the re-match compare them); else the original boxes
  Box4* rb = DESKEW ? reinterpret_cast<Box4*>(w + ro_ws_words(cap)) : ob;
  Box4* sb = ob + cap;
  int* cnt = reinterpret_cast<int*>(sb + cap);
  const long P = ro_pair_cap(cap);
  int* pairs = cnt + cap + 4;
  int* sorted = pairs + 2 * P;
  int* lineof = sorted + cap;
  int* seq = lineof + cap;
  int* emitted = seq + cap;
  int* keepf = emitted + cap;
  int32_t* oo = order_out + (long)pg * max_cand;
  int32_t* ko = keep_out + (long)pg * max_cand;
  int32_t* dout = desc_out + (long)pg * max_cand * 8;

  __shared__ double lsum[RO_MAXLINES];
  __shared__ int lcnt[RO_MAXLINES], lmaxx[RO_MAXLINES], lstart[RO_MAXLINES];
  __shared__ int wave_tot[RO_T / 64];
  __shared__ int nlines_s, fail_s;
  __shared__ long long hsum_s;

  // ---- word AABBs: np.array(polygon, dtype=np.int32) truncates toward zero, then min / max over the 4 points (_pipeline.py:106-109)
  const float* ib = boxes + (long)pg * max_cand * 9;
  for (int i = tid; i < n; i += RO_T) {
    const Box4 b = box_from_quad(ib + 9 * (long)i);
    ob[i] = b;
    if constexpr (!DESKEW) sb[i] = b;
  }
  if (tid == 0) { fail_s = 0; hsum_s = 0; }
  if constexpr (DESKEW) {
    // ---- page skew (page_skew.h): S1 over the words that vote, S2 and m over those near S1; then the ordering boxes
    __shared__ long long wave_tot64[RO_T / 64];
    long long ax = 0, ay = 0;
    for (int i = tid; i < n; i += RO_T) {
      long long qx, qy;
      if (skew_word(ib + 9 * (long)i, &qx, &qy)) { ax += qx; ay += qy; }
    }
    const long long s1x = block_sum_i64<RO_T>(ax, wave_tot64), s1y = block_sum_i64<RO_T>(ay, wave_tot64);
    long long bx = 0, by = 0, bm = 0;
    for (int i = tid; i < n; i += RO_T) {
      long long qx, qy;
      if (skew_word(ib + 9 * (long)i, &qx, &qy) && skew_near(s1x, s1y, qx, qy)) { bx += qx; by += qy; ++bm; }
    }
    const long long s2x = block_sum_i64<RO_T>(bx, wave_tot64), s2y = block_sum_i64<RO_T>(by, wave_tot64);
    const long long m = block_sum_i64<RO_T>(bm, wave_tot64);
    const bool applied = skew_applied(s2x, s2y, m);
    double cs[2];
    skew_cos_sin(s2x, s2y, applied, cs);
    if (tid == 0) { skew_s[0] = s2x; skew_s[1] = s2y; skew_s[2] = m; skew_s[3] = applied ? 1 : 0; cs_s[0] = cs[0]; cs_s[1] = cs[1]; }
    for (int i = tid; i < n; i += RO_T) {
      const Box4 b = deskew_box(ib + 9 * (long)i, applied, cs[0], cs[1], page_h, page_w);
      rb[i] = b;
      sb[i] = b;
    }
  }
  __threadfence();
  __syncthreads();

  // ---- resolve_intersections: up to 50 sweeps (utils.py:507-546)
  for (int sweep = 0; sweep < 50; ++sweep) {
    for (int i = tid; i < n; i += RO_T) {
      const Box4 a = sb[i];
      int c = 0;
      for (int j = i + 1; j < n; ++j) c += box_hit(a, sb[j]) ? 1 : 0;
      cnt[i] = c;
    }
    __threadfence();
    __syncthreads();
    const int total = ro_block_scan(cnt, n, wave_tot);
    if (total == 0) break;
    if (total > P) {
      if (tid == 0) fail_s = 1;
      break;
    }
    for (int i = tid; i < n; i += RO_T) {
      const Box4 a = sb[i];
      int o = cnt[i];
      for (int j = i + 1; j < n; ++j)
        if (box_hit(a, sb[j])) { pairs[2 * (long)o] = i; pairs[2 * (long)o + 1] = j; ++o; }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {  // the sequential sweep, restricted to the candidate pairs, with the live boxes
      for (int p = 0; p < total; ++p) {
        const int i = pairs[2 * (long)p], j = pairs[2 * (long)p + 1];
        Box4 a = sb[i], b = sb[j];
        if (!box_hit(a, b)) continue;
        box_shrink(a);
        box_shrink(b);
        sb[i] = a; sb[j] = b;
      }
    }
    __threadfence();
    __syncthreads();
  }
  __syncthreads();
  if (fail_s) {
    verdict(-1, -1);
    return;
  }

  // ---- sort_boxes_reading_order on the shrunk boxes (utils.py:550-607)
  {
    long long h = 0;
    for (int i = tid; i < n; i += RO_T) h += (long long)(sb[i].y1 - sb[i].y0);
    for (int o = 32; o > 0; o >>= 1) h += __shfl_down(h, o);
    if ((tid & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&hsum_s), (unsigned long long)h);
  }
  // stable sort by cy = (y0 + y1) / 2: rank on the integer 2*cy, ties by index
  for (int i = tid; i < n; i += RO_T) {
    const int ki = sb[i].y0 + sb[i].y1;
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const int kj = sb[j].y0 + sb[j].y1;
      r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    sorted[r] = i;
    seq[i] = r;
  }
  __threadfence();
  __syncthreads();
  const double avg_h = (double)hsum_s / (double)n;  // np.mean of ints: exact sum, one division
  const double tol = avg_h * y_tol_ratio, gap = avg_h * x_gap_ratio;
  if (tid < 64) {  // one wave walks the cy-sorted boxes; its lanes test 64 lines at a time, the FIRST matching line wins
    const int lane = tid;
    int L = 0;
    bool over = false;
    for (int s = 0; s < n && !over; ++s) {
      const int i = sorted[s];
      const Box4 b = sb[i];
      const double c = (double)(b.y0 + b.y1) / 2.0;
      int home = -1;
      for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        bool ok = false;
        if (l < L) {
          const double line_cy = lsum[l] / (double)lcnt[l];
          ok = fabs(c - line_cy) <= tol && (double)(b.x0 - lmaxx[l]) <= gap;
        }
        const unsigned long long bal = __ballot(ok);
        if (bal) { home = l0 + (int)__ffsll((long long)bal) - 1; break; }
      }
      if (home < 0) {
        if (L >= RO_MAXLINES) { over = true; break; }
        if (lane == 0) { lsum[L] = c; lcnt[L] = 1; lmaxx[L] = b.x1; lineof[i] = L; }
        ++L;
      } else if (lane == 0) {
        lsum[home] += c; lcnt[home] += 1; lmaxx[home] = max(lmaxx[home], b.x1); lineof[i] = home;
      }
      __atomic_signal_fence(__ATOMIC_SEQ_CST);  // lane 0's LDS stores stay ahead of the next iteration's reads (in-order per wave)
      __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) { nlines_s = L; if (over) fail_s = 1; }
  }
  __threadfence();
  __syncthreads();
  if (fail_s) {
    verdict(-1, -1);
    return;
  }
  const int L = nlines_s;
  // lines sorted by their mean cy (stable: creation order breaks ties), then the first output position of every line;
  // LINES: the same comparison counts the lines in front, which is the line's index in reading order (lmaxx[] is free again)
  int* lrank = lmaxx;
  for (int l = tid; l < L; l += RO_T) {
    const double m = lsum[l] / (double)lcnt[l];
    int start = 0, rank = 0;
    for (int k = 0; k < L; ++k) {
      const double mk = lsum[k] / (double)lcnt[k];
      if (mk < m || (mk == m && k < l)) {
        start += lcnt[k];
        if constexpr (LINES) ++rank;
      }
    }
    lstart[l] = start;
    if constexpr (LINES) lrank[l] = rank;
  }
  __syncthreads();
  // inside a line: stable sort by x0 (insertion order = cy-sorted order breaks ties)
  for (int i = tid; i < n; i += RO_T) {
    const int li = lineof[i], xi = sb[i].x0, si = seq[i];
    int r = 0;
    for (int m = 0; m < n; ++m)
      if (lineof[m] == li) {
        const int xm = sb[m].x0;
        r += (xm < xi || (xm == xi && seq[m] < si)) ? 1 : 0;
      }
    emitted[lstart[li] + r] = i;
  }
  __threadfence();
  __syncthreads();
  // shrunk box -> original (dict: the LAST box with an equal shrunk box, utils.py:639) -> the FIRST word with an equal
  // original box (_pipeline.py:113-121); size filter, clamped crop window, ResizeAndPadA's size arithmetic
  for (int pos = tid; pos < n; pos += RO_T) {
    const int i = emitted[pos];
    const Box4 si = sb[i];
    int back = i;
    for (int j = n - 1; j > i; --j)
      if (box_same(sb[j], si)) { back = j; break; }
    const Box4 o = rb[back];
    int wi = back;
    for (int j = 0; j < back; ++j)
      if (box_same(rb[j], o)) { wi = j; break; }
    oo[pos] = wi;
    int win[4];
    const int keep = box_crop_window(ob[wi], page_h, page_w, min_text, win) ? 1 : 0;
    keepf[pos] = keep;
    ko[pos] = keep;
    if (keep) {  // staged at the word's position, compacted below
      const CanvasFit f = canvas_fit((double)(win[2] - win[0]), (double)(win[3] - win[1]), img_h, img_w);
      int32_t* t = dout + 8 * (long)pos;
      t[0] = page_base + pg; t[1] = win[0]; t[2] = win[1]; t[3] = win[2]; t[4] = win[3]; t[5] = f.new_w; t[6] = f.new_h; t[7] = f.y0;
    }
  }
  __threadfence();
  __syncthreads();
  if constexpr (LINES) {
    // one thread per line walks the line's span of positions: the line index of every position and the union of the words'
    // original AABBs (oo[] is complete: the barrier above)
    int32_t* lno = lo.line + (long)pg * max_cand;
    int32_t* rec = lo.lines + (long)pg * lo.rows * 6;  // L <= min(n, RO_MAXLINES) <= rows
    for (int l = tid; l < L; l += RO_T) {
      const int first = lstart[l], count = lcnt[l], rank = lrank[l];
      Box4 u = ob[oo[first]];
      lno[first] = rank;
      for (int pos = first + 1; pos < first + count; ++pos) {
        const Box4 b = ob[oo[pos]];
        u.x0 = min(u.x0, b.x0); u.y0 = min(u.y0, b.y0); u.x1 = max(u.x1, b.x1); u.y1 = max(u.y1, b.y1);
        lno[pos] = rank;
      }
      int32_t* t = rec + 6 * (long)rank;
      t[0] = first; t[1] = count; t[2] = u.x0; t[3] = u.y0; t[4] = u.x1; t[5] = u.y1;
    }
  }
  const int nk = ro_block_scan(keepf, n, wave_tot);  // keepf[pos] = index of the crop among the page's crops
  // compaction through a staging buffer (pairs[] holds >= 16 * cap words and is free again)
  for (int pos = tid; pos < n; pos += RO_T)
    if (ko[pos])
      for (int e = 0; e < 8; ++e) pairs[8 * (long)keepf[pos] + e] = dout[8 * (long)pos + e];
  __threadfence();
  __syncthreads();
  for (long k = tid; k < 8L * nk; k += RO_T) dout[k] = pairs[k];
  verdict(nk, L);
}

template <bool LINES, bool DESKEW = false>
int ro_launch(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w, int min_text_size, int img_h,
              int img_w, double y_tol_ratio, double x_gap_ratio, int page_base, int32_t* order_out, int32_t* keep_out,
              int32_t* desc_out, int32_t* ncrop_out, void* workspace, RoLineOut lo, void* stream,
              RoSkewOut so = RoSkewOut{nullptr, nullptr}) {
  if (!boxes || !nbox || !order_out || !keep_out || !desc_out || !ncrop_out || !workspace) return MSOCR_E_ARG;
  if (N <= 0 || max_cand <= 0 || page_h <= 0 || page_w <= 0 || img_h <= 0 || img_w <= 0 || page_base < 0) return MSOCR_E_ARG;
  if ((uintptr_t)workspace & 15) return MSOCR_E_ARG;
  MSOCR_LAUNCH((reading_order_kernel<LINES, DESKEW>), dim3(N), dim3(RO_T), 0, (hipStream_t)stream, boxes, nbox, max_cand, ro_cap(max_cand),
               page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base, order_out, keep_out, desc_out,
               ncrop_out, (int32_t*)workspace, lo, so);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}
}  // namespace

extern "C" int64_t msocr_reading_order_workspace_bytes(int N, int max_cand) {
  return (N > 0 && max_cand > 0) ? (int64_t)N * ro_ws_words(ro_cap(max_cand)) * 4 : 0;
}

extern "C" int msocr_reading_order_crops(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                                         int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                         int page_base, int32_t* order_out, int32_t* keep_out, int32_t* desc_out,
                                         int32_t* ncrop_out, void* workspace, void* stream) {
  return ro_launch<false>(boxes, nbox, N, max_cand, page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base,
                          order_out, keep_out, desc_out, ncrop_out, workspace, RoLineOut{nullptr, nullptr, nullptr, 0}, stream);
}

extern "C" int msocr_reading_order_line_rows(int max_cand) { return max_cand < RO_MAXLINES ? max_cand : RO_MAXLINES; }

extern "C" int msocr_reading_order_lines(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                                         int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                         int page_base, int32_t* order_out, int32_t* keep_out, int32_t* desc_out,
                                         int32_t* ncrop_out, int32_t* line_out, int32_t* lines_out, int32_t* nlines_out,
                                         void* workspace, void* stream) {
  if (!line_out || !lines_out || !nlines_out) return MSOCR_E_ARG;
  return ro_launch<true>(boxes, nbox, N, max_cand, page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base,
                         order_out, keep_out, desc_out, ncrop_out, workspace,
                         RoLineOut{line_out, lines_out, nlines_out, msocr_reading_order_line_rows(max_cand)}, stream);
}

extern "C" int64_t msocr_reading_order_deskew_workspace_bytes(int N, int max_cand) {
  return (N > 0 && max_cand > 0) ? (int64_t)N * (ro_ws_words(ro_cap(max_cand)) + 4L * ro_cap(max_cand)) * 4 : 0;
}

extern "C" int msocr_reading_order_deskew(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                                          int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                          int page_base, int32_t* order_out, int32_t* keep_out, int32_t* desc_out,
                                          int32_t* ncrop_out, int32_t* line_out, int32_t* lines_out, int32_t* nlines_out,
                                          int64_t* skew_out, double* cs_out, void* workspace, void* stream) {
  if (!skew_out || !cs_out) return MSOCR_E_ARG;
  const int given = (line_out ? 1 : 0) + (lines_out ? 1 : 0) + (nlines_out ? 1 : 0);
  if (given != 0 && given != 3) return MSOCR_E_ARG;  // the line outputs: all three or none
  const RoSkewOut so{skew_out, cs_out};
  if (given == 0)
    return ro_launch<false, true>(boxes, nbox, N, max_cand, page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio,
                                  page_base, order_out, keep_out, desc_out, ncrop_out, workspace, RoLineOut{nullptr, nullptr, nullptr, 0},
                                  stream, so);
  return ro_launch<true, true>(boxes, nbox, N, max_cand, page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base,
                               order_out, keep_out, desc_out, ncrop_out, workspace,
                               RoLineOut{line_out, lines_out, nlines_out, msocr_reading_order_line_rows(max_cand)}, stream, so);
}
