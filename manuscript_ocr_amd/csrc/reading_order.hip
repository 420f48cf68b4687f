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
// msocr_reading_order_regions launches it with REGIONS = true (Pipeline.columns): between the shrink and the
// line walk an XY-cut splits the page at its wide empty bands into regions, level by level over the whole workgroup; a line then
// belongs to one region, takes its tolerances from that region's mean height, and the lines are ordered region-major.  Bit-identical
// to msocr_reading_regions_host.
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
#include "page_regions.h"
#include "page_skew.h"
#include "word_boxes.h"

namespace {
constexpr int RO_T = 1024;         // threads per page
constexpr int RO_CAP = 16384;      // boxes per page
constexpr int RO_MAXLINES = 4096;  // text lines per page (line state lives in LDS)
constexpr int RO_MAXREGIONS = 256; // regions per page (REGIONS; the region tables live in LDS)

__host__ __device__ inline int ro_cap(int max_cand) { return max_cand < RO_CAP ? max_cand : RO_CAP; }
__host__ __device__ inline long ro_pair_cap(int cap) { return 8L * cap + 4096; }
// per-page workspace in 4-byte words: ob[4c] sb[4c] cnt[c+4] pairs[2P] sorted[c] lineof[c] seq[c] emitted[c] keepf[c]
__host__ __device__ inline long ro_ws_words(int cap) { return (4L * cap + 4L * cap + (cap + 4) + 2 * ro_pair_cap(cap) + 5L * cap + 3) / 4 * 4; }
// REGIONS, behind the ordering boxes rb[4c] of DESKEW (reserved with or without it): reg[c] regn[c] startf[c]
__host__ __device__ inline long ro_region_words(int cap) { return (3L * cap + 3) / 4 * 4; }

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

// the page's regions as a result, and the thresholds of the cut (msocr_reading_order_regions); unused and compiled out with REGIONS = false
struct RoRegionOut {
  int32_t* region;    // [N][max_cand]
  int32_t* regions;   // [N][rows][6]
  int32_t* nregions;  // [N]
  int rows;
  double col_gap_ratio, row_gap_ratio, col_min_height_ratio;
};

// REGIONS: the region of every line and the tables of the regions, in LDS
struct RoRegionLds {
  int lreg[RO_MAXLINES];
  int lo[RO_MAXREGIONS], hi[RO_MAXREGIONS];    // the cut: min y0 / max y1 of the region;  the records: min x0 / max x1
  int lo2[RO_MAXREGIONS], hi2[RO_MAXREGIONS];  // the records: min y0 / max y1
  int axis[RO_MAXREGIONS];                     // the attempt of this level: 0 = vertical (walk along x), 1 = horizontal (along y)
  int nseg[RO_MAXREGIONS];                     // start words the attempt found: more than one = the region is cut
  int base[RO_MAXREGIONS];                     // the cut: ordinal of the region's first child;  the records: its first position
  int cnt[RO_MAXREGIONS];                      // words of the region
  unsigned long long hsum[RO_MAXREGIONS];      // exact sum of their shrunk heights (two's complement)
  double tol[RO_MAXREGIONS], gap[RO_MAXREGIONS];
  int nreg, cut;
};
__device__ __forceinline__ RoRegionLds& ro_region_lds() {
  __shared__ RoRegionLds s;
  return s;
}

// REGIONS: one attempt of a level over the regions whose axis[] is `ax`.  Every word of such a region finds the running maximum of
// the high edges of the words before it in (low edge, index) and whether it starts a segment (startf[]); nseg[] counts the starts.
__device__ __forceinline__ void ro_region_attempt(RoRegionLds& g, int ax, double thr, const Box4* sb, const int* reg, int* startf, int n) {
  for (int i = threadIdx.x; i < n; i += RO_T) {
    const int r = reg[i];
    if (g.axis[r] != ax) continue;
    const Box4 a = sb[i];
    const int li = ax ? a.y0 : a.x0;
    bool has = false;
    int run = 0;
    for (int j = 0; j < n; ++j) {
      if (reg[j] != r) continue;
      const Box4 b = sb[j];
      const int lj = ax ? b.y0 : b.x0, hj = ax ? b.y1 : b.x1;
      if (region_before(lj, j, li, i)) {
        run = has ? max(run, hj) : hj;
        has = true;
      }
    }
    const int st = (!has || region_gap(li, run, thr)) ? 1 : 0;
    startf[i] = st;
    if (st) atomicAdd(&g.nseg[r], 1);
  }
  __threadfence();
  __syncthreads();
}

template <bool LINES, bool DESKEW, bool REGIONS>
__global__ __launch_bounds__(RO_T) void reading_order_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ nbox,
                                                              int max_cand, int cap, int page_h, int page_w, int min_text,
                                                              int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                                              int page_base, int32_t* __restrict__ order_out,
                                                              int32_t* __restrict__ keep_out, int32_t* __restrict__ desc_out,
                                                              int32_t* __restrict__ ncrop_out, int32_t* __restrict__ ws, RoLineOut lo,
                                                              RoSkewOut so, RoRegionOut go) {
  const int pg = blockIdx.x, tid = threadIdx.x;
  const int n = nbox[pg];
  __shared__ long long skew_s[4];  // DESKEW: {S2x, S2y, m, applied}, written out with the verdict of a page that is not flagged
  __shared__ double cs_s[2];
  // the page's verdict: crops (and lines) of the page, 0 for an empty page, -1 = the host path takes it
  auto verdict = [&](int ncrop, int nlines, int nregions) {
    if (tid == 0) {
      ncrop_out[pg] = ncrop;
      if constexpr (LINES) lo.nlines[pg] = nlines;
      if constexpr (REGIONS) go.nregions[pg] = nregions;
      if constexpr (DESKEW)
        if (ncrop >= 0) {
          for (int k = 0; k < 4; ++k) so.skew[4 * (long)pg + k] = (n > 0 ? skew_s[k] : 0LL);
          so.cs[2 * (long)pg] = n > 0 ? cs_s[0] : 1.0;
          so.cs[2 * (long)pg + 1] = n > 0 ? cs_s[1] : 0.0;
        }
    }
  };
  if (n < 0 || n > cap) {
    verdict(-1, -1, -1);
    return;
  }
  if (n == 0) {
    verdict(0, 0, 0);
    return;
  }
  int32_t* w = ws + (long)pg * (ro_ws_words(cap) + (DESKEW || REGIONS ? 4L * cap : 0L) + (REGIONS ? ro_region_words(cap) : 0L));
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
    verdict(-1, -1, -1);
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
  int* reg = nullptr;  // REGIONS: the region of every word
  if constexpr (REGIONS) {
    // ---- XY-cut (msocr.h, msocr_reading_order_regions): at most RG_MAXDEPTH levels; at every level each region tries the vertical
    // cut where it is tall enough, else (or where that found one segment) the horizontal one.  A region that is not cut is tried
    // again at the next level with the same outcome, so its depth never grows and no leaf flag is kept; the children take the
    // parent's place in the numbering, so the ordinal is the depth-first leaf order.
    RoRegionLds& g = ro_region_lds();
    reg = w + ro_ws_words(cap) + 4L * cap;
    int* regn = reg + cap;
    int* startf = regn + cap;
    const RegionParams rp = region_params(avg_h, go.col_gap_ratio, go.row_gap_ratio, go.col_min_height_ratio);
    for (int i = tid; i < n; i += RO_T) reg[i] = 0;
    if (tid == 0) g.nreg = 1;
    __threadfence();
    __syncthreads();
    for (int level = 0; level < RG_MAXDEPTH; ++level) {
      const int nreg = g.nreg;
      for (int r = tid; r < nreg; r += RO_T) { g.lo[r] = INT32_MAX; g.hi[r] = INT32_MIN; g.nseg[r] = 0; }
      __syncthreads();
      for (int i = tid; i < n; i += RO_T) {
        const int r = reg[i];
        atomicMin(&g.lo[r], sb[i].y0);
        atomicMax(&g.hi[r], sb[i].y1);
      }
      __syncthreads();
      for (int r = tid; r < nreg; r += RO_T) g.axis[r] = region_tall(g.lo[r], g.hi[r], rp.col_min_h) ? 0 : 1;
      __syncthreads();
      ro_region_attempt(g, 0, rp.col_gap, sb, reg, startf, n);
      for (int r = tid; r < nreg; r += RO_T)
        if (g.axis[r] == 0 && g.nseg[r] <= 1) { g.axis[r] = 1; g.nseg[r] = 0; }
      __syncthreads();
      ro_region_attempt(g, 1, rp.row_gap, sb, reg, startf, n);
      if (tid == 0) {
        int run = 0, cut = 0;
        for (int r = 0; r < nreg; ++r) {
          g.base[r] = run;
          const int kids = g.nseg[r] > 1 ? g.nseg[r] : 1;
          cut |= kids > 1 ? 1 : 0;
          run = run + kids > RO_MAXREGIONS ? RO_MAXREGIONS + 1 : run + kids;  // saturates: nseg may be n in every region
        }
        g.cut = cut;
        g.nreg = run;
        if (run > RO_MAXREGIONS) fail_s = 1;
      }
      __syncthreads();
      if (fail_s || !g.cut) break;
      // the segment of a word = the start words of its region at or before it, less one
      for (int i = tid; i < n; i += RO_T) {
        const int r = reg[i];
        int seg = 0;
        if (g.nseg[r] > 1) {
          const int ax = g.axis[r];
          const int li = ax ? sb[i].y0 : sb[i].x0;
          for (int j = 0; j < n; ++j)
            if (reg[j] == r && startf[j]) {
              const int lj = ax ? sb[j].y0 : sb[j].x0;
              seg += (j == i || region_before(lj, j, li, i)) ? 1 : 0;
            }
          seg -= 1;
        }
        regn[i] = g.base[r] + seg;
      }
      __threadfence();
      __syncthreads();
      for (int i = tid; i < n; i += RO_T) reg[i] = regn[i];
      __threadfence();
      __syncthreads();
    }
    __syncthreads();
    if (fail_s) {
      verdict(-1, -1, -1);
      return;
    }
    // every region's own mean height: the tolerances of its lines
    const int nreg = g.nreg;
    for (int r = tid; r < nreg; r += RO_T) { g.hsum[r] = 0ULL; g.cnt[r] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += RO_T) {
      const int r = reg[i];
      atomicAdd(&g.hsum[r], (unsigned long long)(long long)(sb[i].y1 - sb[i].y0));
      atomicAdd(&g.cnt[r], 1);
    }
    __syncthreads();
    for (int r = tid; r < nreg; r += RO_T) {
      const double ah = (double)(long long)g.hsum[r] / (double)g.cnt[r];
      g.tol[r] = ah * y_tol_ratio;
      g.gap[r] = ah * x_gap_ratio;
    }
    __syncthreads();
  }
  if (tid < 64) {  // one wave walks the cy-sorted boxes; its lanes test 64 lines at a time, the FIRST matching line wins
    const int lane = tid;
    int L = 0;
    bool over = false;
    for (int s = 0; s < n && !over; ++s) {
      const int i = sorted[s];
      const Box4 b = sb[i];
      const double c = (double)(b.y0 + b.y1) / 2.0;
      int ri = 0;
      double tol_i = tol, gap_i = gap;
      if constexpr (REGIONS) {
        ri = reg[i];
        tol_i = ro_region_lds().tol[ri];
        gap_i = ro_region_lds().gap[ri];
      }
      int home = -1;
      for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        bool ok = false;
        if (l < L) {
          const double line_cy = lsum[l] / (double)lcnt[l];
          ok = fabs(c - line_cy) <= tol_i && (double)(b.x0 - lmaxx[l]) <= gap_i;
          if constexpr (REGIONS) ok = ok && ro_region_lds().lreg[l] == ri;
        }
        const unsigned long long bal = __ballot(ok);
        if (bal) { home = l0 + (int)__ffsll((long long)bal) - 1; break; }
      }
      if (home < 0) {
        if (L >= RO_MAXLINES) { over = true; break; }
        if (lane == 0) {
          lsum[L] = c; lcnt[L] = 1; lmaxx[L] = b.x1; lineof[i] = L;
          if constexpr (REGIONS) ro_region_lds().lreg[L] = ri;
        }
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
    verdict(-1, -1, -1);
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
      bool front = mk < m || (mk == m && k < l);
      if constexpr (REGIONS) {  // region-major
        const int rk = ro_region_lds().lreg[k], rl = ro_region_lds().lreg[l];
        front = rk < rl || (rk == rl && front);
      }
      if (front) {
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
  if constexpr (REGIONS) {
    // the region of every position, and one record per region: its span of positions (the positions are region-major) and the
    // union of the words' original AABBs (oo[] is complete: the barrier above)
    RoRegionLds& g = ro_region_lds();
    const int nreg = g.nreg;
    int32_t* rno = go.region + (long)pg * max_cand;
    int32_t* rec = go.regions + (long)pg * go.rows * 6;  // nreg <= min(n, RO_MAXREGIONS) <= rows
    for (int r = tid; r < nreg; r += RO_T) {
      g.lo[r] = INT32_MAX; g.hi[r] = INT32_MIN; g.lo2[r] = INT32_MAX; g.hi2[r] = INT32_MIN;
      int first = 0;
      for (int k = 0; k < r; ++k) first += g.cnt[k];
      g.base[r] = first;
    }
    __syncthreads();
    for (int pos = tid; pos < n; pos += RO_T) {
      const int r = reg[emitted[pos]];
      const Box4 b = ob[oo[pos]];
      rno[pos] = r;
      atomicMin(&g.lo[r], b.x0); atomicMax(&g.hi[r], b.x1); atomicMin(&g.lo2[r], b.y0); atomicMax(&g.hi2[r], b.y1);
    }
    __syncthreads();
    for (int r = tid; r < nreg; r += RO_T) {
      int32_t* t = rec + 6 * (long)r;
      t[0] = g.base[r]; t[1] = g.cnt[r]; t[2] = g.lo[r]; t[3] = g.lo2[r]; t[4] = g.hi[r]; t[5] = g.hi2[r];
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
  int nregions = 0;
  if constexpr (REGIONS) nregions = ro_region_lds().nreg;
  verdict(nk, L, nregions);
}

template <bool LINES, bool DESKEW = false, bool REGIONS = false>
int ro_launch(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w, int min_text_size, int img_h,
              int img_w, double y_tol_ratio, double x_gap_ratio, int page_base, int32_t* order_out, int32_t* keep_out,
              int32_t* desc_out, int32_t* ncrop_out, void* workspace, RoLineOut lo, void* stream,
              RoSkewOut so = RoSkewOut{nullptr, nullptr}, RoRegionOut go = RoRegionOut{nullptr, nullptr, nullptr, 0, 0.0, 0.0, 0.0}) {
  if (!boxes || !nbox || !order_out || !keep_out || !desc_out || !ncrop_out || !workspace) return MSOCR_E_ARG;
  if (N <= 0 || max_cand <= 0 || page_h <= 0 || page_w <= 0 || img_h <= 0 || img_w <= 0 || page_base < 0) return MSOCR_E_ARG;
  if ((uintptr_t)workspace & 15) return MSOCR_E_ARG;
  MSOCR_LAUNCH((reading_order_kernel<LINES, DESKEW, REGIONS>), dim3(N), dim3(RO_T), 0, (hipStream_t)stream, boxes, nbox, max_cand, ro_cap(max_cand),
               page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base, order_out, keep_out, desc_out,
               ncrop_out, (int32_t*)workspace, lo, so, go);
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

extern "C" int msocr_reading_order_region_rows(int max_cand) { return max_cand < RO_MAXREGIONS ? max_cand : RO_MAXREGIONS; }

extern "C" int64_t msocr_reading_order_regions_workspace_bytes(int N, int max_cand) {
  const int cap = ro_cap(max_cand);
  return (N > 0 && max_cand > 0) ? (int64_t)N * (ro_ws_words(cap) + 4L * cap + ro_region_words(cap)) * 4 : 0;
}

extern "C" int msocr_reading_order_regions(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                                           int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio,
                                           int page_base, double col_gap_ratio, double row_gap_ratio, double col_min_height_ratio,
                                           int deskew, int32_t* order_out, int32_t* keep_out, int32_t* desc_out, int32_t* ncrop_out,
                                           int32_t* line_out, int32_t* lines_out, int32_t* nlines_out, int64_t* skew_out,
                                           double* cs_out, int32_t* region_out, int32_t* regions_out, int32_t* nregions_out,
                                           void* workspace, void* stream) {
  if (!region_out || !regions_out || !nregions_out) return MSOCR_E_ARG;
  if (!region_ratio_ok(col_gap_ratio) || !region_ratio_ok(row_gap_ratio) || !region_ratio_ok(col_min_height_ratio)) return MSOCR_E_ARG;
  if (deskew != 0 && deskew != 1) return MSOCR_E_ARG;
  if (deskew && (!skew_out || !cs_out)) return MSOCR_E_ARG;
  const int given = (line_out ? 1 : 0) + (lines_out ? 1 : 0) + (nlines_out ? 1 : 0);
  if (given != 0 && given != 3) return MSOCR_E_ARG;  // the line outputs: all three or none
  const RoSkewOut so{skew_out, cs_out};
  const RoRegionOut go{region_out, regions_out, nregions_out, msocr_reading_order_region_rows(max_cand), col_gap_ratio, row_gap_ratio,
                       col_min_height_ratio};
  const RoLineOut lo = given ? RoLineOut{line_out, lines_out, nlines_out, msocr_reading_order_line_rows(max_cand)}
                             : RoLineOut{nullptr, nullptr, nullptr, 0};
#define RO_REGIONS(L, D)                                                                                                              \
  ro_launch<L, D, true>(boxes, nbox, N, max_cand, page_h, page_w, min_text_size, img_h, img_w, y_tol_ratio, x_gap_ratio, page_base, \
                        order_out, keep_out, desc_out, ncrop_out, workspace, lo, stream, so, go)
  if (deskew) return given ? RO_REGIONS(true, true) : RO_REGIONS(false, true);
  return given ? RO_REGIONS(true, false) : RO_REGIONS(false, false);
#undef RO_REGIONS
}
