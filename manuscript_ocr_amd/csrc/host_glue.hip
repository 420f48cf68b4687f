// host_glue.hip — HOST-side helper of the Pipeline glue (no device code): reading order of the word boxes of a page.
//
// The reference does this in pure Python per page (an O(n^2) shrink loop of up to 50 sweeps plus a line-grouping loop);
// after the GPU offload that Python became the longest host stage between "boxes arrive" and "recogniser enqueued"
// (4 ms per 480-word page), i.e. device idle time.  Same integer / double arithmetic, literally the reference's loops:
//   detectors/_east/utils.py:500-547 (resolve_intersections), :550-607 (sort_boxes_reading_order),
//   :610-644 (sort_boxes_reading_order_with_resolutions: dict(zip(shrunk, boxes)) — later duplicate wins),
//   _pipeline.py:113-121 (re-match a sorted box to the FIRST word with an equal box).
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "msocr.h"
#include "page_regions.h"
#include "page_skew.h"
#include "word_boxes.h"

namespace {
struct BoxLess {  // the order of the std::map keys (any strict total order of the four coordinates serves)
  bool operator()(const Box4& a, const Box4& b) const { return std::tie(a.x0, a.y0, a.x1, a.y1) < std::tie(b.x0, b.y0, b.x1, b.y1); }
};

// The XY-cut of msocr_reading_regions_host (msocr.h), literally: `words` (ascending indices) is a region at `depth`; its leaves are
// appended to `leaves` in depth-first order.  The comparisons are page_regions.h's, the kernel's.
void region_cut(const std::vector<Box4>& b, const std::vector<int>& words, int depth, const RegionParams& rp,
                std::vector<std::vector<int>>& leaves) {
  if (depth < RG_MAXDEPTH && words.size() > 1) {
    int min_y0 = b[words[0]].y0, max_y1 = b[words[0]].y1;
    for (int i : words) { min_y0 = std::min(min_y0, b[i].y0); max_y1 = std::max(max_y1, b[i].y1); }
    for (int ax = 0; ax < 2; ++ax) {  // the vertical attempt (a walk along x), then the horizontal one
      if (ax == 0 && !region_tall(min_y0, max_y1, rp.col_min_h)) continue;
      auto lo = [&](int i) { return ax ? b[i].y0 : b[i].x0; };
      auto hi = [&](int i) { return ax ? b[i].y1 : b[i].x1; };
      std::vector<int> walk(words);
      std::sort(walk.begin(), walk.end(), [&](int u, int v) { return region_before(lo(u), u, lo(v), v); });
      std::vector<std::vector<int>> segs;
      int run = 0;  // the maximum of the high edges of the words before the current one
      for (int i : walk) {
        if (segs.empty() || region_gap(lo(i), run, ax ? rp.row_gap : rp.col_gap)) segs.emplace_back();
        run = i == walk[0] ? hi(i) : std::max(run, hi(i));
        segs.back().push_back(i);
      }
      if (segs.size() > 1) {
        for (std::vector<int>& seg : segs) {
          std::sort(seg.begin(), seg.end());
          region_cut(b, seg, depth + 1, rp, leaves);
        }
        return;
      }
    }
  }
  leaves.push_back(words);
}

// The sequential twin of reading_order_kernel's ordering: box test, shrink and equality are the kernel's (word_boxes.h); sums and
// differences of coordinates are formed in 64 bits, so it is defined for any int32 boxes.  With line_out / lines_out / nlines_out
// (all three or none) the text lines the order is built from leave as well: the line index of every position and one record
// {first, count, x0, y0, x1, y1} per line, the box being the union of the original boxes of the words written at its positions.
// With `ratios` (col_gap_ratio, row_gap_ratio, col_min_height_ratio) the page is cut into regions first and the rule runs inside
// every leaf with the leaf's own mean height; the region outputs are then written like the line outputs.
int reading_order_body(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio, int32_t* order_out_host,
                       int32_t* line_out, int32_t* lines_out, int32_t* nlines_out, const double* ratios = nullptr,
                       int32_t* region_out = nullptr, int32_t* regions_out = nullptr, int32_t* nregions_out = nullptr) {
  if (n < 0 || (n > 0 && (!boxes_host || !order_out_host))) return MSOCR_E_ARG;
  if (nlines_out) *nlines_out = 0;
  if (nregions_out) *nregions_out = 0;
  if (n == 0) return MSOCR_OK;
  std::vector<Box4> orig(n), b(n);
  for (int i = 0; i < n; ++i) orig[i] = b[i] = Box4{boxes_host[4 * i], boxes_host[4 * i + 1], boxes_host[4 * i + 2], boxes_host[4 * i + 3]};
  // resolve_intersections: both members of every intersecting pair shrink by 10 % towards their top-left corner
  for (int sweep = 0; sweep < 50; ++sweep) {
    bool dirty = false;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) {
        if (!box_hit(b[i], b[j])) continue;
        box_shrink(b[i]);
        box_shrink(b[j]);
        dirty = true;
      }
    if (!dirty) break;
  }
  // dict(zip(shrunk, boxes)): identical shrunk boxes collapse, the later original wins;  first word with an equal box
  std::map<Box4, int, BoxLess> back, first;
  for (int i = 0; i < n; ++i) back[b[i]] = i;
  for (int i = n - 1; i >= 0; --i) first[orig[i]] = i;
  // the leaves of the cut in reading order; without `ratios` the page is the one leaf
  std::vector<std::vector<int>> leaves;
  {
    std::vector<int> all(n);
    for (int i = 0; i < n; ++i) all[i] = i;
    if (ratios) {
      long long hs = 0;
      for (int i = 0; i < n; ++i) hs += (long long)b[i].y1 - b[i].y0;
      region_cut(b, all, 0, region_params((double)hs / (double)n, ratios[0], ratios[1], ratios[2]), leaves);
    } else {
      leaves.push_back(all);
    }
  }
  int k = 0, rank = 0, region = 0;
  for (const std::vector<int>& leaf : leaves) {
    const int m = (int)leaf.size(), region_first = k;
    // sort_boxes_reading_order on the leaf's shrunk boxes
    double hsum = 0.0;
    for (int i : leaf) hsum += (double)((long long)b[i].y1 - b[i].y0);
    const double avg_h = hsum / m, tol = avg_h * y_tol_ratio, gap = avg_h * x_gap_ratio;
    std::vector<int> idx(leaf);
    auto cy = [&](int i) { return (double)((long long)b[i].y0 + b[i].y1) / 2.0; };
    std::stable_sort(idx.begin(), idx.end(), [&](int u, int v) { return cy(u) < cy(v); });
    std::vector<std::vector<int>> lines;
    std::vector<double> sums;
    std::vector<int> maxx;
    for (int i : idx) {
      const double c = cy(i);
      int home = -1;
      for (size_t li = 0; li < lines.size(); ++li) {
        const double line_cy = sums[li] / (double)lines[li].size();
        if (fabs(c - line_cy) <= tol && (double)((long long)b[i].x0 - maxx[li]) <= gap) { home = (int)li; break; }
      }
      if (home < 0) {
        lines.push_back({i}); sums.push_back(c); maxx.push_back(b[i].x1);
      } else {
        lines[home].push_back(i); sums[home] += c; maxx[home] = std::max(maxx[home], b[i].x1);
      }
    }
    std::vector<int> lorder(lines.size());
    for (size_t li = 0; li < lines.size(); ++li) lorder[li] = (int)li;
    std::stable_sort(lorder.begin(), lorder.end(),
                     [&](int u, int v) { return sums[u] / (double)lines[u].size() < sums[v] / (double)lines[v].size(); });
    for (int li : lorder) {
      std::vector<int>& ln = lines[li];
      std::stable_sort(ln.begin(), ln.end(), [&](int u, int v) { return b[u].x0 < b[v].x0; });
      const int start = k;
      for (int i : ln) order_out_host[k++] = first[orig[back[b[i]]]];
      if (nlines_out) {
        Box4 u = orig[order_out_host[start]];
        for (int pos = start; pos < k; ++pos) {
          const Box4& o = orig[order_out_host[pos]];
          u.x0 = std::min(u.x0, o.x0); u.y0 = std::min(u.y0, o.y0); u.x1 = std::max(u.x1, o.x1); u.y1 = std::max(u.y1, o.y1);
          line_out[pos] = rank;
        }
        const int32_t rec[6] = {start, k - start, u.x0, u.y0, u.x1, u.y1};
        std::copy(rec, rec + 6, lines_out + 6 * (long)rank);
      }
      ++rank;
    }
    if (nregions_out) {
      Box4 u = orig[order_out_host[region_first]];
      for (int pos = region_first; pos < k; ++pos) {
        const Box4& o = orig[order_out_host[pos]];
        u.x0 = std::min(u.x0, o.x0); u.y0 = std::min(u.y0, o.y0); u.x1 = std::max(u.x1, o.x1); u.y1 = std::max(u.y1, o.y1);
        region_out[pos] = region;
      }
      const int32_t rec[6] = {region_first, k - region_first, u.x0, u.y0, u.x1, u.y1};
      std::copy(rec, rec + 6, regions_out + 6 * (long)region);
    }
    ++region;
  }
  if (nlines_out) *nlines_out = rank;
  if (nregions_out) *nregions_out = region;
  return MSOCR_OK;
}
}  // namespace

extern "C" int msocr_reading_order_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio,
                                        int32_t* order_out_host) {
  return reading_order_body(boxes_host, n, y_tol_ratio, x_gap_ratio, order_out_host, nullptr, nullptr, nullptr);
}

extern "C" int msocr_reading_lines_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio,
                                        int32_t* order_out_host, int32_t* line_out_host, int32_t* lines_out_host,
                                        int32_t* nlines_out_host) {
  if (!nlines_out_host || (n > 0 && (!line_out_host || !lines_out_host))) return MSOCR_E_ARG;
  return reading_order_body(boxes_host, n, y_tol_ratio, x_gap_ratio, order_out_host, line_out_host, lines_out_host, nlines_out_host);
}

extern "C" int msocr_reading_regions_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio,
                                          double col_gap_ratio, double row_gap_ratio, double col_min_height_ratio,
                                          int32_t* order_out_host, int32_t* line_out_host, int32_t* lines_out_host,
                                          int32_t* nlines_out_host, int32_t* region_out_host, int32_t* regions_out_host,
                                          int32_t* nregions_out_host) {
  if (!nlines_out_host || !nregions_out_host) return MSOCR_E_ARG;
  if (n > 0 && (!line_out_host || !lines_out_host || !region_out_host || !regions_out_host)) return MSOCR_E_ARG;
  if (!region_ratio_ok(col_gap_ratio) || !region_ratio_ok(row_gap_ratio) || !region_ratio_ok(col_min_height_ratio)) return MSOCR_E_ARG;
  const double ratios[3] = {col_gap_ratio, row_gap_ratio, col_min_height_ratio};
  return reading_order_body(boxes_host, n, y_tol_ratio, x_gap_ratio, order_out_host, line_out_host, lines_out_host, nlines_out_host,
                            ratios, region_out_host, regions_out_host, nregions_out_host);
}

// --------------------------------------------------------------------------------------------- page skew
// Host twins of reading_order_kernel's DESKEW part (Pipeline.deskew): the per-word arithmetic is page_skew.h's,
// the sums are int64.  n <= 65536 keeps every product of a sum and a word inside int64 (the kernel takes at most 16384 words).
extern "C" int msocr_page_skew_host(const float* quads_host, int n, int64_t* skew_out_host, double* cs_out_host) {
  if (n < 0 || n > 65536 || !skew_out_host || !cs_out_host || (n > 0 && !quads_host)) return MSOCR_E_ARG;
  long long s1x = 0, s1y = 0, s2x = 0, s2y = 0, m = 0, qx, qy;
  for (int i = 0; i < n; ++i)
    if (skew_word(quads_host + 8 * (size_t)i, &qx, &qy)) { s1x += qx; s1y += qy; }
  for (int i = 0; i < n; ++i)
    if (skew_word(quads_host + 8 * (size_t)i, &qx, &qy) && skew_near(s1x, s1y, qx, qy)) { s2x += qx; s2y += qy; ++m; }
  const bool applied = skew_applied(s2x, s2y, m);
  skew_out_host[0] = s2x; skew_out_host[1] = s2y; skew_out_host[2] = m; skew_out_host[3] = applied ? 1 : 0;
  skew_cos_sin(s2x, s2y, applied, cs_out_host);
  return MSOCR_OK;
}

extern "C" int msocr_deskew_boxes_host(const float* quads_host, int n, int page_h, int page_w, const int64_t* skew_host,
                                       const double* cs_host, int32_t* boxes_out_host) {
  if (n < 0 || page_h <= 0 || page_w <= 0 || !skew_host || !cs_host || (n > 0 && (!quads_host || !boxes_out_host))) return MSOCR_E_ARG;
  for (int i = 0; i < n; ++i) {
    const Box4 b = deskew_box(quads_host + 8 * (size_t)i, skew_host[3] != 0, cs_host[0], cs_host[1], page_h, page_w);
    boxes_out_host[4 * (size_t)i] = b.x0; boxes_out_host[4 * (size_t)i + 1] = b.y0;
    boxes_out_host[4 * (size_t)i + 2] = b.x1; boxes_out_host[4 * (size_t)i + 3] = b.y1;
  }
  return MSOCR_OK;
}

// --------------------------------------------------------------------------------------------- lexicon
// Validator of a lexicon's prefix tree over HOST copies of its arrays (msocr.h, msocr_lexicon): what recognizers/_trba/lexicon.py calls
// once per Lexicon, since the decode entry points receive device pointers and cannot look.  Breadth-first node order makes every check
// one pass: a node's depth is known when its edges are read, because its parent (a smaller id) was read before it.
extern "C" int msocr_lexicon_check_host(const int32_t* edge_begin, const int32_t* edge_tok, const int32_t* edge_child, const uint8_t* terminal,
                                        int n_nodes, int n_edges, int V, int max_depth) {
  if (!edge_begin || !terminal || n_nodes < 1 || n_edges < 0 || V <= 0 || max_depth < 0) return MSOCR_E_ARG;
  if (n_edges > 0 && (!edge_tok || !edge_child)) return MSOCR_E_ARG;
  if (edge_begin[0] != 0 || edge_begin[n_nodes] != n_edges) return MSOCR_E_ARG;
  for (int n = 0; n < n_nodes; ++n)
    if (edge_begin[n + 1] < edge_begin[n] || edge_begin[n + 1] > n_edges) return MSOCR_E_ARG;
  std::vector<int32_t> depth((size_t)n_nodes, -1);  // -1 = no parent seen yet
  depth[0] = 0;
  for (int n = 0; n < n_nodes; ++n) {
    if (depth[n] < 0) return MSOCR_E_ARG;  // n > 0 and no smaller node points at it
    const int lo = edge_begin[n], hi = edge_begin[n + 1];
    if (lo == hi && !terminal[n]) return MSOCR_E_ARG;  // a childless node ends a word
    for (int e = lo; e < hi; ++e) {
      const int tk = edge_tok[e], ch = edge_child[e];
      if (tk < 0 || tk >= V || (e > lo && edge_tok[e - 1] >= tk)) return MSOCR_E_ARG;
      if (ch <= n || ch >= n_nodes || depth[ch] >= 0) return MSOCR_E_ARG;  // parent < child < n_nodes, one parent
      depth[ch] = depth[n] + 1;
      if (depth[ch] > max_depth) return MSOCR_E_ARG;
    }
  }
  return MSOCR_OK;
}
