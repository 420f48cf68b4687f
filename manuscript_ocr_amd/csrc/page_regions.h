// page_regions.h — the comparisons of the column-aware reading order (Pipeline.columns), written once for
// reading_order_kernel and its host twin msocr_reading_regions_host.  The XY-cut splits a set of words at every empty band that is at
// least a threshold wide; differences of int32 coordinates are formed in 64 bits (a box of a non-finite corner lies at INT_MIN) and
// compared as f64, without contraction (compile with -ffp-contract=off).
#pragma once
#include "word_boxes.h"

constexpr int RG_MAXDEPTH = 6;  // a region at this depth is a leaf

struct RegionParams { double col_gap, row_gap, col_min_h; };  // the three ratios, times the page's mean shrunk height

// NaN or a negative ratio is refused; +inf is taken and never cuts
WB_HD bool region_ratio_ok(double r) { return r >= 0.0; }

WB_HD RegionParams region_params(double avg_h, double col_gap_ratio, double row_gap_ratio, double col_min_height_ratio) {
  return RegionParams{col_gap_ratio * avg_h, row_gap_ratio * avg_h, col_min_height_ratio * avg_h};
}

// the vertical attempt is allowed: the region is at least mh tall (a band one line high is never split at its word spaces)
WB_HD bool region_tall(int min_y0, int max_y1, double mh) { return (double)((long long)max_y1 - (long long)min_y0) >= mh; }

// a word starts a new segment: its low edge lies at least g behind the running maximum of the high edges before it
WB_HD bool region_gap(int lo, int run_max, double g) { return (double)((long long)lo - (long long)run_max) >= g; }

// the walk's order on an axis: (low edge, word index)
WB_HD bool region_before(int lo_a, int a, int lo_b, int b) { return lo_a < lo_b || (lo_a == lo_b && a < b); }
