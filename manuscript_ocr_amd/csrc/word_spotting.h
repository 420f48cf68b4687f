// word_spotting.h — word spotting by example: the dynamic-time-warping distance between sequences of unit frames, Q queries against
// N indexed words, and the selection of the k nearest (include/msocr.h, "word spotting"; DESIGN.md sections 4.25, 4.28).  Host and device:
// the kernels of word_spotting.hip share the argument checks, the frame rule and the ordering key below; the host twins
// msocr_frame_normalize_host, msocr_dtw_distances_host, msocr_dtw_subsequence_host and msocr_topk_smallest_host are
// ws_normalize_host, ws_dtw_host, ws_dtw_sub_host and ws_topk_host; plain C++ programs feed them garbage lengths, non-finite features
// and heap blocks of their exact size under the address and undefined-behaviour sanitizers (tests/native/word_spotting_fuzz.cpp,
// tests/native/word_spotting_partial_fuzz.cpp).  Whatever the length arrays hold, every index formed here lies inside the arrays the
// caller described.
#ifndef MSOCR_WORD_SPOTTING_H
#define MSOCR_WORD_SPOTTING_H
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "msocr.h"

#if defined(__HIPCC__)
#define MSOCR_WS_HD __host__ __device__ __forceinline__
#else
#define MSOCR_WS_HD inline
#endif

// the shapes every entry point accepts: 1 <= T <= 64, H a multiple of 64 in 64 .. 512, count >= 0, count * T * H < 2^31
MSOCR_WS_HD bool ws_shape_ok(int64_t count, int T, int H) {
  if (count < 0 || T < 1 || T > MSOCR_SPOT_MAX_T || H < 64 || H > MSOCR_SPOT_MAX_H || (H & 63)) return false;
  return count * (int64_t)T * (int64_t)H < ((int64_t)1 << 31);
}

// a frame's squared norm decides whether it has a direction: not finite (an Inf or NaN element, or an overflow of the sum) or
// below FLT_MIN -> the zero frame, which costs 1 against everything
MSOCR_WS_HD bool ws_norm_ok(float ss) { return ss >= FLT_MIN && ss <= FLT_MAX; }

// The order of the f32 sum of squares, on the device and in the host twin alike: 64 partial sums, partial l takes the elements
// l, l + 64, l + 128, .. in ascending order, each by one fmaf; the partials are then folded by a butterfly over the lane masks
// 32, 16, 8, 4, 2, 1 (p[l] = p[l] + p[l ^ mask] for every l at once), after which all 64 hold the same sum.
inline float ws_sumsq_host(const float* x, int H) {
  float p[64], t[64];
  for (int l = 0; l < 64; ++l) {
    float s = 0.f;
    for (int e = l; e < H; e += 64) s = fmaf(x[e], x[e], s);
    p[l] = s;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = p[l] + p[l ^ m];
    memcpy(p, t, sizeof p);
  }
  return p[0];
}

// msocr_frame_normalize_host: lengths are clamped into [0, T] (the device does the same), frames t >= len are zeros and never read
inline void ws_normalize_host(const float* feat, const int32_t* len, int N, int T, int H, float* out) {
  for (int n = 0; n < N; ++n) {
    const int L = std::min(std::max(len[n], 0), T);
    for (int t = 0; t < T; ++t) {
      float* u = out + ((size_t)n * T + t) * H;
      if (t >= L) {
        for (int e = 0; e < H; ++e) u[e] = 0.f;
        continue;
      }
      const float* x = feat + ((size_t)n * T + t) * H;
      const float ss = ws_sumsq_host(x, H);
      if (!ws_norm_ok(ss)) {
        for (int e = 0; e < H; ++e) u[e] = 0.f;
        continue;
      }
      const float nrm = sqrtf(ss);
      for (int e = 0; e < H; ++e) u[e] = x[e] / nrm;
    }
  }
}

// every length inside [1, T]?
inline bool ws_lens_ok(const int32_t* len, int count, int T) {
  for (int i = 0; i < count; ++i)
    if (len[i] < 1 || len[i] > T) return false;
  return true;
}

// The definition in f64: local costs 1 - <u_i, v_j> with the products and their sum in f64 (ascending k), the table in f64, one
// rounding to f32 at the end.  a [La][H], b [Lb][H]; row is scratch of Lb doubles.
inline float ws_dtw_pair_host(const float* a, int La, const float* b, int Lb, int H, double* row) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < La; ++i) {
    double diag = inf, left = inf;  // D(i-1, j-1) and D(i, j-1)
    for (int j = 0; j < Lb; ++j) {
      double dot = 0.0;
      for (int k = 0; k < H; ++k) dot += (double)a[(size_t)i * H + k] * (double)b[(size_t)j * H + k];
      const double up = i > 0 ? row[j] : inf;
      double best = std::min(diag, std::min(up, left));
      if (i == 0 && j == 0) best = 0.0;
      diag = up;
      left = (1.0 - dot) + best;
      row[j] = left;
    }
  }
  return (float)(row[Lb - 1] / (double)(La + Lb));
}

// msocr_dtw_distances_host after its argument check
inline void ws_dtw_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                        const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist) {
  std::vector<double> row((size_t)T);
  for (int q = 0; q < Q; ++q)
    for (int n = 0; n < N; ++n) {
      const int Ln = c_len[n];
      float d = std::numeric_limits<float>::infinity();
      if (Ln >= len_lo[q] && Ln <= len_hi[q])
        d = ws_dtw_pair_host(q_unit + (size_t)q * T * H, q_len[q], c_unit + (size_t)n * T * H, Ln, H, row.data());
      dist[(size_t)q * N + n] = d;
    }
}

// ---- the subsequence form (msocr.h, "word spotting", "Subsequence distance"): the query may start and end
// anywhere on the word's axis.
// what msocr_dtw_subsequence and its host twin check alike before anything else (the device route adds the alignment of the frames)
inline bool ws_sub_args_ok(const void* q_unit, const void* q_len, const void* len_lo, const void* len_hi, int Q, const void* c_unit,
                           const void* c_len, int N, int T, int H, const void* dist, const void* span) {
  if (!ws_shape_ok(Q, T, H) || !ws_shape_ok(N, T, H)) return false;
  return q_unit && q_len && len_lo && len_hi && c_unit && c_len && dist && span;
}

// The definition in f64, as ws_dtw_pair_host forms it: S(0, j) = c(0, j) (a free start: row 0 takes no left step), S(i, j) = c(i, j) +
// min(S(i-1, j-1), S(i-1, j), S(i, j-1)); every cell carries the column at which its path left row 0: among equal predecessors the
// diagonal one wins, then the upper, then the left (strict < in that order).  The end is the smallest j that attains min_j
// S(La-1, j).  a [La][H] is the query, b [Lb][H] the word; row and start are scratch of Lb entries each.
// -> d = min / La rounded to f32 once; span[0..2) = [start, end + 1) in word frames.
inline float ws_dtw_sub_pair_host(const float* a, int La, const float* b, int Lb, int H, double* row, int32_t* start, int32_t* span) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < La; ++i) {
    double diag = inf, left = inf;  // S(i-1, j-1) and S(i, j-1)
    int32_t sdiag = -1, sleft = -1;
    for (int j = 0; j < Lb; ++j) {
      double dot = 0.0;
      for (int k = 0; k < H; ++k) dot += (double)a[(size_t)i * H + k] * (double)b[(size_t)j * H + k];
      const double up = i > 0 ? row[j] : inf;
      const int32_t sup = i > 0 ? start[j] : -1;
      double best = diag;
      int32_t st = sdiag;
      if (up < best) best = up, st = sup;
      if (left < best) best = left, st = sleft;
      if (i == 0) best = 0.0, st = j;
      diag = up;
      sdiag = sup;
      left = (1.0 - dot) + best;
      sleft = st;
      row[j] = left;
      start[j] = st;
    }
  }
  int e = 0;
  for (int j = 1; j < Lb; ++j)
    if (row[j] < row[e]) e = j;
  span[0] = start[e];
  span[1] = e + 1;
  return (float)(row[e] / (double)La);
}

// msocr_dtw_subsequence_host after its argument check: a gated-out pair is +inf and (-1, -1) without arithmetic
inline void ws_dtw_sub_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                            const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, int32_t* span) {
  std::vector<double> row((size_t)T);
  std::vector<int32_t> start((size_t)T);
  for (int q = 0; q < Q; ++q)
    for (int n = 0; n < N; ++n) {
      const int Ln = c_len[n];
      const size_t at = (size_t)q * N + n;
      dist[at] = std::numeric_limits<float>::infinity();
      span[2 * at] = span[2 * at + 1] = -1;
      if (Ln >= len_lo[q] && Ln <= len_hi[q])
        dist[at] = ws_dtw_sub_pair_host(q_unit + (size_t)q * T * H, q_len[q], c_unit + (size_t)n * T * H, Ln, H, row.data(), start.data(),
                                        span + 2 * at);
    }
}

// The order of the selection, as an unsigned key: finite floats ascending, -0.0 and +0.0 equal.  Comparisons only.
MSOCR_WS_HD bool ws_finite_bits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
MSOCR_WS_HD uint32_t ws_key_bits(uint32_t bits) {
  if ((bits << 1) == 0u) bits = 0u;  // -0.0 orders as +0.0
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
inline uint32_t ws_bits_host(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

// msocr_topk_smallest_host after its argument check: per row the k smallest finite values ascending, equal values by ascending
// index, the value copied as stored (a -0.0 stays -0.0); unused slots -1 / +inf.  May throw std::bad_alloc.
inline void ws_topk_host(const float* dist, int Q, int N, int k, int32_t* idx, float* val) {
  std::vector<uint64_t> keys;
  for (int q = 0; q < Q; ++q) {
    const float* row = dist + (size_t)q * N;
    keys.clear();
    for (int i = 0; i < N; ++i) {
      const uint32_t b = ws_bits_host(row[i]);
      if (ws_finite_bits(b)) keys.push_back(((uint64_t)ws_key_bits(b) << 32) | (uint32_t)i);
    }
    const size_t kk = std::min((size_t)k, keys.size());
    std::partial_sort(keys.begin(), keys.begin() + kk, keys.end());
    for (int s = 0; s < k; ++s) {
      const bool used = (size_t)s < kk;
      const int32_t i = used ? (int32_t)(keys[s] & 0xffffffffu) : -1;
      idx[(size_t)q * k + s] = i;
      val[(size_t)q * k + s] = used ? row[i] : std::numeric_limits<float>::infinity();
    }
  }
}

#endif
