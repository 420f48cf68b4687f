// edit_distance_long_kernels.h — the device code that msocr_edit_distance_long (edit_distance_long.hip) and msocr_edit_alignment
// (edit_alignment.hip) share: the two kernels that build the match-mask tables, their launch, and the systolic sweep of one wave
// over one pair, which the alignment instantiates once more with the trace stores of edit_alignment.h.  Each file that includes
// this gets kernels of its own (internal linkage).
#ifndef MSOCR_EDIT_DISTANCE_LONG_KERNELS_H
#define MSOCR_EDIT_DISTANCE_LONG_KERNELS_H
#include "edit_alignment.h"
#include "internal.h"

constexpr int EDL_AHEAD = 4;      // steps between the load of a mask word and its use
constexpr int EDL_ZERO_T = 256;
constexpr int EDL_MASK_T = 256;

static __global__ __launch_bounds__(EDL_ZERO_T) void edl_zero_kernel(uint64_t* __restrict__ tab, long words) {
  const long stride = (long)gridDim.x * EDL_ZERO_T;
  for (long i = (long)blockIdx.x * EDL_ZERO_T + threadIdx.x; i < words; i += stride) tab[i] = 0ull;
}

static __global__ __launch_bounds__(EDL_MASK_T) void edl_masks_kernel(const edl_pair* __restrict__ heads, const int32_t* __restrict__ a_tok,
                                                                      uint64_t* __restrict__ tab) {
  const edl_pair p = heads[blockIdx.x];
  const int j = blockIdx.y * EDL_MASK_T + threadIdx.x;
  if (j >= p.m) return;
  const int32_t c = a_tok[(size_t)p.a0 + j];
  if (c < 0 || c >= p.v) return;
  atomicOr((unsigned long long*)(tab + p.tab + (int64_t)c * p.nb + (j >> 6)), 1ull << (j & 63));
}

// tabs [words] <- the match masks of all N pairs (heads on the device, max_m = the longest pattern); nothing is launched for no words
static inline int edl_launch_masks(const edl_pair* heads_dev, const int32_t* a_tok, uint64_t* tabs, long words, int N, int max_m,
                                   hipStream_t s) {
  if (words <= 0) return MSOCR_OK;
  int rc;
  const long want = (words + EDL_ZERO_T - 1) / EDL_ZERO_T;
  MSOCR_LAUNCH(edl_zero_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(EDL_ZERO_T), 0, s, tabs, words);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(edl_masks_kernel, dim3(N, (max_m + EDL_MASK_T - 1) / EDL_MASK_T), dim3(EDL_MASK_T), 0, s, heads_dev, a_tok, tabs);
  return LAUNCH_OK();
}

// the mask words of this lane's K blocks for text symbol t (none outside the text)
template <int K>
__device__ __forceinline__ void edl_fetch(const uint64_t* __restrict__ tab, const int32_t* tx, int n, int v, int nb, int blk0, int t,
                                          uint64_t (&eq)[K]) {
  int32_t c = -1;
  if (t >= 0 && t < n) c = tx[t];
  const bool ok = c >= 0 && c < v;
  const uint64_t* row = tab + (int64_t)(ok ? c : 0) * nb + blk0;
#pragma unroll
  for (int j = 0; j < K; ++j) eq[j] = (ok && blk0 + j < nb) ? row[j] : 0ull;
}

// One wave over one pair.  Lane l owns the K consecutive pattern blocks from l * K; at step s it advances them by text symbol s - l
// and hands the carry of its last block to lane l + 1 (edit_distance_long.hip, "distance").  TRACE: every block also stores its
// eal_cell of the column, one 16-byte store, at trace [block][column] (trace: this pair's, [nb][n]); without it trace is not used.
template <int K, bool TRACE>
__device__ __forceinline__ void edl_sweep(const edl_pair& p, const uint64_t* __restrict__ tab, const int32_t* tx, int lane,
                                          int32_t* __restrict__ dist, eal_cell* __restrict__ trace) {
  const int m = p.m, n = p.n, v = p.v, nb = p.nb;
  const int lanes = (nb + K - 1) / K;  // lanes that own a block
  const int blk0 = lane * K;
  uint64_t pv[K], mv[K];
  int top[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    pv[j] = blk0 + j < nb ? edl_begin_pv(m, blk0 + j) : 0ull;
    mv[j] = 0ull;
    top[j] = edl_top_bit(m, blk0 + j);
  }
  const int jl = nb - 1 - blk0;  // the last block's place in this lane, if it is in 0 .. K - 1
  int score = m, hin = 1;
  uint64_t eq[EDL_AHEAD][K];
#pragma unroll
  for (int d = 0; d < EDL_AHEAD; ++d) edl_fetch<K>(tab, tx, n, v, nb, blk0, d - lane, eq[d]);
  const int steps = n + lanes - 1;
  for (int s0 = 0; s0 < steps; s0 += EDL_AHEAD) {
#pragma unroll
    for (int d = 0; d < EDL_AHEAD; ++d) {
      const int t = s0 + d - lane;  // a step past the last one finds every lane outside the text
      int h = lane == 0 ? 1 : hin;
      if (lane < lanes && t >= 0 && t < n) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (blk0 + j < nb) {
            if constexpr (TRACE) {
              eal_cell cell;
              h = eal_advance(pv[j], mv[j], eq[d][j], h, top[j], cell.d0);
              cell.pv = pv[j];
              trace[(int64_t)(blk0 + j) * n + t] = cell;  // blk0 + j < nb and 0 <= t < n: inside [nb][n]
            } else {
              h = edl_advance(pv[j], mv[j], eq[d][j], h, top[j]);
            }
            if (j == jl) score += h;
          }
        }
      }
      hin = __shfl_up(h, 1, 64);  // every lane takes part; lane l + 1 reads it at its next step, for the same text symbol
      edl_fetch<K>(tab, tx, n, v, nb, blk0, t + EDL_AHEAD, eq[d]);
    }
  }
  if (jl >= 0 && jl < K) *dist = score;
}

// the body of the two sweep kernels: one wave (a workgroup of its own) per pair, the text staged in LDS (text_lds [n])
template <bool TRACE>
__device__ __forceinline__ void edl_sweep_pair(const edl_pair& p, const int32_t* __restrict__ b_tok, const uint64_t* __restrict__ tabs,
                                               int32_t* text_lds, int32_t* __restrict__ dist, eal_cell* __restrict__ trace) {
  const int lane = threadIdx.x;
  if (p.m <= 0 || p.n <= 0) {  // uniform over the wave
    if (lane == 0) *dist = p.m <= 0 ? p.n : p.m;
    return;
  }
  for (int i = lane; i < p.n; i += 64) text_lds[i] = b_tok[(size_t)p.b0 + i];
  __syncthreads();
  const uint64_t* tab = tabs + p.tab;
  switch ((p.nb + 63) >> 6) {
    case 1: edl_sweep<1, TRACE>(p, tab, text_lds, lane, dist, trace); break;
    case 2: edl_sweep<2, TRACE>(p, tab, text_lds, lane, dist, trace); break;
    case 3: edl_sweep<3, TRACE>(p, tab, text_lds, lane, dist, trace); break;
    default: edl_sweep<4, TRACE>(p, tab, text_lds, lane, dist, trace); break;
  }
}
#endif
