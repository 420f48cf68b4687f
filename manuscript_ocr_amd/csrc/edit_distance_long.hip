// edit_distance_long.hip — msocr_edit_distance_long: the exact Levenshtein distance of N pairs of int32 token sequences of up to
// MSOCR_EDL_MAX_LEN tokens each (include/msocr.h, "page-level error rates").  The recurrence and the host
// twin are csrc/edit_distance_long.h.
//
// Three kernels:
//   zero      clears the mask tables of all pairs (one range of the workspace).
//   masks     one thread per pattern token: a 64-bit atomic OR of its bit into word [token][block] of its pair's table.
//   distance  one wave (a workgroup of its own) per pair.  Lane l owns the K = ceil(nb / 64) consecutive pattern blocks from l * K
//             (K <= 4); at step s it advances them by text symbol s - l and hands the carry of its last block to lane l + 1, which
//             consumes it at step s + 1: a systolic sweep of n + lanes - 1 steps, the anti-diagonals of the block table.  The carry
//             moves by __shfl_up (one ds_bpermute per step; nothing goes through memory and no barrier is needed: one wave).  The
//             text is staged in LDS (64 KB at the cap), so that the symbol of a later step costs an LDS read: the mask words of step
//             s + EDL_AHEAD are loaded while step s computes, which hides most of the latency of a load a wave would otherwise wait
//             out every step.  A batch of a few long pairs occupies a few waves of the chip and is latency-bound: accepted
//             (an evaluation call; splitting a pair over several waves is not provided).
#include <new>
#include <stdexcept>
#include <vector>

#include "edit_distance_long.h"
#include "internal.h"

namespace {

constexpr int EDL_AHEAD = 4;      // steps between the load of a mask word and its use
constexpr int EDL_ZERO_T = 256;
constexpr int EDL_MASK_T = 256;

__global__ __launch_bounds__(EDL_ZERO_T) void edl_zero_kernel(uint64_t* __restrict__ tab, long words) {
  const long stride = (long)gridDim.x * EDL_ZERO_T;
  for (long i = (long)blockIdx.x * EDL_ZERO_T + threadIdx.x; i < words; i += stride) tab[i] = 0ull;
}

__global__ __launch_bounds__(EDL_MASK_T) void edl_masks_kernel(const edl_pair* __restrict__ heads, const int32_t* __restrict__ a_tok,
                                                               uint64_t* __restrict__ tab) {
  const edl_pair p = heads[blockIdx.x];
  const int j = blockIdx.y * EDL_MASK_T + threadIdx.x;
  if (j >= p.m) return;
  const int32_t c = a_tok[(size_t)p.a0 + j];
  if (c < 0 || c >= p.v) return;
  atomicOr((unsigned long long*)(tab + p.tab + (int64_t)c * p.nb + (j >> 6)), 1ull << (j & 63));
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

template <int K>
__device__ __forceinline__ void edl_sweep(const edl_pair& p, const uint64_t* __restrict__ tab, const int32_t* tx, int lane,
                                          int32_t* __restrict__ dist) {
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
            h = edl_advance(pv[j], mv[j], eq[d][j], h, top[j]);
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

__global__ __launch_bounds__(64) void edl_distance_kernel(const edl_pair* __restrict__ heads, const int32_t* __restrict__ b_tok,
                                                          const uint64_t* __restrict__ tabs, int32_t* __restrict__ dist) {
  extern __shared__ int32_t edl_text[];  // [n] of this pair
  const edl_pair p = heads[blockIdx.x];
  const int lane = threadIdx.x;
  if (p.m <= 0 || p.n <= 0) {  // uniform over the wave
    if (lane == 0) dist[blockIdx.x] = p.m <= 0 ? p.n : p.m;
    return;
  }
  for (int i = lane; i < p.n; i += 64) edl_text[i] = b_tok[(size_t)p.b0 + i];
  __syncthreads();
  const uint64_t* tab = tabs + p.tab;
  int32_t* out = dist + blockIdx.x;
  switch ((p.nb + 63) >> 6) {
    case 1: edl_sweep<1>(p, tab, edl_text, lane, out); break;
    case 2: edl_sweep<2>(p, tab, edl_text, lane, out); break;
    case 3: edl_sweep<3>(p, tab, edl_text, lane, out); break;
    default: edl_sweep<4>(p, tab, edl_text, lane, out); break;
  }
}

}  // namespace

extern "C" int64_t msocr_edit_distance_long_ws_bytes(const int32_t* a_off_host, const int32_t* b_off_host, const int32_t* v_host, int N) {
  const int64_t bytes = edl_check_heads(a_off_host, b_off_host, v_host, N);
  return bytes < 0 ? MSOCR_E_ARG : bytes;
}

extern "C" int msocr_edit_distance_long(const int32_t* a_tok, const int32_t* a_off_host, const int32_t* b_tok, const int32_t* b_off_host,
                                        const int32_t* v_host, int N, int32_t* dist_out, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const int64_t need = edl_check_heads(a_off_host, b_off_host, v_host, N);
  if (need < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok || !b_tok || !dist_out || !workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return MSOCR_E_ARG;
  std::vector<edl_pair> heads;
  try {
    heads.resize((size_t)N);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  edl_fill_heads(a_off_host, b_off_host, v_host, N, heads.data());
  int max_m = 0, max_n = 0;
  for (const edl_pair& h : heads) {
    max_m = h.m > max_m ? h.m : max_m;
    max_n = h.n > max_n ? h.n : max_n;
  }
  const long words = (long)((need - (int64_t)N * (int64_t)sizeof(edl_pair)) / 8);
  hipStream_t s = (hipStream_t)stream;
  edl_pair* heads_dev = (edl_pair*)workspace;
  uint64_t* tabs = (uint64_t*)(heads_dev + N);
  // the heads leave a host buffer of this call: wait for the copy before it goes (the kernels behind it do not block the host)
  if (hipMemcpyAsync(heads_dev, heads.data(), (size_t)N * sizeof(edl_pair), hipMemcpyHostToDevice, s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return MSOCR_E_LAUNCH;
  int rc;
  if (words > 0) {
    const long want = (words + EDL_ZERO_T - 1) / EDL_ZERO_T;
    MSOCR_LAUNCH(edl_zero_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(EDL_ZERO_T), 0, s, tabs, words);
    if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
    MSOCR_LAUNCH(edl_masks_kernel, dim3(N, (max_m + EDL_MASK_T - 1) / EDL_MASK_T), dim3(EDL_MASK_T), 0, s, heads_dev, a_tok, tabs);
    if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  }
  const int lds = max_n * (int)sizeof(int32_t);  // <= 64 KB
  if ((rc = msocr_internal_lds_limit((const void*)edl_distance_kernel, MSOCR_EDL_MAX_LEN * (int)sizeof(int32_t))) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(edl_distance_kernel, dim3(N), dim3(64), lds, s, heads_dev, b_tok, tabs, dist_out);
  return LAUNCH_OK();
}

extern "C" int msocr_edit_distance_long_host(const int32_t* a_tok_host, const int32_t* a_off_host, const int32_t* b_tok_host,
                                             const int32_t* b_off_host, const int32_t* v_host, int N, int32_t* dist_out) {
  if (edl_check_heads(a_off_host, b_off_host, v_host, N) < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok_host || !b_tok_host || !dist_out) return MSOCR_E_ARG;
  std::vector<uint64_t> tab, pv(MSOCR_EDL_MAX_BLOCKS), mv(MSOCR_EDL_MAX_BLOCKS);
  for (int p = 0; p < N; ++p) {
    const int m = a_off_host[p + 1] - a_off_host[p], n = b_off_host[p + 1] - b_off_host[p];
    const int32_t *a = a_tok_host + a_off_host[p], *b = b_tok_host + b_off_host[p];
    if (m == 0 || n == 0) {
      dist_out[p] = m == 0 ? n : m;
      continue;
    }
    try {
      tab.resize((size_t)edl_table_words(m, v_host[p]) + 1);
    } catch (const std::bad_alloc&) {  // an alphabet far beyond the pattern's tokens: no memory for its table
      return MSOCR_E_ARG;
    } catch (const std::length_error&) {
      return MSOCR_E_ARG;
    }
    edl_build_table_host(a, m, v_host[p], tab.data());
    dist_out[p] = edl_distance_host(tab.data(), m, v_host[p], b, n, pv.data(), mv.data());
  }
  return MSOCR_OK;
}
