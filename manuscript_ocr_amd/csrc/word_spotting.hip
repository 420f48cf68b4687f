// word_spotting.hip — msocr_frame_normalize, msocr_dtw_distances, msocr_dtw_subsequence, msocr_topk_smallest and their host twins
// (include/msocr.h, "word spotting"; DESIGN.md sections 4.25 and 4.28).  The definitions in f64, the frame rule, the ordering key and
// the argument checks are csrc/word_spotting.h.
//
// Four kernels:
//   normalize  one wave per frame: lane l sums the squares of elements l, l + 64, .. (fmaf), a butterfly folds the 64 partials, every
//              lane divides its own elements by the root.  Frames at or beyond a word's length are written as zeros and not read.
//   dtw        a workgroup of four waves owns MSOCR_SPOT_TILE = 4 corpus words, one per wave, and walks all queries (the queries of
//              its grid row).  Per pair the wave builds the cost tile with the exact f32 MFMA (v_mfma_f32_32x32x2_f32): query frames
//              are the rows (A), word frames the columns (B), K = H, one 32x32 block at a time (one to four by the two lengths).
//              Lane l holds row l & 31 of the block and loads 16 bytes of it per step, elements 8s + 4 (l >> 5) .. + 3, which it
//              feeds to four MFMAs as k = 0 / 1 of each: A and B use the same map, so every k is summed once (in the order 0..3,
//              8..11, .. on the low half of the instruction's k, 4..7, 12..15, .. on the high half).  Rows at or beyond a length
//              are fed as zeros without being read.  The block's cells inside Lq x Ln go, as 1 - acc, to the wave's own LDS tile of
//              T rows at a pitch of P floats (T rounded up to even); then the anti-diagonal wavefront: lane i owns row i, step s
//              computes cell (i, s - i), the upper neighbour is lane i - 1's last value (one DPP move per step), the diagonal one
//              is the upper neighbour of the step before, the left one the lane's own last value.  LDS address (P - 1) i + s: an
//              odd stride, no bank conflict.  Cells outside Lq x Ln are +inf by index, never by value.  No block-wide barrier: a
//              wave's LDS traffic stays in order, the waves of a workgroup never wait for each other.
//              The word frames are NOT staged in LDS: one word of the envelope's largest shape is 128 KB, and at T = 33, H = 256
//              four words (135 KB) beside the cost tiles leave one workgroup per CU.  Both operands come through L1 / L2 instead;
//              the corpus leaves HBM once per grid row of queries.
//   dtw_sub    the subsequence form on dtw's grid, cost tile (one copy of the product-and-store part, ws_cost_tile) and LDS
//              discipline: row 0 starts afresh in every column, every lane carries the start column of its cell's path beside the
//              value (a second DPP move per step), lane Lq - 1 keeps the first smallest cell of the last row with its end and start.
//   topk       one workgroup per query: a radix select over the ordering key (four passes of 8 bits, LDS histogram) finds the key
//              of rank k among the finite entries; one more pass gathers everything below it and, walking in index order, the first
//              entries equal to it; a bitonic sort of the at most 256 (key, index) pairs in LDS orders them.  Comparisons only, so
//              the result is the host twin's bit for bit.
#include <new>
#include <vector>

#include "internal.h"
#include "split_mma.h"
#include "word_spotting.h"

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_WAVES = WS_THREADS / 64;
static_assert(WS_WAVES == MSOCR_SPOT_TILE, "one wave per word of a tile");
static_assert(WS_THREADS == MSOCR_SPOT_MAX_K, "one thread per slot of the selection");

__global__ __launch_bounds__(WS_THREADS) void ws_normalize_kernel(const float* __restrict__ feat, const int32_t* __restrict__ len, int N, int T,
                                                                  int H, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t frames = (int64_t)N * T;
  const int64_t stride = (int64_t)gridDim.x * WS_WAVES;
  for (int64_t f = (int64_t)blockIdx.x * WS_WAVES + (threadIdx.x >> 6); f < frames; f += stride) {
    const int n = (int)(f / T), t = (int)(f - (int64_t)n * T);
    const int L = min(max(len[n], 0), T);
    const float* x = feat + f * H;
    float* u = out + f * H;
    if (t >= L) {
      for (int e = lane; e < H; e += 64) u[e] = 0.f;
      continue;
    }
    float v[MSOCR_SPOT_MAX_H / 64];
    float ss = 0.f;
#pragma unroll
    for (int r = 0; r < MSOCR_SPOT_MAX_H / 64; ++r) {
      v[r] = 64 * r < H ? x[64 * r + lane] : 0.f;
      if (64 * r < H) ss = fmaf(v[r], v[r], ss);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
    const bool ok = ws_norm_ok(ss);
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int r = 0; r < MSOCR_SPOT_MAX_H / 64; ++r)
      if (64 * r < H) u[64 * r + lane] = ok ? v[r] / nrm : 0.f;
  }
}

// a wave's LDS stores stay ahead of its later LDS loads, and the other way round (in order per wave; this keeps the compiler
// from moving them)
__device__ __forceinline__ void ws_wave_lds_order() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_wave_barrier();
}

// the cells of one 32 x 32 accumulator block that lie inside Lq x Ln, as costs, into the wave's tile of pitch P
__device__ __forceinline__ void ws_store_block(float* __restrict__ tile, const f32x16& acc, int row0, int col, int Lq, int Ln, int P) {
  const int half = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = row0 + acc_row(e, half);
    if (row < Lq && col < Ln) tile[row * P + col] = 1.f - acc[e];
  }
}

// lane i's value of lane i - 1 (lane 0: `first`): one DPP move, wave_shr:1, no LDS round trip
__device__ __forceinline__ float ws_from_lane_below(float x, float first) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(x), 0x138, 0xf, 0xf, false));
}

// lane i's start column of lane i - 1 (lane 0: `first`): the same move on the integer the subsequence walk carries beside its value
__device__ __forceinline__ int ws_int_from_lane_below(int x, int first) {
  return __builtin_amdgcn_update_dpp(first, x, 0x138, 0xf, 0xf, false);
}

constexpr int WS_KGROUP = 32;  // elements of K per trip of the product loop: four 16-byte loads per operand row in flight at once

// The cost tile of one pair, for both table walks: one 32 x 32 block at a time (one accumulator: the registers this saves are waves
// per SIMD, and most pairs of words are one block); a lane's row of A / B beyond the length is fed as zeros and never read.  qbase /
// wbase: the pair's frames + 4 (lane >> 5); r = lane & 31.  The caller orders the wave's LDS traffic around it.
__device__ __forceinline__ void ws_cost_tile(float* __restrict__ tile, const float* __restrict__ qbase, const float* __restrict__ wbase,
                                             int Lq, int Ln, int H, int P, int r) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int mb = 0; mb < Lq; mb += 32)
    for (int nb = 0; nb < Ln; nb += 32) {
      const float* pa = mb + r < Lq ? qbase + (size_t)(mb + r) * H : nullptr;
      const float* pb = nb + r < Ln ? wbase + (size_t)(nb + r) * H : nullptr;
      f32x16 acc = {0};
      for (int k = 0; k < H; k += WS_KGROUP) {  // H is a multiple of 64
        f32x4 av[WS_KGROUP / 8], bv[WS_KGROUP / 8];
#pragma unroll
        for (int u = 0; u < WS_KGROUP / 8; ++u) {
          av[u] = pa ? *reinterpret_cast<const f32x4*>(pa + k + 8 * u) : zero4;
          bv[u] = pb ? *reinterpret_cast<const f32x4*>(pb + k + 8 * u) : zero4;
        }
#pragma unroll
        for (int u = 0; u < WS_KGROUP / 8; ++u) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][e], bv[u][e], acc, 0, 0, 0);
        }
      }
      ws_store_block(tile, acc, mb, nb + r, Lq, Ln, P);
    }
}

// grid (tiles of MSOCR_SPOT_TILE words, query rows), 256 threads, dynamic LDS: WS_WAVES cost tiles of T rows at a pitch of P floats
// (T rounded up to even: lane i reads word (P - 1) i + s at step s, and an odd stride puts 64 lanes on 64 banks)
__global__ __launch_bounds__(WS_THREADS) void ws_dtw_kernel(const float* __restrict__ q_unit, const int32_t* __restrict__ q_len,
                                                            const int32_t* __restrict__ len_lo, const int32_t* __restrict__ len_hi, int Q,
                                                            const float* __restrict__ c_unit, const int32_t* __restrict__ c_len, int N,
                                                            int T, int H, int P, float* __restrict__ dist) {
  extern __shared__ float tiles[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // the wave's number, in an SGPR
  const int r = lane & 31, half = lane >> 5;
  float* tile = tiles + (size_t)wave * T * P;
  const int64_t n64 = (int64_t)blockIdx.x * WS_WAVES + wave;
  if (n64 >= N) return;  // no block-wide barrier below
  const int n = (int)n64;
  const int Ln = __builtin_amdgcn_readfirstlane(c_len[n]);  // one word per wave: lengths and block counts are wave-uniform
  const bool word_ok = Ln >= 1 && Ln <= T;
  const float inf = __builtin_inff();
  const float* wbase = c_unit + (size_t)n * T * H + 4 * half;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    const int Lq = __builtin_amdgcn_readfirstlane(q_len[q]);
    float* out = dist + (size_t)q * N + n;
    if (!word_ok || Lq < 1 || Lq > T || Ln < len_lo[q] || Ln > len_hi[q]) {  // the gate: no arithmetic
      if (lane == 0) *out = inf;
      continue;
    }
    ws_wave_lds_order();  // the table walk of the pair before this one has read the tile
    ws_cost_tile(tile, q_unit + (size_t)q * T * H + 4 * half, wbase, Lq, Ln, H, P, r);
    ws_wave_lds_order();
    // the wavefront: lane i = row i; d1 = this row's cell of the step before (its left neighbour now)
    const int i = lane;
    float d1 = inf, up_prev = inf;
    const int steps = Lq + Ln - 1;
    for (int s = 0; s < steps; ++s) {
      const int j = s - i;
      const float up = ws_from_lane_below(d1, inf);  // row 0 has no upper neighbour
      const bool cell = i < Lq && j >= 0 && j < Ln;
      const float c = cell ? tile[i * P + j] : 0.f;
      float best = fminf(up_prev, fminf(up, d1));
      if (s == 0 && i == 0) best = 0.f;
      up_prev = up;
      d1 = cell ? c + best : inf;
    }
    if (i == Lq - 1) *out = d1 / (float)(Lq + Ln);
  }
}

// The subsequence form on ws_dtw_kernel's grid, cost tile and LDS discipline: the walk alone differs.  Lane i carries, beside its
// row's last value, the column at which that cell's path left row 0; both come from lane i - 1 by one DPP move each, the diagonal
// pair is the upper pair of the step before.  Row 0 starts afresh in every column (best = 0, start = j).  Among equal predecessors
// the diagonal wins, then the upper, then the left: strict < in that order, as the host twin compares.  Lane Lq - 1 sees its Ln
// cells in ascending j and keeps the first smallest one with its end and start.  span [Q][N][2].
__global__ __launch_bounds__(WS_THREADS) void ws_dtw_sub_kernel(const float* __restrict__ q_unit, const int32_t* __restrict__ q_len,
                                                                const int32_t* __restrict__ len_lo, const int32_t* __restrict__ len_hi,
                                                                int Q, const float* __restrict__ c_unit, const int32_t* __restrict__ c_len,
                                                                int N, int T, int H, int P, float* __restrict__ dist,
                                                                int32_t* __restrict__ span) {
  extern __shared__ float tiles[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane & 31, half = lane >> 5;
  float* tile = tiles + (size_t)wave * T * P;
  const int64_t n64 = (int64_t)blockIdx.x * WS_WAVES + wave;
  if (n64 >= N) return;  // no block-wide barrier below
  const int n = (int)n64;
  const int Ln = __builtin_amdgcn_readfirstlane(c_len[n]);
  const bool word_ok = Ln >= 1 && Ln <= T;
  const float inf = __builtin_inff();
  const float* wbase = c_unit + (size_t)n * T * H + 4 * half;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    const int Lq = __builtin_amdgcn_readfirstlane(q_len[q]);
    const size_t at = (size_t)q * N + n;
    if (!word_ok || Lq < 1 || Lq > T || Ln < len_lo[q] || Ln > len_hi[q]) {  // the gate: no arithmetic
      if (lane == 0) {
        dist[at] = inf;
        span[2 * at] = -1;
        span[2 * at + 1] = -1;
      }
      continue;
    }
    ws_wave_lds_order();  // the table walk of the pair before this one has read the tile
    ws_cost_tile(tile, q_unit + (size_t)q * T * H + 4 * half, wbase, Lq, Ln, H, P, r);
    ws_wave_lds_order();
    const int i = lane;
    float d1 = inf, up_prev = inf, low = inf;  // low / low_end / low_start: the last row's running minimum (lane Lq - 1 alone)
    int st1 = -1, ups_prev = -1, low_end = -1, low_start = -1;
    const int steps = Lq + Ln - 1;
    for (int s = 0; s < steps; ++s) {
      const int j = s - i;
      const float up = ws_from_lane_below(d1, inf);  // row 0 has no upper neighbour
      const int ups = ws_int_from_lane_below(st1, -1);
      const bool cell = i < Lq && j >= 0 && j < Ln;
      const float c = cell ? tile[i * P + j] : 0.f;
      float best = up_prev;
      int st = ups_prev;
      if (up < best) best = up, st = ups;
      if (d1 < best) best = d1, st = st1;
      if (i == 0) best = 0.f, st = j;  // the free start
      up_prev = up;
      ups_prev = ups;
      d1 = cell ? c + best : inf;
      st1 = st;
      if (cell && d1 < low) low = d1, low_end = j, low_start = st;
    }
    if (i == Lq - 1) {
      dist[at] = low / (float)Lq;
      span[2 * at] = low_start;
      span[2 * at + 1] = low_end < 0 ? -1 : low_end + 1;  // no cell below +inf: only frames that are not unit frames do that
    }
  }
}

// grid (queries), 256 threads
__global__ __launch_bounds__(WS_THREADS) void ws_topk_kernel(const float* __restrict__ dist, int N, int k, int32_t* __restrict__ idx_out,
                                                             float* __restrict__ val_out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sel[MSOCR_SPOT_MAX_K];
  __shared__ unsigned s_prefix, s_remaining, s_kk, s_less;
  __shared__ unsigned wave_cnt[WS_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* row = dist + (size_t)blockIdx.x * N;
  int32_t* idx_row = idx_out + (size_t)blockIdx.x * k;
  float* val_row = val_out + (size_t)blockIdx.x * k;
  unsigned prefix = 0u, mask = 0u, kk = 0u;
  for (int p = 3; p >= 0; --p) {
    hist[tid] = 0u;
    __syncthreads();
    for (int64_t i = tid; i < N; i += WS_THREADS) {
      const uint32_t b = __float_as_uint(row[i]);
      if (!ws_finite_bits(b)) continue;
      const uint32_t key = ws_key_bits(b);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> (8 * p)) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned rem;
      if (p == 3) {  // every finite entry was counted: the rank asked for is min(k, their number)
        unsigned total = 0u;
        for (int b = 0; b < 256; ++b) total += hist[b];
        rem = total < (unsigned)k ? total : (unsigned)k;
        s_kk = rem;
      } else {
        rem = s_remaining;
      }
      if (rem > 0u) {  // the bin that holds rank rem, 1-based, among the entries that share the prefix
        unsigned cum = 0u;
        int b = 0;
        for (; b < 255; ++b) {
          if (cum + hist[b] >= rem) break;
          cum += hist[b];
        }
        s_prefix = prefix | ((unsigned)b << (8 * p));
        s_remaining = rem - cum;
      }
    }
    __syncthreads();
    kk = s_kk;
    if (kk == 0u) break;
    prefix = s_prefix;
    mask |= 255u << (8 * p);
  }
  if (kk == 0u) {
    if (tid < k) {
      idx_row[tid] = -1;
      val_row[tid] = __builtin_inff();
    }
    return;
  }
  const unsigned kth = prefix;          // the key of rank kk
  const unsigned need_eq = s_remaining;  // entries equal to it that belong to the result: the first ones in index order
  const unsigned n_less = kk - need_eq;
  sel[tid] = ~0ull;
  if (tid == 0) s_less = 0u;
  __syncthreads();
  unsigned running_eq = 0u;
  for (int64_t base = 0; base < N; base += WS_THREADS) {
    const int64_t i = base + tid;
    bool eq = false;
    uint32_t key = 0u;
    if (i < N) {
      const uint32_t b = __float_as_uint(row[i]);
      if (ws_finite_bits(b)) {
        key = ws_key_bits(b);
        if (key < kth) {  // n_less < kk of them; the bound is checked all the same, a slot outside sel is never written
          const unsigned slot = atomicAdd(&s_less, 1u);
          if (slot < n_less) sel[slot] = ((unsigned long long)key << 32) | (uint32_t)i;
        }
        eq = key == kth;
      }
    }
    if (running_eq >= need_eq) continue;  // the same decision in every thread
    const int total = __syncthreads_count(eq);
    if (total == 0) continue;
    const unsigned long long bal = __ballot(eq);
    if (lane == 0) wave_cnt[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned pos = running_eq + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    if (eq && pos < need_eq) sel[n_less + pos] = ((unsigned long long)key << 32) | (uint32_t)i;
    __syncthreads();  // wave_cnt is free again
    running_eq += (unsigned)total;
  }
  // bitonic sort of the 256 slots, ascending by (key, index); unused slots hold the largest value
  for (int size = 2; size <= MSOCR_SPOT_MAX_K; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int partner = tid ^ stride;
      if (partner > tid) {
        const bool ascending = (tid & size) == 0;
        const unsigned long long a = sel[tid], b = sel[partner];
        if ((a > b) == ascending) {
          sel[tid] = b;
          sel[partner] = a;
        }
      }
    }
  __syncthreads();
  if (tid < k) {
    const bool used = (unsigned)tid < kk && sel[tid] != ~0ull;
    const int32_t i = used ? (int32_t)(sel[tid] & 0xffffffffull) : -1;
    idx_row[tid] = i;
    val_row[tid] = used ? row[i] : __builtin_inff();
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the grid of both pair kernels, and the pitch of their LDS tiles
int ws_pair_grid(int Q, int N, int T, dim3* grid, int* P) {
  int cu = 0, rc;
  if ((rc = msocr_internal_cu_count(&cu)) != MSOCR_OK) return rc;
  // grid rows share the queries when the corpus alone leaves CUs without work: about four workgroups per CU
  const int64_t tiles = ((int64_t)N + WS_WAVES - 1) / WS_WAVES;
  int64_t rows = ((int64_t)cu * 4 + tiles - 1) / tiles;
  rows = rows < 1 ? 1 : rows > Q ? Q : rows > 65535 ? 65535 : rows;
  *grid = dim3((unsigned)tiles, (unsigned)rows);
  *P = (T + 1) & ~1;  // at most 64: WS_WAVES tiles are at most 64 KB of dynamic LDS, inside the default limit
  return MSOCR_OK;
}

}  // namespace

extern "C" int msocr_frame_normalize(const float* feat, const int32_t* len, int N, int T, int H, float* unit_out, void* stream) {
  if (!ws_shape_ok(N, T, H) || !feat || !len || !unit_out) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  int cu = 0, rc;
  if ((rc = msocr_internal_cu_count(&cu)) != MSOCR_OK) return rc;
  const int64_t want = ((int64_t)N * T + WS_WAVES - 1) / WS_WAVES;
  const int64_t cap = (int64_t)cu * 32;
  MSOCR_LAUNCH(ws_normalize_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(WS_THREADS), 0, (hipStream_t)stream, feat, len, N, T, H,
               unit_out);
  return LAUNCH_OK();
}

extern "C" int msocr_frame_normalize_host(const float* feat, const int32_t* len, int N, int T, int H, float* unit_out) {
  if (!ws_shape_ok(N, T, H) || !feat || !len || !unit_out) return MSOCR_E_ARG;
  ws_normalize_host(feat, len, N, T, H, unit_out);
  return MSOCR_OK;
}

extern "C" int msocr_dtw_distances(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                                   const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, void* stream) {
  if (!ws_shape_ok(Q, T, H) || !ws_shape_ok(N, T, H)) return MSOCR_E_ARG;
  if (!q_unit || !q_len || !len_lo || !len_hi || !c_unit || !c_len || !dist || !aligned16(q_unit) || !aligned16(c_unit)) return MSOCR_E_ARG;
  if (Q == 0 || N == 0) return MSOCR_OK;
  dim3 grid;
  int P, rc;
  if ((rc = ws_pair_grid(Q, N, T, &grid, &P)) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(ws_dtw_kernel, grid, dim3(WS_THREADS), (size_t)WS_WAVES * T * P * sizeof(float), (hipStream_t)stream, q_unit, q_len, len_lo,
               len_hi, Q, c_unit, c_len, N, T, H, P, dist);
  return LAUNCH_OK();
}

extern "C" int msocr_dtw_distances_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                                        const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist) {
  if (!ws_shape_ok(Q, T, H) || !ws_shape_ok(N, T, H)) return MSOCR_E_ARG;
  if (!q_unit || !q_len || !len_lo || !len_hi || !c_unit || !c_len || !dist) return MSOCR_E_ARG;
  if (!ws_lens_ok(q_len, Q, T) || !ws_lens_ok(c_len, N, T)) return MSOCR_E_ARG;
  for (int q = 0; q < Q; ++q)
    if (len_lo[q] > len_hi[q]) return MSOCR_E_ARG;
  try {
    ws_dtw_host(q_unit, q_len, len_lo, len_hi, Q, c_unit, c_len, N, T, H, dist);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  return MSOCR_OK;
}

extern "C" int msocr_dtw_subsequence(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                                     const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, int32_t* span,
                                     void* stream) {
  if (!ws_sub_args_ok(q_unit, q_len, len_lo, len_hi, Q, c_unit, c_len, N, T, H, dist, span) || !aligned16(q_unit) || !aligned16(c_unit))
    return MSOCR_E_ARG;
  if (Q == 0 || N == 0) return MSOCR_OK;
  dim3 grid;
  int P, rc;
  if ((rc = ws_pair_grid(Q, N, T, &grid, &P)) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(ws_dtw_sub_kernel, grid, dim3(WS_THREADS), (size_t)WS_WAVES * T * P * sizeof(float), (hipStream_t)stream, q_unit, q_len,
               len_lo, len_hi, Q, c_unit, c_len, N, T, H, P, dist, span);
  return LAUNCH_OK();
}

extern "C" int msocr_dtw_subsequence_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                                          const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, int32_t* span) {
  if (!ws_sub_args_ok(q_unit, q_len, len_lo, len_hi, Q, c_unit, c_len, N, T, H, dist, span)) return MSOCR_E_ARG;
  if (!ws_lens_ok(q_len, Q, T) || !ws_lens_ok(c_len, N, T)) return MSOCR_E_ARG;
  for (int q = 0; q < Q; ++q)
    if (len_lo[q] > len_hi[q]) return MSOCR_E_ARG;
  try {
    ws_dtw_sub_host(q_unit, q_len, len_lo, len_hi, Q, c_unit, c_len, N, T, H, dist, span);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  return MSOCR_OK;
}

extern "C" int msocr_topk_smallest(const float* dist, int Q, int N, int k, int32_t* idx, float* val, void* stream) {
  if (Q < 0 || N < 0 || k < 1 || k > MSOCR_SPOT_MAX_K || (!dist && Q > 0 && N > 0) || !idx || !val) return MSOCR_E_ARG;
  if (Q == 0) return MSOCR_OK;
  MSOCR_LAUNCH(ws_topk_kernel, dim3((unsigned)Q), dim3(WS_THREADS), 0, (hipStream_t)stream, dist, N, k, idx, val);
  return LAUNCH_OK();
}

extern "C" int msocr_topk_smallest_host(const float* dist, int Q, int N, int k, int32_t* idx, float* val) {
  if (Q < 0 || N < 0 || k < 1 || k > MSOCR_SPOT_MAX_K || (!dist && Q > 0 && N > 0) || !idx || !val) return MSOCR_E_ARG;
  try {
    ws_topk_host(dist, Q, N, k, idx, val);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  return MSOCR_OK;
}
