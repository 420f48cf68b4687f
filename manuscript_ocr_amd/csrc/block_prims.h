// block_prims.h — device-only building blocks shared by the page post-processing kernels (east_post.hip, east_tail.hip,
// reading_order.hip, quad_crop.hip): the workgroup exclusive scan and the lane-owned bit words of a greedy wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Exclusive prefix sum of one integer per thread over a workgroup of T threads (T a multiple of 64, at most 1024; every thread
// must call it).  Returns the sum of v over the threads before this one; *total = the sum over all of them, in every thread.
// wave_tot is the caller's LDS, int[T / 64].  The first barrier publishes the wave totals.  The SECOND, after every thread has
// read them, is what makes back-to-back calls on the same wave_tot safe (east_decode_kernel: one call per 1024-cell chunk;
// reading_order_kernel: one per sweep and one at the end): without it a fast wave's next call would overwrite its total while a
// slow wave still sums the previous ones.
template <int T>
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_tot, int* total) {
  static_assert(T % 64 == 0 && T >= 64 && T <= 1024, "whole waves, one workgroup");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wave_tot[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma nounroll  // unrolled, the T / 64 LDS reads are in flight at once and cost reading_order_kernel 5 VGPRs
  for (int q = 0; q < T / 64; ++q) {
    if (q == wv) base = tot;
    tot += wave_tot[q];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// Sum of one int64 per thread over a workgroup of T threads, in every thread (every thread must call it).  Integer, so exact and
// independent of the order.  wave_tot is the caller's LDS, long long[T / 64]; the two barriers serve as in block_exclusive_scan.
template <int T>
__device__ __forceinline__ long long block_sum_i64(long long v, long long* wave_tot) {
  static_assert(T % 64 == 0 && T >= 64 && T <= 1024, "whole waves, one workgroup");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  long long tot = 0;
#pragma nounroll
  for (int q = 0; q < T / 64; ++q) tot += wave_tot[q];
  __syncthreads();
  return tot;
}

// The bit words a greedy wave keeps in registers: a mask of 64 * KW * 32 bits, word l + 64 k owned by lane l in w[k].  w[] is
// only ever indexed by the counter of a fully unrolled loop, so the words stay in registers; the one dynamic access, "the word
// that holds bit i", is a select chain + __shfl.  All 64 lanes call every operation with the same (wave-uniform) arguments;
// row = a matrix row of which W words are in use, words = all 64 * KW words of a mask in memory.
template <int KW>
struct LaneBits {
  uint32_t w[KW];
  template <typename F>
  __device__ __forceinline__ void each(F f) {  // f(owned word, its index in the mask)
#pragma unroll
    for (int k = 0; k < KW; ++k) f(w[k], (int)(threadIdx.x & 63) + 64 * k);
  }
  __device__ __forceinline__ void fill(uint32_t v) { each([&](uint32_t& x, int) { x = v; }); }
  __device__ __forceinline__ void load(const uint32_t* words) { each([&](uint32_t& x, int wd) { x = words[wd]; }); }
  __device__ __forceinline__ void store(uint32_t* words) { each([&](uint32_t& x, int wd) { words[wd] = x; }); }
  __device__ __forceinline__ bool test(int i) {  // bit i
    uint32_t mine = 0u;
    each([&](uint32_t& x, int wd) { mine = (wd >> 6) == (i >> 11) ? x : mine; });
    return (__shfl(mine, (i >> 5) & 63) >> (i & 31)) & 1u;
  }
  __device__ __forceinline__ void clear(int i) { each([&](uint32_t& x, int wd) { x &= wd == (i >> 5) ? ~(1u << (i & 31)) : ~0u; }); }
  __device__ __forceinline__ void or_row(const uint32_t* row, int W) { each([&](uint32_t& x, int wd) { if (wd < W) x |= row[wd]; }); }
  __device__ __forceinline__ bool and_any(const uint32_t* row, int W) {  // (mask & row) != 0
    uint32_t v = 0u;
    each([&](uint32_t& x, int wd) { if (wd < W) v |= row[wd] & x; });
    return __any(v != 0u);
  }
};
