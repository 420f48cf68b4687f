// split_mma.h — the split-operand ("bf16x3") arithmetic every kernel of that family shares: conv_split.hip, conv_split_pp.hip, the
// fused Winograd kernels (winograd.hip) and the recurrent kernels (split_rows32.h).  An f32 value is the exact sum of three bf16
// values, a = a0 + a1 + a2; an f32 product is six bf16 MFMA products with f32 accumulation (conv_split.hip has the error bound).
// Not part of the C ABI.
#ifndef MSOCR_SPLIT_MMA_H
#define MSOCR_SPLIT_MMA_H
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// one step of the exact three-term split: two f32 -> the packed bf16 pair of their leading terms; x and y keep the residuals
__device__ __forceinline__ uint32_t split_step(float& x, float& y) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {x, y};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);  // v_cvt_pk_bf16_f32, round to nearest even
  const uint32_t pk = __builtin_bit_cast(uint32_t, h);
  x -= __uint_as_float(pk << 16);          // exact: the leading term shares x's exponent
  y -= __uint_as_float(pk & 0xffff0000u);
  return pk;
}

// The six kept products in the order every kernel issues them, SMALLEST TERMS FIRST: product t multiplies plane split_pa(t) of A
// with plane split_pb(t) of B — a2b0, a0b2, a1b1, a1b0, a0b1, a0b0.  A numerical contract: the f64 tests' bounds assume it.
__device__ constexpr int split_pa(int t) {
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
  return PA[t];
}
__device__ constexpr int split_pb(int t) {
  constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
  return PB[t];
}

// c += a * b for one 32x32x16 / one 16x16x32 block, a and b as their three planes
__device__ __forceinline__ void mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& c) {
#pragma unroll
  for (int t = 0; t < 6; ++t) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[split_pa(t)], b[split_pb(t)], c, 0, 0, 0);
}
__device__ __forceinline__ void mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4& c) {
#pragma unroll
  for (int t = 0; t < 6; ++t) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[split_pa(t)], b[split_pb(t)], c, 0, 0, 0);
}

// row of accumulator register e in the 32x32 MFMA output layout (lane half = lane >> 5)
__device__ __forceinline__ int acc_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

#endif
