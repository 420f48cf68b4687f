// se_tail.h — the phases of the squeeze-excite tail, out = relu(x * sigmoid(W2 relu(W1 mean_hw(x))) + identity), as device functions
// over a pixel loader: se_residual_kernel (trba_kernels.hip) reads x from global memory, wino44_output_kernel_se (winograd.hip) from
// the crop its output transform left in LDS.  Not part of the C ABI.
//
// The order of every addition is part of the result and does not depend on the caller's thread count NT: the mean is summed by VT
// "virtual threads" (VT = 1024 for f32, 256 for bf16; a workgroup of NT < VT threads takes several each), virtual thread v = pixel
// group v / (C/4) of PG = VT / (C/4), channels 4 * (v % (C/4)) ..., pixels pg, pg + PG, ... ascending; the groups are summed
// ascending, then x 1/HW; hid[j] is the per-lane fmaf chain over c = lane, lane + 64, ... followed by wave_sum; the gate is the fmaf
// chain over j; the scale is v * g + r, uncontracted (-ffp-contract=off).
#ifndef MSOCR_SE_TAIL_H
#define MSOCR_SE_TAIL_H
#include <hip/hip_runtime.h>
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// LDS scratch of the tail in floats: part[PG][C] | mean[C] | hid[C/16] | gate[C]
__host__ __device__ inline int se_scratch_floats(int VT, int C) { return (VT / (C / 4)) * C + 2 * C + C / 16; }

// the virtual threads of this thread: f(v) for v = tid, tid + NT, ... < VT (one call, no loop, where NT == VT)
template <int VT, int NT, typename F>
__device__ __forceinline__ void se_virtual_threads(int tid, F f) {
  static_assert(VT % NT == 0, "whole rounds of the workgroup");
  if constexpr (VT == NT) {
    f(tid);
  } else {
    for (int v = tid; v < VT; v += NT) f(v);
  }
}

// Phase 1: part[pg][c] = sum of x over the pixels of group pg.  ldx(p, c) loads channels c ... c + 3 of pixel p.
// Four loads in flight per thread, added in the order of the one-at-a-time loop (same sums): with one load per iteration
// se_residual_kernel sat at 0.45 of the HBM rate — too few bytes in flight per CU for a 2 us round trip
template <int VT, int NT, typename LoadX>
__device__ __forceinline__ void se_partial_sums(LoadX ldx, int HW, int C, float* part, int tid) {
  const int C4 = C / 4, PG = VT / C4;  // host guarantees C in {64,128,256,512,1024}: C4 divides VT
  se_virtual_threads<VT, NT>(tid, [&](int vt) {
    const int cg = vt % C4, pg = vt / C4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int p = pg;
    for (; p + 3 * PG < HW; p += 4 * PG) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ldx(p + u * PG, cg * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) { s[0] += v[u][0]; s[1] += v[u][1]; s[2] += v[u][2]; s[3] += v[u][3]; }
    }
    for (; p < HW; p += PG) {
      const f32x4 v = ldx(p, cg * 4);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    *reinterpret_cast<f32x4*>(&part[pg * C + cg * 4]) = s;
  });
}

// Phases 2-4: mean over the pixel groups, hid = relu(W1 mean) (one wave per output, lanes over C), gate = sigmoid(W2 hid), kept in
// LDS and written to gate_row[C].  sm = the scratch above with part filled in by this workgroup; barriers before, between and after.
template <int VT, int NT>
__device__ __forceinline__ const float* se_gate(float* sm, int HW, int C, const float* __restrict__ w1, const float* __restrict__ w2,
                                                float* __restrict__ gate_row, int tid) {
  const int PG = VT / (C / 4);
  float* part = sm;
  float* mean = sm + PG * C;
  float* hid = mean + C;
  float* gate = hid + C / 16;
  __syncthreads();
  const float inv = 1.0f / (float)HW;
  for (int c = tid; c < C; c += NT) {
    float s = 0.f;
    for (int g = 0; g < PG; ++g) s += part[g * C + c];
    mean[c] = s * inv;
  }
  __syncthreads();
  const int Cr = C / 16;
  {
    const int lane = tid & 63, wv = tid >> 6;
    for (int j = wv; j < Cr; j += NT / 64) {
      float a = 0.f;
      for (int c = lane; c < C; c += 64) a = fmaf(w1[(long)j * C + c], mean[c], a);
      a = wave_sum(a);
      if (lane == 0) hid[j] = fmaxf(a, 0.f);
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += NT) {
    float a = 0.f;
    for (int j = 0; j < Cr; ++j) a = fmaf(w2[(long)c * Cr + j], hid[j], a);
    const float g = sigmoidf_(a);
    gate[c] = g;
    gate_row[c] = g;
  }
  __syncthreads();
  return gate;
}

// Phase 5: out = relu(x * gate + identity) over the pixels of phase 1, in its thread map.  ldx / ldr(p, c) load x / the identity,
// sto(p, c, y) stores.
template <int VT, int NT, typename LoadX, typename LoadR, typename Store>
__device__ __forceinline__ void se_scale(LoadX ldx, LoadR ldr, Store sto, int HW, int C, const float* gate, int tid) {
  const int C4 = C / 4, PG = VT / C4;
  se_virtual_threads<VT, NT>(tid, [&](int vt) {
    const int cg = vt % C4, pg = vt / C4;
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(&gate[cg * 4]);
    int p = pg;
    for (; p + 3 * PG < HW; p += 4 * PG) {
      f32x4 v[4], r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = ldx(p + u * PG, cg * 4);
        r[u] = ldr(p + u * PG, cg * 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaxf(v[u][e] * g4[e] + r[u][e], 0.f);
        sto(p + u * PG, cg * 4, y);
      }
    }
    for (; p < HW; p += PG) {
      const f32x4 v = ldx(p, cg * 4), r = ldr(p, cg * 4);
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fmaxf(v[e] * g4[e] + r[e], 0.f);
      sto(p, cg * 4, y);
    }
  });
}

#endif
