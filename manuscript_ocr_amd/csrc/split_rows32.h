// split_rows32.h — device helpers shared by the recurrent kernels that keep a 32-row hidden state (one MFMA row block, 256 units) in
// LDS and multiply it with a weight matrix streamed from L2 in the split-operand form: attn_beam_mfma.hip (beam and greedy decode)
// and bilstm_mfma.hip (encoder BiLSTM).  Three parts: the split-operand products (mfma_cols32_split, mfma_gates_split), the two
// grades of the LSTM nonlinearities (FastMath, LibmMath), and the row-block LSTM step on the gate accumulators (lstm_cell,
// store_h_planes).  Not part of the C ABI.
#ifndef MSOCR_SPLIT_ROWS32_H
#define MSOCR_SPLIT_ROWS32_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "split_mma.h"

namespace split_rows32 {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int H = 256;  // hidden units = reduction length
constexpr int R = 32;   // state rows = one MFMA row block


// ---- split-operand form of the three matrix products : h is kept in LDS as three bf16 planes with h == p0 + p1 + p2
// exactly (the residual chain of conv_split.hip), the weights come pre-split and packed [plane][k / 16][column][16] bf16
// (msocr_attn_pack_split_host), and every f32 product a * b is the six bf16 products of split_mma.h on
// v_mfma_f32_32x32x16_bf16 with f32 accumulation (dropped terms <= 2^-25 |a b|): 6 MFMAs of 8 passes per 16 k instead of 8 MFMAs of
// 16 passes on the exact-f32 pipe, i.e. 2.7x less matrix-pipe time for the same f32 result up to summation order.
constexpr int PSB = H * 2 + 16;       // bytes per plane row: 528 = 132 dwords, rows shift 4 banks -> ds_read_b128 of 32 rows is conflict-free
constexpr int PPL = R * PSB;          // bytes per plane

// the weight fragments arrive as raw 16-byte loads
__device__ __forceinline__ void mma6(const bf16x8 (&fa)[3], const u32x4 (&wb)[3], f32x16& acc) {
  const bf16x8 fb[3] = {__builtin_bit_cast(bf16x8, wb[0]), __builtin_bit_cast(bf16x8, wb[1]), __builtin_bit_cast(bf16x8, wb[2])};
  ::mma6(fa, fb, acc);
}
__device__ __forceinline__ void read_a3(const unsigned char* sP, int kb, int r32, int half, bf16x8 (&fa)[3]) {
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) fa[pl] = *reinterpret_cast<const bf16x8*>(sP + pl * PPL + r32 * PSB + kb * 32 + half * 16);
}

// D[32 rows][32 columns of this wave] += h * W, W packed [3][16][ncols][16] bf16
__device__ __forceinline__ void mfma_cols32_split(const unsigned char* __restrict__ sP, const uint16_t* __restrict__ Wp, int ncols, int col,
                                                  bool col_ok, int r32, int half, f32x16& acc) {
  constexpr int PF = 4;  // k-blocks (of 16) of weight loads kept in flight
  const int kbstep = ncols * 32, plstep = 16 * kbstep;  // bytes
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)Wp, 0, 3 * plstep, 0x00020000);
  const int voff = col_ok ? col * 32 + half * 16 : 0x7ffffff0;
  u32x4 wb[PF][3];
#pragma unroll
  for (int pq = 0; pq < PF; ++pq)
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wb[pq][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, pl * plstep + pq * kbstep, 0);
#pragma unroll 1
  for (int kb0 = 0; kb0 < H / 16; kb0 += PF) {
#pragma unroll
    for (int pq = 0; pq < PF; ++pq) {
      const int kb = kb0 + pq;
      bf16x8 fa[3];
      read_a3(sP, kb, r32, half, fa);
      u32x4 cur[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) cur[pl] = wb[pq][pl];
      if (kb + PF < H / 16) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) wb[pq][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, pl * plstep + (kb + PF) * kbstep, 0);
      }
      mma6(fa, cur, acc);
    }
  }
}

// gates of hidden units 32w..32w+31: acc[g] += h * W_hh, packed [3][16][4 H (column g * H + j)][16] bf16
__device__ __forceinline__ void mfma_gates_split(const unsigned char* __restrict__ sP, const uint16_t* __restrict__ Wp, int j, int r32, int half,
                                                 f32x16 (&acc)[4]) {
  constexpr int kbstep = 4 * H * 32, plstep = 16 * kbstep, gstep = H * 32;  // bytes
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)Wp, 0, 3 * plstep, 0x00020000);
  const int voff = j * 32 + half * 16;
  u32x4 wb[4][3];  // one k-block of the four gates; a gate's next block is requested as soon as its six MFMAs are issued
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wb[g][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, pl * plstep + g * gstep, 0);
#pragma unroll 2
  for (int kb = 0; kb < H / 16; ++kb) {
    bf16x8 fa[3];
    read_a3(sP, kb, r32, half, fa);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      mma6(fa, wb[g], acc[g]);
      if (kb + 1 < H / 16) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          wb[g][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, pl * plstep + (kb + 1) * kbstep + g * gstep, 0);
      }
    }
  }
}

// ---- the LSTM step on the gate accumulators: wave w owns hidden units 32w..32w+31 with their four gates (i, f, g, o) in acc[0..3],
// element e of every accumulator belonging to state row acc_row(e, half), so the cell update is lane-local.

// The two grades of the nonlinearities, chosen by the kernel at compile time.  FastMath: hardware-rate v_exp_f32 / v_rcp_f32
// (1-2 ulp each) — a recurrent step evaluates 5 x 32 x 256 gate activations (the beam decode another 32 x T x 256 tanh) on the VALU
// between the matrix phases, and the libm forms made that the longest phase.  LibmMath: expf / tanhf, for the kernel whose logits
// are held to a bound the hardware-rate forms miss (attn_greedy_mfma_kernel).
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
struct FastMath {
  static __device__ __forceinline__ float sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + fexp(-x)); }
  static __device__ __forceinline__ float tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(fexp(2.0f * x) + 1.0f); }
};
struct LibmMath {
  static __device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
  static __device__ __forceinline__ float tanh(float x) { return tanhf(x); }
};

// c' = f c + i g,  h' = o tanh(c')  for this lane's 16 rows of its unit
template <class NL>
__device__ __forceinline__ void lstm_cell(const f32x16 (&acc)[4], f32x16& c, float (&hv)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float ig = NL::sigmoid(acc[0][e]), fg = NL::sigmoid(acc[1][e]), gg = NL::tanh(acc[2][e]), og = NL::sigmoid(acc[3][e]);
    c[e] = fg * c[e] + ig * gg;
    hv[e] = og * NL::tanh(c[e]);
  }
}

// h' of unit ju -> the three bf16 planes (hv is consumed: it ends as the residual of the split)
__device__ __forceinline__ void store_h_planes(unsigned char* sP, int ju, int half, float (&hv)[16]) {
#pragma unroll
  for (int e = 0; e < 16; e += 2) {  // acc_row(e + 1) == acc_row(e) + 1
    unsigned char* d = sP + acc_row(e, half) * PSB + ju * 2;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const uint32_t pk = split_step(hv[e], hv[e + 1]);
      *reinterpret_cast<uint16_t*>(d + pl * PPL) = (uint16_t)pk;
      *reinterpret_cast<uint16_t*>(d + pl * PPL + PSB) = (uint16_t)(pk >> 16);
    }
  }
}

}  // namespace split_rows32
#endif
