// conv_split.hip — f32 GEMM / 1x1 convolution on the bf16 matrix pipes with EXACTLY split operands ("bf16x3").
//
// gfx950 runs exact-f32 MFMA (v_mfma_f32_32x32x2_f32) at 1/16 of the bf16 rate.  An f32 value splits exactly into three bf16
// terms, a = a0 + a1 + a2 (round-to-nearest residuals: |a1| <= 2^-9 |a|, |a2| <= 2^-18 |a|), so
//     a * b = a0b0 + (a0b1 + a1b0) + (a1b1 + a0b2 + a2b0) + [a1b2 + a2b1 + a2b2],
// and the bracket is <= 2^-25 |ab|: below the rounding of the f32 accumulation both paths share.  The six kept products run on
// v_mfma_f32_32x32x16_bf16 (products of bf16 values are exact in f32; f32 accumulate), smallest terms first: 6 bf16 MFMAs
// replace 8 f32 MFMAs of 1/16 the rate each — the K loop costs 6 x 32 cycles per 32x32x16 block instead of 8 x 64.
//
// Operands: A = activations (or the Winograd-domain V) as plain f32 in HBM, split IN REGISTERS on the way into LDS (three
// v_cvt_pk_bf16_f32 + two subtractions per pair); B = weights (or the Winograd U), split ONCE at load time into three bf16
// planes [3][Cout][K] (msocr_split_bf16x3_host / ops.py).  Same tile as conv_igemm.hip's lean kernel: 128 x 128 (or 128 x 64) per
// workgroup, 4 waves of 64 x 64 (64 x 32), K-tiles of 32, one LDS stage of six [rows][64 B] planes (16-B chunks XOR-swizzled by
// row), 3 workgroups per CU; tile map, loaders and the epilogue (bias, residual, ReLU, 16-byte stores) are the shared ones of
// conv_common.h, the split arithmetic is split_mma.h's.
//
// Used for every launch the lean exact-f32 GEMM served (1x1 / stride 1 / no padding convolutions, the LSTM / linear GEMMs and
// the batched Winograd-domain GEMMs) unless the caller asks for precision = "fp32-exact".  Reference layers:
//   recognizers/_trba/model/seresnet31.py:37-67 ; detectors/_east/east.py:13-30 ; torchvision Bottleneck conv1 / conv3
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "conv_common.h"

namespace {

// BN in {128, 64}; wave tile 64 x WN (WN = BN / 2); K-tile = 32 elements (A rows 128 B of f32 in HBM, 64 B per bf16 plane in LDS).
// GEN = false: 1x1 / stride 1 / no padding over a dense pixel sequence and the batched GEMMs — a K-tile is a plain pointer
// increment.  GEN = true: any kernel size / stride / padding (the tap loader of conv_common.h: a K-tile lies inside one filter tap
// because Cin % 32 == 0; out-of-image taps read zeros).
template <int BN, int WPE, bool GEN>
__global__ __launch_bounds__(256, WPE) void conv_split_kernel(ConvParams p) {
  using G = SplitTile<BN>;
  constexpr int BM = G::BM, WM = G::WM, WN = G::WN, BK = G::BK;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int ROWB = G::ROWB, A_PLANE = G::A_PLANE, B_PLANE = G::B_PLANE, STAGE_B = G::STAGE_B;
  constexpr int ACH = G::ACH, ARP = G::ARP, A_IT = G::A_IT;  // A: 16-B chunks per f32 row, rows per pass of 256 threads
  constexpr int BCH = G::BCH, B_IT = G::B_IT;                // B: 16-B chunks per bf16 row

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  int batch, tile_m, tile_n;
  tile_coords(p, xcd_tile<int>(blockIdx.x, p.tilesM * p.tilesN * p.nbatch), batch, tile_m, tile_n);
  const char* const g_in = p.in + (long)batch * p.bsA * 4;
  const char* const g_w = p.w + (long)batch * p.bsW * 2;
  char* const g_out = p.out + (long)batch * p.bsO * 4;

  // ---- staging coordinates ----
  // Lean form: every address is a wave-uniform base (SGPRs: batch + K-tile + plane) plus a 32-bit per-thread offset (one VGPR per
  // load), so the loop holds 4 + B_IT address registers instead of ten 64-bit pointers — the 168-register budget of 3 workgroups per
  // CU then leaves no spill in the loop (a spilled, freshly loaded register made every K-tile wait for a memory round trip).
  const int a_chunk = tid % ACH, a_row0 = tid / ACH;
  uint32_t a_off[A_IT];
  ATap<GEN> a_tap[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) a_off[i] = a_row_offset32<GEN>(p, (long)tile_m * BM + a_row0 + i * ARP, a_chunk, a_tap[i]);
  TapCursor tap;
  tap.reset();
  const int b_chunk = tid % BCH, b_row0 = tid / BCH;
  uint32_t b_off[B_IT];
#pragma unroll
  for (int j = 0; j < B_IT; ++j) b_off[j] = b_plane_offset(tile_n * BN + b_row0 + j * G::BRP, p.Cout, b_chunk);
  const long wplane_b = p.wplane * 2;

  u32x4 ra[A_IT], rb[3][B_IT];
  auto load_tile = [&](int kt) {
    // GEN, BN = 128: the compiler spills 4 registers here (20 bytes of scratch) at the 168-register budget of 3 workgroups per CU; the
    // instance runs only with a residual operand or a single K-tile (conv_split_pp.hip takes the rest).  The other three do not spill.
    if constexpr (GEN) load_a_taps32(p, g_in, a_off, a_tap, tap, BK, ra);
    else load_a_rows32(g_in + (long)kt * (BK * 4), a_off, ra);
    load_b_planes<G>(p, g_w, wplane_b, kt, b_row0, b_off, rb);
  };
  auto store_tile = [&](int stage) {
    unsigned char* const sA = smem + stage * STAGE_B;  // [3][BM][ROWB] (one stage: stage == 0)
#pragma unroll
    for (int i = 0; i < A_IT; ++i) split_store_row<G>(sA, a_row0 + i * ARP, a_chunk, ra[i]);
    unsigned char* const sB = sA + 3 * A_PLANE;        // [3][BN][ROWB]
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int j = 0; j < B_IT; ++j)
        if (BN % G::BRP == 0 || b_row0 + j * G::BRP < BN) store_b_row<G>(sB, pl, b_row0 + j * G::BRP, b_chunk, rb[pl][j]);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int r32 = lane & 31, half = lane >> 5;

  auto compute = [&](int stage) {
    const unsigned char* const sA = smem + stage * STAGE_B;
    const unsigned char* const sB = sA + 3 * A_PLANE;
#pragma unroll
    for (int q = 0; q < BK / 16; ++q) {        // k16 steps per K-tile
      const int c = 2 * q + half;
      bf16x8 fa[3][TM], fb[3][TN];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WM + i * 32 + r32;
          fa[pl][i] = *reinterpret_cast<const bf16x8*>(sA + pl * A_PLANE + row * ROWB + ((c ^ swz<ROWB>(row)) << 4));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = wn * WN + j * 32 + r32;
          fb[pl][j] = *reinterpret_cast<const bf16x8*>(sB + pl * B_PLANE + row * ROWB + ((c ^ swz<ROWB>(row)) << 4));
        }
      }
      // the six products (split_mma.h: smallest terms first); consecutive MFMAs of one product class hit different accumulators
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[split_pa(t)][i], fb[split_pb(t)][j], acc[i][j], 0, 0, 0);
    }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();

  // One LDS stage, two barriers per K-tile, 3 workgroups per CU.  Measured alternatives (round 3, gpurun_out/r3_split_variants.txt,
  // f32-equivalent TFLOP/s at K = 512 / 4096 on M = 161280, N = 512): this loop 156 / 182; two LDS stages with K-tiles of 16 (one
  // barrier per tile, 3 per CU) 145 / 148; two stages with K-tiles of 32 (1 per CU) 120 / 148; K-tiles of 16 at 4 per CU 126 / 94;
  // 2 per CU 154 / 176; the weight planes straight into LDS (global_load_lds_dwordx4, double-buffered, 2 per CU) 158 / 189 against
  // 166 / 191 for this loop on the same box.  Timing ablations of this loop: MFMAs + fragment reads alone 266, + restaging 228,
  // + loads that always hit the cache 190.
  for (int kt = 0; kt < p.ktiles; ++kt) {
    if (kt + 1 < p.ktiles) load_tile(kt + 1);  // global loads in flight under the MFMAs
    compute(0);
    __syncthreads();  // everyone is done reading the stage before it is overwritten
    if (kt + 1 < p.ktiles) store_tile(0);
    __syncthreads();
  }

  epilogue_lds<float, BM, BN, WM, WN, 32, true>(p, smem, acc, tile_m, tile_n, g_out, wm, wn, r32, half);
}

template <int BN, int WPE, bool GEN>
int launch_split(ConvParams& p, hipStream_t s) {
  return conv_launch<SplitTile<BN>>(conv_split_kernel<BN, WPE, GEN>, p, s);
}

// Kernel choice: shapes the producer / consumer kernel of conv_split_pp.hip has an instance for go there, the others (a residual
// operand, Cout % 128 != 0) to conv_split_kernel.
int launch_split_one(ConvParams& p, hipStream_t s, bool general) {
  if (msocr_internal_split_pp_takes(p)) return msocr_internal_split_pp_launch(p, s, general);
  if (general) return p.Cout % 128 == 0 ? launch_split<128, 3, true>(p, s) : launch_split<64, 3, true>(p, s);
  return p.Cout % 128 == 0 ? launch_split<128, 3, false>(p, s) : launch_split<64, 3, false>(p, s);
}

// Both loaders address with a per-thread 32-bit byte offset from a wave-uniform base: the lean one unsigned (rows of ONE problem
// must span less than 4 GB), the general one signed (an image range below 2 GB: msocr_conv2d_split splits the batch).  A lean
// single-problem launch whose rows span more is cut into row ranges here (rows are independent; bases advance in 64 bits).
int launch_split_any(ConvParams& p, hipStream_t s, bool general) {
  if (((long)p.Cout * p.Ktot + 32) * 2 >= (1L << 32)) return MSOCR_E_ARG;
  p.w_kt_b = (long)p.Cout * 64;
  if (general) return launch_split_one(p, s, true);
  const long row_b = p.sW * 4;
  const long limit = (1L << 32) - 4096;
  if ((p.M * p.sW + 32) * 4 < limit) return launch_split_one(p, s, false);
  if (p.nbatch != 1 || row_b <= 0 || row_b * 256 >= limit) return MSOCR_E_ARG;
  const long rows_per = (limit / row_b) & ~255L;   // a multiple of every M-tile
  for (long m0 = 0; m0 < p.M; m0 += rows_per) {
    ConvParams q = p;
    q.M = p.M - m0 < rows_per ? p.M - m0 : rows_per;
    q.in = p.in + m0 * row_b;
    q.out = p.out + m0 * p.out_ld * 4;
    if (p.has_res) q.res = p.res + m0 * p.res_ld * 4;
    const int rc = launch_split_one(q, s, false);
    if (rc != MSOCR_OK) return rc;
  }
  return MSOCR_OK;
}

}  // namespace

// HOST helper: w [n] f32 -> planes [3][n] bf16 with w == p0 + p1 + p2 exactly (round-to-nearest-even residual chain, the same
// arithmetic the kernel applies to its activation operand).
extern "C" int msocr_split_bf16x3_host(const float* w_host, int64_t n, uint16_t* planes_out_host) {
  if (!w_host || !planes_out_host || n <= 0) return MSOCR_E_ARG;
  auto rne = [](float f) -> uint16_t {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  };
  auto up = [](uint16_t h) -> float {
    return __builtin_bit_cast(float, (uint32_t)h << 16);
  };
  for (int64_t i = 0; i < n; ++i) {
    float r = w_host[i];
    for (int pl = 0; pl < 3; ++pl) {
      const uint16_t h = rne(r);
      planes_out_host[pl * n + i] = h;
      r -= up(h);
    }
  }
  return MSOCR_OK;
}

// HOST helper: the same split of w [nbatch][rows][k], planes written K-tile-major [3][nbatch][k/32][rows][32] (include/msocr.h).
extern "C" int msocr_split_bf16x3_ktile_host(const float* w_host, int64_t nbatch, int64_t rows, int64_t k, uint16_t* planes_out_host) {
  if (!w_host || !planes_out_host || nbatch <= 0 || rows <= 0 || k <= 0 || k % 32) return MSOCR_E_ARG;
  const int64_t n = nbatch * rows * k;
  uint16_t* tmp = (uint16_t*)malloc((size_t)n * 3 * sizeof(uint16_t));
  if (!tmp) return MSOCR_E_ARG;
  const int rc = msocr_split_bf16x3_host(w_host, n, tmp);
  if (rc == MSOCR_OK) {
    const int64_t kt = k / 32;
    for (int pl = 0; pl < 3; ++pl)
      for (int64_t b = 0; b < nbatch; ++b)
        for (int64_t r = 0; r < rows; ++r)
          for (int64_t t = 0; t < kt; ++t)
            memcpy(planes_out_host + pl * n + ((b * kt + t) * rows + r) * 32, tmp + pl * n + (b * rows + r) * k + t * 32, 64);
  }
  free(tmp);
  return rc;
}

// 1x1 / stride 1 / no padding convolution (a GEMM over pixels) with the weight operand given as three bf16 planes,
// K-tile-major [3][Cin/32][Cout][32] (plane stride Cout * Cin).  Same descriptor, epilogue flags and error behaviour as msocr_conv2d.
extern "C" int msocr_conv1x1_split(const msocr_conv_desc* d, const void* in, const void* weight_planes, const float* bias,
                                   const void* residual, void* out, void* stream) {
  if (!d || d->dtype != MSOCR_F32) return MSOCR_E_ARG;
  if (conv_desc_check(d, in, weight_planes, residual, out, 4, 32, 64, CONV_STRIDES_DENSE) != MSOCR_OK) return MSOCR_E_ARG;
  ConvParams p = conv_params(d, in, weight_planes, bias, residual, out);
  p.wplane = (long)d->Cout * d->Cin;
  return launch_split_any(p, (hipStream_t)stream, false);
}

// Any kernel size / stride / padding with the weight operand as three K-tile-major bf16 planes of [Cout][KH*KW*Cin] (the strided 3x3 and 1x1
// convolutions of the ResNet trunks that have no Winograd form).  Same descriptor rules as msocr_conv2d for MSOCR_F32, plus
// Cin % 32 == 0 and Cout % 64 == 0.
extern "C" int msocr_conv2d_split(const msocr_conv_desc* d, const void* in, const void* weight_planes, const float* bias,
                                  const void* residual, void* out, void* stream) {
  if (!d || d->dtype != MSOCR_F32) return MSOCR_E_ARG;
  if (conv_desc_check(d, in, weight_planes, residual, out, 4, 32, 64, CONV_STRIDES_ALIGNED) != MSOCR_OK) return MSOCR_E_ARG;
  ConvParams p = conv_params(d, in, weight_planes, bias, residual, out);
  p.wplane = (long)d->Cout * p.Ktot;
  // the general loader keeps signed 32-bit byte offsets from the input pointer: a batch whose input extent reaches 2 GB is launched
  // image range by image range (outputs of different images are independent)
  const long img_bytes = (long)d->in_sN * 4;
  if (img_bytes >= (1L << 31)) return MSOCR_E_ARG;
  const int per = (int)(((1L << 31) - 1) / (img_bytes > 0 ? img_bytes : 1));
  if (d->N <= per) return launch_split_any(p, (hipStream_t)stream, true);
  const long out_img = (long)d->Ho * d->Wo * d->out_ld * 4, res_img = (long)d->Ho * d->Wo * d->res_ld * 4;
  for (int n0 = 0; n0 < d->N; n0 += per) {
    ConvParams q = p;
    q.N = d->N - n0 < per ? d->N - n0 : per;
    q.M = (long)q.N * d->Ho * d->Wo;
    q.in = p.in + (long)n0 * img_bytes;
    q.out = p.out + (long)n0 * out_img;
    if (p.has_res) q.res = p.res + (long)n0 * res_img;
    const int rc = launch_split_any(q, (hipStream_t)stream, true);
    if (rc != MSOCR_OK) return rc;
  }
  return MSOCR_OK;
}

// nbatch independent GEMMs of one shape in ONE launch, C[b][m][n] = sum_k A[b][m][k] * B[b][n][k]: A f32 [nbatch][M][K],
// B as three K-tile-major bf16 planes [3][nbatch][K/32][N][32], C f32 [nbatch][M][N].  The Winograd-domain GEMMs (winograd.hip).
int msocr_internal_gemm_split_batched(const float* A, const uint16_t* Bplanes, float* C, long M, int N, int K, int nbatch, hipStream_t s) {
  ConvParams p;
  if (gemm_params(A, Bplanes, C, M, N, K, nbatch, 64, 32, &p) != MSOCR_OK) return MSOCR_E_ARG;
  p.wplane = (long)nbatch * N * K;
  return launch_split_any(p, s, false);
}
