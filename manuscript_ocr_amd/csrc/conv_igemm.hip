// conv_igemm.hip — im2col-free implicit-GEMM convolution on MFMA for gfx950 (MI355X).
//
// GEMM view: D[M = N*Ho*Wo][Cout] = A[M][K = KH*KW*Cin] * W^T, NHWC activations, weights
// [Cout][KH][KW][Cin].  Both operands are K-contiguous, so both LDS tiles are [rows][BK]
// with 16-byte chunks XOR-swizzled by row (ds_read_b128 conflict-free), and one code path
// serves f32 (v_mfma_f32_32x32x2_f32, exact f32) and bf16 (v_mfma_f32_32x32x16_bf16).
// A K-tile never straddles a filter tap (Cin % BK == 0), so an A row is one 16-B-aligned
// contiguous run of the input: plain global_load_dwordx4 with a zero fill for padding.
// 256 threads = 4 waves, each wave owns a (WM x WN) sub-tile as 32x32 MFMA tiles.
// Epilogue: accumulators -> LDS -> (bias, residual, ReLU) -> 16-byte coalesced stores.
//
// Replaces nn.Conv2d+BatchNorm2d(+ReLU)(+residual add) on the reference hot path:
//   detectors/_east/east.py:13-30,56-67 ; recognizers/_trba/model/seresnet31.py:37-45,81-89,129-155
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv_common.h"

// LEAN: 1x1 kernel without padding (every 1x1 convolution and the batched GEMMs of the Winograd path) — a K-tile is a plain
// pointer increment, no tap decoding, no bounds masks (rows >= M load valid garbage that the epilogue never stores).  PMC on
// the Winograd GEMM counted 1.9 VALU + 1.2 SALU instructions per MFMA in the general loader; they share the SIMD's issue port.
// WPE: workgroups per CU the register allocation is held to (0 = 3 for the one-stage 128-byte-row form, else 2).
template <typename T, int BM, int BN, int BKB, int WM, int WN, int STAGES = 2, bool LEAN = false, int MT = 32, int WPE = 0>
__global__ __launch_bounds__(256, WPE ? WPE : ((STAGES == 1 && BKB <= 128) ? 3 : 2)) void conv_igemm_kernel(ConvParams p) {
  using G = IgemmTile<T, BM, BN, BKB, WM, STAGES>;
  constexpr int ES = sizeof(T);
  constexpr int CPR = G::CPR;
  constexpr int EPC = 16 / ES;   // elements per chunk
  constexpr int BK = G::BK;
  constexpr int WAVES_N = BN / WN;
  static_assert(MT == 32 || (MT == 16 && sizeof(T) == 4), "16x16x4 is the f32 shape");
  constexpr int TM = WM / MT, TN = WN / MT;
  constexpr int AE = MT == 32 ? 16 : 4;
  constexpr int CQ = 64 / MT;
  using AccT = typename std::conditional<MT == 32, f32x16, f32x4>::type;
  static_assert((BM / WM) * WAVES_N == 4, "4 waves");
  constexpr int RPP = G::RPP, A_IT = G::A_IT, B_IT = G::B_IT;
  constexpr int A_BYTES = G::A_BYTES, STAGE = G::STAGE;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  int batch, tile_m, tile_n;
  tile_coords(p, xcd_tile<int>(blockIdx.x, p.tilesM * p.tilesN * p.nbatch), batch, tile_m, tile_n);
  const char* const g_in = p.in + (long)batch * p.bsA * ES;
  const char* const g_w = p.w + (long)batch * p.bsW * ES;
  char* const g_out = p.out + (long)batch * p.bsO * ES;

  // ---- per-thread staging coordinates (fixed over the K loop).  This kernel keeps 64-bit element offsets / pointers per row (its
  //      registers allow it), and rows past M read the zero block ----
  const int chunk = tid % CPR;
  const int row0 = tid / CPR;
  long a_base[A_IT];
  ATap<true> a_tap[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const long m = (long)tile_m * BM + row0 + i * RPP;
    if (m < p.M) {
      a_base[i] = a_row_origin(p, m, a_tap[i]) + chunk * EPC;
    } else {
      a_tap[i].hi0 = -0x40000000;  // never in range
      a_tap[i].wi0 = 0;
      a_base[i] = 0;
    }
  }
  const char* b_ptr[B_IT];
#pragma unroll
  for (int j = 0; j < B_IT; ++j) {
    const int co = tile_n * BN + row0 + j * RPP;
    b_ptr[j] = g_w + ((long)co * p.Ktot + chunk * EPC) * ES;
  }

  u32x4 ra[A_IT], rb[B_IT];
  TapCursor tap;
  tap.reset();

  const char* a_ptr[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) a_ptr[i] = g_in + a_base[i] * ES;
  auto load_tile = [&](int kt) {
    if constexpr (LEAN) {
#pragma unroll
      for (int i = 0; i < A_IT; ++i) ra[i] = *reinterpret_cast<const u32x4*>(a_ptr[i] + (long)kt * BKB);
#pragma unroll
      for (int j = 0; j < B_IT; ++j) {
        if (BN % RPP == 0 || row0 + j * RPP < BN) rb[j] = *reinterpret_cast<const u32x4*>(b_ptr[j] + (long)kt * BKB);
      }
      return;
    }
    const long koff = tap.offset(p);
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      // branch-free: out-of-image taps read 16 zero bytes
      const char* src = tap.inside(p, a_tap[i]) ? g_in + (a_base[i] + koff) * ES : reinterpret_cast<const char*>(msocr_zero16);
      ra[i] = *reinterpret_cast<const u32x4*>(src);
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      if (BN % RPP == 0 || row0 + j * RPP < BN) rb[j] = *reinterpret_cast<const u32x4*>(b_ptr[j] + (long)kt * BKB);
    }
    tap.advance(p, BK);
  };
  auto store_tile = [&](int stage) {
    unsigned char* sa = smem + stage * STAGE;
    unsigned char* sb = sa + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int row = row0 + i * RPP;
      *reinterpret_cast<u32x4*>(sa + row * BKB + ((chunk ^ swz<BKB>(row)) << 4)) = ra[i];
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      const int row = row0 + j * RPP;
      if (BN % RPP == 0 || row < BN) *reinterpret_cast<u32x4*>(sb + row * BKB + ((chunk ^ swz<BKB>(row)) << 4)) = rb[j];
    }
  };

  AccT acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < AE; ++e) acc[i][j][e] = 0.f;

  const int r32 = lane & (MT - 1), half = lane / MT;

  load_tile(0);
  store_tile(0);
  __syncthreads();

  auto read_frags = [&](const unsigned char* sa, const unsigned char* sb, int q, u32x4 (&fa)[TM], u32x4 (&fb)[TN]) {
    const int c = CQ * q + half;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WM + i * MT + r32;
      fa[i] = *reinterpret_cast<const u32x4*>(sa + row * BKB + ((c ^ swz<BKB>(row)) << 4));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wn * WN + j * MT + r32;
      fb[j] = *reinterpret_cast<const u32x4*>(sb + row * BKB + ((c ^ swz<BKB>(row)) << 4));
    }
  };
  constexpr int NQ = CPR / CQ;
  for (int kt = 0; kt < p.ktiles; ++kt) {
    const int cur = STAGES == 1 ? 0 : (kt & 1);
    if (kt + 1 < p.ktiles) load_tile(kt + 1);  // global loads in flight under the MFMAs
    const unsigned char* sa = smem + cur * STAGE;
    const unsigned char* sb = sa + A_BYTES;
    if constexpr (MT == 16) {
      // 16x16x4: 16 accumulator tiles per wave; fragments are read just in time (8 x b128 per 16 k), no second fragment buffer
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        u32x4 fa[TM], fb[TN];
        read_frags(sa, sb, q, fa, fb);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(fa[i][e]), __uint_as_float(fb[j][e]), acc[i][j], 0, 0, 0);
      }
    } else {
    u32x4 fa[2][TM], fb[2][TN];
      read_frags(sa, sb, 0, fa[0], fb[0]);
  #pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q + 1 < NQ) {  // LDS reads of the next k-group are issued BEFORE this group's MFMAs and stay pinned there
          read_frags(sa, sb, q + 1, fa[(q + 1) & 1], fb[(q + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (sizeof(T) == 4) {
          // k-element outermost: consecutive MFMAs hit different accumulators (no back-to-back dependent issue)
  #pragma unroll
          for (int e = 0; e < 4; ++e)
  #pragma unroll
            for (int i = 0; i < TM; ++i)
  #pragma unroll
              for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[q & 1][i][e]), __uint_as_float(fb[q & 1][j][e]),
                                                                 acc[i][j], 0, 0, 0);
        } else {
  #pragma unroll
          for (int i = 0; i < TM; ++i)
  #pragma unroll
            for (int j = 0; j < TN; ++j) Mma<T>::run(fa[q & 1][i], fb[q & 1][j], acc[i][j]);
        }
      }
    }
    if (STAGES == 1) {  // one LDS stage (3 workgroups per CU): everyone must be done reading before it is overwritten
      __syncthreads();
      if (kt + 1 < p.ktiles) store_tile(0);
    } else if (kt + 1 < p.ktiles) {
      store_tile(cur ^ 1);
    }
    __syncthreads();
  }

  epilogue_lds<T, BM, BN, WM, WN, MT, false, WPE == 4 ? 2 : 1>(p, smem, acc, tile_m, tile_n, g_out, wm, wn, r32, half);
}

template <typename T, int BM, int BN, int BKB, int WM, int WN, int STAGES = 2, bool LEAN = false, int MT = 32, int WPE = 0>
static int launch_cfg(ConvParams& p, hipStream_t s) {
  return conv_launch<IgemmTile<T, BM, BN, BKB, WM, STAGES>>(conv_igemm_kernel<T, BM, BN, BKB, WM, WN, STAGES, LEAN, MT, WPE>, p, s);
}

template <typename T>
static int launch_typed(ConvParams& p, hipStream_t s) {
  constexpr int ES = sizeof(T);
  // row bytes: 128 B when Cin allows (f32: BK 32, bf16: BK 64), else 64 B
  const bool wide = (p.Cin * ES) % 128 == 0;
  // The f32 instances keep ONE LDS stage at 3-4 workgroups per CU (a resident neighbour covers the others' prologue / epilogue: worth
  // 3-5 % at short K); bf16 keeps the register-staged double buffer at 2 per CU.  `lean` = 1x1 kernel without padding.
  const bool lean = p.KH == 1 && p.KW == 1 && p.PH == 0 && p.PW == 0;
  if (p.Cout % 128 == 0) {
    if constexpr (sizeof(T) == 4) {
      // lean: v_mfma_f32_16x16x4_f32 tiles, K-tiles of 16 (64-byte rows), 128 VGPRs, FOUR workgroups per CU (round 2: +2.3 % on the
      // pipeline against K-tiles of 32 at 3 per CU; K-tiles of 64, staggered workgroup starts, two LDS stages and a direct-store
      // epilogue all measured within 1 % of these two and are gone)
      if (wide && lean) return launch_cfg<T, 128, 128, 64, 64, 64, 1, true, 16, 4>(p, s);
      if (wide) return launch_cfg<T, 128, 128, 128, 64, 64, 1>(p, s);
    }
    return wide ? launch_cfg<T, 128, 128, 128, 64, 64>(p, s) : launch_cfg<T, 128, 128, 64, 64, 64>(p, s);
  } else if (p.Cout % 64 == 0) {
    if constexpr (sizeof(T) == 4) {
      if (wide && lean) return launch_cfg<T, 128, 64, 128, 64, 32, 2, true>(p, s);
    }
    return wide ? launch_cfg<T, 128, 64, 128, 64, 32>(p, s) : launch_cfg<T, 128, 64, 64, 64, 32>(p, s);
  } else {
    return wide ? launch_cfg<T, 256, 32, 128, 64, 32>(p, s) : launch_cfg<T, 256, 32, 64, 64, 32>(p, s);
  }
}

extern "C" int msocr_conv2d(const msocr_conv_desc* d, const void* in, const void* weight, const float* bias,
                            const void* residual, void* out, void* stream) {
  if (!d) return MSOCR_E_ARG;
  const int ES = d->dtype == MSOCR_F32 ? 4 : (d->dtype == MSOCR_BF16 ? 2 : 0);
  if (!ES) return MSOCR_E_ARG;
  // Cin: a K-tile (64 bytes at least) lies inside one tap
  if (conv_desc_check(d, in, weight, residual, out, ES, 64 / ES, 32, CONV_STRIDES_TAPS) != MSOCR_OK) return MSOCR_E_ARG;
  ConvParams p = conv_params(d, in, weight, bias, residual, out);
  hipStream_t s = (hipStream_t)stream;
  return d->dtype == MSOCR_F32 ? launch_typed<float>(p, s) : launch_typed<__bf16>(p, s);
}

// nbatch independent f32 GEMMs of one shape in ONE launch: C[b][m][n] = sum_k A[b][m][k] * B[b][n][k]
// (A [nbatch][M][K], B [nbatch][N][K], C [nbatch][M][N], all dense).  Used by the Winograd path (winograd.hip).
int msocr_internal_gemm_f32_batched(const float* A, const float* B, float* C, long M, int N, int K, int nbatch, hipStream_t s) {
  ConvParams p;
  if (gemm_params(A, B, C, M, N, K, nbatch, 32, 16, &p) != MSOCR_OK) return MSOCR_E_ARG;
  return launch_typed<float>(p, s);
}
