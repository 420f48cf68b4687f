// conv_common.h — what the MFMA convolution / GEMM kernels share (conv_igemm.hip: exact-f32 and bf16 operands; conv_split.hip and
// conv_split_pp.hip: f32 operands split into three bf16 terms; winograd.hip: the tile map): types, the tile geometry each kernel and
// its launcher are built from, the loaders' device helpers, the epilogue through LDS, and the host glue between a descriptor and a
// launch.  Not part of the C ABI.
#ifndef MSOCR_CONV_COMMON_H
#define MSOCR_CONV_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "internal.h"
#include "msocr.h"
#include "split_mma.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct ConvParams {
  const char* in;
  const char* w;
  const float* bias;
  const char* res;
  char* out;
  int N, H, W, Cin;
  long sN, sH, sW;
  int KH, KW, SH, SW, PH, PW;
  int Ho, Wo, Cout;
  long M;
  int ktiles, cin_tiles;
  long Ktot;
  long out_ld, res_ld;
  int relu, has_res;
  int tilesM, tilesN;
  int nbatch;           // independent problems of identical shape in one launch (Winograd: the 16 transform points)
  long bsA, bsW, bsO;   // element strides between consecutive problems (input, weight, output)
  long wplane;          // conv_split.hip: elements between the three bf16 planes of the split weight operand
  long w_kt_b;          // conv_split.hip: bytes between consecutive K-tiles of a weight plane (K-tile-major planes: Cout * 64)
};

__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN-preserving
  return *reinterpret_cast<uint16_t*>(&b);
}

template <typename T>
struct Mma;
template <>
struct Mma<float> {
  // one 16-byte chunk = 4 consecutive k for this lane's (row, k-half): 4 MFMA 32x32x2 steps
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[j]), __uint_as_float(b[j]), c, 0, 0, 0);
  }
};
template <>
struct Mma<__bf16> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
    bf16x8 av = __builtin_bit_cast(bf16x8, a);
    bf16x8 bv = __builtin_bit_cast(bf16x8, b);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, c, 0, 0, 0);
  }
};

// conv_split_pp.hip: the producer / consumer form of the split-operand kernel (Cout % 128 == 0); same ConvParams as conv_split_kernel
__attribute__((visibility("hidden"))) bool msocr_internal_split_pp_takes(const ConvParams& p);
__attribute__((visibility("hidden"))) int msocr_internal_split_pp_launch(ConvParams& p, hipStream_t s, bool general);

// BKB = bytes per tile row (64 or 128).  swizzle: 16-B chunk index ^= (row / rows_per_256B) % chunks_per_row
template <int BKB>
__device__ __forceinline__ int swz(int row) {
  constexpr int CPR = BKB / 16;
  constexpr int RPB = 256 / BKB;
  return (row / RPB) & (CPR - 1);
}
// conv_split_pp.hip: LDS rows are 64 bytes (one K-tile of 32 bf16); a 16x16x32 fragment read takes 16-byte chunk lane / 16 of row
// lane % 16.  This XOR of the chunk index by row makes every ds_read_b128 lane group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...)
// hit 16 distinct 16-byte slots (tools/microbench/mfma_energy.hip uses the same map; checked with SQ_LDS_BANK_CONFLICT).
__device__ __forceinline__ int swz16(int row) { return (4 - ((row >> 2) & 3)) & 3; }
// ---- tile geometry: the kernel and its launcher take every size from the same struct ---------------------------------------------
// conv_igemm_kernel: one stage = [BM + BN] rows of BKB bytes, 256 threads stage RPP rows per pass
template <typename T, int BM_, int BN_, int BKB_, int WM_, int STAGES_>
struct IgemmTile {
  static constexpr int BM = BM_, BN = BN_, BKB = BKB_, THREADS = 256, PERSISTENT = 0;
  static constexpr int BK = BKB / (int)sizeof(T);
  static constexpr int CPR = BKB / 16;   // 16-B chunks per tile row
  static constexpr int RPP = 256 / CPR;  // tile rows covered per pass of 256 threads
  static constexpr int A_IT = BM / RPP, B_IT = (BN + RPP - 1) / RPP;
  static constexpr int A_BYTES = BM * BKB, B_BYTES = BN * BKB, STAGE = A_BYTES + B_BYTES;
  static constexpr int EPI = (BM / WM_) * 32 * BN * 4;  // the epilogue's [rows per pass][BN] f32
  static constexpr int LDS = STAGES_ * STAGE > EPI ? STAGES_ * STAGE : EPI;
};
// the split-operand kernels: K-tiles of 32, one stage = three [BM][64 B] planes of A and three [BN][64 B] planes of B; 256 threads
// stage A as 16-B chunks of 4 f32 (ARP rows per pass) and B as 16-B chunks of 8 bf16 (BRP rows per pass)
template <int BM_, int BN_>
struct SplitStage {
  static constexpr int BM = BM_, BN = BN_, BK = 32;
  static constexpr int ROWB = BK * 2;  // bytes per LDS plane row (BK bf16)
  static constexpr int A_PLANE = BM * ROWB, B_PLANE = BN * ROWB;
  static constexpr int STAGE_B = 3 * (A_PLANE + B_PLANE);
  static constexpr int ACH = BK / 4, ARP = 256 / ACH, A_IT = BM / ARP;
  static constexpr int BCH = BK / 8, BRP = 256 / BCH, B_IT = (BN + BRP - 1) / BRP;
};
// conv_split_kernel: 128 x BN, wave tile 64 x BN / 2, one stage (or the epilogue's [64][BN] f32)
template <int BN_>
struct SplitTile : SplitStage<128, BN_> {
  static constexpr int WM = 64, WN = BN_ / 2, THREADS = 256, PERSISTENT = 0;
  static constexpr int EPI = (128 / WM) * 32 * BN_ * 4;
  static constexpr int LDS = SplitStage<128, BN_>::STAGE_B > EPI ? SplitStage<128, BN_>::STAGE_B : EPI;
  static __device__ __forceinline__ int swz(int row) { return ::swz<64>(row); }  // 16-B chunk swizzle of a plane row
};
// conv_split_pp_kernel: 64 TM x 64 TN, two stages and 4 slots of BN bias floats behind them; a persistent grid
template <int TM, int TN>
struct SplitPPTile : SplitStage<64 * TM, 64 * TN> {
  static constexpr int THREADS = 512, PERSISTENT = 1;
  static constexpr int BIAS_OFF = 2 * SplitStage<64 * TM, 64 * TN>::STAGE_B;
  static constexpr int LDS = BIAS_OFF + 4 * 64 * TN * 4;
  static __device__ __forceinline__ int swz(int row) { return swz16(row); }
};

// ---- device helpers ---------------------------------------------------------------------------------------------------------------
// 16 zero bytes: padded (out-of-image) taps load from here, so the operand tile needs no masking.  Mutable on purpose: loads from a
// const block are folded by the compiler and the loaders' select of two addresses turns into a select of two values.
static __device__ __attribute__((aligned(16))) uint32_t msocr_zero16[4] = {0u, 0u, 0u, 0u};

// XCD-aware tile map: workgroups b, b + 8, ... share an XCD and its L2, so XCD x gets a CONTIGUOUS range of the nblk logical tiles
// (neighbouring tiles share operand rows, 3x3 halos and weights): the range's first tile, its length, and the tile of workgroup bid
// when there is one workgroup per tile.
template <typename I>
__device__ __forceinline__ void xcd_range(I x, I nblk, I& first, I& count) {
  const I q = nblk >> 3, r = nblk & 7;
  first = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  count = q + (x < r ? 1 : 0);
}
template <typename I>
__device__ __forceinline__ I xcd_tile(I bid, I nblk) {
  I first, count;
  xcd_range<I>(bid & 7, nblk, first, count);
  return first + (bid >> 3);
}
// logical tile t of a launch -> problem of the batch, M-tile, N-tile (N-tiles fastest)
__device__ __forceinline__ void tile_coords(const ConvParams& p, int t, int& batch, int& tile_m, int& tile_n) {
  const int nblk1 = p.tilesM * p.tilesN;
  batch = t / nblk1;
  t -= batch * nblk1;
  tile_n = t % p.tilesN;
  tile_m = t / p.tilesN;
}

// A operand, general loader: row m of the GEMM is output pixel (n, ho, wo); ATap keeps the input pixel of its tap (0, 0), which may
// lie outside the image.  The lean loaders (a K-tile is a pointer increment) keep nothing per row but the offset.
template <bool GEN>
struct ATap { int hi0, wi0; };
template <>
struct ATap<false> {};
// element offset of that pixel from the input pointer
__device__ __forceinline__ long a_row_origin(const ConvParams& p, long m, ATap<true>& t) {
  const long hw = (long)p.Ho * p.Wo;
  const int n = (int)(m / hw);
  const int rem = (int)(m - (long)n * hw);
  const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
  t.hi0 = ho * p.SH - p.PH;
  t.wi0 = wo * p.SW - p.PW;
  return (long)n * p.sN + (long)t.hi0 * p.sH + (long)t.wi0 * p.sW;
}
// The split kernels address with a wave-uniform 64-bit base plus a 32-bit per-thread byte offset (one VGPR per load instead of a
// pointer).  GEN: signed, < 2 GB in magnitude; lean: row m is pixel m of a dense pixel sequence of stride sW, unsigned, < 4 GB (host
// checks).  Rows past the end take the last row's address: valid memory, values never stored.
template <bool GEN>
__device__ __forceinline__ uint32_t a_row_offset32(const ConvParams& p, long m, int a_chunk, ATap<GEN>& t) {
  if (m >= p.M) m = p.M - 1;
  if constexpr (GEN) return (uint32_t)(int32_t)((a_row_origin(p, m, t) + a_chunk * 4) * 4);
  else return (uint32_t)((m * p.sW + a_chunk * 4) * 4);
}
// (kh, kw, c0) of the NEXT K-tile the general loader fetches, advanced incrementally (K-tiles are visited in order and never straddle
// a tap): no divisions in the K loop
struct TapCursor {
  int kh, kw, c0;
  __device__ __forceinline__ void reset() { kh = kw = c0 = 0; }
  __device__ __forceinline__ long offset(const ConvParams& p) const { return (long)kh * p.sH + (long)kw * p.sW + c0; }  // elements, uniform
  __device__ __forceinline__ bool inside(const ConvParams& p, const ATap<true>& t) const {
    const int hi = t.hi0 + kh, wi = t.wi0 + kw;
    return (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
  }
  __device__ __forceinline__ void advance(const ConvParams& p, int bk) {
    c0 += bk;
    if (c0 == p.Cin) {
      c0 = 0;
      if (++kw == p.KW) { kw = 0; ++kh; }
    }
  }
};
// one K-tile of A through the general loader, branch-free (out-of-image taps read the zero block); 32-bit offsets stay in registers
// and the 64-bit address is formed per load
template <int A_IT>
__device__ __forceinline__ void load_a_taps32(const ConvParams& p, const char* g_in, const uint32_t (&a_off)[A_IT],
                                              const ATap<true> (&tap)[A_IT], TapCursor& t, int bk, u32x4 (&ra)[A_IT]) {
  const int32_t koff = (int32_t)(t.offset(p) * 4);  // uniform
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const char* src = g_in + (long)(int32_t)(a_off[i] + (uint32_t)koff);
    ra[i] = *reinterpret_cast<const u32x4*>(t.inside(p, tap[i]) ? src : reinterpret_cast<const char*>(msocr_zero16));
  }
  t.advance(p, bk);
}
template <int A_IT>
__device__ __forceinline__ void load_a_rows32(const char* ga, const uint32_t (&a_off)[A_IT], u32x4 (&ra)[A_IT]) {
#pragma unroll
  for (int i = 0; i < A_IT; ++i) ra[i] = *reinterpret_cast<const u32x4*>(ga + a_off[i]);
}
// B operand of the split kernels: three K-tile-major bf16 planes [k / 32][Cout][32], so the rows of a tile are one dense block.
// Byte offset of weight row co inside a K-tile of a plane, for the thread that stages 16-B chunk b_chunk of it.  (This helper and
// the two stores below take ONE row by value and leave the loop to the kernel: as whole-array helpers taking the register arrays
// by reference they kept every count of tools/check_isa.sh but reordered conv_split_pp_kernel's producers, measurably.)
__device__ __forceinline__ uint32_t b_plane_offset(int co, int cout, int b_chunk) {
  if (co >= cout) co = cout - 1;
  return (uint32_t)(co * 64 + b_chunk * 16);
}
template <class G>
__device__ __forceinline__ void load_b_planes(const ConvParams& p, const char* g_w, long wplane_b, int kt, int b_row0,
                                              const uint32_t (&b_off)[G::B_IT], u32x4 (&rb)[3][G::B_IT]) {
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const char* const gb = g_w + pl * wplane_b + (long)kt * p.w_kt_b;  // uniform
#pragma unroll
    for (int j = 0; j < G::B_IT; ++j)
      if (G::BN % G::BRP == 0 || b_row0 + j * G::BRP < G::BN) rb[pl][j] = *reinterpret_cast<const u32x4*>(gb + b_off[j]);
  }
}
// registers -> LDS stage: a row's 16 bytes of A are split on the way into the three planes [BM][ROWB], B arrives split; G::swz is
// the kernel's chunk swizzle
template <class G>
__device__ __forceinline__ void split_store_row(unsigned char* sA, int row, int a_chunk, u32x4 r) {
  float x0 = __uint_as_float(r[0]), x1 = __uint_as_float(r[1]), x2 = __uint_as_float(r[2]), x3 = __uint_as_float(r[3]);
  // this thread's 4 elements are bf16 positions 4 * a_chunk .. + 3 of the row: half of 16-B chunk a_chunk / 2
  unsigned char* dst = sA + row * G::ROWB + (((a_chunk >> 1) ^ G::swz(row)) << 4) + ((a_chunk & 1) << 3);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    u32x2 v;
    v[0] = split_step(x0, x1);
    v[1] = split_step(x2, x3);
    *reinterpret_cast<u32x2*>(dst + pl * G::A_PLANE) = v;
  }
}
template <class G>
__device__ __forceinline__ void store_b_row(unsigned char* sB, int pl, int row, int b_chunk, u32x4 v) {
  *reinterpret_cast<u32x4*>(sB + pl * G::B_PLANE + row * G::ROWB + ((b_chunk ^ G::swz(row)) << 4)) = v;
}

// Epilogue of the 4-wave kernels (conv_igemm_kernel, conv_split_kernel): WM / 32 passes of (acc row-block -> LDS [PR][BN] f32 ->
// bias / residual / ReLU -> 16-byte coalesced stores).  acc[tile row][tile column] of MT x MT MFMA tiles, T the element type in HBM.
// BIAS16: the thread's four f32 bias values come as one 16-byte load (conv_split_kernel) instead of one load each (conv_igemm_kernel)
// — the same values; each kernel keeps the load count it was measured with.
// One memory round trip per pass, not one per row: stores count on vmcnt on this target, so a rolled row loop (load the residual
// row, wait, add, store, next row) waits for the previous row's store and its own load on every one of its NR rows.  A tile that lies
// wholly below M therefore runs straight-line code per pass: all residual rows loaded before the accumulator -> LDS write and the
// barriers, all LDS rows read at once, every row in registers of its own, stores never waited for (only LDS reuse orders the passes).
// The row guard has to stay out of that path: loads or stores under a per-row branch make the compiler's wait counts conservative
// again (a skipped later load leaves fewer operations outstanding), so the last, partial M-tile of a launch takes the guarded
// row-by-row loop instead.  NCH = 2 (conv_igemm_kernel at 128 registers): the pass by halves where a later pass's accumulators are
// still alive.  Every path adds in the same order per element, so results do not depend on the path.
template <typename T, int BM, int BN, int WM, int WN, int MT, bool BIAS16, int NCH = 1, typename AccT, int TMA, int TN>
__device__ __forceinline__ void epilogue_lds(const ConvParams& p, unsigned char* smem, const AccT (&acc)[TMA][TN], int tile_m, int tile_n,
                                             char* g_out, int wm, int wn, int r32, int half) {
  constexpr int ES = sizeof(T), EPC = 16 / ES;
  constexpr int AE = MT == 32 ? 16 : 4;
  const int tid = threadIdx.x;
  constexpr int PR = (BM / WM) * 32;  // tile rows handled per pass
  float* sc = reinterpret_cast<float*>(smem);
  constexpr int VPR = BN / EPC;       // 16-B output vectors per tile row
  constexpr int ROWS_PP = 256 / VPR;  // rows per sweep of 256 threads
  const int vcol = (tid % VPR) * EPC;
  const int vrow0 = tid / VPR;
  const int co = tile_n * BN + vcol;
  float bias[EPC];
  if constexpr (BIAS16) {
    static_assert(EPC == 4, "four f32");
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) b = *reinterpret_cast<const f32x4*>(p.bias + co);
    bias[0] = b[0]; bias[1] = b[1]; bias[2] = b[2]; bias[3] = b[3];
  } else {
#pragma unroll
    for (int e = 0; e < EPC; ++e) bias[e] = p.bias ? p.bias[co + e] : 0.f;
  }

  constexpr int TPP = 32 / MT;
  constexpr int NR = PR / ROWS_PP;  // rows of a pass per thread
  static_assert(PR % ROWS_PP == 0 && NR % NCH == 0, "a pass is whole sweeps of 256 threads, a chunk whole rows");
  // whole_tile's row_step needs tile_row(i, vrow0 + r * ROWS_PP) == tile_row(0, vrow0) + tile_row(i, r * ROWS_PP): true when a sweep
  // never straddles a 32-row block (ROWS_PP divides 32) or covers whole blocks from the block's start (ROWS_PP == 64)
  static_assert(32 % ROWS_PP == 0 || ROWS_PP == 64, "tile_row must be additive in the sweep index (see row_step)");
  const long m0 = (long)tile_m * BM;
  // tile row of row lr of pass i
  auto tile_row = [&](int i, int lr) { return (lr >> 5) * WM + i * 32 + (lr & 31); };
  auto lds_write = [&](int i) {
#pragma unroll
    for (int ti = 0; ti < TPP; ++ti)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < AE; ++e) {
          const int rit = MT == 32 ? acc_row(e, half) : 4 * half + e;
          sc[(wm * 32 + ti * MT + rit) * BN + wn * WN + j * MT + r32] = acc[i * TPP + ti][j][e];
        }
  };
  auto lds_row = [&](int lr, float (&v)[EPC]) {
#pragma unroll
    for (int e4 = 0; e4 < EPC; e4 += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(&sc[lr * BN + vcol + e4]);
      v[e4] = t[0]; v[e4 + 1] = t[1]; v[e4 + 2] = t[2]; v[e4 + 3] = t[3];
    }
  };
  // accumulator, + bias, + residual, ReLU, conversion, store: one order per element for every path below
  auto finish_row = [&](float (&v)[EPC], bool res, const u32x4& rv, char* dst) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] += bias[e];
    if (res) {
      if constexpr (ES == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __uint_as_float(rv[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)(rv[e >> 1] >> ((e & 1) * 16)));
      }
    }
    if (p.relu) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    u32x4 o;
    if constexpr (ES == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = __float_as_uint(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (uint32_t)f32_to_bf16(v[2 * e]) | ((uint32_t)f32_to_bf16(v[2 * e + 1]) << 16);
    }
    *reinterpret_cast<u32x4*>(dst) = o;
  };
  // a tile with all BM rows below M (see above).  NCH = 2 reads the LDS rows and stores by halves; its residual rows are all loaded
  // early in the last pass, and by halves while the accumulators of a later pass are alive (128 registers did not hold more without
  // a spill, and a reloaded spill waits for every load in flight).
  auto whole_tile = [&](auto res_c) {
    constexpr bool RES = decltype(res_c)::value;
    constexpr int CR = NR / NCH;  // rows per chunk
    // the thread's rows are its first row plus a compile-time number of tile rows: one 64-bit address per thread and operand, the
    // row steps are wave-uniform
    const long mt = m0 + tile_row(0, vrow0);
    const char* const res_t = RES ? p.res + (mt * p.res_ld + co) * ES : nullptr;
    char* const out_t = g_out + (mt * p.out_ld + co) * ES;
    auto row_step = [&](int i, int r) { return tile_row(i, r * ROWS_PP); };  // vrow0 < ROWS_PP, and ROWS_PP divides 32 or is 64
    auto load_res = [&](int i, int r0, int r1, u32x4 (&rv)[NR]) {
      if constexpr (RES) {
#pragma unroll
        for (int r = r0; r < r1; ++r) rv[r] = *reinterpret_cast<const u32x4*>(res_t + row_step(i, r) * p.res_ld * ES);
      }
    };
#pragma unroll
    for (int i = 0; i < WM / 32; ++i) {
      // rows whose residual is loaded before the barrier: all of them, or (NCH = 2) the first half while a later pass's accumulators
      // are still alive; the second half is then loaded behind the first half's stores
      const int early = (NCH == 1 || i == WM / 32 - 1) ? NR : CR;
      u32x4 rv[NR];
      load_res(i, 0, early, rv);
      if (i) __syncthreads();
      lds_write(i);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float v[CR][EPC];
#pragma unroll
        for (int r = 0; r < CR; ++r) lds_row(vrow0 + (c * CR + r) * ROWS_PP, v[r]);
#pragma unroll
        for (int r = 0; r < CR; ++r) finish_row(v[r], RES, rv[c * CR + r], out_t + row_step(i, c * CR + r) * p.out_ld * ES);
        if (c == 0 && early < NR) load_res(i, early, NR, rv);
      }
    }
  };
  if (m0 + BM <= p.M) {
    if (p.has_res) whole_tile(std::true_type{});
    else whole_tile(std::false_type{});
    return;
  }
  // the last, partial M-tile of a launch: row by row, a row with m >= M is neither loaded nor stored
#pragma unroll
  for (int i = 0; i < WM / 32; ++i) {
    if (i) __syncthreads();
    lds_write(i);
    __syncthreads();
    for (int lr = vrow0; lr < PR; lr += ROWS_PP) {
      const long m = m0 + tile_row(i, lr);
      if (m >= p.M) continue;
      float v[EPC];
      lds_row(lr, v);
      u32x4 rv = {0u, 0u, 0u, 0u};
      if (p.has_res) rv = *reinterpret_cast<const u32x4*>(p.res + (m * p.res_ld + co) * ES);
      finish_row(v, p.has_res != 0, rv, g_out + (m * p.out_ld + co) * ES);
    }
  }
}

// ---- host glue: descriptor -> ConvParams -> launch -------------------------------------------------------------------------------
// What an entry point demands of the input strides (everything else is common to the three):
enum ConvStrideRule {
  CONV_STRIDES_TAPS,     // msocr_conv2d: every pixel a tap can touch starts 16-byte aligned; the pads are not looked at
  CONV_STRIDES_ALIGNED,  // msocr_conv2d_split: all three strides are multiples of a 16-byte chunk, pads >= 0
  CONV_STRIDES_DENSE,    // msocr_conv1x1_split: 1x1 / stride 1 / no padding over ONE dense pixel sequence of stride in_sW
};
// MSOCR_OK or MSOCR_E_ARG.  es = element size of the activations; Cin % cin_mult == 0 and Cout % cout_mult == 0.
static inline int conv_desc_check(const msocr_conv_desc* d, const void* in, const void* weight, const void* residual, const void* out, int es,
                                  int cin_mult, int cout_mult, ConvStrideRule rule) {
  if (!d || !in || !weight || !out) return MSOCR_E_ARG;
  const int EPC = 16 / es;  // elements per 16-byte vector access
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0) return MSOCR_E_ARG;
  if (d->Cin <= 0 || d->Cin % cin_mult || d->Cout <= 0 || d->Cout % cout_mult) return MSOCR_E_ARG;
  if (d->KH <= 0 || d->KW <= 0 || d->stride_h <= 0 || d->stride_w <= 0) return MSOCR_E_ARG;
  if (d->out_ld % EPC || d->out_ld < d->Cout) return MSOCR_E_ARG;
  if (rule == CONV_STRIDES_TAPS) {
    // rows / pixels the kernel can touch: hi = ho*sh - ph + kh, wi = wo*sw - pw + kw; every one must start 16-B aligned
    if (d->in_sN % EPC) return MSOCR_E_ARG;
    if (d->in_sH % EPC) {
      if ((d->stride_h * d->in_sH) % EPC) return MSOCR_E_ARG;
      for (int kh = 0; kh < d->KH; ++kh)
        if (((kh - d->pad_h) * d->in_sH) % EPC) return MSOCR_E_ARG;
    }
    if (d->in_sW % EPC) {  // e.g. the C=4 stem canvas: pixels are 8 B in bf16, only even pixels are read
      if ((d->stride_w * d->in_sW) % EPC) return MSOCR_E_ARG;
      for (int kw = 0; kw < d->KW; ++kw)
        if (((kw - d->pad_w) * d->in_sW) % EPC) return MSOCR_E_ARG;
    }
  } else if (rule == CONV_STRIDES_ALIGNED) {
    if (d->pad_h < 0 || d->pad_w < 0 || d->in_sN % EPC || d->in_sH % EPC || d->in_sW % EPC) return MSOCR_E_ARG;
  } else {
    if (d->KH != 1 || d->KW != 1 || d->stride_h != 1 || d->stride_w != 1 || d->pad_h || d->pad_w || d->Ho != d->H || d->Wo != d->W)
      return MSOCR_E_ARG;
    // pixel stride sW, rows and images contiguous in units of it
    if (d->in_sW % EPC || d->in_sW < d->Cin || (d->H > 1 && d->in_sH != (int64_t)d->W * d->in_sW) ||
        (d->N > 1 && d->in_sN != (int64_t)d->H * d->W * d->in_sW)) return MSOCR_E_ARG;
  }
  if (((uintptr_t)in | (uintptr_t)weight | (uintptr_t)out) & 15) return MSOCR_E_ARG;
  if ((d->flags & MSOCR_CONV_RESIDUAL) && (!residual || d->res_ld % EPC || d->res_ld < d->Cout || ((uintptr_t)residual & 15))) return MSOCR_E_ARG;
  // output extent must agree with the conv arithmetic (guards the kernel's indexing)
  if ((d->H + 2 * d->pad_h - d->KH) / d->stride_h + 1 < d->Ho || (d->W + 2 * d->pad_w - d->KW) / d->stride_w + 1 < d->Wo)
    return MSOCR_E_ARG;
  return MSOCR_OK;
}
// a checked descriptor as kernel arguments (one problem; the tile counts are the launcher's, the plane strides the split entries')
static inline ConvParams conv_params(const msocr_conv_desc* d, const void* in, const void* weight, const float* bias, const void* residual,
                                     void* out) {
  ConvParams p = {};
  p.in = (const char*)in; p.w = (const char*)weight; p.bias = bias; p.res = (const char*)residual; p.out = (char*)out;
  p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin;
  p.sN = d->in_sN; p.sH = d->in_sH; p.sW = d->in_sW;
  p.KH = d->KH; p.KW = d->KW; p.SH = d->stride_h; p.SW = d->stride_w; p.PH = d->pad_h; p.PW = d->pad_w;
  p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout;
  p.M = (long)d->N * d->Ho * d->Wo;
  p.Ktot = (long)d->KH * d->KW * d->Cin;
  p.out_ld = d->out_ld; p.res_ld = d->res_ld;
  p.relu = (d->flags & MSOCR_CONV_RELU) ? 1 : 0;
  p.has_res = (d->flags & MSOCR_CONV_RESIDUAL) ? 1 : 0;
  p.nbatch = 1;
  return p;
}
// nbatch dense GEMMs C[b][m][n] = sum_k A[b][m][k] * B[b][n][k] as a 1x1 convolution over M pixels; MSOCR_E_ARG unless the pointers
// are 16-byte aligned, N % n_mult == 0 and K % k_mult == 0
static inline int gemm_params(const void* A, const void* B, void* C, long M, int N, int K, int nbatch, int n_mult, int k_mult, ConvParams* out) {
  if (!A || !B || !C || M <= 0 || N <= 0 || N % n_mult || K <= 0 || K % k_mult || nbatch <= 0) return MSOCR_E_ARG;
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) return MSOCR_E_ARG;
  if (M > 0x7fffffffL) return MSOCR_E_ARG;
  ConvParams p = {};
  p.in = (const char*)A; p.w = (const char*)B; p.out = (char*)C;
  p.N = 1; p.H = (int)M; p.W = 1; p.Cin = K;
  p.sN = M * (long)K; p.sH = K; p.sW = K;
  p.KH = p.KW = 1; p.SH = p.SW = 1;
  p.Ho = (int)M; p.Wo = 1; p.Cout = N;
  p.M = M; p.Ktot = K;
  p.out_ld = N;
  p.nbatch = nbatch; p.bsA = M * (long)K; p.bsW = (long)N * K; p.bsO = M * (long)N;
  *out = p;
  return MSOCR_OK;
}
// Launch tail: tile counts of geometry G, the kernel's dynamic-LDS limit, one workgroup per tile — or, for a persistent kernel, at
// most one per CU in multiples of 8 (the kernel walks the XCD ranges itself).
template <class G, class Kern>
static int conv_launch(Kern kern, ConvParams& p, hipStream_t s) {
  p.tilesM = (int)((p.M + G::BM - 1) / G::BM);
  p.tilesN = p.Cout / G::BN;
  p.cin_tiles = p.Cin / G::BK;
  p.ktiles = (int)(p.Ktot / G::BK);
  if (msocr_internal_lds_limit(reinterpret_cast<const void*>(kern), G::LDS) != MSOCR_OK) return MSOCR_E_LAUNCH;
  const long nblk = (long)p.tilesM * p.tilesN * p.nbatch;
  if (nblk <= 0 || nblk > 0x7fffffffL) return MSOCR_E_ARG;
  long grid = nblk;
  if (G::PERSISTENT) {
    int n_cu = 0;
    if (msocr_internal_cu_count(&n_cu) != MSOCR_OK) return MSOCR_E_LAUNCH;
    n_cu = n_cu > 8 ? n_cu & ~7 : 8;
    grid = (nblk + 7) & ~7L;
    if (grid > n_cu) grid = n_cu;
  }
  MSOCR_LAUNCH(kern, dim3((unsigned)grid), dim3(G::THREADS), G::LDS, s, p);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

#endif
