// attn_beam_mfma.hip — attention decode of the TRBA recogniser (beam search and greedy) with the step's three matrix products on
// the matrix cores: in the split-operand form (default, precision "fp32": every f32 operand as three bf16 terms, six
// v_mfma_f32_32x32x16_bf16 partial products per 16 k, f32 accumulation) or on the exact-f32 pipe (v_mfma_f32_32x32x2_f32,
// precision "fp32-exact" or no msocr_attn_split_weights; beam only).
//
// One 512-thread workgroup owns 32 state rows = one MFMA row block for the whole step loop: NB = 4 crops x 8 beam slots in
// attn_beam_mfma_kernel, 32 crops in attn_greedy_mfma_kernel (rows of different crops are independent: no inter-workgroup
// hand-off).  Every weight element a workgroup pulls from L2 feeds 32 rows, and the gate arithmetic is off the VALU.  The context
// half of the gate product is hoisted out of the step loop (see ctx_sum).  Per step:
//   (a) ph    = h2h(h)                     [32x256] x [256x256]        MFMA  (wave w: columns 32w..32w+31)
//   (b) e     = score . tanh(proj_H + ph)  32 x T dot products          VALU  (one wave per (crop, t) pair)
//   (c) alpha = softmax_t(e)                                            VALU  (+ optional store of the weights, AttnArgs::alpha_out)
//   (e) gates = sum_t alpha_t P_t + h x W_hh^T + W_ih_tok[token] + b    VALU + [32x256] x [256x1024]  MFMA
//       (wave w owns hidden units 32w..32w+31; one 16-byte load per lane = the unit's 4 gates = B operands of 4 MFMAs,
//        so the LSTM cell update is lane-local in the accumulator layout)
//   (f) logits = generator(h')             [32x256] x [256xV]          MFMA
//   beam:   (g-j) temperature, log-softmax, top-8 of 8*V candidates per crop, back-pointers, beam state permutation   VALU/LDS
//   greedy: (g) arg-max per row
// Structure: (a)-(f) exist once, as the phase functions below, which both kernels call with three compile-time facts: the state
// rows per crop (8 or 1), the grade of the nonlinearities (split_rows32.h: FastMath in beam, LibmMath in greedy) and the operand
// form (HRows<SPLITW>: where h lives in LDS and which MFMA products read it).  The kernel bodies hold the step loop, the barriers
// between the phases, the epilogue of (f) and the phases only they have.
// Same outputs, workspace layout and tie rules as attn_general_kernel (larger value first, then smaller flat index).
//
// Replaces recognizers/_trba/model/model.py:34-46 (AttentionCell.forward), :92-225 (Attention._beam_decode) and :227-259
// (Attention._greedy_decode).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "internal.h"
#include "msocr.h"
#include "split_rows32.h"

using namespace split_rows32;

// The optional output of the attention weights (AttnArgs::alpha_out) is a compile-time fact of the translation unit: this file is
// compiled twice, as itself (ALPHA false: the kernels of the plain entry points) and through attn_beam_mfma_alpha.hip, which defines
// MSOCR_ATTN_ALPHA and includes it (ALPHA true: the same kernels with the store in phase (c), behind msocr_internal_attn_*_mfma_alpha).
// Not a test of the pointer in one kernel, and not a template parameter: the kernels sit at the register limit, and both a
// run-time branch and further instantiations IN THIS UNIT changed the spills of the plain kernels (scratch of the beam kernels
// 212 -> 276 / 332 B and 68 -> 132 / 216 B; profiles/attn_alpha.txt).  A unit of its own leaves their code object as it was.
// Observed with one compiler (ROCm 7's hipcc): when the toolchain moves, try the template split again (tools/check_isa.sh).
// A third compilation, through attn_forced_mfma.hip (MSOCR_ATTN_FORCED with MSOCR_ATTN_ALPHA), holds only the forced-decode kernel and
// its launcher, for the same reason: neither the beam nor the greedy kernel is compiled there, nor the pack helpers.
// A fourth, through attn_lexicon_mfma.hip (MSOCR_ATTN_LEXICON with MSOCR_ATTN_ALPHA), holds the beam kernel under the lexicon constraint
// and its launcher, alone: a trie node per beam slot (a.lex_*, msocr_lexicon), a live slot's candidates are its node's child tokens and
// EOS where a word ends at the node, every other candidate is -inf; the log-sum-exp of (g) stays over the full row.  The lines the
// constraint adds are under #ifdef, so the other three compilations see the text they saw before.
#ifdef MSOCR_ATTN_LEXICON
#include "lexicon_walk.h"
#endif
// A fifth, through attn_lm_mfma.hip (MSOCR_ATTN_LM with MSOCR_ATTN_ALPHA), holds the beam kernel with a character n-gram language model
// fused in (shallow fusion) and its launcher, alone: every slot carries its row of the model's dense table (a.lm_table [n_ctx][V],
// msocr_charlm), and a live slot's candidates gain lm_weight * table[ctx][v] after the log-softmax.  The table values reach the
// candidates through sbuf: (g), where all eight waves hold four rows each, loads its rows' table values before its two reductions, so
// the loads' latency hides under them, and leaves the fused log-probabilities in place of the logits (which the trace already has and
// nobody but (h) reads); (h) then reads one float per candidate, as it always did.  Lines under #ifdef, as above.
#ifdef MSOCR_ATTN_ALPHA
constexpr bool ALPHA = true;
#define ATTN_ENTRY(name) name##_alpha
#else
constexpr bool ALPHA = false;
#define ATTN_ENTRY(name) name
#endif

// Per-phase timestamps of workgroup 0 (dev builds only: tools/attn_phase_times.sh compiles this file with -DMSOCR_ATTN_TIMING)
#if defined(MSOCR_ATTN_TIMING) && !defined(MSOCR_ATTN_ALPHA)
__device__ unsigned long long msocr_attn_timing[64 * 16];
extern "C" int msocr_attn_timing_read(unsigned long long* out_host) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(msocr_attn_timing), sizeof(msocr_attn_timing)) == hipSuccess ? 0 : -2;
}
#define TSTAMP(ph) do { if (blockIdx.x == 0 && threadIdx.x == 0 && s < 64) msocr_attn_timing[s * 16 + (ph)] = wall_clock64(); } while (0)
#else
#define TSTAMP(ph) do { } while (0)
#endif

namespace {

constexpr int KB8 = 8;        // beam slots per crop (ATT_KMAX)
constexpr int NB = 4;         // crops per workgroup (beam)
static_assert(R == NB * KB8, "row block");
constexpr int XS = 2 * H + 4; // row stride of X = [ctx | h] in floats: 516 -> ds_read_b128 of 32 rows is conflict-free
constexpr int NT = 512;       // threads per workgroup

// Wave-wide reductions on the DPP data path (quad_perm / row_half_mirror / row_mirror / row_bcast15 / row_bcast31: a few cycles per
// step) instead of ds_bpermute shuffles (an LDS round trip per step): the decode step runs ~400 of them per wave.  The result is
// complete in lane 63 (every lane of the last row for sums of full rows); *_bcast return it to all lanes through an SGPR.
template <int CTRL, int RMASK = 0xf>
__device__ __forceinline__ float dpp_f(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, RMASK, 0xf, false));
}
template <int CTRL, int RMASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, RMASK, 0xf, false); }
#define DPP_XOR1 0xB1        // quad_perm [1,0,3,2]
#define DPP_XOR2 0x4E        // quad_perm [2,3,0,1]
#define DPP_HMIRROR 0x141    // row_half_mirror: lane i <-> 7 - i inside each group of 8
#define DPP_MIRROR 0x140     // row_mirror: lane i <-> 15 - i inside each row of 16
#define DPP_BCAST15 0x142    // lane 15 of every row -> the next row (row_mask 0xA: rows 1 and 3 take it)
#define DPP_BCAST31 0x143    // lane 31 -> rows 2 and 3 (row_mask 0xC)
__device__ __forceinline__ float wave_sum63(float v) {  // total in lane 63
  v += dpp_f<DPP_XOR1>(0.f, v);
  v += dpp_f<DPP_XOR2>(0.f, v);
  v += dpp_f<DPP_HMIRROR>(0.f, v);
  v += dpp_f<DPP_MIRROR>(0.f, v);
  v += dpp_f<DPP_BCAST15, 0xA>(0.f, v);
  v += dpp_f<DPP_BCAST31, 0xC>(0.f, v);
  return v;
}
__device__ __forceinline__ float wave_max63(float v) {
  v = fmaxf(v, dpp_f<DPP_XOR1>(v, v));
  v = fmaxf(v, dpp_f<DPP_XOR2>(v, v));
  v = fmaxf(v, dpp_f<DPP_HMIRROR>(v, v));
  v = fmaxf(v, dpp_f<DPP_MIRROR>(v, v));
  v = fmaxf(v, dpp_f<DPP_BCAST15, 0xA>(v, v));
  v = fmaxf(v, dpp_f<DPP_BCAST31, 0xC>(v, v));
  return v;
}
__device__ __forceinline__ float bcast63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
// arg-max with the beam search's tie rule (larger value first, then smaller flat index; NaN never wins): result in lane 63
template <int CTRL, int RMASK = 0xf>
__device__ __forceinline__ void argmax_step(float& v, int& i) {
  const float ov = dpp_f<CTRL, RMASK>(v, v);
  const int oi = dpp_i<CTRL, RMASK>(i, i);
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argmax63(float& v, int& i) {
  argmax_step<DPP_XOR1>(v, i);
  argmax_step<DPP_XOR2>(v, i);
  argmax_step<DPP_HMIRROR>(v, i);
  argmax_step<DPP_MIRROR>(v, i);
  argmax_step<DPP_BCAST15, 0xA>(v, i);
  argmax_step<DPP_BCAST31, 0xC>(v, i);
}

// No packed-f32 VALU in this unit: a v_pk_fma_f32 whose low result takes the high dword of a source pair returns wrong low results
// in lanes 48..63 while the other wave of the SIMD runs v_mfma_f32_32x32x16_bf16 (profiles/r04_pk_fma_probe.txt,
// tools/microbench/pk_fma_beside_mfma.hip), and the sums of phase (e) run beside exactly those MFMAs.  So the file is compiled
// without packed-f32 instructions (csrc/Makefile, NOPK_OBJS), and the sums stay plain C, not inline assembly, so that the
// compiler's hazard recogniser sees them.

// Weight streams use buffer loads: ONE per-lane byte offset in a VGPR (loop-invariant) + a scalar byte offset per load, so
// the 12-16 loads in flight cost no address VGPRs (a global_load needs a 64-bit VGPR address each); out-of-range lanes
// (generator columns >= V) read 0 by the buffer range check.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, int nfloats) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, nfloats * 4, 0x00020000);
}

// D[32 rows][32 columns of this wave] += X[:, k0 : k0+256] * W[k][col], W row-major with `ldw` floats per k, one dword per lane.
__device__ __forceinline__ void mfma_cols32(const float* __restrict__ sX, int k0, const float* __restrict__ W, int ldw, int col,
                                            bool col_ok, int r32, int half, f32x16& acc) {
  constexpr int PFQ = 4;  // k-groups (of 8) of weight loads kept in flight
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(W, H * ldw);
  const int voff = col_ok ? (4 * half * ldw + col) * 4 : 0x7ffffff0;
  const int kstep = ldw * 4;  // bytes between consecutive k
  float wb[PFQ][4];
#pragma unroll
  for (int pq = 0; pq < PFQ; ++pq)
#pragma unroll
    for (int e = 0; e < 4; ++e) wb[pq][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (8 * pq + e) * kstep, 0));
#pragma unroll 1
  for (int q0 = 0; q0 < H / 8; q0 += PFQ) {
#pragma unroll
    for (int pq = 0; pq < PFQ; ++pq) {
      const int q = q0 + pq;
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(&sX[r32 * XS + k0 + 8 * q + 4 * half]);
      float cur[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) cur[e] = wb[pq][e];
      const int qn = q + PFQ;
      if (qn < H / 8) {
#pragma unroll
        for (int e = 0; e < 4; ++e) wb[pq][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (8 * qn + e) * kstep, 0));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], cur[e], acc, 0, 0, 0);
    }
  }
}

// gates of hidden units 32w..32w+31: acc[g] += X[:, k0 : k0+256] * Wt[k][j][g]   (Wt gate-interleaved: [k][j][4])
__device__ __forceinline__ void mfma_gates(const float* __restrict__ sX, int k0, const float* __restrict__ Wt, int j, int r32, int half,
                                           f32x16 (&acc)[4]) {
  constexpr int PFQ = 4;
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(Wt, H * H * 4);
  const int voff = (4 * half * H + j) * 16;
  constexpr int kstep = H * 16;
  f32x4 wb[PFQ][4];
#pragma unroll
  for (int pq = 0; pq < PFQ; ++pq)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      wb[pq][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (8 * pq + e) * kstep, 0));
#pragma unroll 1
  for (int q0 = 0; q0 < H / 8; q0 += PFQ) {
#pragma unroll
    for (int pq = 0; pq < PFQ; ++pq) {
      const int q = q0 + pq;
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(&sX[r32 * XS + k0 + 8 * q + 4 * half]);
      f32x4 cur[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) cur[e] = wb[pq][e];
      const int qn = q + PFQ;
      if (qn < H / 8) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          wb[pq][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (8 * qn + e) * kstep, 0));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], cur[e][g], acc[g], 0, 0, 0);
    }
  }
}

// Dynamic LDS of both kernels: the h rows in their operand form, then sbuf [R][H] (ph, then logits, then scratch of the beam
// permutation), then salpha [R][64] (scores, then attention weights).
extern __shared__ __attribute__((aligned(16))) float lds[];

// ---- operand form: the 32 state rows of h as the three products read them, named once per kernel.  HRows<true>: three bf16 planes
// [3][R][PSB], split-operand products with the packed split weights.  HRows<false>: f32 in columns 256..511 of X = [ctx | h], [R][XS]
// (the layout of the un-hoisted product), exact-f32 MFMA with the transposed f32 weights.  FLOATS = the LDS floats the form takes.
template <bool SPLITW>
struct HRows;
template <class HS>
__device__ __forceinline__ float* sbuf_of() { return lds + HS::FLOATS; }
template <class HS>
__device__ __forceinline__ float* salpha_of() { return lds + HS::FLOATS + R * H; }
template <>
struct HRows<true> {
  static constexpr int FLOATS = 3 * PPL / 4;
  typedef uint32_t Moved[3][KB8];
  static __device__ __forceinline__ unsigned char* planes() { return reinterpret_cast<unsigned char*>(lds); }
  static __device__ __forceinline__ void zero(int tid) {
    for (int i = tid; i < FLOATS; i += NT) lds[i] = 0.f;
  }
  // acc[32 rows][column col] += h * W, W [256][n]: packed with the columns padded by zeros to a multiple of 32
  static __device__ __forceinline__ void cols32(const uint16_t* Wp, const float*, int n, int col, int r32, int half, f32x16& acc) {
    mfma_cols32_split(planes(), Wp, (n + 31) & ~31, col, true, r32, half, acc);
  }
  static __device__ __forceinline__ void gates(const AttnArgs& a, int j, int r32, int half, f32x16 (&acc)[4]) {
    mfma_gates_split(planes(), a.whh_p, j, r32, half, acc);
  }
  static __device__ __forceinline__ void store_h(int ju, int half, float (&hv)[16]) { store_h_planes(planes(), ju, half, hv); }
  // beam permutation: thread = (column pair, crop) takes the crop's 8 rows of the three planes, row rb from row src[rb]
  static __device__ __forceinline__ void load_moved(int tid, int KB, const int* s_src, Moved& m) {
    const int j2 = tid & 127, nb = tid >> 7;
#pragma unroll
    for (int rb = 0; rb < KB8; ++rb) {
      const int src = rb < KB ? s_src[nb * KB8 + rb] : rb;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        m[pl][rb] = *reinterpret_cast<const uint32_t*>(planes() + pl * PPL + (nb * KB8 + src) * PSB + j2 * 4);
    }
  }
  static __device__ __forceinline__ void store_moved(int tid, const Moved& m) {
    const int j2 = tid & 127, nb = tid >> 7;
#pragma unroll
    for (int rb = 0; rb < KB8; ++rb)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        *reinterpret_cast<uint32_t*>(planes() + pl * PPL + (nb * KB8 + rb) * PSB + j2 * 4) = m[pl][rb];
  }
};
template <>
struct HRows<false> {
  static constexpr int FLOATS = R * XS;
  typedef float Moved[R / 2];
  static __device__ __forceinline__ void zero(int tid) {
    for (int i = tid; i < R * H; i += NT) lds[(i >> 8) * XS + H + (i & 255)] = 0.f;
  }
  static __device__ __forceinline__ void cols32(const uint16_t*, const float* W, int n, int col, int r32, int half, f32x16& acc) {
    mfma_cols32(lds, H, W, n, col, col < n, r32, half, acc);
  }
  static __device__ __forceinline__ void gates(const AttnArgs& a, int j, int r32, int half, f32x16 (&acc)[4]) {
    mfma_gates(lds, H, a.w.whh_t, j, r32, half, acc);
  }
  static __device__ __forceinline__ void store_h(int ju, int half, const float (&hv)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) lds[acc_row(e, half) * XS + H + ju] = hv[e];
  }
  // beam permutation: thread = (column, half of the rows)
  static __device__ __forceinline__ void load_moved(int tid, int KB, const int* s_src, Moved& m) {
    const int j = tid & 255, ch = tid >> 8;
#pragma unroll
    for (int q = 0; q < R / 2; ++q) {
      const int r = ch * (R / 2) + q, nb = r / KB8, rb = r % KB8;
      const int src = rb < KB ? s_src[r] : rb;
      m[q] = lds[(nb * KB8 + src) * XS + H + j];
    }
  }
  static __device__ __forceinline__ void store_moved(int tid, const Moved& m) {
    const int j = tid & 255, ch = tid >> 8;
#pragma unroll
    for (int q = 0; q < R / 2; ++q) lds[(ch * (R / 2) + q) * XS + H + j] = m[q];
  }
};

// a thread's place in the workgroup: wave wv owns hidden unit / output column ju and rows acc_row(e, half) in the MFMA phases
struct Lane {
  int tid, lane, wv, r32, half, ju;
  __device__ __forceinline__ explicit Lane(int t)
      : tid(t), lane(t & 63), wv(t >> 6), r32(lane & 31), half(lane >> 5), ju(32 * wv + r32) {}
};

// ---- the decode phases both kernels share.  RPC = state rows per crop (8: beam slots, 1: greedy), b0 = first crop of the
// workgroup, so row r belongs to crop b0 + r / RPC; crops past B repeat the last one (computed, never stored).  NL = grade of the
// nonlinearities (split_rows32.h), HS = operand form.

// (a) ph[r][j] = h2h_b[j] + sum_k h[r][k] * h2h_wt[k][j]  -> sbuf
template <class HS>
__device__ __forceinline__ void phase_h2h(const AttnArgs& a, const Lane& l) {
  float* const sbuf = sbuf_of<HS>();
  f32x16 acc;
  const float bj = a.w.h2h_b[l.ju];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = bj;
  HS::cols32(a.h2h_p, a.w.h2h_wt, H, l.ju, l.r32, l.half, acc);
#pragma unroll
  for (int e = 0; e < 16; ++e) sbuf[acc_row(e, l.half) * H + l.ju] = acc[e];
}

// (b) e[r][t] = sum_j score_w[j] * tanh(proj_H[crop][t][j] + ph[r][j]) -> salpha: one wave per (crop, t) group — the proj_H row is
//     read once for the crop's RPC rows; the rows of up to GB groups are in flight together
template <int RPC, class NL, class HS>
__device__ __forceinline__ void phase_scores(const AttnArgs& a, const Lane& l, int b0) {
  const float* const sbuf = sbuf_of<HS>();
  float* const salpha = salpha_of<HS>();
  constexpr int GB = 4;
  const int T = a.T, lane = l.lane;
  float sw[H / 64];
#pragma unroll
  for (int q = 0; q < H / 64; ++q) sw[q] = a.w.score_w[lane + 64 * q];
  const int ngroups = (R / RPC) * T;
  for (int g0 = l.wv; g0 < ngroups; g0 += GB * (NT / 64)) {
    float pr[GB][H / 64];
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      const int g = g0 + u * (NT / 64);
      if (g < ngroups) {
        const int nb = g / T, t = g - nb * T;
        const float* pP = a.proj_H + ((long)min(b0 + nb, a.B - 1) * T + t) * H;
#pragma unroll
        for (int q = 0; q < H / 64; ++q) pr[u][q] = pP[lane + 64 * q];
      }
    }
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      const int g = g0 + u * (NT / 64);
      if (g < ngroups) {
        const int nb = g / T, t = g - nb * T;
        float sacc[RPC];
#pragma unroll
        for (int rb = 0; rb < RPC; ++rb) {
          const int r = nb * RPC + rb;
          sacc[rb] = 0.f;
#pragma unroll
          for (int q = 0; q < H / 64; ++q) sacc[rb] = fmaf(sw[q], NL::tanh(pr[u][q] + sbuf[r * H + lane + 64 * q]), sacc[rb]);
        }
        // RPC independent wave sums on the DPP path, totals in lane 63
#pragma unroll
        for (int rb = 0; rb < RPC; ++rb) sacc[rb] = wave_sum63(sacc[rb]);
        if (lane == 63) {
#pragma unroll
          for (int rb = 0; rb < RPC; ++rb) salpha[(nb * RPC + rb) * 64 + t] = sacc[rb];
        }
      }
    }
  }
}

// (c) softmax over t in salpha: wave w handles rows 4w..4w+3, lane = t (T <= 64).  ALPHA (a compile-time fact of the translation
//     unit, see above; so uniform over the workgroup): the lanes that hold the weights of a live row (crop < B, beam slot < K) also
//     store them to a.alpha_out, step s of [B][steps][RPC == 1 ? 1 : K][T]: the slot is the one the step's logits are stored at.
template <int RPC, class HS>
__device__ __forceinline__ void phase_softmax_t(const AttnArgs& a, const Lane& l, int b0, int s) {
  float* const salpha = salpha_of<HS>();
  const int T = a.T;
  for (int r = 4 * l.wv; r < 4 * l.wv + 4; ++r) {
    const float ev0 = l.lane < T ? salpha[r * 64 + l.lane] : -INFINITY;
    const float m = bcast63(wave_max63(ev0));
    const float ev = l.lane < T ? expf(ev0 - m) : 0.f;
    const float sum = bcast63(wave_sum63(ev));
    if (l.lane < T) {
      const float al = ev / sum;
      salpha[r * 64 + l.lane] = al;
      if constexpr (ALPHA) {
        const int b = b0 + r / RPC, rb = r % RPC, slots = RPC == 1 ? 1 : a.K;
        if (b < a.B && rb < slots) a.alpha_out[(((long)b * a.steps + s) * slots + rb) * T + l.lane] = al;
      }
    }
  }
}

// The context half of the LSTMCell input product is hoisted out of the step loop.  The reference computes
// gates = W_ih [ctx ; onehot] + W_hh h with ctx = sum_t alpha_t batch_H_t (model.py:40-45); since W_ih[:, :H] ctx =
// sum_t alpha_t (W_ih[:, :H] batch_H_t), the products P_t = W_ih[:, :H] batch_H_t are computed ONCE per crop by a GEMM before the
// kernel (a.ctx_gates, [B][T][H][4]) and a step only forms sum_t alpha_t P_t on the VALU (13 x 1024 FMAs per row instead of
// 256 x 1024 MACs): half of the step's matrix work, 1 of its 2.5 MB of weights and the context phase disappear.  Same arithmetic
// up to the order of the f32 summation.
//
// acc[gate][e] += sum_t alpha[row][t] * P[crop(row)][t][ju][gate].  A lane's 16 accumulator elements are E consecutive rows of
// 16 / E crops (E = 4 of a beam crop's 8 slots, the other half-wave has the other 4; E = 1 in greedy): a crop's frames (T x 16 B
// per lane, 8 in flight) are loaded once for its E rows, then the FMAs.
template <int RPC, class HS>
__device__ __forceinline__ void ctx_sum(const AttnArgs& a, const Lane& l, int b0, f32x16 (&acc)[4]) {
  const float* const salpha = salpha_of<HS>();
  constexpr int E = RPC == 1 ? 1 : 4;
  static_assert(RPC == 1 || RPC == 8, "rows of a crop in one lane");
  const int T = a.T;
#pragma unroll
  for (int e0 = 0; e0 < 16; e0 += E) {
    const int row0 = acc_row(e0, l.half);
    // the rows' crop, b0 + row0 / RPC: spelled without the half-wave term for a beam crop, whose 8 rows both half-waves share, so that
    // it is a constant per e0 (with the term the exact-form beam kernel came out at 82 spilled VGPRs instead of 52)
    const int crop = b0 + (RPC == 1 ? row0 : acc_row(e0, 0) / RPC);
    const float* pP = a.ctx_gates + ((long)min(crop, a.B - 1) * T * H + l.ju) * 4;
    const float* pa = salpha + row0 * 64;
    for (int t0 = 0; t0 < T; t0 += 8) {
      f32x4 pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < T) pv[u] = *reinterpret_cast<const f32x4*>(pP + (long)(t0 + u) * H * 4);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < T) {
#pragma unroll
          for (int i = 0; i < E; ++i) {
            const float al = pa[i * 64 + t0 + u];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g][e0 + i] = fmaf(al, pv[u][g], acc[g][e0 + i]);
          }
        }
    }
    if constexpr (RPC == 1) __builtin_amdgcn_sched_barrier(0);  // keep the rows' loads from piling up across iterations (registers)
  }
}

// (e) gates = b + W_ih_tok[token] + sum_t alpha_t P_t + h W_hh^T, LSTM cell for units ju and rows acc_row(e, half), h' -> the h rows.
//     Holds the barrier between the last read of the old h and the store of the new one.
template <int RPC, class NL, bool STAGGER, class HS>
__device__ __forceinline__ void phase_gates_cell(const AttnArgs& a, const Lane& l, int b0, const int* s_tok, f32x16& c) {
  f32x16 acc[4];
  const f32x4 b4 = *reinterpret_cast<const f32x4*>(&a.w.b_gates[l.ju * 4]);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int tk = s_tok[acc_row(e, l.half)];
    const f32x4 t4 = *reinterpret_cast<const f32x4*>(&a.w.wih_tok[((long)tk * H + l.ju) * 4]);
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g][e] = b4[g] + t4[g];
  }
  if constexpr (STAGGER) {
    // The context sum is load-latency and VALU work, the recurrent product matrix-pipe work, and the two are independent: the two
    // waves of a SIMD (w and w + 4) take them in opposite orders, so one's loads and FMAs run under the other's MFMAs instead of
    // both waiting for memory and then both queueing on the pipe.
    const bool mfma_first = __builtin_amdgcn_readfirstlane(l.wv) >= 4;
    if (!mfma_first) ctx_sum<RPC, HS>(a, l, b0, acc);
    HS::gates(a, l.ju, l.r32, l.half, acc);
    if (mfma_first) ctx_sum<RPC, HS>(a, l, b0, acc);
  } else {
    ctx_sum<RPC, HS>(a, l, b0, acc);
    HS::gates(a, l.ju, l.r32, l.half, acc);
  }
  __syncthreads();  // every wave has read the old h
  float hv[16];
  lstm_cell<NL>(acc, c, hv);
  HS::store_h(l.ju, l.half, hv);
}

// (f) logits[r][v] = gen_b[v] + sum_k h'[r][k] * gen_wt[k][v] for column v = ju, up to the accumulator (columns >= V: unspecified)
template <class HS>
__device__ __forceinline__ f32x16 phase_generator(const AttnArgs& a, const Lane& l) {
  f32x16 acc;
  const float bv = l.ju < a.V ? a.w.gen_b[l.ju] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = bv;
  if (32 * l.wv < a.V) HS::cols32(a.gen_p, a.w.gen_wt, a.V, l.ju, l.r32, l.half, acc);
  return acc;
}

#ifndef MSOCR_ATTN_FORCED
// Beam decode: 4 crops x 8 beam slots per workgroup.  SPLITW: the operand form.  Nonlinearities at hardware rate; the context sum
// staggered against the recurrent product in the split form (phase_gates_cell).
template <bool SPLITW>
__global__ __launch_bounds__(NT, 1) void attn_beam_mfma_kernel(AttnArgs a) {
  typedef HRows<SPLITW> HS;
  float* const sbuf = sbuf_of<HS>();
  __shared__ float s_score[R], s_lse[R], s_top[R];
  __shared__ int s_tok[R], s_done[R], s_src[R], s_nxt[R], s_fin[NB], s_exit;
#ifdef MSOCR_ATTN_LEXICON
  __shared__ int s_node[R];          // the slot's trie node; -1 = dead (it left the trie, or was filled from an all -inf round)
  __shared__ unsigned s_mask[R * 8]; // allowed tokens of every slot in this step, one bit per token (V <= 256), rebuilt every step
#endif
#ifdef MSOCR_ATTN_LM
  __shared__ int s_ctx[R];  // the slot's row of the language model's table, in [0, lm_nctx)
#endif

  const Lane l(threadIdx.x);
  const int tid = l.tid, lane = l.lane, wv = l.wv, half = l.half, ju = l.ju;
  const int V = a.V, KB = a.K;
  const int b0 = blockIdx.x * NB;

  HS::zero(tid);  // h = 0
  f32x16 c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  if (tid < R) {
    s_score[tid] = (tid % KB8) == 0 ? 0.f : -INFINITY;
    s_tok[tid] = a.sos_id;
    s_done[tid] = 0;
#ifdef MSOCR_ATTN_LEXICON
    s_node[tid] = 0;  // the root
#endif
#ifdef MSOCR_ATTN_LM
    s_ctx[tid] = a.lm_ctx0;  // "all SOS"; the unused slots rb >= KB keep it, so every row's table reads stay inside the table
#endif
  }
  if (tid < NB) s_fin[tid] = a.steps;
  __syncthreads();
  const float temp = fmaxf(a.temperature, 1e-6f);

  for (int s = 0; s < a.steps; ++s) {
    TSTAMP(0);
    phase_h2h<HS>(a, l);
    __syncthreads();
    TSTAMP(1);
    phase_scores<KB8, FastMath, HS>(a, l, b0);
    __syncthreads();
    TSTAMP(2);
    phase_softmax_t<KB8, HS>(a, l, b0, s);
    __syncthreads();
    TSTAMP(3);
    TSTAMP(4);  // (d) is empty, the context product being hoisted; the stamp keeps tools/attn_phase_times.sh's phase numbering
    phase_gates_cell<KB8, FastMath, SPLITW, HS>(a, l, b0, s_tok, c);
    __syncthreads();
    TSTAMP(5);
    // ---- (f) logits; temperature; trace store
#ifdef MSOCR_ATTN_LEXICON
    if (tid < R * 8) s_mask[tid] = 0u;  // last read by (h) of the step before, barriers back; filled in (g), a barrier on
#endif
    {
      const f32x16 acc = phase_generator<HS>(a, l);
      if (ju < V) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = acc_row(e, half);
          float v = (ju == a.blank_id) ? -1e4f : acc[e];
          if (a.temperature != 1.0f) v = v / temp;  // true f32 division (model.py:135-137)
          sbuf[r * H + ju] = v;
          const int b = b0 + r / KB8, rb = r % KB8;
          if (rb < KB && b < a.B) a.logits_out[(((long)b * a.steps + s) * KB + rb) * V + ju] = v;
        }
      }
    }
    __syncthreads();
    TSTAMP(6);
    // ---- (g) log-sum-exp per row: wave w handles rows 4w..4w+3
    for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
#ifdef MSOCR_ATTN_LM
      // the table values of a live slot's row for this lane's tokens v = lane + 64 i (coalesced), issued before the reductions that
      // hide their latency; 0 for a finished or unused slot, whose candidates (h) forms by the plain rule or not at all
      float lmv[4];
      {
        const bool live = (r % KB8) < KB && !s_done[r];
        const float* const trow = a.lm_table + s_ctx[r] * V;
#pragma unroll
        for (int i = 0; i < 4; ++i) lmv[i] = (live && lane + 64 * i < V) ? trow[lane + 64 * i] : 0.f;
      }
#endif
      float m = -INFINITY;
      for (int v = lane; v < V; v += 64) m = fmaxf(m, sbuf[r * H + v]);
      m = bcast63(wave_max63(m));
      float sum = 0.f;
      for (int v = lane; v < V; v += 64) sum += expf(sbuf[r * H + v] - m);
      sum = wave_sum63(sum);
      if (lane == 63) s_lse[r] = m + logf(sum);  // libm-grade exp / log: the scores of a beam search are sums of these
#ifdef MSOCR_ATTN_LM
      // fused log-probabilities in place of the row's logits, each lane its own tokens: (logit - lse) + lm_weight * table value, one
      // rounding after the subtraction (weight 0 and a finite table: the subtraction's result, bit for bit)
      {
        const float lse = bcast63(m + logf(sum));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = lane + 64 * i;
          if (v < V) sbuf[r * H + v] = fmaf(a.lm_weight, lmv[i], sbuf[r * H + v] - lse);
        }
      }
#endif
#ifdef MSOCR_ATTN_LEXICON
      // the row's allowed tokens: a live slot's edge list strided over the wave (an edge token outside [0, V) is ignored), EOS where
      // its node is terminal; a finished slot keeps the plain rule (EOS alone); a dead slot has none
      const int node = s_node[r];
      if ((r % KB8) < KB && node >= 0) {
        const int dn = s_done[r];
        if (!dn) {
          int lo, hi;
          lex_edge_range(a.lex_begin, a.lex_nodes, a.lex_edges, node, lo, hi);
          for (int e = lo + lane; e < hi; e += 64) {
            const int tk = a.lex_tok[e];
            if (tk >= 0 && tk < V) atomicOr(&s_mask[r * 8 + (tk >> 5)], 1u << (tk & 31));
          }
        }
        if (lane == 0 && a.eos_id >= 0 && a.eos_id < V && (dn || lex_terminal(a.lex_terminal, a.lex_nodes, node)))
          atomicOr(&s_mask[r * 8 + (a.eos_id >> 5)], 1u << (a.eos_id & 31));
      }
#endif
    }
    __syncthreads();
    TSTAMP(7);
    // ---- (h) top-K of the K*V candidates of every crop: ONE wave per crop (lane owns v = lane + 64 i), the K rounds of
    //      arg-max + winner removal need no workgroup barrier.  Order: larger value, then smaller flat index beam*V + v.
    const float lp = a.lp ? a.lp[s] : 1.0f;
    if (wv < NB) {
      const int nb = wv;
      constexpr int VI = 4;  // V <= 256
      float cv[VI][KB8];
      float lse_r[KB8], sc_r[KB8];
      int dn_r[KB8];
#pragma unroll
      for (int rb = 0; rb < KB8; ++rb) {  // per-beam values once, not once per candidate
        lse_r[rb] = s_lse[nb * KB8 + rb];
        sc_r[rb] = s_score[nb * KB8 + rb];
        dn_r[rb] = s_done[nb * KB8 + rb];
      }
#pragma unroll
      for (int i = 0; i < VI; ++i) {
        const int v = lane + 64 * i;
#pragma unroll
        for (int rb = 0; rb < KB8; ++rb) {
          cv[i][rb] = -INFINITY;
          const int r = nb * KB8 + rb;
#ifdef MSOCR_ATTN_LEXICON
          const unsigned mw = s_mask[r * 8 + 2 * i + (lane >> 5)];  // the word that holds token v = lane + 64 i
#endif
          if (v < V && rb < KB) {
#ifdef MSOCR_ATTN_LM
            float logp = sbuf[r * H + v];  // (g) left the fused log-probability there
#else
            float logp = sbuf[r * H + v] - lse_r[rb];
#endif
            if (dn_r[rb]) logp = (v == a.eos_id) ? 0.f : -INFINITY;
#ifdef MSOCR_ATTN_LEXICON
            if (!((mw >> (lane & 31)) & 1u)) logp = -INFINITY;
#endif
            float tot = sc_r[rb] + logp;
            if (a.lp) tot = tot / lp;
            cv[i][rb] = tot;
          }
        }
      }
      // per-lane cache: best candidate of every v-slot over the beams, and the lane's best over its slots.  A round then costs one
      // wave arg-max + the rescan of the winner's slot (8 entries) instead of a scan of all 32 entries per lane.
      float sv[VI], lv;
      int sf[VI], lf;
      auto rescan_slot = [&](int i) {
        float bv = -INFINITY;
        int bf = 0x7fffffff;
        const int v = lane + 64 * i;
#pragma unroll
        for (int rb = 0; rb < KB8; ++rb) {
          const float x = cv[i][rb];
          const int fi = rb * V + v;
          if (v < V && rb < KB && (x > bv || (x == bv && fi < bf))) { bv = x; bf = fi; }
        }
        sv[i] = bv; sf[i] = bf;
      };
      auto rescan_lane = [&]() {
        lv = sv[0]; lf = sf[0];
#pragma unroll
        for (int i = 1; i < VI; ++i)
          if (sv[i] > lv || (sv[i] == lv && sf[i] < lf)) { lv = sv[i]; lf = sf[i]; }
      };
#pragma unroll
      for (int i = 0; i < VI; ++i) rescan_slot(i);
      rescan_lane();
      for (int kk = 0; kk < KB; ++kk) {
        float bvv = lv;
        int bii = lf;
        wave_argmax63(bvv, bii);
        bvv = bcast63(bvv);
        bii = __builtin_amdgcn_readlane(bii, 63);
        int wi_ = bii;
        if (wi_ == 0x7fffffff) wi_ = 0;  // every candidate NaN: degenerate input
        const int wr = wi_ / V, wc = wi_ - wr * V;
        if (lane == 0) {
          s_top[nb * KB8 + kk] = bvv;
          s_src[nb * KB8 + kk] = wr;
          s_nxt[nb * KB8 + kk] = wc;
        }
        // the winner never wins again (NaN); wr, wc are wave-uniform, so is the slot wc >> 6: one slot is rescanned
        const int wslot = wc >> 6;
        const bool mine = (wc & 63) == lane;
#pragma unroll
        for (int i = 0; i < VI; ++i)
          if (i == wslot) {
#pragma unroll
            for (int rb = 0; rb < KB8; ++rb)
              if (mine && rb == wr) cv[i][rb] = __int_as_float(0x7fc00000);
            rescan_slot(i);
          }
        rescan_lane();
      }
    }
    __syncthreads();
    TSTAMP(8);
    // ---- (i) bookkeeping per state row
    int nd = 1;
#ifdef MSOCR_ATTN_LEXICON
    int nn = -1;  // the new slot's node: its parent's where the hypothesis is finished, else the child along the token; -1 = dead
    if (tid < R) {
      const int nb = tid / KB8, rb = tid % KB8;
      if (rb < KB) {
        const int src = nb * KB8 + s_src[tid], nxt = s_nxt[tid], ended = s_done[src] | (nxt == a.eos_id);
        nn = ended ? s_node[src] : lex_child(a.lex_begin, a.lex_tok, a.lex_child, a.lex_nodes, a.lex_edges, s_node[src], nxt);
        if (!isfinite(s_top[tid])) nn = -1;
        nd = ended | (nn < 0);  // no legal continuation counts as finished: fin_step and the chunk early exit still fire
      }
    }
#else
    if (tid < R) {
      const int nb = tid / KB8, rb = tid % KB8;
      if (rb < KB) nd = s_done[nb * KB8 + s_src[tid]] | (s_nxt[tid] == a.eos_id);
    }
#endif
#ifdef MSOCR_ATTN_LM
    int nc = 0;  // the new slot's table row: its source's where the hypothesis is finished, else the source's shifted by the token
    if (tid < R) {
      const int nb = tid / KB8, rb = tid % KB8;
      if (rb < KB) {
        const int cs = s_ctx[nb * KB8 + s_src[tid]];  // s_src in [0, KB), s_nxt in [0, V): wi_ / V and wi_ - wr * V of wi_ < KB * V
        nc = nd ? cs : (cs * V + s_nxt[tid]) % a.lm_nctx;  // cs * V + nxt < n_ctx * V <= 2^26
      }
    }
#endif
    __syncthreads();
    if (tid < R) {
      const int nb = tid / KB8, rb = tid % KB8, b = b0 + nb;
      if (rb < KB) {
        if (b < a.B) {
          const long o = ((long)b * a.steps + s) * KB + rb;
          a.back[o] = s_src[tid];
          a.tokv[o] = s_nxt[tid];
#ifdef MSOCR_ATTN_LEXICON
          a.node_out[o] = nn;
#endif
#ifdef MSOCR_ATTN_LM
          a.ctx_out[o] = nc;
#endif
        }
        s_score[tid] = a.lp ? s_top[tid] * lp : s_top[tid];  // f32 round trip of the reference (model.py:188-192)
        s_tok[tid] = s_nxt[tid];
#ifdef MSOCR_ATTN_LEXICON
        s_node[tid] = nn;
#endif
#ifdef MSOCR_ATTN_LM
        s_ctx[tid] = nc;
#endif
      }
      s_done[tid] = nd;
    }
    __syncthreads();
    if (tid < NB) {
      int best = 0, all = 1;
      float bs = s_score[tid * KB8];
      for (int r = 0; r < KB; ++r) {
        if (r && s_score[tid * KB8 + r] > bs) { bs = s_score[tid * KB8 + r]; best = r; }
        all &= s_done[tid * KB8 + r];
      }
      if (b0 + tid < a.B) a.best_at[(long)(b0 + tid) * a.steps + s] = best;
      if (all && s_fin[tid] == a.steps) {
        s_fin[tid] = s + 1;
        if (a.chunk_state && b0 + tid < a.B) {  // publish: max finish step first, then the count that readers test
          const int ch = a.chunk_id[b0 + tid];
          atomicMax(&a.chunk_state[2 * ch + 1], s + 1);
          __threadfence();
          atomicAdd(&a.chunk_state[2 * ch], 1);
        }
      }
    }
    TSTAMP(9);
    // ---- (j) permute beam state by src within every crop: c through sbuf (logits are consumed), h through registers
    {
#pragma unroll
      for (int e = 0; e < 16; ++e) sbuf[acc_row(e, half) * H + ju] = c[e];
      typename HS::Moved hm;
      HS::load_moved(tid, KB, s_src, hm);
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = acc_row(e, half), nb = r / KB8, rb = r % KB8;
        const int src = rb < KB ? s_src[r] : rb;
        c[e] = sbuf[(nb * KB8 + src) * H + ju];
      }
      HS::store_moved(tid, hm);
    }
    __syncthreads();
    TSTAMP(10);
    // ---- early exit (model.py:215 breaks the loop once every beam of every row of the chunk is finished): leave after
    //      step s when every chunk this workgroup's crops belong to has all its crops finished at steps <= s + 1, i.e. the
    //      chunk's run length T_run = max finish step is covered.  Nobody waits: a workgroup that cannot see the others'
    //      flags yet just runs further steps, whose outputs are then unused.
    if (a.chunk_state) {
      if (tid == 0) {
        int ex = 1;
        for (int nb = 0; nb < NB && ex; ++nb) {
          const int b = b0 + nb;
          if (b >= a.B) continue;
          if (s_fin[nb] == a.steps) { ex = 0; break; }
          const int ch = a.chunk_id[b];
          if (__hip_atomic_load(&a.chunk_state[2 * ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.chunk_size[ch]) { ex = 0; break; }
          __threadfence();
          if (__hip_atomic_load(&a.chunk_state[2 * ch + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > s + 1) ex = 0;
        }
        s_exit = ex;
      }
      __syncthreads();
      if (s_exit) break;
    }
  }
  if (tid < NB && b0 + tid < a.B) a.fin_step[b0 + tid] = s_fin[tid];
}

#if !defined(MSOCR_ATTN_LEXICON) && !defined(MSOCR_ATTN_LM)
// Greedy decode (Attention._greedy_decode, model.py:227-259): 32 CROPS per workgroup, one state row each, all `steps` steps in one
// launch.  The rows are independent (the reference keeps every row running after its own EOS and only stops a chunk when all rows
// emit EOS in the same step; the host derives those run lengths from the ids, recognizers/_trba/__init__.py), so a step is (a)-(f)
// without any beam bookkeeping — no log-softmax, no top-k, no state permutation — followed by an arg-max per row (larger value,
// then smaller index; blank masked to -1e4 as in attn_general_kernel).  Always the split form.  Each row reads ITS crop's proj_H /
// ctx_gates frames (8x the beam kernel's traffic per row, from L2 / the Infinity Cache).
// Nonlinearities libm-grade: the greedy logits are held to the decoder-only bound (2e-4 of max |logit| against the oracle's decoder
// over 41 chained steps of the all-random decoder, tests/test_gpu_trba.py DECODER_LOGIT_RTOL), which the hardware-rate forms miss
// by 5 % on one row of 96; greedy is not the pipeline's default mode.
__global__ __launch_bounds__(NT, 1) void attn_greedy_mfma_kernel(AttnArgs a) {
  typedef HRows<true> HS;
  float* const sbuf = sbuf_of<HS>();
  __shared__ int s_tok[R];
  const Lane l(threadIdx.x);
  const int tid = l.tid, lane = l.lane, wv = l.wv, half = l.half, ju = l.ju;
  const int V = a.V;
  const int b0 = blockIdx.x * R;
  HS::zero(tid);  // h = 0
  f32x16 c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  if (tid < R) s_tok[tid] = a.sos_id;
  __syncthreads();

  for (int s = 0; s < a.steps; ++s) {
    phase_h2h<HS>(a, l);
    __syncthreads();
    phase_scores<1, LibmMath, HS>(a, l, b0);
    __syncthreads();
    phase_softmax_t<1, HS>(a, l, b0, s);
    __syncthreads();
    phase_gates_cell<1, LibmMath, false, HS>(a, l, b0, s_tok, c);
    __syncthreads();
    // ---- (f) logits; trace store
    {
      const f32x16 acc = phase_generator<HS>(a, l);
      if (ju < V) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = acc_row(e, half);
          const float v = (ju == a.blank_id) ? -1e4f : acc[e];
          sbuf[r * H + ju] = v;
          if (b0 + r < a.B) a.logits_out[((long)(b0 + r) * a.steps + s) * V + ju] = v;
        }
      }
    }
    __syncthreads();
    // ---- (g) arg-max per row (larger value, then smaller index): wave w handles rows 4w..4w+3
    for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        const float x = sbuf[r * H + v];
        if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
      }
      wave_argmax63(bv, bi);
      if (lane == 63) {
        if (bi == 0x7fffffff) bi = 0;  // every logit NaN: degenerate input
        s_tok[r] = bi;
        if (b0 + r < a.B) a.ids_out[(long)(b0 + r) * a.steps + s] = bi;
      }
    }
    __syncthreads();
  }
}
#endif  // MSOCR_ATTN_LEXICON, MSOCR_ATTN_LM

#else  // MSOCR_ATTN_FORCED
// Forced (teacher-forced) decode, Attention.forward(is_train=True) of the reference (model.py:287-320) with sampling_prob 0: the greedy
// kernel's step loop over 32 independent rows per workgroup, fed the GIVEN token of every step (a.tok_in [B][steps], column 0 = SOS)
// instead of the arg-max of the step before.  Phases (a)-(f) are the greedy kernel's own instantiations (one state row per crop,
// libm-grade nonlinearities, split form), so a row fed greedy's ids reproduces greedy's logits and attention weights bit for bit;
// phase (g) is gone, and with it the copy of the logits to LDS and the barrier that ordered it: (f) of step s and (a) of step s + 1
// both only read the h rows.  Writes logits_out [B][steps][V] and alpha_out [B][steps][T]; no ids.  Rows past B take sos_id (computed,
// never stored); an id outside [0, V) is replaced by sos_id before it is used as the row index into wih_tok.
__global__ __launch_bounds__(NT, 1) void attn_forced_mfma_kernel(AttnArgs a) {
  typedef HRows<true> HS;
  __shared__ int s_tok[R];
  const Lane l(threadIdx.x);
  const int tid = l.tid, half = l.half, ju = l.ju;
  const int V = a.V;
  const int b0 = blockIdx.x * R;
  HS::zero(tid);  // h = 0
  f32x16 c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  __syncthreads();

  for (int s = 0; s < a.steps; ++s) {
    // the step's input tokens; read by phase (e), three barriers on.  The last reader of the old ones, (e) of step s - 1, is a barrier back.
    if (tid < R) {
      int tk = b0 + tid < a.B ? a.tok_in[(long)(b0 + tid) * a.steps + s] : a.sos_id;
      if (tk < 0 || tk >= V) tk = a.sos_id;
      s_tok[tid] = tk;
    }
    phase_h2h<HS>(a, l);
    __syncthreads();
    phase_scores<1, LibmMath, HS>(a, l, b0);
    __syncthreads();
    phase_softmax_t<1, HS>(a, l, b0, s);
    __syncthreads();
    phase_gates_cell<1, LibmMath, false, HS>(a, l, b0, s_tok, c);
    __syncthreads();
    // ---- (f) logits; trace store
    const f32x16 acc = phase_generator<HS>(a, l);
    if (ju < V) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = acc_row(e, half);
        const float v = (ju == a.blank_id) ? -1e4f : acc[e];
        if (b0 + r < a.B) a.logits_out[((long)(b0 + r) * a.steps + s) * V + ju] = v;
      }
    }
  }
}
#endif  // MSOCR_ATTN_FORCED

// dynamic LDS of a decode kernel: the h rows in their form, sbuf, salpha
template <bool SPLITW>
constexpr size_t lds_bytes() { return (size_t)(HRows<SPLITW>::FLOATS + R * H + R * 64) * sizeof(float); }

}  // namespace

#if defined(MSOCR_ATTN_LM)
// the one kernel of attn_lm_mfma.hip (both operand forms)
int msocr_internal_attn_lm_mfma(const AttnArgs& a, hipStream_t s) {
  if (!a.ctx_gates || !a.alpha_out || !a.ctx_out || !a.lm_table) return MSOCR_E_ARG;
  if (a.lm_nctx < 1 || a.lm_ctx0 < 0 || a.lm_ctx0 >= a.lm_nctx || (long)a.lm_nctx * a.V > (1L << 26)) return MSOCR_E_ARG;
  const size_t ldsz = lds_bytes<false>(), ldsz_split = lds_bytes<true>();
  if (msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<false>, (int)ldsz) != MSOCR_OK ||
      msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<true>, (int)ldsz_split) != MSOCR_OK)
    return MSOCR_E_LAUNCH;
  const dim3 grid((a.B + NB - 1) / NB);
  if (a.h2h_p)
    MSOCR_LAUNCH((attn_beam_mfma_kernel<true>), grid, dim3(NT), ldsz_split, s, a);
  else
    MSOCR_LAUNCH((attn_beam_mfma_kernel<false>), grid, dim3(NT), ldsz, s, a);
  return LAUNCH_OK();
}
#elif defined(MSOCR_ATTN_LEXICON)
// the one kernel of attn_lexicon_mfma.hip (both operand forms)
int msocr_internal_attn_lexicon_mfma(const AttnArgs& a, hipStream_t s) {
  if (!a.ctx_gates || !a.alpha_out || !a.node_out) return MSOCR_E_ARG;
  if (!a.lex_begin || !a.lex_tok || !a.lex_child || !a.lex_terminal || a.lex_nodes < 1 || a.lex_edges < 0) return MSOCR_E_ARG;
  const size_t ldsz = lds_bytes<false>(), ldsz_split = lds_bytes<true>();
  if (msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<false>, (int)ldsz) != MSOCR_OK ||
      msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<true>, (int)ldsz_split) != MSOCR_OK)
    return MSOCR_E_LAUNCH;
  const dim3 grid((a.B + NB - 1) / NB);
  if (a.h2h_p)
    MSOCR_LAUNCH((attn_beam_mfma_kernel<true>), grid, dim3(NT), ldsz_split, s, a);
  else
    MSOCR_LAUNCH((attn_beam_mfma_kernel<false>), grid, dim3(NT), ldsz, s, a);
  return LAUNCH_OK();
}
#elif defined(MSOCR_ATTN_FORCED)
// the one kernel of attn_forced_mfma.hip
int msocr_internal_attn_forced_mfma(const AttnArgs& a, hipStream_t s) {
  if (!a.ctx_gates || !a.h2h_p || !a.whh_p || !a.gen_p || !a.alpha_out || !a.tok_in || !a.logits_out) return MSOCR_E_ARG;
  if (a.sos_id < 0 || a.sos_id >= a.V) return MSOCR_E_ARG;
  const size_t ldsz_split = lds_bytes<true>();
  if (msocr_internal_lds_limit((const void*)attn_forced_mfma_kernel, (int)ldsz_split) != MSOCR_OK) return MSOCR_E_LAUNCH;
  MSOCR_LAUNCH(attn_forced_mfma_kernel, dim3((a.B + R - 1) / R), dim3(NT), ldsz_split, s, a);
  return LAUNCH_OK();
}
#else
// the kernels of this unit: with the attention-weight output in attn_beam_mfma_alpha.hip's copy (the _alpha names), without it here
int ATTN_ENTRY(msocr_internal_attn_beam_mfma)(const AttnArgs& a, hipStream_t s) {
  if (!a.ctx_gates || ALPHA != (a.alpha_out != nullptr)) return MSOCR_E_ARG;
  const size_t ldsz = lds_bytes<false>(), ldsz_split = lds_bytes<true>();
  if (msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<false>, (int)ldsz) != MSOCR_OK ||
      msocr_internal_lds_limit((const void*)attn_beam_mfma_kernel<true>, (int)ldsz_split) != MSOCR_OK)
    return MSOCR_E_LAUNCH;
  const dim3 grid((a.B + NB - 1) / NB);
  if (a.h2h_p)
    MSOCR_LAUNCH((attn_beam_mfma_kernel<true>), grid, dim3(NT), ldsz_split, s, a);
  else
    MSOCR_LAUNCH((attn_beam_mfma_kernel<false>), grid, dim3(NT), ldsz, s, a);
  return LAUNCH_OK();
}

int ATTN_ENTRY(msocr_internal_attn_greedy_mfma)(const AttnArgs& a, hipStream_t s) {
  if (!a.ctx_gates || !a.h2h_p || !a.whh_p || !a.gen_p || ALPHA != (a.alpha_out != nullptr)) return MSOCR_E_ARG;
  const size_t ldsz_split = lds_bytes<true>();
  if (msocr_internal_lds_limit((const void*)attn_greedy_mfma_kernel, (int)ldsz_split) != MSOCR_OK) return MSOCR_E_LAUNCH;
  MSOCR_LAUNCH(attn_greedy_mfma_kernel, dim3((a.B + R - 1) / R), dim3(NT), ldsz_split, s, a);
  return LAUNCH_OK();
}

#endif  // MSOCR_ATTN_FORCED

#ifndef MSOCR_ATTN_ALPHA
// HOST helper: a transposed f32 weight matrix of the decoder ([256][N] row-major: h2h_wt, gen_wt; or gate-interleaved
// [256][N / 4][4]: whh_t) -> the packed split form the matrix-core beam kernel reads: out[plane][k / 16][column][k % 16] bf16 with
// w == p0 + p1 + p2 exactly; columns padded with zeros to a multiple of 32; gate-interleaved input: column = gate * (N / 4) + unit.
extern "C" int64_t msocr_attn_pack_split_elems(int N) { return N > 0 ? (int64_t)3 * H * ((N + 31) & ~31) : 0; }
extern "C" int msocr_attn_pack_split_host(const float* wt_host, int N, int gate_interleaved, uint16_t* out_host) {
  if (!wt_host || !out_host || N <= 0 || (gate_interleaved && N % 4)) return MSOCR_E_ARG;
  const int Np = (N + 31) & ~31;
  const int64_t plane = (int64_t)H * Np;
  for (int64_t i = 0; i < 3 * plane; ++i) out_host[i] = 0;
  auto rne = [](float f) -> uint16_t {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  };
  for (int k = 0; k < H; ++k)
    for (int n = 0; n < N; ++n) {
      const int col = gate_interleaved ? (n & 3) * (N / 4) + (n >> 2) : n;
      float r = wt_host[(int64_t)k * N + n];
      for (int pl = 0; pl < 3; ++pl) {
        const uint16_t hb = rne(r);
        out_host[pl * plane + ((int64_t)(k >> 4) * Np + col) * 16 + (k & 15)] = hb;
        r -= __builtin_bit_cast(float, (uint32_t)hb << 16);
      }
    }
  return MSOCR_OK;
}
#endif
