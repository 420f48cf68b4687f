// trba_kernels.hip — the non-convolutional part of the TRBA recogniser on gfx950:
// squeeze-excite tail, mean over H, BiLSTM recurrence, the attention decoder's entry points
// and the recognition confidence.  These stages are bandwidth/latency bound:
// they run on the VALU in exact f32 with coalesced weight streams (weights pre-transposed so
// lane j reads column j), LDS-resident per-row state and wave-level reductions; no MFMA.
// The sequential loop (T encoder steps) lives INSIDE one launch: rows are independent, so
// one workgroup owns a few rows for the whole loop and no inter-workgroup hand-off exists.
// The decode kernels themselves are in attn_beam_mfma.hip (and its further compilations attn_beam_mfma_alpha.hip and attn_forced_mfma.hip)
// and attn_general.hip (and attn_general_forced.hip).
//
//   msocr_se_residual       <- recognizers/_trba/model/seresnet31.py:5-20, 61-66
//   msocr_mean_over_h       <- recognizers/_trba/model/model.py:388-390
//   msocr_bilstm_recurrent  <- model.py:9-21 (nn.LSTM, gate order i,f,g,o)
//   msocr_attn_decode       <- model.py:34-46 + 227-259 (greedy), 92-225 (beam, with msocr_attn_beam_finalize), 287-320 (forced: the
//                              teacher-forced pass, as an inference call)
//   msocr_seq_confidence    <- recognizers/_trba/__init__.py:413-431
//   msocr_seq_logp          summed log-probability of given ids (no counterpart: the reference has the training loss only)
//   msocr_seq_char_details  per-symbol probability and attention position (no counterpart: the reference drops both)
// A decode with alpha_out keeps the attention weights of every step (model.py:40-46 returns them, its callers drop them).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "internal.h"
#include "msocr.h"
#include "se_tail.h"

__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return *reinterpret_cast<uint16_t*>(&b);
}
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<uint16_t>(const uint16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<uint16_t>(uint16_t* p, float v) { *p = f2bf(v); }

// --------------------------------------------------------------------------------------------- SE tail
// One workgroup per sample: mean over HW (coalesced over channels), two tiny FCs, then
// out = relu(x * gate + identity).  x is re-read from L2 for the last phase.
// 4 channels per lane (16-byte f32 / 8-byte bf16 accesses); the 256 threads split into PG = 1024/C pixel groups whose
// partial channel sums are combined through LDS in a fixed order (deterministic).
template <typename T>
__device__ __forceinline__ f32x4 ld4(const T* p);
template <>
__device__ __forceinline__ f32x4 ld4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <>
__device__ __forceinline__ f32x4 ld4<uint16_t>(const uint16_t* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  f32x4 r = {bf2f((uint16_t)(v.x & 0xffff)), bf2f((uint16_t)(v.x >> 16)), bf2f((uint16_t)(v.y & 0xffff)), bf2f((uint16_t)(v.y >> 16))};
  return r;
}
template <typename T>
__device__ __forceinline__ void st4(T* p, f32x4 v);
template <>
__device__ __forceinline__ void st4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <>
__device__ __forceinline__ void st4<uint16_t>(uint16_t* p, f32x4 v) {
  uint2 o;
  o.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
  o.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
  *reinterpret_cast<uint2*>(p) = o;
}

// Measured and dropped (round 3): keeping the summed x values of a 4 x 13 map in registers (26 x 16 B per thread) so that the scale
// pass does not read x again — 0.118 against 0.091 ms per 960 crops: the second read hits L2, and 163 registers cost occupancy.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void se_residual_kernel(const T* __restrict__ x, const T* __restrict__ idt, int HW, int C,
                                                           const float* __restrict__ w1, const float* __restrict__ w2,
                                                           float* __restrict__ gate_ws, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // part[PG][C] | mean[C] | hid[C/16] | gate[C]
  const int n = blockIdx.x, tid = threadIdx.x;
  const T* xs = x + (long)n * HW * C;
  const T* is = idt + (long)n * HW * C;
  T* os = out + (long)n * HW * C;
  // the phases are se_tail.h's, with NT virtual threads = this workgroup's own
  auto ldx = [&](int p, int c) { return ld4<T>(xs + (long)p * C + c); };
  se_partial_sums<NT, NT>(ldx, HW, C, sm, tid);
  const float* gate = se_gate<NT, NT>(sm, HW, C, w1, w2, gate_ws + (long)n * C, tid);
  se_scale<NT, NT>(ldx, [&](int p, int c) { return ld4<T>(is + (long)p * C + c); },
                   [&](int p, int c, f32x4 y) { st4<T>(os + (long)p * C + c, y); }, HW, C, gate, tid);
}

extern "C" int msocr_se_residual(const void* x, const void* identity, int N, int HW, int C, int dtype, const float* w1, const float* w2,
                                 float* gate_ws, void* out, void* stream) {
  if (!x || !identity || !w1 || !w2 || !gate_ws || !out || N <= 0 || HW <= 0 || C < 64 || C > 1024 || (C & (C - 1))) return MSOCR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  // f32: 1024-thread workgroups (2 per CU: 512 crops in flight).  A crop is read twice (mean, then scale); with 256-thread workgroups
  // all 1920 crops of a sub-batch are resident at once — 0.8 GB between the two reads of a crop, nothing of it left in L2 / MALL.
  // Measured per 1920 crops: 0.587 / 0.311 / 0.173 ms (16x50x128 / 8x25x256 / 4x13x512) -> 0.541 / 0.249 / 0.151.  The size is the
  // same for every batch size (the order of the mean's additions depends on it, and results must not depend on the batch
  // composition).
  if (dtype == MSOCR_F32) {
    MSOCR_LAUNCH((se_residual_kernel<float, 1024>), dim3(N), dim3(1024), (size_t)se_scratch_floats(1024, C) * sizeof(float), s,
                 (const float*)x, (const float*)identity, HW, C, w1, w2, gate_ws, (float*)out);
  } else if (dtype == MSOCR_BF16) {
    MSOCR_LAUNCH((se_residual_kernel<uint16_t, 256>), dim3(N), dim3(256), (size_t)se_scratch_floats(256, C) * sizeof(float), s,
                 (const uint16_t*)x, (const uint16_t*)identity, HW, C, w1, w2, gate_ws, (uint16_t*)out);
  } else {
    return MSOCR_E_ARG;
  }
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- mean over H
template <typename T>
__global__ void mean_over_h_kernel(const T* __restrict__ in, int N, int H, int W, int C, float* __restrict__ out) {
  const long total = (long)N * W * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long t = i / C;
    const int w = (int)(t % W);
    const int n = (int)(t / W);
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += ldf<T>(in + (((long)n * H + h) * W + w) * C + c);
    out[i] = s / (float)H;
  }
}
extern "C" int msocr_mean_over_h(const void* in, int N, int H, int W, int C, int dtype, float* out, void* stream) {
  if (!in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MSOCR_E_ARG;
  const long total = (long)N * W * C;
  long g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MSOCR_F32)
    MSOCR_LAUNCH(mean_over_h_kernel<float>, dim3((unsigned)g), dim3(256), 0, s, (const float*)in, N, H, W, C, out);
  else if (dtype == MSOCR_BF16)
    MSOCR_LAUNCH(mean_over_h_kernel<uint16_t>, dim3((unsigned)g), dim3(256), 0, s, (const uint16_t*)in, N, H, W, C, out);
  else
    return MSOCR_E_ARG;
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- BiLSTM recurrence
// grid (ceil(B/RB), 2 directions), 256 threads = hidden units (H == 256).  Thread j owns unit j's
// four gates for RB batch rows; h_{t-1} of the RB rows sits in LDS as [k][r] so one
// ds_read_b128 pair broadcasts the 8 row values of column k; W_hh^T rows stream from L2,
// coalesced over j.  xproj already holds x W_ih^T + b_ih + b_hh.
#define LSTM_RB 4
template <int H>
__global__ __launch_bounds__(H) void bilstm_kernel(const float* __restrict__ xproj, const float* __restrict__ whh_t, int B, int T,
                                                    float* __restrict__ hcat) {
  constexpr int G = 4 * H, RB = LSTM_RB;
  __shared__ __attribute__((aligned(16))) float hs[2][H][RB];
  const int j = threadIdx.x, d = blockIdx.y;
  const int b0 = blockIdx.x * RB;
  const float* wt = whh_t + (long)d * H * G;
  float c[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    c[r] = 0.f;
    hs[0][j][r] = 0.f;
  }
  __syncthreads();
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    const int cur = s & 1;
    float acc[4][RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int b = b0 + r < B ? b0 + r : B - 1;
      const float* xp = xproj + (((long)b * T + t) * 2 + d) * G;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][r] = xp[g * H + j];
    }
#pragma unroll 1
    for (int k0 = 0; k0 < H; k0 += 8) {
      f32x4 wq[8];  // gates i,f,g,o of unit j: 8 x 16-B loads in flight per lane
#pragma unroll
      for (int u = 0; u < 8; ++u) wq[u] = *reinterpret_cast<const f32x4*>(&wt[((long)(k0 + u) * H + j) * 4]);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float hv[RB];
#pragma unroll
        for (int r4 = 0; r4 < RB; r4 += 4) {
          const f32x4 hq = *reinterpret_cast<const f32x4*>(&hs[cur][k0 + u][r4]);
          hv[r4] = hq[0]; hv[r4 + 1] = hq[1]; hv[r4 + 2] = hq[2]; hv[r4 + 3] = hq[3];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int r = 0; r < RB; ++r) acc[g][r] = fmaf(wq[u][g], hv[r], acc[g][r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const float ig = sigmoidf_(acc[0][r]), fg = sigmoidf_(acc[1][r]), gg = tanhf(acc[2][r]), og = sigmoidf_(acc[3][r]);
      c[r] = fg * c[r] + ig * gg;
      const float h = og * tanhf(c[r]);
      hs[cur ^ 1][j][r] = h;
      if (b0 + r < B) hcat[((long)(b0 + r) * T + t) * (2 * H) + d * H + j] = h;
    }
    __syncthreads();
  }
}

extern "C" int msocr_bilstm_recurrent(const float* xproj, const float* w_hh_t, int B, int T, int H, float* hcat_out, void* stream) {
  if (!xproj || !w_hh_t || !hcat_out || B <= 0 || T <= 0) return MSOCR_E_ARG;
  const dim3 grid((B + LSTM_RB - 1) / LSTM_RB, 2);
  // hidden_size comes from the checkpoint's config (recognizers/_trba/__init__.py:142-151): 256 is the reference default
  if (H == 256) MSOCR_LAUNCH(bilstm_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 128) MSOCR_LAUNCH(bilstm_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 512) MSOCR_LAUNCH(bilstm_kernel<512>, grid, dim3(512), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 64) MSOCR_LAUNCH(bilstm_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 192) MSOCR_LAUNCH(bilstm_kernel<192>, grid, dim3(192), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 320) MSOCR_LAUNCH(bilstm_kernel<320>, grid, dim3(320), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 384) MSOCR_LAUNCH(bilstm_kernel<384>, grid, dim3(384), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else if (H == 448) MSOCR_LAUNCH(bilstm_kernel<448>, grid, dim3(448), 0, (hipStream_t)stream, xproj, w_hh_t, B, T, hcat_out);
  else return MSOCR_E_ARG;
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- attention decoder
// The decode kernels live in attn_beam_mfma.hip (matrix cores: a descriptor with ctx_gates) and attn_general.hip (every shape: one
// without); this file keeps the one entry point, its argument checks, the beam workspace layout and the finalize step.

// finalize: walk the back-pointers from (t_run-1, best_at[t_run-1]) and gather the path's logits; with alpha_ws [B][steps][K][T] also the
// path's attention weights -> alpha_out [B][steps][T] (zeros for t >= t_run)
__global__ void attn_beam_finalize_kernel(const float* __restrict__ ws_logits, const int32_t* __restrict__ back,
                                          const int32_t* __restrict__ tokv, const int32_t* __restrict__ best_at,
                                          const int32_t* __restrict__ trun, int V, int steps, int K, float* __restrict__ logits_out,
                                          int32_t* __restrict__ ids_out, const float* __restrict__ alpha_ws, int T,
                                          float* __restrict__ alpha_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ int path[64];
  const int tr = trun[b];
  if (tid == 0) {
    int cur = best_at[(long)b * steps + tr - 1];
    for (int t = tr - 1; t >= 0; --t) {
      const long o = ((long)b * steps + t) * K + cur;
      ids_out[(long)b * steps + t] = tokv[o];
      path[t] = back[o];  // row of the PARENT beam whose logits produced this token (model.py:198-201)
      cur = back[o];
    }
    for (int t = tr; t < steps; ++t) ids_out[(long)b * steps + t] = -1;
  }
  __syncthreads();
  for (int t = 0; t < tr; ++t)
    for (int v = tid; v < V; v += blockDim.x)
      logits_out[((long)b * steps + t) * V + v] = ws_logits[(((long)b * steps + t) * K + path[t]) * V + v];
  if (alpha_ws)
    for (int i = tid; i < steps * T; i += blockDim.x) {
      const int t = i / T, j = i - t * T;
      alpha_out[((long)b * steps + t) * T + j] = t < tr ? alpha_ws[(((long)b * steps + t) * K + path[t]) * T + j] : 0.f;
    }
}

// shapes of the matrix-core kernels (attn_beam_mfma.hip: hidden 256, the logits of a row in 256 LDS floats, T <= 48; beam <= 8)
static bool attn_mfma_shape(int T, int H, int V) { return H == 256 && V <= 256 && T <= 48; }
static int check_attn(const float* bh, const float* ph, const msocr_attn_weights* w, int B, int T, int H, int V, int steps) {
  if (!bh || !ph || !w || B <= 0 || T <= 0 || T > 64 || H < 64 || H > 512 || H % 64 || V <= 0 || V > 512 || steps <= 0 || steps > 64)
    return MSOCR_E_ARG;
  if (!w->h2h_wt || !w->h2h_b || !w->score_w || !w->wih_ctx_t || !w->wih_tok || !w->whh_t || !w->b_gates || !w->gen_wt || !w->gen_b)
    return MSOCR_E_ARG;
  return MSOCR_OK;
}

// workspace: logits [B][steps][K][V] f32 | back [B][steps][K] i32 | tokv [B][steps][K] i32 | best_at [B][steps] i32
static inline int64_t beam_ws_logits(int B, int steps, int K, int V) { return (int64_t)B * steps * K * V * 4; }
extern "C" int64_t msocr_attn_beam_workspace_bytes(int B, int steps, int beam, int V) {
  if (B <= 0 || steps <= 0 || beam <= 0 || V <= 0) return 0;
  return beam_ws_logits(B, steps, beam, V) + (int64_t)B * steps * beam * 8 + (int64_t)B * steps * 4 + 256;
}
// the separate attention-weight workspace of a beam decode with alpha_out: [B][steps][K][T] f32, slot-indexed like the logits trace
extern "C" int64_t msocr_attn_beam_alpha_bytes(int B, int steps, int beam, int T) {
  if (B <= 0 || steps <= 0 || beam <= 0 || T <= 0) return 0;
  return (int64_t)B * steps * beam * T * 4;
}

// whether the struct describes a table this decode can index: order 1..3, the decode's V, n_ctx = V^(order - 1), n_ctx * V <= 2^26
static bool charlm_ok(const msocr_charlm* lm, int V) {
  if (!lm || !lm->table || lm->order < 1 || lm->order > 3 || lm->V != V || V <= 0) return false;
  int64_t n = 1;
  for (int i = 1; i < lm->order; ++i) n *= V;
  return lm->n_ctx == n && n * V <= ((int64_t)1 << 26);
}

// msocr_attn_decode (msocr.h) in three parts: what a descriptor must satisfy, AttnArgs from it, the launcher for it.
static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

static int attn_desc_check(const msocr_attn_desc* d) {
  if (!d || d->struct_bytes != (int32_t)sizeof(msocr_attn_desc)) return MSOCR_E_ARG;
  const bool beam = d->mode == MSOCR_ATTN_MODE_BEAM, forced = d->mode == MSOCR_ATTN_MODE_FORCED;
  if (!beam && !forced && d->mode != MSOCR_ATTN_MODE_GREEDY) return MSOCR_E_ARG;
  // a pointer the mode does not read must be NULL: a call that mixes modes is refused, not half-ignored
  if (beam ? d->logits_out || d->ids_out
           : d->lp || d->workspace || d->fin_step_out || d->chunk_id || d->chunk_size || d->chunk_state || d->lexicon || d->lm)
    return MSOCR_E_ARG;
  if ((forced ? d->ids_out != nullptr : d->tok_in != nullptr) || (d->ws && !d->ctx_gates) || (d->node_out && !d->lexicon) ||
      (d->ctx_out && !d->lm))
    return MSOCR_E_ARG;
  // every mode: the envelope, the weights, the start token
  if (check_attn(d->batch_H, d->proj_H, d->w, d->B, d->T, d->H, d->V, d->steps) || d->sos_id < 0 || d->sos_id >= d->V) return MSOCR_E_ARG;
  // what the mode reads and writes
  if (beam) {
    if (!d->fin_step_out || !d->workspace || misaligned16(d->workspace) || misaligned16(d->alpha_out) || d->beam < 1 || d->beam > 16)
      return MSOCR_E_ARG;
  } else if (!d->logits_out || (forced ? !d->tok_in || !d->alpha_out : !d->ids_out)) {
    return MSOCR_E_ARG;
  }
  // ctx_gates given: the matrix-core kernels, their shapes and alignments; greedy and forced need the split weights, beam runs on
  // exact f32 without them
  if (d->ctx_gates) {
    const msocr_attn_split_weights* ws = d->ws;
    if (misaligned16(d->ctx_gates) || !attn_mfma_shape(d->T, d->H, d->V) || (beam && d->beam > 8) || (!ws && !beam)) return MSOCR_E_ARG;
    if (ws && (!ws->h2h_p || !ws->whh_p || !ws->gen_p || misaligned16(ws->h2h_p) || misaligned16(ws->whh_p) || misaligned16(ws->gen_p)))
      return MSOCR_E_ARG;
  }
  // the two beam options: one at a time, each with its trace and the weight trace (their kernels have the weight output on)
  const msocr_lexicon* lex = d->lexicon;
  if (lex && (d->lm || !lex->edge_begin || !lex->edge_tok || !lex->edge_child || !lex->terminal || lex->n_nodes < 1 || lex->n_edges < 0 ||
              !d->node_out || !d->alpha_out || d->beam * d->H > 4096))
    return MSOCR_E_ARG;
  if (d->lm && (!charlm_ok(d->lm, d->V) || !d->ctx_out || !d->alpha_out || !(d->lm_weight >= 0.f) || !std::isfinite(d->lm_weight) ||
                d->beam * d->H > 4096))
    return MSOCR_E_ARG;
  return MSOCR_OK;
}

static AttnArgs attn_args(const msocr_attn_desc* d) {
  const bool beam = d->mode == MSOCR_ATTN_MODE_BEAM;
  AttnArgs a{};
  a.batch_H = d->batch_H; a.proj_H = d->proj_H; a.w = *d->w; a.ctx_gates = d->ctx_gates;
  if (d->ws) { a.h2h_p = d->ws->h2h_p; a.whh_p = d->ws->whh_p; a.gen_p = d->ws->gen_p; }
  a.B = d->B; a.T = d->T; a.V = d->V; a.steps = d->steps; a.K = beam ? d->beam : 1;
  a.sos_id = d->sos_id; a.blank_id = d->blank_id;
  a.eos_id = d->mode == MSOCR_ATTN_MODE_FORCED ? -1 : d->eos_id;  // the forced decode ends no row
  a.temperature = beam ? d->temperature : 1.0f;
  a.alpha_out = d->alpha_out;  // nullptr: off
  a.tok_in = d->tok_in;
  if (!beam) {
    a.logits_out = d->logits_out; a.ids_out = d->ids_out;
    return a;
  }
  a.lp = d->lp;
  char* p = (char*)d->workspace;
  a.logits_out = (float*)p; p += beam_ws_logits(d->B, d->steps, d->beam, d->V);
  a.back = (int32_t*)p; p += (int64_t)d->B * d->steps * d->beam * 4;
  a.tokv = (int32_t*)p; p += (int64_t)d->B * d->steps * d->beam * 4;
  a.best_at = (int32_t*)p;
  a.fin_step = d->fin_step_out;
  if (d->chunk_id && d->chunk_size && d->chunk_state) { a.chunk_id = d->chunk_id; a.chunk_size = d->chunk_size; a.chunk_state = d->chunk_state; }
  if (const msocr_lexicon* lex = d->lexicon) {
    a.lex_begin = lex->edge_begin; a.lex_tok = lex->edge_tok; a.lex_child = lex->edge_child; a.lex_terminal = lex->terminal;
    a.lex_nodes = lex->n_nodes; a.lex_edges = lex->n_edges; a.node_out = d->node_out;
  }
  if (const msocr_charlm* lm = d->lm) {  // every slot starts at the "all SOS" row
    a.lm_table = lm->table; a.lm_nctx = (int)lm->n_ctx; a.lm_weight = d->lm_weight; a.ctx_out = d->ctx_out;
    for (int i = 1; i < lm->order; ++i) a.lm_ctx0 = a.lm_ctx0 * d->V + d->sos_id;
  }
  return a;
}

// ctx_gates == nullptr: the general kernels, every shape of the envelope; otherwise the matrix-core kernels.  The forced, lexicon and
// language-model kernels are in translation units of their own; so are the matrix-core kernels with the weight output on.
static int attn_launch(const msocr_attn_desc* d, const AttnArgs& a, hipStream_t s) {
  const bool mfma = d->ctx_gates != nullptr, beam = d->mode == MSOCR_ATTN_MODE_BEAM;
  if (d->mode == MSOCR_ATTN_MODE_FORCED) return mfma ? msocr_internal_attn_forced_mfma(a, s) : msocr_internal_attn_general_forced(a, d->H, s);
  if (d->lexicon) return mfma ? msocr_internal_attn_lexicon_mfma(a, s) : msocr_internal_attn_general_lexicon(a, d->H, s);
  if (d->lm) return mfma ? msocr_internal_attn_lm_mfma(a, s) : msocr_internal_attn_general_lm(a, d->H, s);
  if (!mfma) return msocr_internal_attn_general(a, d->H, beam, s);
  if (beam) return a.alpha_out ? msocr_internal_attn_beam_mfma_alpha(a, s) : msocr_internal_attn_beam_mfma(a, s);
  return a.alpha_out ? msocr_internal_attn_greedy_mfma_alpha(a, s) : msocr_internal_attn_greedy_mfma(a, s);
}

extern "C" int msocr_attn_decode(const msocr_attn_desc* d, void* stream) {
  if (attn_desc_check(d)) return MSOCR_E_ARG;
  return attn_launch(d, attn_args(d), (hipStream_t)stream);
}

// the size of node_out (lexicon) and of ctx_out (language model): [B][steps][beam] i32, one entry per slot and step
extern "C" int64_t msocr_attn_beam_slots_bytes(int B, int steps, int beam) {
  if (B <= 0 || steps <= 0 || beam <= 0) return 0;
  return (int64_t)B * steps * beam * 4;
}

// the four parts of a finished beam workspace (device memory, or a host copy of it), for the steps that read it back
struct BeamTrace {
  const float* logits;     // [B][steps][K][V]: row k of step t = the logits of the hypothesis in slot k when step t is computed
  const int32_t* back;     // [B][steps][K]: the row of logits[t] that the survivor in slot k of step t was extended from
  const int32_t* tokv;     // [B][steps][K]: the token it was extended by
  const int32_t* best_at;  // [B][steps]: the slot with the largest score after step t
};
static inline BeamTrace beam_ws_trace(const void* workspace, int B, int steps, int K, int V) {
  const char* p = (const char*)workspace;
  BeamTrace w;
  w.logits = (const float*)p; p += beam_ws_logits(B, steps, K, V);
  w.back = (const int32_t*)p; p += (int64_t)B * steps * K * 4;
  w.tokv = (const int32_t*)p; p += (int64_t)B * steps * K * 4;
  w.best_at = (const int32_t*)p;
  return w;
}

// alpha_ws [B][steps][beam][T] (a beam decode's alpha_out), T and alpha_out [B][steps][T]: also gathers the path's attention weights;
// NULL, 0, NULL: off (a T or an alpha_out without alpha_ws is refused)
extern "C" int msocr_attn_beam_finalize(const void* workspace, int B, int V, int steps, int beam, const int32_t* trun_dev,
                                        float* logits_out, int32_t* ids_out, const void* alpha_ws, int T, float* alpha_out,
                                        void* stream) {
  if (!workspace || !trun_dev || !logits_out || !ids_out || B <= 0 || V <= 0 || steps <= 0 || steps > 64 || beam < 1 || beam > 16)
    return MSOCR_E_ARG;
  if (alpha_ws ? misaligned16(alpha_ws) || !alpha_out || T <= 0 || T > 64 : alpha_out || T) return MSOCR_E_ARG;
  const BeamTrace w = beam_ws_trace(workspace, B, steps, beam, V);
  MSOCR_LAUNCH(attn_beam_finalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, w.logits, w.back, w.tokv, w.best_at, trun_dev, V,
               steps, beam, logits_out, ids_out, (const float*)alpha_ws, T, alpha_out);
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- confidence
// TRBA.predict's confidence (recognizers/_trba/__init__.py:413-431): log_softmax over V of the returned logits,
// exp of the chosen token's log-prob, mean over ALL t_run generated positions.  One wave per row.

// log_softmax(x[0 .. V))[id] by one wave, in every lane: the log-probability of the chosen token of one decode step
__device__ __forceinline__ float token_logp(const float* __restrict__ x, int V, int id, int lane) {
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
  s = wave_sum(s);
  return (x[id] - m) - logf(s);
}
// its exponential: the probability of that token
__device__ __forceinline__ float token_prob(const float* __restrict__ x, int V, int id, int lane) { return expf(token_logp(x, V, id, lane)); }
// the confidence of a row from the f32 sum, in step order, of its t_run token probabilities
__host__ __device__ __forceinline__ float mean_prob(float acc, int tr) { return tr > 0 ? acc / (float)tr : 0.f; }

__global__ __launch_bounds__(64) void seq_confidence_kernel(const float* __restrict__ logits, const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ trun, int V, int steps,
                                                             float* __restrict__ conf) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int tr = trun[b];
  float acc = 0.f;
  for (int t = 0; t < tr; ++t) acc += token_prob(logits + ((long)b * steps + t) * V, V, ids[(long)b * steps + t], lane);
  if (lane == 0) conf[b] = mean_prob(acc, tr);
}

extern "C" int msocr_seq_confidence(const float* logits, const int32_t* ids, const int32_t* trun_dev, int B, int V, int steps,
                                    float* conf_out, void* stream) {
  if (!logits || !ids || !trun_dev || !conf_out || B <= 0 || V <= 0 || steps <= 0) return MSOCR_E_ARG;
  MSOCR_LAUNCH(seq_confidence_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, ids, trun_dev, V, steps, conf_out);
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- per-symbol details
// What the word confidence is the mean of, and where the decoder looked: one wave per (row, step), lane = encoder frame (T <= 64).
//   prob   = token_prob of the step (the mean of prob[b][: t_run] is msocr_seq_confidence's value up to the order of the sum)
//   centre = sum_j alpha[j] * (j + 0.5), in frames; summed in f64 (64 terms: the f32 result is the rounded exact sum)
//   peak   = arg-max frame, the smaller index on ties
// Steps t >= t_run: 0, 0, -1.
constexpr int CD_WAVES = 4;
__global__ __launch_bounds__(64 * CD_WAVES) void seq_char_details_kernel(const float* __restrict__ logits, const int32_t* __restrict__ ids,
                                                                         const float* __restrict__ alpha, const int32_t* __restrict__ trun,
                                                                         int B, int V, int steps, int T, float* __restrict__ prob,
                                                                         float* __restrict__ centre, int32_t* __restrict__ peak) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * CD_WAVES + (threadIdx.x >> 6);  // (row, step) of this wave
  if (p >= (long)B * steps) return;
  const int b = (int)(p / steps), t = (int)(p - (long)b * steps);
  if (t >= trun[b]) {
    if (lane == 0) { prob[p] = 0.f; centre[p] = 0.f; peak[p] = -1; }
    return;
  }
  const float pr = token_prob(logits + p * V, V, ids[p], lane);
  float av = lane < T ? alpha[p * T + lane] : -INFINITY;
  double c = lane < T ? (double)av * ((double)lane + 0.5) : 0.0;
  int ai = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o);
    const float ov = __shfl_xor(av, o);
    const int oi = __shfl_xor(ai, o);
    if (ov > av || (ov == av && oi < ai)) { av = ov; ai = oi; }
  }
  if (lane == 0) { prob[p] = pr; centre[p] = (float)c; peak[p] = ai; }
}

extern "C" int msocr_seq_char_details(const float* logits, const int32_t* ids, const float* alpha, const int32_t* trun_dev, int B, int V,
                                      int steps, int T, float* prob_out, float* centre_out, int32_t* peak_out, void* stream) {
  if (!logits || !ids || !alpha || !trun_dev || !prob_out || !centre_out || !peak_out || B <= 0 || V <= 0 || steps <= 0 || T <= 0 || T > 64)
    return MSOCR_E_ARG;
  const long n = (long)B * steps;
  MSOCR_LAUNCH(seq_char_details_kernel, dim3((unsigned)((n + CD_WAVES - 1) / CD_WAVES)), dim3(64 * CD_WAVES), 0, (hipStream_t)stream, logits,
               ids, alpha, trun_dev, B, V, steps, T, prob_out, centre_out, peak_out);
  return LAUNCH_OK();
}

// --------------------------------------------------------------------------------------------- n-best readings
// A second read-out of the beam workspace: the K hypotheses a row's search ends with, not only the best.  Both beam kernels pick a
// step's K survivors by K rounds of arg-max with winner removal (larger value first, then the smaller flat index), so the slots of
// a step are in rank order and the r-th best final hypothesis is the back-trace from slot r of step t_run-1; nothing is re-ranked.
//   rank 0  = the slot best_at[t_run-1], attn_beam_finalize_kernel's own start (the same walk, the same ids)
//   rank 1..= the remaining slots in slot order
// Per (row, rank): ids and token_prob of every step of the path, the confidence of the path (mean_prob of the f32 sum in step
// order: seq_confidence_kernel's arithmetic) and its summed log-probability, the quantity the search ranks by: the token_logp terms
// up to and including the path's first EOS (a finished hypothesis is extended by EOS at log-probability 0, model.py:145-156),
// accumulated in f64 in step order and rounded once.  Steps t >= t_run: id -1, probability 0.
// One workgroup per (row, rank): one thread walks the back-pointers into LDS, the waves take the steps round-robin (token_logp, one
// wave per step), one thread does the two ordered sums.

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the path of rank `rank` of row b: row[t] = its row of logits[t], tok[t] = its token, t < tr (1 <= tr <= steps).  Slots read from the
// workspace are clamped to [0, K): a workspace that holds no finished search cannot send the walk out of bounds.
__host__ __device__ inline void nbest_walk(const BeamTrace& w, int b, int steps, int K, int tr, int rank, int* row, int* tok) {
  const int best = clampi(w.best_at[(long)b * steps + tr - 1], 0, K - 1);
  int cur = rank == 0 ? best : (rank <= best ? rank - 1 : rank);
  for (int t = tr - 1; t >= 0; --t) {
    const long o = ((long)b * steps + t) * K + cur;
    tok[t] = w.tokv[o];
    cur = row[t] = clampi(w.back[o], 0, K - 1);
  }
}
// the two ordered sums over a path's steps: p[t] = token_prob, lp[t] = token_logp of step t
__host__ __device__ inline void nbest_sums(const float* p, const float* lp, const int* tok, int tr, int eos_id, float* conf, float* logp) {
  float acc = 0.f;
  double sum = 0.0;
  bool open = true;  // no EOS yet
  for (int t = 0; t < tr; ++t) {
    acc += p[t];
    if (open) {
      sum += (double)lp[t];
      open = tok[t] != eos_id;
    }
  }
  *conf = mean_prob(acc, tr);
  *logp = (float)sum;
}

constexpr int NB_WAVES = 4;
__global__ __launch_bounds__(64 * NB_WAVES) void attn_beam_nbest_kernel(BeamTrace w, const int32_t* __restrict__ trun, int V, int steps, int K,
                                                                        int n_best, int eos_id, int32_t* __restrict__ ids_out,
                                                                        float* __restrict__ prob_out, float* __restrict__ conf_out,
                                                                        float* __restrict__ logp_out) {
  const int b = blockIdx.x / n_best, rank = blockIdx.x - b * n_best;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int s_row[64], s_tok[64];
  __shared__ float s_p[64], s_lp[64];
  const int tr = clampi(trun[b], 1, steps);
  const long o = (long)blockIdx.x * steps;  // (b * n_best + rank) * steps
  if (threadIdx.x == 0) nbest_walk(w, b, steps, K, tr, rank, s_row, s_tok);
  __syncthreads();
  for (int t = wave; t < steps; t += NB_WAVES) {
    float lp = 0.f, p = 0.f;
    int id = -1;
    if (t < tr) {  // wave-uniform
      id = s_tok[t];
      lp = token_logp(w.logits + (((long)b * steps + t) * K + s_row[t]) * V, V, clampi(id, 0, V - 1), lane);
      p = expf(lp);  // token_prob
    }
    if (lane == 0) {
      s_lp[t] = lp;
      s_p[t] = p;
      ids_out[o + t] = id;
      prob_out[o + t] = p;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) nbest_sums(s_p, s_lp, s_tok, tr, eos_id, conf_out + blockIdx.x, logp_out + blockIdx.x);
}

static bool nbest_args_ok(const void* workspace, int B, int V, int steps, int beam, int n_best, const int32_t* trun,
                          const int32_t* ids_out, const float* prob_out, const float* conf_out, const float* logp_out) {
  return workspace && trun && ids_out && prob_out && conf_out && logp_out && B > 0 && V > 0 && V <= 512 && steps > 0 && steps <= 64 &&
         beam >= 1 && beam <= 16 && n_best >= 1 && n_best <= beam;
}

extern "C" int msocr_attn_beam_nbest(const void* workspace, int B, int V, int steps, int beam, int n_best, int eos_id,
                                     const int32_t* trun_dev, int32_t* ids_out, float* prob_out, float* conf_out, float* logp_out,
                                     void* stream) {
  if (!nbest_args_ok(workspace, B, V, steps, beam, n_best, trun_dev, ids_out, prob_out, conf_out, logp_out)) return MSOCR_E_ARG;
  if ((int64_t)B * n_best > 0x7fffffff) return MSOCR_E_ARG;
  MSOCR_LAUNCH(attn_beam_nbest_kernel, dim3((unsigned)(B * n_best)), dim3(64 * NB_WAVES), 0, (hipStream_t)stream,
               beam_ws_trace(workspace, B, steps, beam, V), trun_dev, V, steps, beam, n_best, eos_id, ids_out, prob_out, conf_out, logp_out);
  return LAUNCH_OK();
}

// token_logp as one wave evaluates it, on the host: 64 strided partial sums combined by the xor butterfly of wave_sum, so that the
// twin differs from the kernel only by what expf / logf differ between the device and libm
static float token_logp_host(const float* x, int V, int id) {
  float m = -INFINITY;
  for (int v = 0; v < V; ++v) m = fmaxf(m, x[v]);
  float part[64], next[64];
  for (int l = 0; l < 64; ++l) {
    part[l] = 0.f;
    for (int v = l; v < V; v += 64) part[l] += expf(x[v] - m);
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; ++l) next[l] = part[l] + part[l ^ o];
    for (int l = 0; l < 64; ++l) part[l] = next[l];
  }
  return (x[id] - m) - logf(part[0]);
}

// msocr_attn_beam_nbest over host copies of the workspace and of t_run: the same walk, the same order of sums
extern "C" int msocr_attn_beam_nbest_host(const void* workspace_host, int B, int V, int steps, int beam, int n_best, int eos_id,
                                          const int32_t* trun_host, int32_t* ids_out_host, float* prob_out_host, float* conf_out_host,
                                          float* logp_out_host) {
  if (!nbest_args_ok(workspace_host, B, V, steps, beam, n_best, trun_host, ids_out_host, prob_out_host, conf_out_host, logp_out_host))
    return MSOCR_E_ARG;
  const BeamTrace w = beam_ws_trace(workspace_host, B, steps, beam, V);
  for (int b = 0; b < B; ++b)
    for (int rank = 0; rank < n_best; ++rank) {
      int row[64], tok[64];
      float p[64], lp[64];
      const int tr = clampi(trun_host[b], 1, steps);
      const long q = (long)b * n_best + rank, o = q * steps;
      nbest_walk(w, b, steps, beam, tr, rank, row, tok);
      for (int t = 0; t < steps; ++t) {
        const bool on = t < tr;
        lp[t] = on ? token_logp_host(w.logits + (((long)b * steps + t) * beam + row[t]) * V, V, clampi(tok[t], 0, V - 1)) : 0.f;
        p[t] = on ? expf(lp[t]) : 0.f;
        ids_out_host[o + t] = on ? tok[t] : -1;
        prob_out_host[o + t] = p[t];
      }
      nbest_sums(p, lp, tok, tr, eos_id, conf_out_host + q, logp_out_host + q);
    }
  return MSOCR_OK;
}

// --------------------------------------------------------------------------------------------- log-probability of given ids
// How well a given token sequence fits the logits of a (forced) decode: per step log_softmax(logits / temperature)[id] in f32 with
// max subtraction (the division is a true f32 division and is skipped at temperature 1, as in the beam kernels), and per row the sum
// over t < t_run, accumulated in f64 in step order and rounded once (msocr_attn_beam_nbest's convention for logp_out).  Steps
// t >= t_run hold 0.  An id outside [0, V) at a step t < t_run makes that step and the row's sum NaN; nothing is read through it.
// The kernel and its host twin share the three pieces below; they differ in how the 64 lane partials are combined (cross-lane
// exchange on the device, the same xor butterfly over an array on the host) and in what expf / logf differ between the two.

struct SeqScale {  // logits / temperature as the beam kernels apply it
  float temp;
  bool div;
  __host__ __device__ explicit SeqScale(float temperature) : temp(temperature > 1e-6f ? temperature : 1e-6f), div(temperature != 1.0f) {}
  __host__ __device__ __forceinline__ float operator()(float x) const { return div ? x / temp : x; }
};
// lane `lane` of 64: its part of the maximum, and of the sum of exponentials under the maximum m
__host__ __device__ __forceinline__ float seq_lane_max(const float* x, int V, int lane, const SeqScale& sc) {
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, sc(x[v]));
  return m;
}
__host__ __device__ __forceinline__ float seq_lane_sum(const float* x, int V, int lane, float m, const SeqScale& sc) {
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(sc(x[v]) - m);
  return s;
}
// the step's value from the maximum and the sum
__host__ __device__ __forceinline__ float seq_step_logp(const float* x, int V, int id, float m, float sum, const SeqScale& sc) {
  return id >= 0 && id < V ? (sc(x[id]) - m) - logf(sum) : __builtin_nanf("");
}
// a row: zeros behind t_run, the f64 sum in step order of what is before it
__host__ __device__ inline void seq_row_sum(float* lp_steps, int steps, int tr, float* logp) {
  double sum = 0.0;
  for (int t = 0; t < steps; ++t) {
    if (t < tr) sum += (double)lp_steps[t];
    else lp_steps[t] = 0.f;
  }
  *logp = (float)sum;
}

constexpr int LP_WAVES = 4;
// one workgroup per row, one wave per (row, step): the waves take the steps round-robin, thread 0 does the ordered sum
__global__ __launch_bounds__(64 * LP_WAVES) void seq_logp_kernel(const float* __restrict__ logits, const int32_t* __restrict__ ids,
                                                                  const int32_t* __restrict__ trun, int V, int steps, float temperature,
                                                                  float* __restrict__ logp_steps, float* __restrict__ logp) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tr = clampi(trun[b], 0, steps);
  const SeqScale sc(temperature);
  __shared__ float s_lp[64];
  for (int t = wave; t < tr; t += LP_WAVES) {
    const float* x = logits + ((long)b * steps + t) * V;
    float m = seq_lane_max(x, V, lane, sc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float sum = wave_sum(seq_lane_sum(x, V, lane, m, sc));
    if (lane == 0) s_lp[t] = seq_step_logp(x, V, ids[(long)b * steps + t], m, sum, sc);
  }
  __syncthreads();
  if (threadIdx.x == 0) seq_row_sum(s_lp, steps, tr, logp + b);
  __syncthreads();
  if (threadIdx.x < steps) logp_steps[(long)b * steps + threadIdx.x] = s_lp[threadIdx.x];
}

static bool seq_logp_args_ok(const float* logits, const int32_t* ids, const int32_t* trun, int B, int V, int steps, const float* lps,
                             const float* lp) {
  return logits && ids && trun && lps && lp && B > 0 && V > 0 && V <= 512 && steps > 0 && steps <= 64;
}

extern "C" int msocr_seq_logp(const float* logits, const int32_t* ids, const int32_t* trun_dev, int B, int V, int steps, float temperature,
                              float* logp_steps_out, float* logp_out, void* stream) {
  if (!seq_logp_args_ok(logits, ids, trun_dev, B, V, steps, logp_steps_out, logp_out)) return MSOCR_E_ARG;
  MSOCR_LAUNCH(seq_logp_kernel, dim3(B), dim3(64 * LP_WAVES), 0, (hipStream_t)stream, logits, ids, trun_dev, V, steps, temperature,
               logp_steps_out, logp_out);
  return LAUNCH_OK();
}

// msocr_seq_logp over host arrays
extern "C" int msocr_seq_logp_host(const float* logits_host, const int32_t* ids_host, const int32_t* trun_host, int B, int V, int steps,
                                   float temperature, float* logp_steps_out_host, float* logp_out_host) {
  if (!seq_logp_args_ok(logits_host, ids_host, trun_host, B, V, steps, logp_steps_out_host, logp_out_host)) return MSOCR_E_ARG;
  const SeqScale sc(temperature);
  for (int b = 0; b < B; ++b) {
    const int tr = clampi(trun_host[b], 0, steps);
    float* const out = logp_steps_out_host + (long)b * steps;
    for (int t = 0; t < tr; ++t) {
      const float* x = logits_host + ((long)b * steps + t) * V;
      float m = -INFINITY, part[64], next[64];
      for (int l = 0; l < 64; ++l) m = fmaxf(m, seq_lane_max(x, V, l, sc));
      for (int l = 0; l < 64; ++l) part[l] = seq_lane_sum(x, V, l, m, sc);
      for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; ++l) next[l] = part[l] + part[l ^ o];
        for (int l = 0; l < 64; ++l) part[l] = next[l];
      }
      out[t] = seq_step_logp(x, V, ids_host[(long)b * steps + t], m, part[0], sc);
    }
    seq_row_sum(out, steps, tr, logp_out_host + b);
  }
  return MSOCR_OK;
}
