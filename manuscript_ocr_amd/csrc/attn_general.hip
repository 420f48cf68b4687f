// attn_general.hip — attention decode of the TRBA recogniser for every shape of the envelope: hidden sizes 64..512 (the reference
// reads hidden_size from the checkpoint's config, recognizers/_trba/__init__.py:142-151), charsets of up to 512 tokens, beam widths
// of up to 16 (TRBA.predict exposes beam_size, :295-299; the reference's own Optuna script sweeps 2..12).  The plain entry points
// (msocr_attn_greedy / msocr_attn_beam) run it; the recogniser takes it for the shapes the matrix-core kernels (attn_beam_mfma.hip:
// hidden 256, <= 256 tokens, <= 48 frames, beam <= 8) do not take, and for greedy decoding under precision "fp32-exact".  Exact f32
// with libm-grade expf / tanhf; same outputs, workspace layout and tie rules as the matrix-core kernels: one 256-thread workgroup
// per batch row runs the whole step loop, the K beam rows' state (h, c, context, h2h projection, logits) lives in LDS, every phase
// is a strided loop over (row, unit) or (row, token) pairs, weights stream from L2.  Written for generality, not speed: the default
// configuration (hidden 256, 194 tokens, beam 8, precision "fp32") never comes here.
//
// Replaces recognizers/_trba/model/model.py:34-46 (AttentionCell.forward), :227-259 (_greedy_decode), :92-225 (_beam_decode).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "internal.h"
#include "msocr.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The forced decode is a compile-time fact of the translation unit, like the attention-weight output of attn_beam_mfma.hip: this file
// is compiled twice, as itself (FORCED false: the greedy and beam kernels behind msocr_internal_attn_general) and through
// attn_general_forced.hip, which defines MSOCR_ATTN_FORCED and includes it (FORCED true: the greedy instantiation alone, behind
// msocr_internal_attn_general_forced).  A second kernel in THIS unit, through a shared body, moved the beam kernel from 77 to 78
// VGPRs (profiles/attn_forced.txt); a unit of its own leaves both kernels' code as it was.
// FORCED = Attention.forward(is_train=True) of the reference (model.py:287-320) with sampling_prob 0: the token fed to step s is
// a.tok_in[b][s] instead of the arg-max of step s - 1 (an id outside [0, V) is replaced by sos_id before it indexes wih_tok); logits
// and weights are stored as in greedy, the arg-max and the ids are not computed.
#ifdef MSOCR_ATTN_FORCED
constexpr bool FORCED = true;
#else
constexpr bool FORCED = false;
#endif
// The lexicon constraint is the same kind of fact: attn_general_lexicon.hip defines MSOCR_ATTN_LEXICON and includes this file, which then
// holds the beam instantiation alone, behind msocr_internal_attn_general_lexicon.  Every beam slot carries a node of the lexicon's prefix
// tree (a.lex_*, msocr_lexicon); a live slot's candidates are its node's child tokens, and EOS where a word ends at the node; every other
// candidate is -inf.  The log-sum-exp stays over the full row: a path's score is the model's own joint log-probability of that text.
// The lines the constraint adds are under #ifdef, so this file compiled as itself is the text it was.
#ifdef MSOCR_ATTN_LEXICON
#include "lexicon_walk.h"
#endif
// And so is the fusion of a character n-gram language model (shallow fusion): attn_general_lm.hip defines MSOCR_ATTN_LM and includes this
// file, which then holds the beam instantiation alone, behind msocr_internal_attn_general_lm.  Every beam slot carries the row of the
// model's dense table it stands at (a.lm_table [n_ctx][V], msocr_charlm; the slot's context = its last order - 1 tokens); a live slot's
// candidates gain lm_weight * table[ctx][v] after the log-softmax, whose log-sum-exp stays over the full row; a finished slot keeps the
// plain rule.  Nothing is forbidden.  The logits trace holds the model's logits, not fused values.  ctx stays inside [0, n_ctx) and the
// token inside [0, V) by construction, and no index is formed from a table value.  Lines under #ifdef, as above.

namespace {

constexpr int NTH = 256;
constexpr int KCAP = 16;  // beam rows

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// block-wide arg-max, "larger value first, then smaller index"; NaN never wins
__device__ __forceinline__ void block_argmax(float v, int idx, float* s_val, int* s_idx, int tid, float& out_v, int& out_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  if ((tid & 63) == 0) { s_val[tid >> 6] = v; s_idx[tid >> 6] = idx; }
  __syncthreads();
  out_v = s_val[0];
  out_i = s_idx[0];
  for (int w = 1; w < NTH / 64; ++w)
    if (s_val[w] > out_v || (s_val[w] == out_v && s_idx[w] < out_i)) { out_v = s_val[w]; out_i = s_idx[w]; }
  __syncthreads();
}

// dynamic LDS: h [K][H] | c [K][H] | ctx [K][H] | ph [K][H] | logits [K][V] | alpha [K][64]
template <bool BEAM>
__global__ __launch_bounds__(NTH) void attn_general_kernel(AttnArgs a, int H) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int K = BEAM ? a.K : 1, T = a.T, V = a.V;
  float* sh = lds;
  float* sc = sh + K * H;
  float* sctx = sc + K * H;
  float* sph = sctx + K * H;
  float* slog = sph + K * H;
  float* salpha = slog + K * V;
  __shared__ float s_val[NTH / 64];
  __shared__ int s_idx[NTH / 64];
  __shared__ float s_score[KCAP], s_lse[KCAP], s_top[KCAP];
  __shared__ int s_tok[KCAP], s_done[KCAP], s_src[KCAP], s_nxt[KCAP];
#ifdef MSOCR_ATTN_LEXICON
  __shared__ int s_node[KCAP];             // the slot's trie node; -1 = dead (it left the trie, or was filled from an all -inf round)
  __shared__ unsigned s_mask[KCAP * 16];   // allowed tokens of every slot in this step, one bit per token (V <= 512), rebuilt every step
#endif
#ifdef MSOCR_ATTN_LM
  __shared__ int s_ctx[KCAP];  // the slot's row of the language model's table, in [0, lm_nctx)
#endif
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* bH = a.batch_H + (long)b * T * H;
  const float* pH = a.proj_H + (long)b * T * H;
  for (int i = tid; i < K * H; i += NTH) { sh[i] = 0.f; sc[i] = 0.f; }
  if (tid < K) {
    s_score[tid] = tid == 0 ? 0.f : -INFINITY;
    s_tok[tid] = a.sos_id;
    s_done[tid] = 0;
#ifdef MSOCR_ATTN_LEXICON
    s_node[tid] = 0;  // the root
#endif
#ifdef MSOCR_ATTN_LM
    s_ctx[tid] = a.lm_ctx0;  // "all SOS"
#endif
  }
  __syncthreads();
  int fin = a.steps;
  const float temp = fmaxf(a.temperature, 1e-6f);
  for (int s = 0; s < a.steps; ++s) {
    if constexpr (FORCED) {  // read by (e), four barriers on; the last reader of the old one, (e) of step s - 1, is barriers back
      if (tid == 0) {
        int tk = a.tok_in[(long)b * a.steps + s];
        if (tk < 0 || tk >= V) tk = a.sos_id;
        s_tok[0] = tk;
      }
    }
    // (a) ph[r][j] = h2h_b[j] + sum_k h[r][k] * h2h_wt[k][j]
    for (int i = tid; i < K * H; i += NTH) {
      const int r = i / H, j = i - r * H;
      float acc = a.w.h2h_b[j];
      for (int k = 0; k < H; ++k) acc = fmaf(a.w.h2h_wt[(long)k * H + j], sh[r * H + k], acc);
      sph[i] = acc;
    }
    __syncthreads();
    // (b) e[r][t] = sum_j score_w[j] * tanh(proj_H[t][j] + ph[r][j]) : one wave per (r, t)
    for (int p = wv; p < K * T; p += NTH / 64) {
      const int r = p / T, t = p - r * T;
      float e = 0.f;
      for (int j = lane; j < H; j += 64) e = fmaf(a.w.score_w[j], tanhf(pH[t * H + j] + sph[r * H + j]), e);
      e = wsum(e);
      if (lane == 0) salpha[r * 64 + t] = e;
    }
    __syncthreads();
    // (c) softmax over t
    if (tid < K) {
      float m = -INFINITY;
      for (int t = 0; t < T; ++t) m = fmaxf(m, salpha[tid * 64 + t]);
      float sum = 0.f;
      for (int t = 0; t < T; ++t) {
        const float ev = expf(salpha[tid * 64 + t] - m);
        salpha[tid * 64 + t] = ev;
        sum += ev;
      }
      // optional trace of the weights (AttnArgs::alpha_out, a kernel argument: uniform over the workgroup), [B][steps][K][T], from the
      // thread that holds the row
      float* const ao = a.alpha_out ? a.alpha_out + (((long)b * a.steps + s) * K + tid) * T : nullptr;
      for (int t = 0; t < T; ++t) {
        const float al = salpha[tid * 64 + t] / sum;
        salpha[tid * 64 + t] = al;
        if (ao) ao[t] = al;
      }
    }
    __syncthreads();
    // (d) ctx[r][j] = sum_t alpha[r][t] * batch_H[t][j]
    for (int i = tid; i < K * H; i += NTH) {
      const int r = i / H, j = i - r * H;
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = fmaf(salpha[r * 64 + t], bH[t * H + j], acc);
      sctx[i] = acc;
    }
    __syncthreads();
    // (e) LSTMCell: gates = W_ih[:, :H] ctx + W_ih[:, H + tok] + W_hh h + b ; new h into ph (dead since (b)), c in place
    for (int i = tid; i < K * H; i += NTH) {
      const int r = i / H, j = i - r * H;
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(&a.w.b_gates[j * 4]);
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(&a.w.wih_tok[((long)s_tok[r] * H + j) * 4]);
      f32x4 g = b4 + t4;
      for (int k = 0; k < H; ++k) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(&a.w.wih_ctx_t[((long)k * H + j) * 4]);
        const float x = sctx[r * H + k];
        g[0] = fmaf(w4[0], x, g[0]); g[1] = fmaf(w4[1], x, g[1]); g[2] = fmaf(w4[2], x, g[2]); g[3] = fmaf(w4[3], x, g[3]);
      }
      for (int k = 0; k < H; ++k) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(&a.w.whh_t[((long)k * H + j) * 4]);
        const float x = sh[r * H + k];
        g[0] = fmaf(w4[0], x, g[0]); g[1] = fmaf(w4[1], x, g[1]); g[2] = fmaf(w4[2], x, g[2]); g[3] = fmaf(w4[3], x, g[3]);
      }
      const float ig = sigm(g[0]), fg = sigm(g[1]), gg = tanhf(g[2]), og = sigm(g[3]);
      const float cn = fg * sc[i] + ig * gg;
      sc[i] = cn;
      sph[i] = og * tanhf(cn);
    }
    __syncthreads();
    for (int i = tid; i < K * H; i += NTH) sh[i] = sph[i];
    __syncthreads();
    // (f) logits[r][v] = gen_b[v] + sum_k h'[r][k] * gen_wt[k][v]
    for (int i = tid; i < K * V; i += NTH) {
      const int r = i / V, v = i - r * V;
      float acc = a.w.gen_b[v];
      for (int k = 0; k < H; ++k) acc = fmaf(a.w.gen_wt[(long)k * V + v], sh[r * H + k], acc);
      slog[i] = (v == a.blank_id) ? -1e4f : acc;
    }
    __syncthreads();
    if constexpr (FORCED) {
      for (int v = tid; v < V; v += NTH) a.logits_out[((long)b * a.steps + s) * V + v] = slog[v];  // rewritten by (f), barriers on
    } else if constexpr (!BEAM) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int v = tid; v < V; v += NTH) {
        const float x = slog[v];
        a.logits_out[((long)b * a.steps + s) * V + v] = x;
        if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
      }
      float wv_;
      int wi_;
      block_argmax(bv, bi, s_val, s_idx, tid, wv_, wi_);
      if (wi_ == 0x7fffffff) wi_ = 0;
      if (tid == 0) {
        s_tok[0] = wi_;
        a.ids_out[(long)b * a.steps + s] = wi_;
      }
      __syncthreads();
    } else {
      const int KB = K;
      // temperature (true f32 division, model.py:135-137) + trace
      for (int i = tid; i < K * V; i += NTH) {
        float x = slog[i];
        if (a.temperature != 1.0f) x = x / temp;
        slog[i] = x;
        const int r = i / V, v = i - r * V;
        a.logits_out[(((long)b * a.steps + s) * KB + r) * V + v] = x;
      }
#ifdef MSOCR_ATTN_LEXICON
      for (int i = tid; i < K * 16; i += NTH) s_mask[i] = 0u;
#endif
      __syncthreads();
      for (int r = wv; r < K; r += NTH / 64) {  // log-sum-exp per row
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, slog[r * V + v]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(slog[r * V + v] - m);
        sum = wsum(sum);
        if (lane == 0) s_lse[r] = m + logf(sum);
      }
#ifdef MSOCR_ATTN_LEXICON
      // allowed tokens: a live slot's edge list strided over the workgroup (an edge token outside [0, V) is ignored), EOS where its node
      // is terminal; a finished slot keeps today's rule (EOS alone); a dead slot has none
      for (int r = 0; r < K; ++r) {
        const int node = s_node[r];
        if (node < 0) continue;
        if (!s_done[r]) {
          int lo, hi;
          lex_edge_range(a.lex_begin, a.lex_nodes, a.lex_edges, node, lo, hi);
          for (int e = lo + tid; e < hi; e += NTH) {
            const int tk = a.lex_tok[e];
            if (tk >= 0 && tk < V) atomicOr(&s_mask[r * 16 + (tk >> 5)], 1u << (tk & 31));
          }
        }
        if (tid == 0 && a.eos_id >= 0 && a.eos_id < V && (s_done[r] || lex_terminal(a.lex_terminal, a.lex_nodes, node)))
          atomicOr(&s_mask[r * 16 + (a.eos_id >> 5)], 1u << (a.eos_id & 31));
      }
#endif
      __syncthreads();
      // candidates in place: (score[r] + logp[r][v]) / lp ; finished beams: only EOS with logp 0 (model.py:140-160)
      const float lp = a.lp ? a.lp[s] : 1.0f;
      for (int i = tid; i < K * V; i += NTH) {
        const int r = i / V, v = i - r * V;
        float logp = slog[i] - s_lse[r];
        if (s_done[r]) logp = (v == a.eos_id) ? 0.f : -INFINITY;
#ifdef MSOCR_ATTN_LEXICON
        if (!((s_mask[r * 16 + (v >> 5)] >> (v & 31)) & 1u)) logp = -INFINITY;
#endif
#ifdef MSOCR_ATTN_LM
        if (!s_done[r]) logp = fmaf(a.lm_weight, a.lm_table[s_ctx[r] * V + v], logp);  // weight 0, finite table: logp as it was, bit for bit
#endif
        float tot = s_score[r] + logp;
        if (a.lp) tot = tot / lp;
        slog[i] = tot;
      }
      __syncthreads();
      for (int kk = 0; kk < KB; ++kk) {  // top-K by K rounds of block arg-max over the flat index r * V + v
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < K * V; i += NTH) {
          const float x = slog[i];
          if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; }
        }
        float wv_;
        int wi_;
        block_argmax(bv, bi, s_val, s_idx, tid, wv_, wi_);
        if (wi_ == 0x7fffffff) wi_ = 0;  // every candidate NaN: degenerate input
        if (tid == 0) {
          s_top[kk] = wv_;
          s_src[kk] = wi_ / V;
          s_nxt[kk] = wi_ % V;
          slog[wi_] = __int_as_float(0x7fc00000);  // the winner never wins again
        }
        __syncthreads();
      }
      // reorder the beam state by src through ctx / ph (both dead here)
      for (int i = tid; i < K * H; i += NTH) {
        const int r = i / H, j = i - r * H;
        sctx[i] = sh[s_src[r] * H + j];
        sph[i] = sc[s_src[r] * H + j];
      }
      __syncthreads();
      for (int i = tid; i < K * H; i += NTH) { sh[i] = sctx[i]; sc[i] = sph[i]; }
      int nd = 1;
#ifdef MSOCR_ATTN_LEXICON
      int nn = -1;  // the new slot's node: its parent's where the hypothesis is finished, else the child along the token; -1 = dead
      if (tid < K) {
        const int src = s_src[tid], nxt = s_nxt[tid], ended = s_done[src] | (nxt == a.eos_id);
        nn = ended ? s_node[src] : lex_child(a.lex_begin, a.lex_tok, a.lex_child, a.lex_nodes, a.lex_edges, s_node[src], nxt);
        if (!isfinite(s_top[tid])) nn = -1;
        nd = ended | (nn < 0);  // no legal continuation counts as finished: fin_step still fires
      }
#else
      if (tid < K) nd = s_done[s_src[tid]] | (s_nxt[tid] == a.eos_id);
#endif
#ifdef MSOCR_ATTN_LM
      int nc = 0;  // the new slot's table row: its source's where the hypothesis is finished, else the source's shifted by the token
      if (tid < K) {
        const int src = s_src[tid], nxt = s_nxt[tid];  // src in [0, K), nxt in [0, V): the top-K's wi_ / V and wi_ % V of wi_ < K * V
        nc = nd ? s_ctx[src] : (int)(((long)s_ctx[src] * V + nxt) % a.lm_nctx);
      }
#endif
      __syncthreads();
      if (tid < K) {
        const long o = ((long)b * a.steps + s) * KB + tid;
        a.back[o] = s_src[tid];
        a.tokv[o] = s_nxt[tid];
        s_score[tid] = a.lp ? s_top[tid] * lp : s_top[tid];  // f32 round trip of the reference (model.py:188-192)
        s_tok[tid] = s_nxt[tid];
        s_done[tid] = nd;
#ifdef MSOCR_ATTN_LEXICON
        s_node[tid] = nn;
        a.node_out[o] = nn;
#endif
#ifdef MSOCR_ATTN_LM
        s_ctx[tid] = nc;
        a.ctx_out[o] = nc;
#endif
      }
      __syncthreads();
      if (tid == 0) {
        int best = 0, all = 1;
        float bs = s_score[0];
        for (int r = 0; r < KB; ++r) {
          if (r && s_score[r] > bs) { bs = s_score[r]; best = r; }
          all &= s_done[r];
        }
        a.best_at[(long)b * a.steps + s] = best;
        s_idx[0] = all;
      }
      __syncthreads();
      if (s_idx[0] && fin == a.steps) fin = s + 1;
      __syncthreads();
    }
  }
  if (BEAM && tid == 0) a.fin_step[b] = fin;
}

}  // namespace

#if defined(MSOCR_ATTN_LM)
// the one kernel of attn_general_lm.hip: the beam loop with the language model's addend.  Same shapes as msocr_internal_attn_general.
int msocr_internal_attn_general_lm(const AttnArgs& a, int H, hipStream_t s) {
  if (!a.lm_table || !a.ctx_out || !a.alpha_out || a.lm_nctx < 1 || a.lm_ctx0 < 0 || a.lm_ctx0 >= a.lm_nctx) return MSOCR_E_ARG;
  const int K = a.K;
  if (H < 64 || H > 512 || H % 64 || a.V <= 0 || a.V > 512 || a.T <= 0 || a.T > 64 || a.steps <= 0 || a.steps > 64 || K < 1 || K > KCAP ||
      K * H > 4096 || a.B <= 0 || (long)a.lm_nctx * a.V > (1L << 26))
    return MSOCR_E_ARG;
  const size_t ldsz = (size_t)(4 * K * H + K * a.V + K * 64) * sizeof(float);
  auto kb = attn_general_kernel<true>;
  if (msocr_internal_lds_limit((const void*)kb, 112 * 1024) != MSOCR_OK) return MSOCR_E_LAUNCH;
  if (ldsz > 112 * 1024) return MSOCR_E_ARG;
  MSOCR_LAUNCH(kb, dim3(a.B), dim3(NTH), ldsz, s, a, H);
  return LAUNCH_OK();
}
#elif defined(MSOCR_ATTN_LEXICON)
// the one kernel of attn_general_lexicon.hip: the beam loop under the lexicon constraint.  Same shapes as msocr_internal_attn_general.
int msocr_internal_attn_general_lexicon(const AttnArgs& a, int H, hipStream_t s) {
  if (!a.lex_begin || !a.lex_tok || !a.lex_child || !a.lex_terminal || a.lex_nodes < 1 || a.lex_edges < 0 || !a.node_out) return MSOCR_E_ARG;
  const int K = a.K;
  if (H < 64 || H > 512 || H % 64 || a.V <= 0 || a.V > 512 || a.T <= 0 || a.T > 64 || a.steps <= 0 || a.steps > 64 || K < 1 || K > KCAP ||
      K * H > 4096 || a.B <= 0)
    return MSOCR_E_ARG;
  const size_t ldsz = (size_t)(4 * K * H + K * a.V + K * 64) * sizeof(float);
  auto kb = attn_general_kernel<true>;
  if (msocr_internal_lds_limit((const void*)kb, 112 * 1024) != MSOCR_OK) return MSOCR_E_LAUNCH;
  if (ldsz > 112 * 1024) return MSOCR_E_ARG;
  MSOCR_LAUNCH(kb, dim3(a.B), dim3(NTH), ldsz, s, a, H);
  return LAUNCH_OK();
}
#elif defined(MSOCR_ATTN_FORCED)
// the one kernel of attn_general_forced.hip: the greedy loop along a.tok_in.  Same shapes as below with one row per crop.
int msocr_internal_attn_general_forced(const AttnArgs& a, int H, hipStream_t s) {
  if (!a.tok_in || !a.alpha_out || !a.logits_out || a.sos_id < 0 || a.sos_id >= a.V) return MSOCR_E_ARG;
  if (H < 64 || H > 512 || H % 64 || a.V <= 0 || a.V > 512 || a.T <= 0 || a.T > 64 || a.steps <= 0 || a.steps > 64 || a.B <= 0) return MSOCR_E_ARG;
  const size_t ldsz = (size_t)(4 * H + a.V + 64) * sizeof(float);
  auto kg = attn_general_kernel<false>;
  if (msocr_internal_lds_limit((const void*)kg, 112 * 1024) != MSOCR_OK) return MSOCR_E_LAUNCH;
  MSOCR_LAUNCH(kg, dim3(a.B), dim3(NTH), ldsz, s, a, H);
  return LAUNCH_OK();
}
#else
// Shapes taken: H % 64 == 0, 64 <= H <= 512, V <= 512, T <= 64, steps <= 64, beam <= 16, beam * H <= 4096 (the state of the beam
// rows must fit in LDS).  beam = 0 selects the greedy loop.
int msocr_internal_attn_general(const AttnArgs& a, int H, bool beam, hipStream_t s) {
  const int K = beam ? a.K : 1;
  if (H < 64 || H > 512 || H % 64 || a.V <= 0 || a.V > 512 || a.T <= 0 || a.T > 64 || a.steps <= 0 || a.steps > 64 || K < 1 || K > KCAP ||
      K * H > 4096)
    return MSOCR_E_ARG;
  const size_t ldsz = (size_t)(4 * K * H + K * a.V + K * 64) * sizeof(float);
  auto kb = attn_general_kernel<true>;
  auto kg = attn_general_kernel<false>;
  if (msocr_internal_lds_limit((const void*)kb, 112 * 1024) != MSOCR_OK || msocr_internal_lds_limit((const void*)kg, 112 * 1024) != MSOCR_OK)
    return MSOCR_E_LAUNCH;
  if (ldsz > 112 * 1024) return MSOCR_E_ARG;
  if (beam)
    MSOCR_LAUNCH(kb, dim3(a.B), dim3(NTH), ldsz, s, a, H);
  else
    MSOCR_LAUNCH(kg, dim3(a.B), dim3(NTH), ldsz, s, a, H);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}
#endif  // MSOCR_ATTN_FORCED
