// internal.h — symbols shared between the translation units of libmsocr.so (not part of the C ABI).
#ifndef MSOCR_INTERNAL_H
#define MSOCR_INTERNAL_H
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "msocr.h"

// Clear any stale (sticky) HIP error left by earlier runtime calls of the host process before a launch, so that the status read
// back after it (LAUNCH_OK) belongs to this launch.
#define MSOCR_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH)

// conv_igemm.hip: nbatch independent f32 GEMMs of one shape in one launch,
// C[b][m][n] = sum_k A[b][m][k] * B[b][n][k]  (A [nbatch][M][K], B [nbatch][N][K], C [nbatch][M][N], dense, 16-B aligned).
__attribute__((visibility("hidden"))) int msocr_internal_gemm_f32_batched(const float* A, const float* B, float* C, long M, int N,
                                                                          int K, int nbatch, hipStream_t s);

// conv_split.hip: the same with B given as three K-tile-major bf16 planes [3][nbatch][K/32][N][32] (B == p0 + p1 + p2 exactly), A split in
// registers: six bf16 MFMA products per f32 product, f32 accumulate (K % 32 == 0, N % 64 == 0).
__attribute__((visibility("hidden"))) int msocr_internal_gemm_split_batched(const float* A, const uint16_t* Bplanes, float* C, long M,
                                                                            int N, int K, int nbatch, hipStream_t s);

// Per-device launch state.  hipFuncSetAttribute applies to the current device's copy of a kernel, and grid sizes follow the current
// device's CU count, so both are cached per device (the first by kernel pointer) behind a mutex: safe to call from several host
// threads.  Inline, so that every translation unit stands alone and the library still holds one cache of each.  Both return
// MSOCR_OK or MSOCR_E_LAUNCH.
// msocr_internal_lds_limit: raise the dynamic-LDS limit of `kernel` to `bytes` on the current device, once per (kernel, device).
__attribute__((visibility("hidden"))) inline int msocr_internal_lds_limit(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> raised;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MSOCR_E_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  if (raised.count({kernel, dev})) return MSOCR_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return MSOCR_E_LAUNCH;
  raised.insert({kernel, dev});
  return MSOCR_OK;
}
// msocr_internal_cu_count: the current device's CU count.
__attribute__((visibility("hidden"))) inline int msocr_internal_cu_count(int* n) {
  static std::mutex mu;
  static std::map<int, int> cu_count;  // device -> CU count
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MSOCR_E_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cu_count.find(dev);
  if (it == cu_count.end()) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return MSOCR_E_LAUNCH;
    it = cu_count.emplace(dev, cu).first;
  }
  *n = it->second;
  return MSOCR_OK;
}

// attention decoder arguments shared by trba_kernels.hip (entry points), attn_beam_mfma.hip (matrix-core kernels) and attn_general.hip
struct AttnArgs {
  const float* batch_H;
  const float* proj_H;
  const float* ctx_gates;  // matrix-core kernels: [B][T][H][4] = batch_H x rnn.weight_ih[:, :H]^T, hoisted out of the step loop
  msocr_attn_weights w;
  const uint16_t *h2h_p, *whh_p, *gen_p;  // matrix-core kernels: msocr_attn_split_weights (greedy: required; beam: nullptr = exact f32)
  int B, T, V, steps, K;
  int sos_id, eos_id, blank_id;
  float temperature;
  const float* lp;      // [steps] f32 length-penalty factors (beam, alpha > 0) or nullptr
  float* logits_out;    // greedy: [B][steps][V]; beam: workspace [B][steps][K][V]
  int32_t* ids_out;     // greedy: [B][steps]
  int32_t* back;        // beam: [B][steps][K]
  int32_t* tokv;        // beam: [B][steps][K]
  int32_t* best_at;     // beam: [B][steps]
  int32_t* fin_step;    // beam: [B]
  const int32_t* chunk_id;    // beam, optional: [B] index of the reference chunk (one predict() slice of batch_size crops) of each crop
  const int32_t* chunk_size;  // [nchunks] crops per chunk
  int32_t* chunk_state;       // [2*nchunks] zeroed by the caller: {crops finished, max finish step}; enables the early exit
  float* alpha_out;     // optional attention weights of every step (nullptr = off): greedy [B][steps][T]; beam [B][steps][K][T], slot-
                        // indexed like the logits trace (the weights of step s at slot rb belong to the hypothesis whose logits are there)
  const int32_t* tok_in;  // forced decode: [B][steps] the token fed to step s of every row (nullptr everywhere else); the forced kernels
                          // replace an id outside [0, V) by sos_id before it indexes wih_tok, and write no ids
  // lexicon-constrained beam decode (attn_general_lexicon.hip, attn_lexicon_mfma.hip; null / zero everywhere else): the lexicon's prefix
  // tree as CSR arrays on the device (msocr_lexicon) and the trie node of every slot after every step, [B][steps][K] i32 (-1 = dead)
  const int32_t *lex_begin, *lex_tok, *lex_child;
  const uint8_t* lex_terminal;
  int lex_nodes, lex_edges;
  int32_t* node_out;
  // beam decode with a character n-gram language model fused in (attn_general_lm.hip, attn_lm_mfma.hip; null / zero everywhere else):
  // the dense table [lm_nctx][V] f32 of natural-log probabilities on the device (msocr_charlm), the "all SOS" row every slot starts at,
  // the weight of the addend, and the table row of every slot after every step, [B][steps][K] i32
  const float* lm_table;
  int lm_nctx, lm_ctx0;
  float lm_weight;
  int32_t* ctx_out;
};
// attn_beam_mfma.hip: beam decode with 4 crops x 8 beams per workgroup on the matrix cores (H == 256, V <= 256, T <= 48, beam <= 8;
// needs ctx_gates): split-operand products with the split weights, exact-f32 MFMA without them
__attribute__((visibility("hidden"))) int msocr_internal_attn_beam_mfma(const AttnArgs& a, hipStream_t s);
// attn_beam_mfma.hip: greedy decode with 32 crops per workgroup on the matrix cores (same shapes; needs ctx_gates and the split weights)
__attribute__((visibility("hidden"))) int msocr_internal_attn_greedy_mfma(const AttnArgs& a, hipStream_t s);
// attn_beam_mfma_alpha.hip: the same two with the attention weights of every step stored to a.alpha_out (required; the two above
// require it to be nullptr)
__attribute__((visibility("hidden"))) int msocr_internal_attn_beam_mfma_alpha(const AttnArgs& a, hipStream_t s);
__attribute__((visibility("hidden"))) int msocr_internal_attn_greedy_mfma_alpha(const AttnArgs& a, hipStream_t s);
// attn_forced_mfma.hip: forced decode (the greedy step loop along a.tok_in instead of its own arg-max) with 32 rows per workgroup on
// the matrix cores; same shapes and weights as the greedy kernel, a.alpha_out and a.tok_in required
__attribute__((visibility("hidden"))) int msocr_internal_attn_forced_mfma(const AttnArgs& a, hipStream_t s);
// attn_general.hip: greedy / beam decode for every shape of the envelope (see its header), H == 256 included; msocr_attn_decode
// runs it for a descriptor without ctx_gates.  Same outputs and workspace layout as the matrix-core kernels; a.alpha_out optional.
__attribute__((visibility("hidden"))) int msocr_internal_attn_general(const AttnArgs& a, int H, bool beam, hipStream_t s);
// attn_general_forced.hip: the forced decode for the same shapes (one row per crop): a.tok_in and a.alpha_out required; logits and
// weights as the greedy loop stores them, no ids
__attribute__((visibility("hidden"))) int msocr_internal_attn_general_forced(const AttnArgs& a, int H, hipStream_t s);
// attn_general_lexicon.hip: the beam decode constrained to a lexicon's prefix tree, for the same shapes: a.lex_* and a.node_out required
__attribute__((visibility("hidden"))) int msocr_internal_attn_general_lexicon(const AttnArgs& a, int H, hipStream_t s);
// attn_lexicon_mfma.hip: the same on the matrix cores (the beam kernel's shapes; needs ctx_gates); a.alpha_out, a.lex_* and a.node_out
// required
__attribute__((visibility("hidden"))) int msocr_internal_attn_lexicon_mfma(const AttnArgs& a, hipStream_t s);
// attn_general_lm.hip: the beam decode with the language model's addend, for the shapes of attn_general.hip: a.lm_table, a.ctx_out and
// a.alpha_out required, lm_ctx0 inside [0, lm_nctx), lm_nctx * V <= 2^26
__attribute__((visibility("hidden"))) int msocr_internal_attn_general_lm(const AttnArgs& a, int H, hipStream_t s);
// attn_lm_mfma.hip: the same on the matrix cores (the beam kernel's shapes; needs ctx_gates)
__attribute__((visibility("hidden"))) int msocr_internal_attn_lm_mfma(const AttnArgs& a, hipStream_t s);
#endif
