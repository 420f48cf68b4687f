// edit_distance_long.hip — msocr_edit_distance_long: the exact Levenshtein distance of N pairs of int32 token sequences of up to
// MSOCR_EDL_MAX_LEN tokens each (include/msocr.h, "page-level error rates").  The recurrence and the host
// twin are csrc/edit_distance_long.h; the kernels' bodies are csrc/edit_distance_long_kernels.h, which msocr_edit_alignment
// (edit_alignment.hip) instantiates once more with its trace stores.
//
// Three kernels:
//   zero      clears the mask tables of all pairs (one range of the workspace).
//   masks     one thread per pattern token: a 64-bit atomic OR of its bit into word [token][block] of its pair's table.
//   distance  one wave (a workgroup of its own) per pair.  Lane l owns the K = ceil(nb / 64) consecutive pattern blocks from l * K
//             (K <= 4); at step s it advances them by text symbol s - l and hands the carry of its last block to lane l + 1, which
//             consumes it at step s + 1: a systolic sweep of n + lanes - 1 steps, the anti-diagonals of the block table.  The carry
//             moves by __shfl_up (one ds_bpermute per step; nothing goes through memory and no barrier is needed: one wave).  The
//             text is staged in LDS (64 KB at the cap), so that the symbol of a later step costs an LDS read: the mask words of step
//             s + EDL_AHEAD are loaded while step s computes, which hides most of the latency of a load a wave would otherwise wait
//             out every step.  A batch of a few long pairs occupies a few waves of the chip and is latency-bound: accepted
//             (an evaluation call; splitting a pair over several waves is not provided).
#include <new>
#include <stdexcept>
#include <vector>

#include "edit_distance_long_kernels.h"

namespace {

__global__ __launch_bounds__(64) void edl_distance_kernel(const edl_pair* __restrict__ heads, const int32_t* __restrict__ b_tok,
                                                          const uint64_t* __restrict__ tabs, int32_t* __restrict__ dist) {
  extern __shared__ int32_t edl_text[];  // [n] of this pair
  const edl_pair p = heads[blockIdx.x];
  edl_sweep_pair<false>(p, b_tok, tabs, edl_text, dist + blockIdx.x, nullptr);
}

}  // namespace

extern "C" int64_t msocr_edit_distance_long_ws_bytes(const int32_t* a_off_host, const int32_t* b_off_host, const int32_t* v_host, int N) {
  const int64_t bytes = edl_check_heads(a_off_host, b_off_host, v_host, N);
  return bytes < 0 ? MSOCR_E_ARG : bytes;
}

extern "C" int msocr_edit_distance_long(const int32_t* a_tok, const int32_t* a_off_host, const int32_t* b_tok, const int32_t* b_off_host,
                                        const int32_t* v_host, int N, int32_t* dist_out, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const int64_t need = edl_check_heads(a_off_host, b_off_host, v_host, N);
  if (need < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok || !b_tok || !dist_out || !workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return MSOCR_E_ARG;
  std::vector<edl_pair> heads;
  try {
    heads.resize((size_t)N);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  edl_fill_heads(a_off_host, b_off_host, v_host, N, heads.data());
  int max_m = 0, max_n = 0;
  for (const edl_pair& h : heads) {
    max_m = h.m > max_m ? h.m : max_m;
    max_n = h.n > max_n ? h.n : max_n;
  }
  const long words = (long)((need - (int64_t)N * (int64_t)sizeof(edl_pair)) / 8);
  hipStream_t s = (hipStream_t)stream;
  edl_pair* heads_dev = (edl_pair*)workspace;
  uint64_t* tabs = (uint64_t*)(heads_dev + N);
  // the heads leave a host buffer of this call: wait for the copy before it goes (the kernels behind it do not block the host)
  if (hipMemcpyAsync(heads_dev, heads.data(), (size_t)N * sizeof(edl_pair), hipMemcpyHostToDevice, s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return MSOCR_E_LAUNCH;
  int rc;
  if ((rc = edl_launch_masks(heads_dev, a_tok, tabs, words, N, max_m, s)) != MSOCR_OK) return rc;
  const int lds = max_n * (int)sizeof(int32_t);  // <= 64 KB
  if ((rc = msocr_internal_lds_limit((const void*)edl_distance_kernel, MSOCR_EDL_MAX_LEN * (int)sizeof(int32_t))) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(edl_distance_kernel, dim3(N), dim3(64), lds, s, heads_dev, b_tok, tabs, dist_out);
  return LAUNCH_OK();
}

extern "C" int msocr_edit_distance_long_host(const int32_t* a_tok_host, const int32_t* a_off_host, const int32_t* b_tok_host,
                                             const int32_t* b_off_host, const int32_t* v_host, int N, int32_t* dist_out) {
  if (edl_check_heads(a_off_host, b_off_host, v_host, N) < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok_host || !b_tok_host || !dist_out) return MSOCR_E_ARG;
  std::vector<uint64_t> tab, pv(MSOCR_EDL_MAX_BLOCKS), mv(MSOCR_EDL_MAX_BLOCKS);
  for (int p = 0; p < N; ++p) {
    const int m = a_off_host[p + 1] - a_off_host[p], n = b_off_host[p + 1] - b_off_host[p];
    const int32_t *a = a_tok_host + a_off_host[p], *b = b_tok_host + b_off_host[p];
    if (m == 0 || n == 0) {
      dist_out[p] = m == 0 ? n : m;
      continue;
    }
    try {
      tab.resize((size_t)edl_table_words(m, v_host[p]) + 1);
    } catch (const std::bad_alloc&) {  // an alphabet far beyond the pattern's tokens: no memory for its table
      return MSOCR_E_ARG;
    } catch (const std::length_error&) {
      return MSOCR_E_ARG;
    }
    edl_build_table_host(a, m, v_host[p], tab.data());
    dist_out[p] = edl_distance_host(tab.data(), m, v_host[p], b, n, pv.data(), mv.data());
  }
  return MSOCR_OK;
}
