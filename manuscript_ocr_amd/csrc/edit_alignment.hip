// edit_alignment.hip — msocr_edit_alignment: one optimal alignment of N pairs of int32 token sequences of up to MSOCR_EDL_MAX_LEN
// tokens each, by the rule of csrc/edit_alignment.h (include/msocr.h, "alignment behind the error rates").
// The rule, the trace layout and the host twin are that header; the mask kernels and the sweep are csrc/edit_distance_long_kernels.h.
//
// Four kernels:
//   zero, masks  the match-mask tables, as for msocr_edit_distance_long.
//   sweep        the distance kernel's systolic sweep (one wave per pair), which here also stores every block's {d0, pv} of every
//                column, one 16-byte store a block and step, at trace [block][column].
//   traceback    a launch of its own behind the sweep: the kernel boundary is what makes the trace visible.  One wave per pair
//                walks from (m, n) to an edge of the table.  The walk is a serial chain of at most m + n steps, so it pays no memory
//                latency per step: at a refill lane l loads, for the pattern block of row i and the column j - 64 + l, the trace
//                cell and the match-mask word of that column's text token (one coalesced 16-byte load, one text token, one gathered
//                table word) and keeps the rule's words of its column (eal_moves).  The wave then walks inside that window of 64 rows
//                x 64 columns, a run of equal steps at a time: each lane tests its own cell of the diagonal through (i, j), a ballot
//                gives the length of the run of hits and substitutions from (i, j); failing that, a ballot along row i the run of
//                insertions; failing that, the word of column j (v_readlane) the run of deletions.  The walk leaves the window when
//                i crosses the block's edge or j the window's.  The state (i, j, counts) is wave-uniform and lives in SGPRs.
//                A row or column that the walk leaves puts its map entry into the register of the lane that owns it
//                in the window; at the next refill the wave stores the rows and the columns it left, coalesced.  Every i and every j
//                is left exactly once, so every map element is written exactly once and no two stores hit one address; the run left
//                over at an edge of the table is written by the whole wave.
#include <new>
#include <stdexcept>
#include <vector>

#include "edit_distance_long_kernels.h"

namespace {

__global__ __launch_bounds__(64) void eal_sweep_kernel(const edl_pair* __restrict__ heads, const int64_t* __restrict__ trace_off,
                                                       const int32_t* __restrict__ b_tok, const uint64_t* __restrict__ tabs,
                                                       eal_cell* __restrict__ traces, int32_t* __restrict__ dist) {
  extern __shared__ int32_t eal_text[];  // [n] of this pair
  const edl_pair p = heads[blockIdx.x];
  edl_sweep_pair<true>(p, b_tok, tabs, eal_text, dist + blockIdx.x, traces + trace_off[blockIdx.x]);
}

// lane `src` 's x, src wave-uniform and in 0 .. 63
__device__ __forceinline__ uint64_t eal_lane64(uint64_t x, int src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// how many consecutive bits of x are set from bit `top` (0 .. 63) downwards: 0 .. top + 1
__device__ __forceinline__ int eal_run(uint64_t x, int top) {
  const uint64_t y = ~(x << (63 - top));  // the zeros shifted in read as "not set"
  return y ? __clzll((long long)y) : 64;
}

// a_base, b_base = a_off[0], b_off[0]: the maps start at the first pair's tokens
__global__ __launch_bounds__(64) void eal_traceback_kernel(const edl_pair* __restrict__ heads, const int64_t* __restrict__ trace_off,
                                                           const int32_t* __restrict__ b_tok, const uint64_t* __restrict__ tabs,
                                                           const eal_cell* __restrict__ traces, int a_base, int b_base,
                                                           int32_t* __restrict__ a_map, int32_t* __restrict__ b_map,
                                                           int32_t* __restrict__ counts) {
  const edl_pair p = heads[blockIdx.x];
  const int lane = threadIdx.x;
  const int n = p.n;
  int32_t* am = a_map + ((int64_t)p.a0 - a_base);  // [m]
  int32_t* bm = b_map + ((int64_t)p.b0 - b_base);  // [n]
  const int32_t* tx = b_tok + (size_t)p.b0;
  const uint64_t* tab = tabs + p.tab;
  const eal_cell* trace = traces + trace_off[blockIdx.x];
  int i = p.m, j = n;
  int hits = 0, subs = 0, dels = 0, inss = 0;
  while (i > 0 && j > 0) {
    // refill: rows 64 blk + 1 .. 64 blk + 64, columns c0 + 1 .. c0 + 64 = j (lane l: text token c0 + l)
    const int blk = (i - 1) >> 6, c0 = j - 64;
    const int t = c0 + lane;
    uint64_t eq = 0, diag = 0, del = 0;
    const bool valid = t >= 0;
    if (valid) {  // 0 <= t < j <= n and blk < nb: inside the text, the trace [nb][n] and (edl_eq) the table
      const eal_cell cell = trace[(int64_t)blk * n + t];
      eq = edl_eq(tab, p.v, p.nb, tx[t], blk);
      eal_moves(eq, cell.d0, cell.pv, diag, del);
    }
    const int i_lo = blk * 64, j_lo = c0 > 0 ? c0 : 0;
    int32_t a_val = 0, b_val = 0;
    bool a_set = false, b_set = false;
    while (i > i_lo && j > j_lo) {
      // a run of equal steps at once.  r, c: the row and the column (= lane) of cell (i, j) in the window
      const int r = (i - 1) & 63, c = j - 1 - c0;
      const int row = r - c + lane;  // this lane's row on the diagonal through (r, c)
      const uint64_t cell = (valid && lane <= c && row >= 0) ? 1ull << row : 0ull;
      int k = eal_run(__ballot((diag & cell) != 0), c);
      if (k > 0) {  // k steps up the diagonal: hits and substitutions
        const bool mine = lane <= c && lane > c - k;
        const int h = __popcll(__ballot(mine && (eq & cell) != 0));
        hits += h;
        subs += k - h;
        if (mine) {
          b_val = i - 1 - (c - lane);
          b_set = true;
        }
        if (lane <= r && lane > r - k) {
          a_val = j - 1 - (r - lane);
          a_set = true;
        }
        i -= k;
        j -= k;
      } else if ((k = eal_run(__ballot(valid && lane <= c && !(((diag | del) >> r) & 1)), c)) > 0) {  // k insertions along row r
        if (lane <= c && lane > c - k) {
          b_val = -1;
          b_set = true;
        }
        inss += k;
        j -= k;
      } else {  // neither: deletions down column c, at least this cell
        k = eal_run(eal_lane64(del, c), r);
        if (lane <= r && lane > r - k) {
          a_val = -1;
          a_set = true;
        }
        dels += k;
        i -= k;
      }
    }
    if (a_set) am[i_lo + lane] = a_val;  // a_set: row i_lo + lane + 1 <= m was left in this window
    if (b_set) bm[c0 + lane] = b_val;    // b_set: column c0 + lane + 1 in 1 .. n was left in this window
  }
  for (int k = lane; k < i; k += 64) am[k] = -1;
  for (int k = lane; k < j; k += 64) bm[k] = -1;
  if (lane == 0) {
    int32_t* out = counts + (int64_t)blockIdx.x * 4;
    out[EAL_HIT] = hits;
    out[EAL_SUB] = subs;
    out[EAL_DEL] = dels + i;
    out[EAL_INS] = inss + j;
  }
}

}  // namespace

extern "C" int64_t msocr_edit_alignment_ws_bytes(const int32_t* a_off_host, const int32_t* b_off_host, const int32_t* v_host, int N) {
  const int64_t bytes = eal_check_heads(a_off_host, b_off_host, v_host, N);
  return bytes < 0 ? MSOCR_E_ARG : bytes;
}

extern "C" int msocr_edit_alignment(const int32_t* a_tok, const int32_t* a_off_host, const int32_t* b_tok, const int32_t* b_off_host,
                                    const int32_t* v_host, int N, int32_t* dist_out, int32_t* a_map_out, int32_t* b_map_out,
                                    int32_t* counts_out, void* workspace, int64_t workspace_bytes, void* stream) {
  eal_layout lay;
  const int64_t need = eal_check_heads(a_off_host, b_off_host, v_host, N, &lay);
  if (need < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok || !b_tok || !dist_out || !a_map_out || !b_map_out || !counts_out || !workspace || ((uintptr_t)workspace & 15) ||
      workspace_bytes < need)
    return MSOCR_E_ARG;
  // heads and trace offsets as they lie in the workspace: one upload
  std::vector<uint64_t> up;
  try {
    up.resize((size_t)lay.tables / 8);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  edl_pair* heads = (edl_pair*)up.data();
  edl_fill_heads(a_off_host, b_off_host, v_host, N, heads);
  eal_fill_trace_offsets(a_off_host, b_off_host, N, (int64_t*)(up.data() + lay.trace_off / 8));
  int max_m = 0, max_n = 0;
  for (int p = 0; p < N; ++p) {
    max_m = heads[p].m > max_m ? heads[p].m : max_m;
    max_n = heads[p].n > max_n ? heads[p].n : max_n;
  }
  const long words = (long)lay.table_words;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const edl_pair* heads_dev = (const edl_pair*)ws;
  const int64_t* trace_off_dev = (const int64_t*)(ws + lay.trace_off);
  uint64_t* tabs = (uint64_t*)(ws + lay.tables);
  eal_cell* traces = (eal_cell*)(ws + lay.trace);
  // the heads leave a host buffer of this call: wait for the copy before it goes (the kernels behind it do not block the host)
  if (hipMemcpyAsync(ws, up.data(), (size_t)lay.tables, hipMemcpyHostToDevice, s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return MSOCR_E_LAUNCH;
  int rc;
  if ((rc = edl_launch_masks(heads_dev, a_tok, tabs, words, N, max_m, s)) != MSOCR_OK) return rc;
  const int lds = max_n * (int)sizeof(int32_t);  // <= 64 KB
  if ((rc = msocr_internal_lds_limit((const void*)eal_sweep_kernel, MSOCR_EDL_MAX_LEN * (int)sizeof(int32_t))) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(eal_sweep_kernel, dim3(N), dim3(64), lds, s, heads_dev, trace_off_dev, b_tok, tabs, traces, dist_out);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(eal_traceback_kernel, dim3(N), dim3(64), 0, s, heads_dev, trace_off_dev, b_tok, (const uint64_t*)tabs,
               (const eal_cell*)traces, (int)a_off_host[0], (int)b_off_host[0], a_map_out, b_map_out, counts_out);
  return LAUNCH_OK();
}

extern "C" int msocr_edit_alignment_host(const int32_t* a_tok_host, const int32_t* a_off_host, const int32_t* b_tok_host,
                                         const int32_t* b_off_host, const int32_t* v_host, int N, int32_t* dist_out,
                                         int32_t* a_map_out, int32_t* b_map_out, int32_t* counts_out) {
  if (eal_check_heads(a_off_host, b_off_host, v_host, N) < 0) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  if (!a_tok_host || !b_tok_host || !dist_out || !a_map_out || !b_map_out || !counts_out) return MSOCR_E_ARG;
  std::vector<uint64_t> tab, pv(MSOCR_EDL_MAX_BLOCKS), mv(MSOCR_EDL_MAX_BLOCKS);
  std::vector<eal_cell> trace;
  for (int p = 0; p < N; ++p) {
    const int m = a_off_host[p + 1] - a_off_host[p], n = b_off_host[p + 1] - b_off_host[p];
    const int32_t *a = a_tok_host + a_off_host[p], *b = b_tok_host + b_off_host[p];
    int32_t* a_map = a_map_out + (a_off_host[p] - a_off_host[0]);
    int32_t* b_map = b_map_out + (b_off_host[p] - b_off_host[0]);
    dist_out[p] = m == 0 ? n : m;
    if (m > 0 && n > 0) {
      try {
        tab.resize((size_t)edl_table_words(m, v_host[p]) + 1);
        trace.resize((size_t)eal_trace_cells(m, n));
      } catch (const std::bad_alloc&) {  // no memory for the table (an alphabet far beyond the pattern's tokens) or the trace
        return MSOCR_E_ARG;
      } catch (const std::length_error&) {
        return MSOCR_E_ARG;
      }
      edl_build_table_host(a, m, v_host[p], tab.data());
      dist_out[p] = eal_forward_host(tab.data(), m, v_host[p], b, n, pv.data(), mv.data(), trace.data());
    }
    eal_traceback_host(tab.data(), m, v_host[p], b, n, trace.data(), a_map, b_map, counts_out + (int64_t)p * 4);
  }
  return MSOCR_OK;
}
