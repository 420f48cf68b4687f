// text_search_weighted.hip — msocr_text_search_weighted: every place where one of Q patterns of up to 64 int32 tokens ends in one of T
// texts at a confusion-weighted cost of at most k_q (include/msocr.h, "The same search under confusion-weighted costs"; DESIGN.md
// section 4.27).  The cost functions, the profile entries, the column step, the argument check and the host twin are
// csrc/text_search_weighted.h; the segment window is text_search.h's, the token load and the ballot append text_search_kernels.h's.
//
// Two kernels:
//   zero   clears the hit counter.
//   scan   every text is cut into segments of MSOCR_SEARCH_SEGMENT tokens; a lane owns one (pattern, segment).  A workgroup of 256
//          lanes shares one pattern (grid y, stride loop) and at every pattern switch builds in LDS what a text token costs against
//          it: prof [(v + 1)][72] u8, row c = reading token c as each of the 64 positions (the pattern sits against their END, row v
//          stands for every token outside [0, v)), hdel [v + 1] = dropping c, and the sixteen packed words of the positions' insert
//          costs.  It also sums the inserts: the bound k' = min(k, sum - 1) and the warm-up W = m + k' / dmin come from there.  The
//          lane keeps its column in 64 registers, each cell one key cost << 16 | (65535 - (start - first)), so the start of a hit
//          is read from the bottom cell and no second kernel walks back.  Groups of 8 positions in front of the pattern are
//          skipped.  Window, 16-byte token loads and append: as in ts_scan_kernel.  Integer arithmetic only.
#include <new>
#include <vector>

#include "internal.h"
#include "text_search_kernels.h"
#include "text_search_weighted.h"

namespace {

constexpr int TSW_T = 256;  // lanes of a workgroup
constexpr int TSW_MAX_ROWS = 65535;  // grid y: patterns
constexpr int TSW_MAX_COLS = 4096;   // grid x: blocks of TSW_T segments; a workgroup that takes several keeps its pattern's profile

__global__ void tsw_zero_kernel(unsigned long long* __restrict__ count) { *count = 0ull; }

__global__ __launch_bounds__(TSW_T) void tsw_scan_kernel(const int32_t* __restrict__ pat_tok, const int32_t* __restrict__ txt_tok,
                                                         tsw_costs costs, int dmin, const int64_t* __restrict__ seg_pre,
                                                         const int32_t* __restrict__ txt_off, const int32_t* __restrict__ pat_off,
                                                         const int32_t* __restrict__ max_dist, int Q, int T, int64_t segments,
                                                         msocr_search_hit* __restrict__ hits, int64_t capacity,
                                                         unsigned long long* __restrict__ count) {
  extern __shared__ __align__(16) uint8_t tsw_lds[];  // prof [(v + 1)][72], then hdel [v + 1]
  __shared__ int32_t pa[MSOCR_SEARCH_MAX_PATTERN], pca[MSOCR_SEARCH_MAX_PATTERN];  // the pattern's tokens and their classes
  __shared__ uint32_t pins_sh[MSOCR_SEARCH_MAX_PATTERN / 4];
  __shared__ int bound_sh;
  const int v = costs.v;
  uint8_t* prof = tsw_lds;
  uint8_t* hdel = tsw_lds + tsw_lds_hdel(v);
  const int64_t glo = txt_off[0], ghi = txt_off[T];
  const int align = (int)(((uintptr_t)txt_tok >> 2) & 3);  // elements from a 16-byte boundary to txt_tok[0]
  const int64_t seg_blocks = (segments + TSW_T - 1) / TSW_T;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    const int a0 = pat_off[q], m = pat_off[q + 1] - a0;
    const int g0 = tsw_first_group(m);
    __syncthreads();  // the profile of the pattern before this one has been read by every lane
    if (threadIdx.x < m) {
      const int32_t c = pat_tok[(size_t)a0 + threadIdx.x];
      pa[threadIdx.x] = c;
      pca[threadIdx.x] = tsw_class(costs, c);
    }
    __syncthreads();
    {
      const int p0 = g0 * 8, width = MSOCR_SEARCH_MAX_PATTERN - p0;
      for (int idx = threadIdx.x; idx < (v + 1) * width; idx += TSW_T) {
        const int tok = idx / width, p = p0 + idx % width;
        prof[tok * MSOCR_TSW_STRIDE + p] = tsw_profile_entry(costs, pa, pca, m, p, tok);
      }
      for (int tok = threadIdx.x; tok <= v; tok += TSW_T) hdel[tok] = tsw_profile_delete(costs, tok);
      if (threadIdx.x < MSOCR_SEARCH_MAX_PATTERN / 4) {
        uint32_t w = 0u;
        for (int e = 0; e < 4; ++e) w |= (uint32_t)tsw_profile_insert(costs, pca, m, threadIdx.x * 4 + e) << (8 * e);
        pins_sh[threadIdx.x] = w;
      }
      if (threadIdx.x == TSW_T - 1) {
        int sum = 0;
        for (int i = 0; i < m; ++i) sum += tsw_one(costs, costs.ins, pca[i]);
        bound_sh = tsw_clamp(max_dist[q], sum);
      }
    }
    __syncthreads();
    const int k = bound_sh;
    const int W = tsw_warmup(m, k < 0 ? 0 : k, dmin);  // k < 0: a table with a zero insert; nothing is a hit then
    uint32_t pins[MSOCR_SEARCH_MAX_PATTERN / 4];
#pragma unroll
    for (int i = 0; i < MSOCR_SEARCH_MAX_PATTERN / 4; ++i) pins[i] = pins_sh[i];
    const int trips = (W + MSOCR_SEARCH_SEGMENT + 3 + 3) / 4;  // any alignment of the first token is covered
    for (int64_t sb = blockIdx.x; sb < seg_blocks; sb += gridDim.x) {
      const int64_t sidx = sb * TSW_T + threadIdx.x;
      const bool valid = sidx < segments;
      int t = 0, first = 0, lo = 0, hi = 0;  // a lane without a segment owns no token: hi = 0
      int64_t txt0 = glo;
      if (valid) {
        int a = 0, b = T;  // the last t with seg_pre[t] <= sidx: seg_pre[0] = 0 <= sidx < seg_pre[T]
        while (b - a > 1) {
          const int mid = a + ((b - a) >> 1);
          if (seg_pre[mid] <= sidx) a = mid; else b = mid;
        }
        t = a;
        txt0 = txt_off[t];
        ts_window(txt_off[t + 1] - txt_off[t], sidx - seg_pre[t], W, first, lo, hi);
      }
      // global index of the first token of the first trip: at or below txt0 + lo - W, on a 16-byte boundary of the array's memory
      int64_t g = txt0 + lo - W;
      g -= ((g + align) % 4 + 4) % 4;
      int32_t col[MSOCR_SEARCH_MAX_PATTERN];
      tsw_begin(col, pins, g0);
      int4 nxt = ts_load4(txt_tok, g, glo, ghi, valid);
      for (int trip = 0; trip < trips; ++trip, g += 4) {
        const int4 cur = nxt;
        nxt = ts_load4(txt_tok, g + 4, glo, ghi, valid && trip + 1 < trips);
#pragma unroll 1
        for (int e = 0; e < 4; ++e) {
          const int32_t c = e == 0 ? cur.x : e == 1 ? cur.y : e == 2 ? cur.z : cur.w;
          const int64_t p = g + e - txt0;  // the token's place in its text
          bool hit = false;
          int32_t key = 0;
          if (valid && p >= first && p < hi) {
            const int cc = (c >= 0 && c < v) ? c : v;
            key = tsw_step(col, prof + cc * MSOCR_TSW_STRIDE, hdel[cc], pins, g0, (int)p - first);
            hit = p >= lo && tsw_key_cost(key) <= k;
          }
          msocr_search_hit* h = ts_append_slot(hit, hits, capacity, count);
          if (h) {
            h->pattern = q;
            h->text = t;
            h->start = tsw_key_start(key, first);
            h->end = (int32_t)p + 1;
            h->distance = tsw_key_cost(key);
          }
        }
      }
    }
  }
}

// the struct's tables and the class map as the cost functions read them
tsw_costs tsw_view(const msocr_edit_costs* costs, const int32_t* tok_class, int v) {
  tsw_costs c;
  c.sub = costs->sub;
  c.del = costs->del;
  c.ins = costs->ins;
  c.tok_class = tok_class;
  c.V = costs->V;
  c.unknown = costs->unknown;
  c.v = v;
  return c;
}

}  // namespace

extern "C" int64_t msocr_text_search_weighted_ws_bytes(const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                                                       const int32_t* txt_off_host, int T, int v, const msocr_edit_costs* costs) {
  const int64_t bytes = tsw_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, costs, nullptr);
  return bytes < 0 ? MSOCR_E_ARG : bytes;
}

extern "C" int msocr_text_search_weighted(const int32_t* pat_tok, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                                          const int32_t* txt_tok, const int32_t* txt_off_host, int T, int v, const int32_t* tok_class,
                                          const msocr_edit_costs* costs, msocr_search_hit* hits_out, int64_t capacity,
                                          int64_t* count_out, void* workspace, int64_t workspace_bytes, void* stream) {
  ts_layout lay;
  const int64_t need = tsw_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, costs, &lay);
  if (need < 0 || capacity < 0 || !pat_tok || !txt_tok || !tok_class || !hits_out || !count_out) return MSOCR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* count = (unsigned long long*)count_out;
  if (need > 0 && (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)) return MSOCR_E_ARG;
  int rc;
  MSOCR_LAUNCH(tsw_zero_kernel, dim3(1), dim3(1), 0, s, count);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  if (need == 0 || lay.segments == 0) return MSOCR_OK;  // no pattern, no text, or every text is empty: the count alone
  std::vector<int64_t> heads;
  try {
    heads.resize((size_t)(lay.total / 8));
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  ts_fill_heads(pat_off_host, max_dist_host, Q, txt_off_host, T, lay, (unsigned char*)heads.data());
  unsigned char* ws = (unsigned char*)workspace;
  // the heads leave a host buffer of this call: wait for the copy before it goes (the kernel behind it does not block the host)
  if (hipMemcpyAsync(ws, heads.data(), (size_t)lay.total, hipMemcpyHostToDevice, s) != hipSuccess) return MSOCR_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return MSOCR_E_LAUNCH;
  const int64_t seg_blocks = (lay.segments + TSW_T - 1) / TSW_T;
  const dim3 grid((unsigned)(seg_blocks < TSW_MAX_COLS ? seg_blocks : TSW_MAX_COLS), (unsigned)(Q < TSW_MAX_ROWS ? Q : TSW_MAX_ROWS));
  MSOCR_LAUNCH(tsw_scan_kernel, grid, dim3(TSW_T), (size_t)tsw_lds_tail_at(v), s, pat_tok, txt_tok, tsw_view(costs, tok_class, v),
               tsw_dmin(costs->min_del, costs->unknown), (const int64_t*)(ws + lay.seg_pre), (const int32_t*)(ws + lay.txt_off),
               (const int32_t*)(ws + lay.pat_off), (const int32_t*)(ws + lay.max_dist), Q, T, lay.segments, hits_out, capacity, count);
  return LAUNCH_OK();
}

extern "C" int msocr_text_search_weighted_host(const int32_t* pat_tok_host, const int32_t* pat_off_host, const int32_t* max_dist_host,
                                               int Q, const int32_t* txt_tok_host, const int32_t* txt_off_host, int T, int v,
                                               const int32_t* tok_class_host, const msocr_edit_costs* costs_host,
                                               msocr_search_hit* hits_out, int64_t capacity, int64_t* count_out) {
  const int64_t need = tsw_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, costs_host, nullptr);
  if (need < 0 || capacity < 0 || !pat_tok_host || !txt_tok_host || !tok_class_host || !hits_out || !count_out) return MSOCR_E_ARG;
  *count_out = 0;
  if (need == 0) return MSOCR_OK;
  *count_out = tsw_search_host(pat_tok_host, pat_off_host, max_dist_host, Q, txt_tok_host, txt_off_host, T,
                               tsw_view(costs_host, tok_class_host, v), hits_out, capacity);
  return MSOCR_OK;
}
