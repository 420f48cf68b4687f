// text_search.hip — msocr_text_search: every place where one of Q patterns of up to 64 int32 tokens ends in one of T texts with at
// most k_q errors (include/msocr.h, "approximate text search").  The recurrence, the segment window, the
// backward start walk, the host twin and the selection are csrc/text_search.h.
//
// Four kernels:
//   zero    clears the mask tables [Q][2][v] and the hit counter.
//   masks   one thread per pattern token: a 64-bit atomic OR of its bit into word [q][0][c] at bit i and into word [q][1][c] at
//           bit m - 1 - i (the reversed pattern).
//   scan    every text is cut into segments of MSOCR_SEARCH_SEGMENT tokens; a lane owns one (pattern, segment) and its whole state
//           is four registers (pv, mv, score, position).  A workgroup of 256 lanes shares one pattern, whose forward mask row (v words,
//           at most 16 KB) it holds in LDS: eq = row[c] is an LDS gather.  The lane finds its text by a binary search of the
//           uploaded prefix of segment counts, starts W = m + k tokens before its segment (clamped at the text's own start) with
//           the fresh column, and reports the ends inside its segment.  Tokens are read four at a time (one 16-byte load per lane
//           where the four lie inside the token array, else element by element), the next four while the current four are
//           computed.  Every lane of a workgroup makes the same number of trips, so the hit append can ballot: one 64-bit atomic
//           add per wave and hit column, the slot of a lane = the wave's base + the hits in the lanes below it.
//   start   one lane per written record: the backward walk of ts_start with the reversed mask row read from global memory.
#include <new>
#include <vector>

#include "internal.h"
#include "text_search.h"
#include "text_search_kernels.h"

namespace {

constexpr int TS_T = 256;   // lanes of a workgroup of every kernel here
constexpr int TS_MAX_GRID = 65535;

__global__ __launch_bounds__(TS_T) void ts_zero_kernel(uint64_t* __restrict__ tab, long words, unsigned long long* __restrict__ count) {
  const long stride = (long)gridDim.x * TS_T;
  const long i0 = (long)blockIdx.x * TS_T + threadIdx.x;
  if (i0 == 0) *count = 0ull;
  for (long i = i0; i < words; i += stride) tab[i] = 0ull;
}

// grid (patterns, 1), 64 threads: thread i owns token i of pattern blockIdx.x
__global__ __launch_bounds__(64) void ts_masks_kernel(const int32_t* __restrict__ pat_tok, const int32_t* __restrict__ pat_off, int v,
                                                      uint64_t* __restrict__ tab) {
  const int q = blockIdx.x;
  const int a0 = pat_off[q], m = pat_off[q + 1] - a0;
  const int i = threadIdx.x;
  if (i >= m) return;
  const int32_t c = pat_tok[(size_t)a0 + i];
  if (c < 0 || c >= v) return;
  uint64_t* rows = tab + (size_t)q * 2 * v;
  atomicOr((unsigned long long*)(rows + c), 1ull << i);
  atomicOr((unsigned long long*)(rows + v + c), 1ull << (m - 1 - i));
}

// every lane of the wave calls this; those with `hit` append one record each (the start is the start kernel's)
__device__ __forceinline__ void ts_append(bool hit, int32_t q, int32_t t, int32_t end, int32_t dist, msocr_search_hit* __restrict__ hits,
                                          int64_t capacity, unsigned long long* __restrict__ count) {
  msocr_search_hit* h = ts_append_slot(hit, hits, capacity, count);
  if (h) {
    h->pattern = q;
    h->text = t;
    h->end = end;
    h->distance = dist;
  }
}

__global__ __launch_bounds__(TS_T) void ts_scan_kernel(const int32_t* __restrict__ txt_tok, const uint64_t* __restrict__ tab,
                                                       const int64_t* __restrict__ seg_pre, const int32_t* __restrict__ txt_off,
                                                       const int32_t* __restrict__ pat_off, const int32_t* __restrict__ max_dist, int Q,
                                                       int T, int v, int64_t segments, msocr_search_hit* __restrict__ hits,
                                                       int64_t capacity, unsigned long long* __restrict__ count) {
  __shared__ uint64_t row[MSOCR_SEARCH_MAX_ALPHABET];
  const int64_t glo = txt_off[0], ghi = txt_off[T];
  const int align = (int)(((uintptr_t)txt_tok >> 2) & 3);  // elements from a 16-byte boundary to txt_tok[0]
  const int64_t seg_blocks = (segments + TS_T - 1) / TS_T;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    const int m = pat_off[q + 1] - pat_off[q], k = max_dist[q];
    const int W = m + k;
    __syncthreads();  // the row of the pattern before this one has been read by every lane
    for (int c = threadIdx.x; c < v; c += TS_T) row[c] = tab[(size_t)q * 2 * v + c];
    __syncthreads();
    const int trips = (W + MSOCR_SEARCH_SEGMENT + 3 + 3) / 4;  // any alignment of the first token is covered
    for (int64_t sb = blockIdx.x; sb < seg_blocks; sb += gridDim.x) {
      const int64_t sidx = sb * TS_T + threadIdx.x;
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
      uint64_t pv = edl_begin_pv(m, 0), mv = 0ull;
      int score = m;
      int4 nxt = ts_load4(txt_tok, g, glo, ghi, valid);
      for (int trip = 0; trip < trips; ++trip, g += 4) {
        const int4 cur = nxt;
        nxt = ts_load4(txt_tok, g + 4, glo, ghi, valid && trip + 1 < trips);
        const int32_t tok[4] = {cur.x, cur.y, cur.z, cur.w};
        int sc[4];
        unsigned found = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t p = g + e - txt0;  // the token's place in its text
          if (valid && p >= first && p < hi) {
            score += ts_scan_step(pv, mv, ts_eq(row, v, tok[e]), m);
            if (p >= lo && score <= k) found |= 1u << e;
          }
          sc[e] = score;
        }
        if (__ballot(found != 0u) != 0ull) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ts_append((found >> e) & 1u, q, t, (int32_t)(g + e - txt0) + 1, sc[e], hits, capacity, count);
        }
      }
    }
  }
}

__global__ __launch_bounds__(TS_T) void ts_start_kernel(const int32_t* __restrict__ txt_tok, const uint64_t* __restrict__ tab,
                                                        const int32_t* __restrict__ txt_off, const int32_t* __restrict__ pat_off, int v,
                                                        msocr_search_hit* __restrict__ hits, int64_t capacity,
                                                        const unsigned long long* __restrict__ count) {
  const unsigned long long found = *count;
  const int64_t n = found < (unsigned long long)capacity ? (int64_t)found : capacity;
  const int64_t stride = (int64_t)gridDim.x * TS_T;
  for (int64_t i = (int64_t)blockIdx.x * TS_T + threadIdx.x; i < n; i += stride) {
    msocr_search_hit* h = hits + i;
    const int q = h->pattern;
    const int m = pat_off[q + 1] - pat_off[q];
    h->start = ts_start(tab + ((size_t)q * 2 + 1) * v, v, m, txt_tok + txt_off[h->text], h->end, h->distance);
  }
}

}  // namespace

extern "C" int64_t msocr_text_search_ws_bytes(const int32_t* pat_off_host, const int32_t* max_dist_host, int Q, const int32_t* txt_off_host,
                                              int T, int v) {
  const int64_t bytes = ts_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, nullptr);
  return bytes < 0 ? MSOCR_E_ARG : bytes;
}

extern "C" int msocr_text_search(const int32_t* pat_tok, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                                 const int32_t* txt_tok, const int32_t* txt_off_host, int T, int v, msocr_search_hit* hits_out,
                                 int64_t capacity, int64_t* count_out, void* workspace, int64_t workspace_bytes, void* stream) {
  ts_layout lay;
  const int64_t need = ts_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, &lay);
  if (need < 0 || capacity < 0 || !pat_tok || !txt_tok || !hits_out || !count_out) return MSOCR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* count = (unsigned long long*)count_out;
  if (need == 0) {  // no pattern or no text: the count alone
    MSOCR_LAUNCH(ts_zero_kernel, dim3(1), dim3(TS_T), 0, s, (uint64_t*)nullptr, 0l, count);
    return LAUNCH_OK();
  }
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return MSOCR_E_ARG;
  std::vector<int64_t> heads;
  try {
    heads.resize((size_t)((lay.total - lay.seg_pre) / 8));
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  ts_fill_heads(pat_off_host, max_dist_host, Q, txt_off_host, T, lay, (unsigned char*)heads.data());
  unsigned char* ws = (unsigned char*)workspace;
  uint64_t* tab = (uint64_t*)ws;
  // the heads leave a host buffer of this call: wait for the copy before it goes (the kernels behind it do not block the host)
  if (hipMemcpyAsync(ws + lay.seg_pre, heads.data(), (size_t)(lay.total - lay.seg_pre), hipMemcpyHostToDevice, s) != hipSuccess)
    return MSOCR_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return MSOCR_E_LAUNCH;
  const int64_t* seg_pre = (const int64_t*)(ws + lay.seg_pre);
  const int32_t* txt_off = (const int32_t*)(ws + lay.txt_off);
  const int32_t* pat_off = (const int32_t*)(ws + lay.pat_off);
  const int32_t* max_dist = (const int32_t*)(ws + lay.max_dist);
  int rc;
  const long words = (long)(lay.seg_pre / 8);
  const long zero_blocks = (words + TS_T - 1) / TS_T;
  MSOCR_LAUNCH(ts_zero_kernel, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(TS_T), 0, s, tab, words, count);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  MSOCR_LAUNCH(ts_masks_kernel, dim3((unsigned)Q), dim3(64), 0, s, pat_tok, pat_off, v, tab);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  if (lay.segments == 0) return MSOCR_OK;  // every text is empty
  const int64_t seg_blocks = (lay.segments + TS_T - 1) / TS_T;
  const dim3 grid((unsigned)(seg_blocks < TS_MAX_GRID ? seg_blocks : TS_MAX_GRID), (unsigned)(Q < TS_MAX_GRID ? Q : TS_MAX_GRID));
  MSOCR_LAUNCH(ts_scan_kernel, grid, dim3(TS_T), 0, s, txt_tok, tab, seg_pre, txt_off, pat_off, max_dist, Q, T, v, lay.segments, hits_out,
               capacity, count);
  if ((rc = LAUNCH_OK()) != MSOCR_OK) return rc;
  if (capacity == 0) return MSOCR_OK;
  const int64_t start_blocks = (capacity + TS_T - 1) / TS_T;
  MSOCR_LAUNCH(ts_start_kernel, dim3((unsigned)(start_blocks < 4096 ? start_blocks : 4096)), dim3(TS_T), 0, s, txt_tok, tab, txt_off,
               pat_off, v, hits_out, capacity, (const unsigned long long*)count);
  return LAUNCH_OK();
}

extern "C" int msocr_text_search_host(const int32_t* pat_tok_host, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                                      const int32_t* txt_tok_host, const int32_t* txt_off_host, int T, int v, msocr_search_hit* hits_out,
                                      int64_t capacity, int64_t* count_out) {
  const int64_t need = ts_check(pat_off_host, max_dist_host, Q, txt_off_host, T, v, nullptr);
  if (need < 0 || capacity < 0 || !pat_tok_host || !txt_tok_host || !hits_out || !count_out) return MSOCR_E_ARG;
  *count_out = 0;
  if (need == 0) return MSOCR_OK;
  std::vector<uint64_t> rows;
  try {
    rows.resize((size_t)2 * v);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
  *count_out = ts_search_host(pat_tok_host, pat_off_host, max_dist_host, Q, txt_tok_host, txt_off_host, T, v, hits_out, capacity, rows.data());
  return MSOCR_OK;
}

extern "C" int64_t msocr_text_search_select_host(msocr_search_hit* hits, int64_t n) {
  if (n < 0 || (n > 0 && !hits)) return MSOCR_E_ARG;
  if (n == 0) return 0;
  try {
    return ts_select(hits, n);
  } catch (const std::bad_alloc&) {
    return MSOCR_E_ARG;
  }
}
