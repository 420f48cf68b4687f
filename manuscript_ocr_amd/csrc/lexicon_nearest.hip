// lexicon_nearest.hip — approximate dictionary lookup on the device: for every recognised row the k words of
// a lexicon with the smallest Levenshtein distance, and the distance between pairs of rows (the recogniser's CER numerator).
//   msocr_lexicon_nearest(_host)      ids [B][steps] x msocr_wordlist -> index / dist [B][k], ascending (distance, index)
//   msocr_edit_distance_pairs(_host)  a_ids [B][steps_a] x b_ids [B][steps_b] -> dist, len_a, len_b [B]
//   msocr_wordlist_check_host         validates host copies of a word list
// The arithmetic is edit_distance.h's, shared with the host twins.
//
// nearest_kernel: one workgroup per (row, slice of the lexicon).  The row's text and its V match masks are built once per workgroup in
// LDS; then every lane walks its own entries of the list: position = slice_lo + it * 256 + thread, whose word index is the position
// itself, or by_length[position] for a list stored in ascending (length, index) order.  In such a list the 64 lanes of a wave hold
// words of one length, or of neighbouring ones, in adjacent memory: the wave's DP loop runs as long as its words are, not as long as
// the longest of 64 random ones, and where the length test below fails it fails for the whole wave.  Each
// wave keeps the k smallest keys (distance << 32 | index) it has seen in the registers of its lanes 0..k-1 (lane r = rank r), with
// the k-th as a wave-uniform threshold: a lane whose key is below it is a candidate, candidates are inserted one by one (a shuffle
// shifts the tail).  Keys are distinct and totally ordered, so the k smallest of a set do not depend on how the set was cut or in
// which order it was met.  A word whose length differs from the row's by more than min(max_distance, the threshold's distance) is
// skipped without its DP: its distance is at least that difference, so it could neither pass the bound nor displace the k-th best.
// The four waves' lists are merged through LDS by wave 0.  With one slice per row the result is written directly; otherwise the
// slice's k keys go to the workspace and nearest_merge_kernel (one wave per row) reduces them the same way.
//
// The same lookup under confusion-weighted costs (the arithmetic is edit_distance_weighted.h's):
//   msocr_lexicon_nearest_weighted(_host)  ... x msocr_edit_costs -> index / dist [B][k], distances in cost units
//   msocr_edit_costs_check_host            validates host copies of the cost tables
// nearest_weighted_kernel keeps the geometry, the per-wave top-k and the merge of nearest_kernel.  Myers' recurrence cannot price a
// symbol pair, so a lane runs the textbook column DP for its word, the column (up to 65 int32) in its registers.  In place of the match
// masks the workgroup builds a query profile in dynamic LDS from the [V][V] table: for every token the costs of reading each of the
// row's symbols as it, 64 contiguous bytes that a lane fetches 8 at a time for its word's current token.  The row sits against the end
// of those 64 positions, so the distance is always the column's last entry and the unrolled loops only skip the groups of 8 in front
// of the row.  The length test compares (n - m) * min_ins or (m - n) * min_del, not the difference in symbols, with the bound;
// the entry point lowers both minima to `unknown` first, which is what a symbol outside [0, V) costs to supply or to drop.
#include "edit_distance_weighted.h"
#include "internal.h"

namespace {
constexpr int NB_THREADS = 256;       // lanes of a nearest workgroup
constexpr int NB_WAVES = NB_THREADS / 64;
constexpr int NB_TARGET_WGS = 1024;   // workgroups a launch aims at when B alone gives fewer: 4 per CU of a 256-CU part
constexpr int NB_MAX_K = 16;

// slices the lexicon is cut into for B rows: enough for NB_TARGET_WGS workgroups, never less than one lane-pass of words per slice.
// A function of (B, n_words) alone, so that the workspace size does not depend on the device.
int nearest_slices(int B, int n_words) {
  const int by_rows = (NB_TARGET_WGS + B - 1) / B;
  const int by_words = (n_words + NB_THREADS - 1) / NB_THREADS;
  const int s = by_rows < by_words ? by_rows : by_words;
  return s < 1 ? 1 : s;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v) {
  const int lo = __shfl_up((int)(uint32_t)v, 1), hi = __shfl_up((int)(uint32_t)(v >> 32), 1);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// the wave's ascending list (lane r < k holds rank r in `mine`) takes the wave-uniform key, which is below the threshold thr
__device__ __forceinline__ void wave_insert(uint64_t& mine, uint64_t& thr, int k, int lane, uint64_t key) {
  const uint64_t prev = shfl_up64(mine);
  if (lane < k && mine > key) mine = (lane == 0 || prev < key) ? key : prev;
  thr = shfl64(mine, k - 1);
}

// every lane's key that is below the threshold goes into the wave's list; all 64 lanes call this together
__device__ __forceinline__ void wave_offer(uint64_t& mine, uint64_t& thr, int k, int lane, uint64_t key) {
  unsigned long long cand = __ballot(key < thr);
  while (cand) {
    const int l = __ffsll((long long)cand) - 1;
    cand &= cand - 1;
    const uint64_t kk = shfl64(key, l);
    if (kk < thr) wave_insert(mine, thr, k, lane, kk);
  }
}

__device__ __forceinline__ void store_rank(uint64_t key, int32_t* index_out, int32_t* dist_out) {
  const bool none = key == MSOCR_ED_NO_KEY;
  *index_out = none ? -1 : (int32_t)(uint32_t)key;
  *dist_out = none ? -1 : (int32_t)(key >> 32);
}

__global__ __launch_bounds__(NB_THREADS) void nearest_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ trun, int B,
                                                              int steps, int V, int eos_id, int pad_id, int blank_id,
                                                              const int32_t* __restrict__ word_begin,
                                                              const int32_t* __restrict__ word_tok,
                                                              const int32_t* __restrict__ by_length, int n_words, int n_tok, int k,
                                                              int max_distance, int slices, int per_slice, uint64_t* partial,
                                                              int32_t* index_out, int32_t* dist_out) {
  __shared__ uint64_t peq[MSOCR_ED_MAX_V];
  __shared__ int32_t raw[MSOCR_ED_MAX_PATTERN], sym[MSOCR_ED_MAX_PATTERN];
  __shared__ uint64_t merge[NB_WAVES][NB_MAX_K];
  __shared__ int m_sh;
  const int b = blockIdx.x / slices, sl = blockIdx.x - b * slices;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b >= B) return;
  if (tid < MSOCR_ED_MAX_PATTERN) raw[tid] = tid < steps ? ids[(size_t)b * steps + tid] : eos_id;
  __syncthreads();
  if (tid == 0) m_sh = ed_row_text(raw, steps, trun[b], eos_id, pad_id, blank_id, sym);  // once per workgroup: at most 64 symbols
  for (int v = tid; v < V; v += NB_THREADS) peq[v] = 0;
  __syncthreads();
  const int m = m_sh;
  if (tid == 0)
    for (int j = 0; j < m; ++j)
      if (sym[j] >= 0 && sym[j] < V) peq[sym[j]] |= 1ull << j;
  __syncthreads();

  uint64_t mine = MSOCR_ED_NO_KEY, thr = MSOCR_ED_NO_KEY;
  const int lo = sl * per_slice;
  const int hi = lo + per_slice < n_words ? lo + per_slice : n_words;
  for (int base = lo; base < hi; base += NB_THREADS) {  // a workgroup-uniform trip count: the shuffles need whole waves
    const int pos = base + tid;
    uint64_t key = MSOCR_ED_NO_KEY;
    const int w = pos >= hi ? -1 : (by_length ? by_length[pos] : pos);
    if (w >= 0 && w < n_words) {  // an entry of by_length outside the list is no word
      int t0, n;
      ed_word_range(word_begin, n_words, n_tok, pos, t0, n);
      const uint32_t thr_d = (uint32_t)(thr >> 32);
      int bound = thr_d > 64u ? 64 : (int)thr_d;
      if (max_distance >= 0 && max_distance < bound) bound = max_distance;
      const int diff = n > m ? n - m : m - n;
      if (diff <= bound) {
        const int d = ed_distance_masks(peq, V, m, word_tok + t0, n);
        if (max_distance < 0 || d <= max_distance) key = ed_key(d, w);
      }
    }
    wave_offer(mine, thr, k, lane, key);
  }
  if (lane < NB_MAX_K) merge[wave][lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < NB_WAVES; ++w)
    for (int r = 0; r < k; ++r) {
      const uint64_t kk = merge[w][r];
      if (kk < thr) wave_insert(mine, thr, k, lane, kk);
    }
  if (lane < k) {
    if (slices == 1) store_rank(mine, index_out + (size_t)b * k + lane, dist_out + (size_t)b * k + lane);
    else partial[((size_t)b * slices + sl) * k + lane] = mine;
  }
}

__global__ __launch_bounds__(64) void nearest_merge_kernel(const uint64_t* __restrict__ partial, int B, int slices, int k,
                                                            int32_t* index_out, int32_t* dist_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const int total = slices * k;
  const uint64_t* p = partial + (size_t)b * total;
  uint64_t mine = MSOCR_ED_NO_KEY, thr = MSOCR_ED_NO_KEY;
  for (int base = 0; base < total; base += 64) {
    const int i = base + lane;
    wave_offer(mine, thr, k, lane, i < total ? p[i] : MSOCR_ED_NO_KEY);
  }
  if (lane < k) store_rank(mine, index_out + (size_t)b * k + lane, dist_out + (size_t)b * k + lane);
}

// LDS bytes of a weighted workgroup's profile and insert costs: V + 1 rows (the last for tokens outside [0, V)), 16-byte multiple
size_t weighted_lds_bytes(int V) { return ((size_t)(V + 1) * (MSOCR_EDW_PROFILE_STRIDE + 1) + 15) & ~(size_t)15; }

__global__ __launch_bounds__(NB_THREADS) void nearest_weighted_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ trun, int B, int steps, int V, int eos_id, int pad_id, int blank_id,
    const int32_t* __restrict__ word_begin, const int32_t* __restrict__ word_tok, const int32_t* __restrict__ by_length, int n_words,
    int n_tok, const uint8_t* __restrict__ sub, const uint8_t* __restrict__ del, const uint8_t* __restrict__ ins, int unknown, int min_ins,
    int min_del, int k, int max_distance, int slices, int per_slice, uint64_t* partial, int32_t* index_out, int32_t* dist_out) {
  extern __shared__ __align__(16) uint8_t weighted_lds[];  // prof [(V + 1)][STRIDE], then insl [V + 1]
  __shared__ int32_t raw[MSOCR_ED_MAX_PATTERN], sym[MSOCR_ED_MAX_PATTERN];
  __shared__ uint32_t dpk_sh[MSOCR_ED_MAX_PATTERN / 4];
  __shared__ uint64_t merge[NB_WAVES][NB_MAX_K];
  __shared__ int m_sh;
  constexpr int STRIDE = MSOCR_EDW_PROFILE_STRIDE;
  uint8_t* prof = weighted_lds;
  uint8_t* insl = weighted_lds + (size_t)(V + 1) * STRIDE;
  const int b = blockIdx.x / slices, sl = blockIdx.x - b * slices;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b >= B) return;
  if (tid < MSOCR_ED_MAX_PATTERN) raw[tid] = tid < steps ? ids[(size_t)b * steps + tid] : eos_id;
  __syncthreads();
  if (tid == 0) m_sh = ed_row_text(raw, steps, trun[b], eos_id, pad_id, blank_id, sym);
  __syncthreads();
  const int m = __builtin_amdgcn_readfirstlane(m_sh);  // 0..64, the same in every lane: the DP's unrolled loops branch on it
  // the workgroup's share of edw_build_profile: delete costs four to a word, insert costs, and the profile with the token as the
  // fast index, so that a wave reads 64 adjacent bytes of one row of sub
  if (tid < MSOCR_ED_MAX_PATTERN / 4) dpk_sh[tid] = edw_profile_deletes(del, V, unknown, sym, m, tid);
  for (int c = tid; c <= V; c += NB_THREADS) insl[c] = (uint8_t)edw_one(ins, V, unknown, c);
  const int p0 = edw_first_group(m) * 8;  // the row sits against the end of the 64 positions; those in front of p0 are never read
  for (int idx = tid; idx < (V + 1) * (MSOCR_ED_MAX_PATTERN - p0); idx += NB_THREADS) {
    const int q = idx / (V + 1), c = idx - q * (V + 1);
    prof[(size_t)c * STRIDE + p0 + q] = edw_profile_entry(sub, V, unknown, sym, m, p0 + q, c);
  }
  __syncthreads();
  uint32_t dpk[MSOCR_ED_MAX_PATTERN / 4];
#pragma unroll
  for (int q = 0; q < MSOCR_ED_MAX_PATTERN / 4; ++q) dpk[q] = dpk_sh[q];

  uint64_t mine = MSOCR_ED_NO_KEY, thr = MSOCR_ED_NO_KEY;
  const int lo = sl * per_slice;
  const int hi = lo + per_slice < n_words ? lo + per_slice : n_words;
  for (int base = lo; base < hi; base += NB_THREADS) {  // a workgroup-uniform trip count: the shuffles need whole waves
    const int pos = base + tid;
    uint64_t key = MSOCR_ED_NO_KEY;
    const int w = pos >= hi ? -1 : (by_length ? by_length[pos] : pos);
    if (w >= 0 && w < n_words) {  // an entry of by_length outside the list is no word
      int t0, n;
      ed_word_range(word_begin, n_words, n_tok, pos, t0, n);
      uint32_t bound = (uint32_t)(thr >> 32);  // the k-th best distance so far, or 2^32 - 1
      if (max_distance >= 0 && (uint32_t)max_distance < bound) bound = (uint32_t)max_distance;
      if ((uint32_t)edw_length_bound(m, n, min_ins, min_del) <= bound) {
        const int d = edw_distance_profile(prof, STRIDE, insl, dpk, V, m, word_tok + t0, n);
        if (max_distance < 0 || d <= max_distance) key = ed_key(d, w);
      }
    }
    wave_offer(mine, thr, k, lane, key);
  }
  if (lane < NB_MAX_K) merge[wave][lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < NB_WAVES; ++w)
    for (int r = 0; r < k; ++r) {
      const uint64_t kk = merge[w][r];
      if (kk < thr) wave_insert(mine, thr, k, lane, kk);
    }
  if (lane < k) {
    if (slices == 1) store_rank(mine, index_out + (size_t)b * k + lane, dist_out + (size_t)b * k + lane);
    else partial[((size_t)b * slices + sl) * k + lane] = mine;
  }
}

// one wave per pair: lane j holds symbol j of a, a ballot gives the match mask of every symbol of b
constexpr int PAIRS_PER_WG = 4;
__global__ __launch_bounds__(64 * PAIRS_PER_WG) void pairs_kernel(const int32_t* __restrict__ a_ids, const int32_t* __restrict__ a_trun,
                                                                   int steps_a, const int32_t* __restrict__ b_ids,
                                                                   const int32_t* __restrict__ b_trun, int steps_b, int B, int V,
                                                                   int eos_id, int pad_id, int blank_id, int32_t* dist_out,
                                                                   int32_t* len_a_out, int32_t* len_b_out) {
  __shared__ int32_t raw[PAIRS_PER_WG][2][MSOCR_ED_MAX_PATTERN];
  __shared__ int32_t txt[PAIRS_PER_WG][2][MSOCR_ED_MAX_PATTERN];
  __shared__ int len[PAIRS_PER_WG][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * PAIRS_PER_WG + wv;
  const bool live = row < B;
  if (live) {
    raw[wv][0][lane] = lane < steps_a ? a_ids[(size_t)row * steps_a + lane] : eos_id;
    raw[wv][1][lane] = lane < steps_b ? b_ids[(size_t)row * steps_b + lane] : eos_id;
  }
  __syncthreads();
  if (live && lane < 2)
    len[wv][lane] = ed_row_text(raw[wv][lane], lane ? steps_b : steps_a, lane ? b_trun[row] : a_trun[row], eos_id, pad_id, blank_id,
                                txt[wv][lane]);
  __syncthreads();
  if (!live) return;
  const int m = len[wv][0], n = len[wv][1];
  int d = n;
  if (m > 0) {
    const int32_t aj = lane < m ? txt[wv][0][lane] : -1;
    ed_state s = ed_begin(m);
    for (int t = 0; t < n; ++t) {
      const int32_t c = txt[wv][1][t];
      ed_step(s, (uint64_t)__ballot(lane < m && c >= 0 && c < V && aj == c));
    }
    d = s.score;
  }
  if (lane == 0) {
    dist_out[row] = d;
    len_a_out[row] = m;
    len_b_out[row] = n;
  }
}

bool nearest_args_ok(const void* ids, const void* trun, int B, int steps, int V, int eos_id, int pad_id, int blank_id,
                     const msocr_wordlist* wl, int k, int max_distance, const void* index_out, const void* dist_out) {
  if (!ids || !trun || !wl || !wl->word_begin || !wl->word_tok || !index_out || !dist_out) return false;
  if (B < 0 || steps < 1 || steps > MSOCR_ED_MAX_PATTERN || V < 1 || V > MSOCR_ED_MAX_V || k < 1 || k > NB_MAX_K) return false;
  if (wl->n_words < 1 || wl->n_tok < 0 || max_distance < -1) return false;
  if (eos_id < 0 || eos_id >= V || pad_id < 0 || pad_id >= V || blank_id < -1 || blank_id >= V) return false;
  return true;
}

bool costs_args_ok(const msocr_edit_costs* c, int V) {
  if (!c || !c->sub || !c->del || !c->ins || c->V != V) return false;
  if (c->unknown < 1 || c->unknown > MSOCR_EDW_MAX_COST) return false;
  return c->min_ins >= 1 && c->min_ins <= MSOCR_EDW_MAX_COST && c->min_del >= 1 && c->min_del <= MSOCR_EDW_MAX_COST;
}

bool pairs_args_ok(const void* a_ids, const void* a_trun, int steps_a, const void* b_ids, const void* b_trun, int steps_b, int B, int V,
                   int eos_id, int pad_id, int blank_id, const void* dist_out, const void* len_a_out, const void* len_b_out) {
  if (!a_ids || !a_trun || !b_ids || !b_trun || !dist_out || !len_a_out || !len_b_out) return false;
  if (B < 0 || steps_a < 1 || steps_a > MSOCR_ED_MAX_PATTERN || steps_b < 1 || steps_b > MSOCR_ED_MAX_PATTERN) return false;
  if (V < 1 || V > MSOCR_ED_MAX_V) return false;
  if (eos_id < 0 || eos_id >= V || pad_id < 0 || pad_id >= V || blank_id < -1 || blank_id >= V) return false;
  return true;
}
}  // namespace

extern "C" int64_t msocr_lexicon_nearest_ws_bytes(int B, int n_words, int k) {
  if (B < 0 || n_words < 1 || k < 1 || k > NB_MAX_K) return MSOCR_E_ARG;
  if (B == 0) return 0;
  const int slices = nearest_slices(B, n_words);
  return slices == 1 ? 0 : (int64_t)B * slices * k * (int64_t)sizeof(uint64_t);
}

extern "C" int msocr_lexicon_nearest(const int32_t* ids, const int32_t* trun_dev, int B, int steps, int V, int eos_id, int pad_id,
                                     int blank_id, const msocr_wordlist* wl, int k, int max_distance, int32_t* index_out,
                                     int32_t* dist_out, void* workspace, void* stream) {
  if (!nearest_args_ok(ids, trun_dev, B, steps, V, eos_id, pad_id, blank_id, wl, k, max_distance, index_out, dist_out)) return MSOCR_E_ARG;
  if (B == 0) return MSOCR_OK;
  const int slices = nearest_slices(B, wl->n_words);
  if (slices > 1 && !workspace) return MSOCR_E_ARG;
  if ((int64_t)B * slices > 0x7fffffffLL) return MSOCR_E_ARG;
  int per_slice = (wl->n_words + slices - 1) / slices;
  per_slice = (per_slice + NB_THREADS - 1) / NB_THREADS * NB_THREADS;  // whole lane-passes; slices * per_slice >= n_words
  MSOCR_LAUNCH(nearest_kernel, dim3(B * slices), dim3(NB_THREADS), 0, (hipStream_t)stream, ids, trun_dev, B, steps, V, eos_id, pad_id,
               blank_id, wl->word_begin, wl->word_tok, wl->by_length, wl->n_words, wl->n_tok, k, max_distance, slices, per_slice, (uint64_t*)workspace,
               index_out, dist_out);
  int rc = LAUNCH_OK();
  if (rc != MSOCR_OK || slices == 1) return rc;
  MSOCR_LAUNCH(nearest_merge_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const uint64_t*)workspace, B, slices, k, index_out,
               dist_out);
  return LAUNCH_OK();
}

extern "C" int msocr_lexicon_nearest_host(const int32_t* ids, const int32_t* trun, int B, int steps, int V, int eos_id, int pad_id,
                                          int blank_id, const msocr_wordlist* wl, int k, int max_distance, int32_t* index_out,
                                          int32_t* dist_out) {
  if (!nearest_args_ok(ids, trun, B, steps, V, eos_id, pad_id, blank_id, wl, k, max_distance, index_out, dist_out)) return MSOCR_E_ARG;
  uint64_t peq[MSOCR_ED_MAX_V];
  for (int b = 0; b < B; ++b) {
    int32_t sym[MSOCR_ED_MAX_PATTERN];
    const int m = ed_row_text(ids + (size_t)b * steps, steps, trun[b], eos_id, pad_id, blank_id, sym);
    ed_build_masks(sym, m, V, peq);
    uint64_t best[NB_MAX_K];
    for (int r = 0; r < k; ++r) best[r] = MSOCR_ED_NO_KEY;
    for (int pos = 0; pos < wl->n_words; ++pos) {
      const int w = wl->by_length ? wl->by_length[pos] : pos;
      if (w < 0 || w >= wl->n_words) continue;
      int t0, n;
      ed_word_range(wl->word_begin, wl->n_words, wl->n_tok, pos, t0, n);
      const int d = ed_distance_masks(peq, V, m, wl->word_tok + t0, n);
      if (max_distance < 0 || d <= max_distance) ed_topk_insert(best, k, ed_key(d, w));
    }
    for (int r = 0; r < k; ++r) {
      const bool none = best[r] == MSOCR_ED_NO_KEY;
      index_out[(size_t)b * k + r] = none ? -1 : (int32_t)(uint32_t)best[r];
      dist_out[(size_t)b * k + r] = none ? -1 : (int32_t)(best[r] >> 32);
    }
  }
  return MSOCR_OK;
}

extern "C" int64_t msocr_lexicon_nearest_weighted_ws_bytes(int B, int n_words, int k) { return msocr_lexicon_nearest_ws_bytes(B, n_words, k); }

extern "C" int msocr_lexicon_nearest_weighted(const int32_t* ids, const int32_t* trun_dev, int B, int steps, int V, int eos_id, int pad_id,
                                              int blank_id, const msocr_wordlist* wl, const msocr_edit_costs* costs, int k,
                                              int max_distance, int32_t* index_out, int32_t* dist_out, void* workspace, void* stream) {
  if (!nearest_args_ok(ids, trun_dev, B, steps, V, eos_id, pad_id, blank_id, wl, k, max_distance, index_out, dist_out)) return MSOCR_E_ARG;
  if (!costs_args_ok(costs, V)) return MSOCR_E_ARG;
  if (B == 0) return MSOCR_OK;
  const int slices = nearest_slices(B, wl->n_words);
  if (slices > 1 && !workspace) return MSOCR_E_ARG;
  if ((int64_t)B * slices > 0x7fffffffLL) return MSOCR_E_ARG;
  int per_slice = (wl->n_words + slices - 1) / slices;
  per_slice = (per_slice + NB_THREADS - 1) / NB_THREADS * NB_THREADS;  // whole lane-passes; slices * per_slice >= n_words
  // the length test needs what ANY symbol costs at the least to supply or to drop: a symbol outside [0, V) costs `unknown`, which may
  // lie below every entry of ins and del (rows carry such symbols: Lexicon.encode_rows gives -1 for a character outside the charset)
  const int low_ins = costs->unknown < costs->min_ins ? costs->unknown : costs->min_ins;
  const int low_del = costs->unknown < costs->min_del ? costs->unknown : costs->min_del;
  MSOCR_LAUNCH(nearest_weighted_kernel, dim3(B * slices), dim3(NB_THREADS), weighted_lds_bytes(V), (hipStream_t)stream, ids, trun_dev, B,
               steps, V, eos_id, pad_id, blank_id, wl->word_begin, wl->word_tok, wl->by_length, wl->n_words, wl->n_tok, costs->sub, costs->del,
               costs->ins, costs->unknown, low_ins, low_del, k, max_distance, slices, per_slice, (uint64_t*)workspace, index_out,
               dist_out);
  int rc = LAUNCH_OK();
  if (rc != MSOCR_OK || slices == 1) return rc;
  MSOCR_LAUNCH(nearest_merge_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const uint64_t*)workspace, B, slices, k, index_out,
               dist_out);
  return LAUNCH_OK();
}

extern "C" int msocr_lexicon_nearest_weighted_host(const int32_t* ids, const int32_t* trun, int B, int steps, int V, int eos_id, int pad_id,
                                                   int blank_id, const msocr_wordlist* wl, const msocr_edit_costs* costs, int k,
                                                   int max_distance, int32_t* index_out, int32_t* dist_out) {
  if (!nearest_args_ok(ids, trun, B, steps, V, eos_id, pad_id, blank_id, wl, k, max_distance, index_out, dist_out)) return MSOCR_E_ARG;
  if (!costs_args_ok(costs, V)) return MSOCR_E_ARG;
  for (int b = 0; b < B; ++b) {
    int32_t sym[MSOCR_ED_MAX_PATTERN];
    const int m = ed_row_text(ids + (size_t)b * steps, steps, trun[b], eos_id, pad_id, blank_id, sym);
    uint64_t best[NB_MAX_K];
    for (int r = 0; r < k; ++r) best[r] = MSOCR_ED_NO_KEY;
    for (int pos = 0; pos < wl->n_words; ++pos) {
      const int w = wl->by_length ? wl->by_length[pos] : pos;
      if (w < 0 || w >= wl->n_words) continue;
      int t0, n;
      ed_word_range(wl->word_begin, wl->n_words, wl->n_tok, pos, t0, n);
      const int d = edw_distance(costs->sub, costs->del, costs->ins, V, costs->unknown, sym, m, wl->word_tok + t0, n);  // no length test
      if (max_distance < 0 || d <= max_distance) ed_topk_insert(best, k, ed_key(d, w));
    }
    for (int r = 0; r < k; ++r) {
      const bool none = best[r] == MSOCR_ED_NO_KEY;
      index_out[(size_t)b * k + r] = none ? -1 : (int32_t)(uint32_t)best[r];
      dist_out[(size_t)b * k + r] = none ? -1 : (int32_t)(best[r] >> 32);
    }
  }
  return MSOCR_OK;
}

extern "C" int msocr_edit_costs_check_host(const uint8_t* sub_host, const uint8_t* del_host, const uint8_t* ins_host, int V, int unknown,
                                           int min_ins, int min_del) {
  if (!sub_host || !del_host || !ins_host || V < 1 || V > MSOCR_ED_MAX_V) return MSOCR_E_ARG;
  if (unknown < 1 || unknown > MSOCR_EDW_MAX_COST) return MSOCR_E_ARG;
  int lo_ins = MSOCR_EDW_MAX_COST + 1, lo_del = MSOCR_EDW_MAX_COST + 1;
  for (int a = 0; a < V; ++a) {
    if (!ins_host[a] || !del_host[a]) return MSOCR_E_ARG;
    if (ins_host[a] < lo_ins) lo_ins = ins_host[a];
    if (del_host[a] < lo_del) lo_del = del_host[a];
    for (int b = 0; b < V; ++b)
      if ((sub_host[(size_t)a * V + b] == 0) != (a == b)) return MSOCR_E_ARG;
  }
  return (min_ins == lo_ins && min_del == lo_del) ? MSOCR_OK : MSOCR_E_ARG;
}

extern "C" int msocr_edit_distance_pairs(const int32_t* a_ids, const int32_t* a_trun, int steps_a, const int32_t* b_ids,
                                         const int32_t* b_trun, int steps_b, int B, int V, int eos_id, int pad_id, int blank_id,
                                         int32_t* dist_out, int32_t* len_a_out, int32_t* len_b_out, void* stream) {
  if (!pairs_args_ok(a_ids, a_trun, steps_a, b_ids, b_trun, steps_b, B, V, eos_id, pad_id, blank_id, dist_out, len_a_out, len_b_out))
    return MSOCR_E_ARG;
  if (B == 0) return MSOCR_OK;
  MSOCR_LAUNCH(pairs_kernel, dim3((B + PAIRS_PER_WG - 1) / PAIRS_PER_WG), dim3(64 * PAIRS_PER_WG), 0, (hipStream_t)stream, a_ids, a_trun,
               steps_a, b_ids, b_trun, steps_b, B, V, eos_id, pad_id, blank_id, dist_out, len_a_out, len_b_out);
  return LAUNCH_OK();
}

extern "C" int msocr_edit_distance_pairs_host(const int32_t* a_ids, const int32_t* a_trun, int steps_a, const int32_t* b_ids,
                                              const int32_t* b_trun, int steps_b, int B, int V, int eos_id, int pad_id, int blank_id,
                                              int32_t* dist_out, int32_t* len_a_out, int32_t* len_b_out) {
  if (!pairs_args_ok(a_ids, a_trun, steps_a, b_ids, b_trun, steps_b, B, V, eos_id, pad_id, blank_id, dist_out, len_a_out, len_b_out))
    return MSOCR_E_ARG;
  for (int r = 0; r < B; ++r) {
    int32_t a[MSOCR_ED_MAX_PATTERN], b[MSOCR_ED_MAX_PATTERN];
    const int m = ed_row_text(a_ids + (size_t)r * steps_a, steps_a, a_trun[r], eos_id, pad_id, blank_id, a);
    const int n = ed_row_text(b_ids + (size_t)r * steps_b, steps_b, b_trun[r], eos_id, pad_id, blank_id, b);
    dist_out[r] = ed_distance_scan(a, m, b, n, V);
    len_a_out[r] = m;
    len_b_out[r] = n;
  }
  return MSOCR_OK;
}

extern "C" int msocr_wordlist_check_host(const int32_t* word_begin_host, const int32_t* word_tok_host, int n_words, int n_tok, int V,
                                         int max_word_len) {
  if (!word_begin_host || !word_tok_host || n_words < 1 || n_tok < 1 || V < 1 || V > MSOCR_ED_MAX_V) return MSOCR_E_ARG;
  if (max_word_len < 1 || max_word_len > MSOCR_ED_MAX_WORD) return MSOCR_E_ARG;
  if (word_begin_host[0] != 0 || word_begin_host[n_words] != n_tok) return MSOCR_E_ARG;
  for (int i = 0; i < n_words; ++i) {
    const int64_t n = (int64_t)word_begin_host[i + 1] - word_begin_host[i];
    if (n < 1 || n > max_word_len) return MSOCR_E_ARG;
  }
  for (int t = 0; t < n_tok; ++t)
    if (word_tok_host[t] < 0 || word_tok_host[t] >= V) return MSOCR_E_ARG;
  return MSOCR_OK;
}
