// text_search_kernels.h — the device pieces the two scan kernels share (text_search.hip, text_search_weighted.hip): the 16-byte
// token load and the ballot append of hit records.
#ifndef MSOCR_TEXT_SEARCH_KERNELS_H
#define MSOCR_TEXT_SEARCH_KERNELS_H
#include "internal.h"
#include "msocr.h"

// the four tokens txt_tok[g .. g + 4): one 16-byte load where they lie inside [glo, ghi) (g is then 16-byte aligned: the caller
// aligned it by the array's own address), else the elements that do, -1 for the others
__device__ __forceinline__ int4 ts_load4(const int32_t* __restrict__ txt_tok, int64_t g, int64_t glo, int64_t ghi, bool want) {
  int4 r = make_int4(-1, -1, -1, -1);
  if (!want) return r;
  if (g >= glo && g + 4 <= ghi) return *reinterpret_cast<const int4*>(txt_tok + g);
  if (g + 0 >= glo && g + 0 < ghi) r.x = txt_tok[g + 0];
  if (g + 1 >= glo && g + 1 < ghi) r.y = txt_tok[g + 1];
  if (g + 2 >= glo && g + 2 < ghi) r.z = txt_tok[g + 2];
  if (g + 3 >= glo && g + 3 < ghi) r.w = txt_tok[g + 3];
  return r;
}

// every lane of the wave calls this; those with `hit` get the record they may write, or nullptr where the capacity is used up: one
// 64-bit atomic add per wave, the slot of a lane = the wave's base + the hits in the lanes below it
__device__ __forceinline__ msocr_search_hit* ts_append_slot(bool hit, msocr_search_hit* __restrict__ hits, int64_t capacity,
                                                            unsigned long long* __restrict__ count) {
  const unsigned long long mask = __ballot(hit);
  if (mask == 0ull) return nullptr;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0ull;
  if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
  base = __shfl(base, leader, 64);
  const unsigned long long slot = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
  return (hit && slot < (unsigned long long)capacity) ? hits + slot : nullptr;
}
#endif
