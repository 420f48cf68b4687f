// east_tiles.hip — tiled detection of large pages (EAST(tile_size=...)): the two data movements around the
// network's run on a batch of overlapping tiles.
//
//   east_tile_gather_kernel   pages [N][H][W][3] u8 -> tiles [N][ny*nx][tile_h][tile_w][3] u8, clamped to the page's edge
//   east_stitch_maps_kernel   tile maps (score, geometry at 1/4 resolution) -> page maps, every page-map pixel from the tile that
//                             owns it, zeros outside the page
//
// east_decode_kernel emits every vertex as cell position x scale + offset x scale: the geometry map holds offsets relative to the
// map pixel itself, so moving a pixel's 8 values from a tile map to the page map needs no coordinate arithmetic.  Both kernels
// move 16-byte vectors, one per thread, no arithmetic on the values, no LDS, no loop.  The grids (origins, owner tables) come from
// detectors/_east/tiles.py, on the device for the kernels and on the host for the argument checks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "internal.h"
#include "msocr.h"

namespace {
constexpr int TILES_T = 256;  // threads per workgroup of both kernels

// One thread = 16 consecutive bytes of one tile row (tile_w * 3 is a multiple of 96).  A page row starts at any byte, so a vector
// that lies inside the page row is read as the 5 aligned dwords around it and shifted into place (left to itself the compiler
// reads such a vector byte by byte); one that reaches past the page's right edge, or whose dwords would reach before the start or
// past the end of `pages`, is put together byte by byte with the column clamped.  Rows below the page repeat its last row.
__device__ __forceinline__ uint32_t shift_bytes(uint32_t lo, uint32_t hi, uint32_t sh) {  // bytes sh .. sh + 3 of {hi, lo}
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
}

__global__ __launch_bounds__(TILES_T) void east_tile_gather_kernel(const uint8_t* __restrict__ pages, size_t page_bytes, int H, int W,
                                                                   const int32_t* __restrict__ oy, const int32_t* __restrict__ ox,
                                                                   int ny, int nx, int tile_h, int tile_w, uint32_t nvec,
                                                                   uint8_t* __restrict__ tiles) {
  const uint32_t v = blockIdx.x * (uint32_t)TILES_T + threadIdx.x;
  if (v >= nvec) return;
  const uint32_t vpr = (uint32_t)tile_w * 3u / 16u;  // vectors per tile row
  const uint32_t row = v / vpr, c = v - row * vpr;   // row = (n * ny * nx + t) * tile_h + y
  const uint32_t nt = row / (uint32_t)tile_h, y = row - nt * (uint32_t)tile_h;
  const uint32_t T = (uint32_t)(ny * nx);
  const uint32_t n = nt / T, t = nt - n * T;
  const uint32_t ty = t / (uint32_t)nx, tx = t - ty * (uint32_t)nx;
  const int sy = min(oy[ty] + (int)y, H - 1);
  const size_t row_off = ((size_t)n * H + sy) * (size_t)W * 3;  // the page row in `pages` (all N pages: page_bytes bytes)
  const int b0 = ox[tx] * 3 + (int)c * 16;                      // first byte of the vector in the unclamped page row
  // `pages` itself may start at any byte (a slice of a batch of odd-sized pages): the dwords are aligned by the absolute address
  const uintptr_t base = (uintptr_t)pages, addr = base + row_off + b0, a4 = addr & ~(uintptr_t)3;
  uint4 out;
  if (b0 + 16 <= W * 3 && a4 >= base && a4 + 20 <= base + page_bytes) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(pages + (a4 - base));  // from `pages`: the loads stay global ones
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4], sh = (uint32_t)(addr & 3);
    out = make_uint4(shift_bytes(d0, d1, sh), shift_bytes(d1, d2, sh), shift_bytes(d2, d3, sh), shift_bytes(d3, d4, sh));
  } else {
    const uint8_t* src = pages + row_off;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int b = b0 + k, px = b / 3;
      w[k >> 2] |= (uint32_t)src[min(px, W - 1) * 3 + (b - px * 3)] << (8 * (k & 3));
    }
    out = make_uint4(w[0], w[1], w[2], w[3]);
  }
  *reinterpret_cast<uint4*>(tiles + (size_t)v * 16) = out;
}

// One thread = one 16-byte vector of the page maps.  A page-map row of Wm pixels has Wm / 4 score vectors (4 pixels each; the
// owner tables change only at multiples of 4 map pixels, so the 4 share an owner and the source is 16-byte aligned) followed
// by 2 * Wm geometry vectors (half a pixel each).  Map pixel (y, x) stands for page pixel (4 y, 4 x): outside the page it is zero.
__global__ __launch_bounds__(TILES_T) void east_stitch_maps_kernel(const float* __restrict__ tile_score, const float* __restrict__ tile_geo,
                                                                   int H, int W, int Hm, int Wm, int nx, int T, int tmh, int tmw,
                                                                   const int32_t* __restrict__ oy, const int32_t* __restrict__ ox,
                                                                   const int32_t* __restrict__ row_tile,
                                                                   const int32_t* __restrict__ col_tile, uint32_t nvec,
                                                                   float* __restrict__ score, float* __restrict__ geo) {
  const uint32_t v = blockIdx.x * (uint32_t)TILES_T + threadIdx.x;
  if (v >= nvec) return;
  const uint32_t nsv = (uint32_t)Wm / 4u, vpr = nsv * 9u;  // score vectors, all vectors per page-map row
  const uint32_t row = v / vpr, i = v - row * vpr;         // row = n * Hm + y
  const uint32_t n = row / (uint32_t)Hm, y = row - n * (uint32_t)Hm;
  const bool is_score = i < nsv;
  const uint32_t x = is_score ? i * 4u : (i - nsv) >> 1;  // first map pixel of the vector
  const uint32_t half = is_score ? 0u : ((i - nsv) & 1u);
  const int ty = row_tile[y], tx = col_tile[x];
  const int ly = (int)y - (oy[ty] >> 2), lx = (int)x - (ox[tx] >> 2);
  const size_t spix = (((size_t)n * T + (size_t)(ty * nx + tx)) * tmh + ly) * (size_t)tmw + lx;  // pixel in the tile maps
  const size_t dpix = (size_t)row * Wm + x;                                                       // pixel in the page maps
  const float* src = is_score ? tile_score + spix : tile_geo + spix * 8 + half * 4;
  float* dst = is_score ? score + dpix : geo + dpix * 8 + half * 4;
  const int xi = 4 * (int)x;  // page column of the vector's first pixel
  float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (4 * (int)y < H && xi < W) val = *reinterpret_cast<const float4*>(src);
  if (is_score) {  // pixels x + 1 .. x + 3 of a score vector may lie past the page's right edge
    if (xi + 4 >= W) val.y = 0.0f;
    if (xi + 8 >= W) val.z = 0.0f;
    if (xi + 12 >= W) val.w = 0.0f;
  }
  *reinterpret_cast<float4*>(dst) = val;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One axis of a grid: n origins, multiples of 32, ascending from 0, every tile inside [0, max(round_up(len, 32), tile)], the last
// one ending there: the tiles cover the axis and none reaches further than the clamped padding allows.  That is what keeps every
// read in bounds; an overlap above tile / 2, which tiles.py refuses, passes here.
bool axis_ok(const int32_t* o, int n, int len, int tile) {
  if (!o || n <= 0 || len <= 0 || tile <= 0 || tile % 32) return false;
  const long L32 = ((long)len + 31) / 32 * 32, end = L32 > tile ? L32 : tile;
  if (o[0] != 0 || (long)o[n - 1] + tile != end) return false;
  for (int i = 0; i < n; ++i) {
    if (o[i] < 0 || o[i] % 32 || (long)o[i] + tile > end) return false;
    if (i > 0 && (o[i] <= o[i - 1] || o[i] > o[i - 1] + tile)) return false;  // ascending, no gap
  }
  return true;
}

// The owner table of one axis: m entries in [0, n), constant over every 4 map pixels, each map pixel inside its owner's tile map.
bool table_ok(const int32_t* tab, int m, const int32_t* o, int n, int tile) {
  if (!tab || m <= 0 || m % 4) return false;
  for (int p = 0; p < m; ++p) {
    const int t = tab[p];
    if (t < 0 || t >= n || t != tab[p & ~3]) return false;
    const int l = p - o[t] / 4;
    if (l < 0 || l >= tile / 4) return false;
  }
  return true;
}
}  // namespace

extern "C" int msocr_east_tile_gather(const uint8_t* pages, int N, int H, int W, const int32_t* oy_dev, const int32_t* ox_dev,
                                      const int32_t* oy_host, const int32_t* ox_host, int ny, int nx, int tile_h, int tile_w,
                                      uint8_t* tiles, void* stream) {
  if (!pages || !oy_dev || !ox_dev || !oy_host || !ox_host || !tiles || N <= 0) return MSOCR_E_ARG;
  if (!axis_ok(oy_host, ny, H, tile_h) || !axis_ok(ox_host, nx, W, tile_w) || !aligned16(tiles)) return MSOCR_E_ARG;
  const long nvec = (long)N * ny * nx * tile_h * ((long)tile_w * 3 / 16);
  if (nvec >= (1L << 31) || (long)W * 3 >= (1L << 30)) return MSOCR_E_ARG;  // 32-bit vector index and row offset
  MSOCR_LAUNCH(east_tile_gather_kernel, dim3((unsigned)((nvec + TILES_T - 1) / TILES_T)), dim3(TILES_T), 0, (hipStream_t)stream, pages,
               (size_t)N * H * W * 3, H, W, oy_dev, ox_dev, ny, nx, tile_h, tile_w, (uint32_t)nvec, tiles);
  return LAUNCH_OK();
}

extern "C" int msocr_east_stitch_maps(const float* tile_score, const float* tile_geo, int N, int H, int W, int ny, int nx, int tile_h,
                                      int tile_w, const int32_t* oy_dev, const int32_t* ox_dev, const int32_t* row_tile_dev,
                                      const int32_t* col_tile_dev, const int32_t* oy_host, const int32_t* ox_host,
                                      const int32_t* row_tile_host, const int32_t* col_tile_host, float* score_out, float* geo_out,
                                      void* stream) {
  if (!tile_score || !tile_geo || !oy_dev || !ox_dev || !row_tile_dev || !col_tile_dev || !score_out || !geo_out || N <= 0)
    return MSOCR_E_ARG;
  if (!axis_ok(oy_host, ny, H, tile_h) || !axis_ok(ox_host, nx, W, tile_w)) return MSOCR_E_ARG;
  const long Hm = ((long)H + 31) / 32 * 8, Wm = ((long)W + 31) / 32 * 8;
  if (Hm >= (1L << 29) || Wm >= (1L << 29)) return MSOCR_E_ARG;
  if (!table_ok(row_tile_host, (int)Hm, oy_host, ny, tile_h) || !table_ok(col_tile_host, (int)Wm, ox_host, nx, tile_w)) return MSOCR_E_ARG;
  if (!aligned16(tile_score) || !aligned16(tile_geo) || !aligned16(score_out) || !aligned16(geo_out)) return MSOCR_E_ARG;
  const long nvec = (long)N * Hm * (Wm / 4 * 9);
  if (nvec >= (1L << 31) || (long)ny * nx >= (1L << 20)) return MSOCR_E_ARG;
  MSOCR_LAUNCH(east_stitch_maps_kernel, dim3((unsigned)((nvec + TILES_T - 1) / TILES_T)), dim3(TILES_T), 0, (hipStream_t)stream,
               tile_score, tile_geo, H, W, (int)Hm, (int)Wm, nx, ny * nx, tile_h / 4, tile_w / 4, oy_dev, ox_dev, row_tile_dev,
               col_tile_dev, (uint32_t)nvec, score_out, geo_out);
  return LAUNCH_OK();
}
