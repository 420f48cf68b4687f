// winograd.hip — 3x3 / stride 1 / pad 1 convolution as Winograd in f32 for gfx950 (MI355X), in four tile forms.
//
// Why here: exact-f32 MFMA (v_mfma_f32_32x32x2_f32) peaks at 157 TFLOP/s, 1/16 of the bf16 rate, while HBM3E
// delivers 8 TB/s — so on this chip an f32 3x3 convolution is worth trading fewer matrix FLOPs for two
// streaming transform passes.  out = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A  per output tile:
//   1. wino*_input_kernel : V[xi*PW+nu][tile][c] = (B^T d B)[xi][nu]      (HBM-bound, 16-B coalesced)
//   2. PH*PW GEMMs in ONE launch (conv_igemm / conv_split): Mw[p][tile][co] = sum_c V[p][tile][c] * U[p][co][c]  (MFMA)
//   3. wino*_output_kernel: out[tile][co] = act(A^T Mw A + bias (+ residual))  (HBM-bound)
// U = G g G^T is computed once at weight-load time in f64 (msocr_winograd_weights_host).
//
// The forms (msocr.h MSOCR_WINO_*), output tile MH x MW, PH x PW = (MH + 2) x (MW + 2) transform points:
//   2X2  F(2x2,3x3)       16 points, 4 multiplies per output (direct: 9).  The transforms only add/subtract and scale by 1/2
//                         (exact), so the result differs from the direct f32 convolution by rounding order only (Lavin & Gray 2016).
//   4X2  F(4,3) x F(2,3)  24 points per 4x2 outputs: 3 multiplies per output, V / Mw 3x the layer's arrays instead of 4x.  Only the
//                         H axis takes the 6-point transform: on the textbook points {0, +-1, +-2, inf} its constants grew the layer's f32
//                         rounding error ~2.5x rms over F(2x2), where the 6x6 form would grow it 6x; since round 4
//                         it runs on the points {0, +-3/2, +-2/3, inf} (wino44_bt / wino44_at): half that error.
//   4X4  F(4,3) x F(4,3)  36 points per 4x4 outputs: 2.25 multiplies and workspace words per output.  On the textbook points its error
//                         is 4.7x the tall form's and cannot pass the f64 arbitration of the tolerances (tests/test_gpu_f64.py); on
//                         {0, +-3/2, +-2/3, inf} — reciprocal pairs keep the Vandermonde entries within [8/27, 27/8] — an f32 simulation of
//                         the whole pipeline of transforms measures 1.05x the tall form's error (and 0.5x for the tall form itself on these
//                         points; tools/winograd_points.py, profiles/r04_winograd_points.txt).
//   4X4_COLTAIL           the square form + tail column, for maps with W % 4 == 1 (the recogniser's 4 x 13): W/4 square tiles per
//                         tile row, then output column W - 1 as one F(4,3) x F(1,3) tile — the 6-point transform along H, the three
//                         taps along W summed directly, 18 points — instead of a fourth square tile that holds one real column:
//                         36 * (W/4) + 18 point rows per tile row, not 36 * (W/4 + 1).  The one form of two parts (WinoPlan, below): one
//                         transform launch per direction over the tiles of both (wino44_*_kernel_coltail), one batched GEMM launch each.
// ops.conv2d() picks the tall form for the Cin = 64 layers (fused kernels, below) and where the square form does not pay; the 2x2
// form when 24 * ceil(H/4) >= 16 * ceil(H/2).
//
// Replaces nn.Conv2d(3x3, stride 1, padding 1)+BatchNorm2d(+ReLU)(+add) of
//   recognizers/_trba/model/seresnet31.py:37-45,81-89 ; detectors/_east/east.py:13-30 (conv3x3 of DecoderBlock)
//   and the stride-1 Bottleneck conv2 of torchvision ResNet-50 (detectors/_east/east.py:56-67).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_common.h"
#include "se_tail.h"

// ---- 1-D transforms, four channels per lane: B^T (M + 2 inputs -> M + 2 points) and A^T (M + 2 points -> M outputs) ----------
template <int M> __device__ void wino_bt1(const f32x4 d[M + 2], f32x4 r[M + 2]);
template <int M> __device__ void wino_at1(const f32x4 m[M + 2], f32x4 y[M]);

// F(2,3) on {0, 1, -1, inf}: B^T rows (d0-d2, d1+d2, d2-d1, d1-d3), A^T rows (m0+m1+m2, m1-m2-m3)
template <> __device__ __forceinline__ void wino_bt1<2>(const f32x4 d[4], f32x4 r[4]) {
  r[0] = d[0] - d[2];
  r[1] = d[1] + d[2];
  r[2] = d[2] - d[1];
  r[3] = d[1] - d[3];
}
template <> __device__ __forceinline__ void wino_at1<2>(const f32x4 m[4], f32x4 y[2]) {
  y[0] = (m[0] + m[1]) + m[2];
  y[1] = (m[1] - m[2]) - m[3];
}

// F(4,3) on the interpolation points {0, 3/2, -3/2, 2/3, -2/3, inf} (round 4).  Matrices (Cook-Toom, wincnn scaling: G carries
// 1 / prod(a_j - a_l)):
//   B^T d:  r0 = d0 - 97/36 d2 + d4          r5 = d1 - 97/36 d3 + d5
//           e1 = d4 - 4/9 d2,  o1 = 3/2 d3 - 2/3 d1:   r1 = e1 + o1,  r2 = e1 - o1        (points +-3/2)
//           e2 = d4 - 9/4 d2,  o2 = 2/3 d3 - 3/2 d1:   r3 = e2 + o2,  r4 = e2 - o2        (points +-2/3)
//   A^T m:  y0 = m0 + (m1 + m2) + (m3 + m4)             y1 = 3/2 (m1 - m2) + 2/3 (m3 - m4)
//           y2 = 9/4 (m1 + m2) + 4/9 (m3 + m4)          y3 = 27/8 (m1 - m2) + 8/27 (m3 - m4) + m5
//   G (host, f64): rows [1,0,0], [8,+-12,18]/65, [-81/2,-+27,-18]/65, [0,0,1].
__device__ __forceinline__ void wino44_bt(const f32x4 d[6], f32x4 r[6]) {
  constexpr float k97_36 = 97.0f / 36.0f, k4_9 = 4.0f / 9.0f, k9_4 = 2.25f, k3_2 = 1.5f, k2_3 = 2.0f / 3.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[0][e] = fmaf(-k97_36, d[2][e], d[0][e]) + d[4][e];
    r[5][e] = fmaf(-k97_36, d[3][e], d[1][e]) + d[5][e];
    const float e1 = fmaf(-k4_9, d[2][e], d[4][e]), o1 = fmaf(k3_2, d[3][e], -k2_3 * d[1][e]);
    const float e2 = fmaf(-k9_4, d[2][e], d[4][e]), o2 = fmaf(k2_3, d[3][e], -k3_2 * d[1][e]);
    r[1][e] = e1 + o1; r[2][e] = e1 - o1;
    r[3][e] = e2 + o2; r[4][e] = e2 - o2;
  }
}
__device__ __forceinline__ void wino44_at(const f32x4 m[6], f32x4 y[4]) {
  constexpr float k3_2 = 1.5f, k2_3 = 2.0f / 3.0f, k9_4 = 2.25f, k4_9 = 4.0f / 9.0f, k27_8 = 3.375f, k8_27 = 8.0f / 27.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float p12 = m[1][e] + m[2][e], d12 = m[1][e] - m[2][e], p34 = m[3][e] + m[4][e], d34 = m[3][e] - m[4][e];
    y[0][e] = (m[0][e] + p12) + p34;
    y[1][e] = fmaf(k3_2, d12, k2_3 * d34);
    y[2][e] = fmaf(k9_4, p12, k4_9 * p34);
    y[3][e] = fmaf(k27_8, d12, k8_27 * d34) + m[5][e];
  }
}
template <> __device__ __forceinline__ void wino_bt1<4>(const f32x4 d[6], f32x4 r[6]) { wino44_bt(d, r); }
template <> __device__ __forceinline__ void wino_at1<4>(const f32x4 m[6], f32x4 y[4]) { wino44_at(m, y); }

// F(1,3): the direct 3-tap sum as a "transform" (the W axis of the tail column, below): B^T and G are the 3 x 3 identity, A^T = [1 1 1]
template <> __device__ __forceinline__ void wino_bt1<1>(const f32x4 d[3], f32x4 r[3]) {
  r[0] = d[0]; r[1] = d[1]; r[2] = d[2];
}
template <> __device__ __forceinline__ void wino_at1<1>(const f32x4 m[3], f32x4 y[1]) { y[0] = (m[0] + m[1]) + m[2]; }


struct WinoGeom {
  int N, H, W;      // image extent (output extent is the same: stride 1, pad 1): bounds the input taps and guards the output stores
  int TH, TW;       // output tiles per image in this pass
  int w0;           // first output column of the pass: its tile column tw covers output columns w0 + MW * tw ...
  long Mt;          // N * TH * TW
};

// ---- 1. input transform: one thread = one tile x 4 channels ------------------------------------------------
// The axis order sets the f32 rounding and is part of each form's result: the forms with a 6-point H axis transform W first (B^T
// per row as the row is loaded), then H per column; F(2x2) loads the whole tile and transforms H first, then W.
template <int MH, int MW>
__device__ __forceinline__ void wino_input_body(const float* in, long sN, long sH, long sW, int C, const WinoGeom& g, long plane_mt, float* V,
                                                long t, int c) {
  constexpr int PH = MH + 2, PW = MW + 2;
  constexpr bool w_first = MH == 4;
  if (t >= g.Mt) return;
  const int tw = (int)(t % g.TW);
  const long r = t / g.TW;
  const int th = (int)(r % g.TH);
  const int n = (int)(r / g.TH);
  const int h0 = MH * th - 1, w0 = g.w0 + MW * tw - 1;
  const float* base = in + (long)n * sN + c;
  f32x4 q[PH][PW];
#pragma unroll
  for (int i = 0; i < PH; ++i) {
    const int hi = h0 + i;
    const bool okh = (unsigned)hi < (unsigned)g.H;
    f32x4 d[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int wi = w0 + j;
      const bool ok = okh && (unsigned)wi < (unsigned)g.W;
      // branch-free: padded taps read the (always valid) first vector of the image row block and are masked to zero
      const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? base + (long)hi * sH + (long)wi * sW : base);
      d[j] = ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (w_first) {
      wino_bt1<MW>(d, q[i]);
    } else {
#pragma unroll
      for (int j = 0; j < PW; ++j) q[i][j] = d[j];
    }
  }
  const long plane = plane_mt * (long)C;
  float* o = V + t * (long)C + c;
  if constexpr (w_first) {  // then H per column, stored as it is transformed
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      f32x4 col[PH], v[PH];
#pragma unroll
      for (int i = 0; i < PH; ++i) col[i] = q[i][j];
      wino_bt1<MH>(col, v);
#pragma unroll
      for (int i = 0; i < PH; ++i) *reinterpret_cast<f32x4*>(o + (i * PW + j) * plane) = v[i];
    }
  } else {  // then W per row i, on row i of the H-transformed columns (the compiler keeps one H transform per column; written
            // row by row, each store follows its own arithmetic: 76 VGPRs where transforming all columns first took 82)
#pragma unroll
    for (int i = 0; i < PH; ++i) {
      f32x4 row[PW], v[PW];
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        f32x4 col[PH], hv[PH];
#pragma unroll
        for (int k = 0; k < PH; ++k) col[k] = q[k][j];
        wino_bt1<MH>(col, hv);
        row[j] = hv[i];
      }
      wino_bt1<MW>(row, v);
#pragma unroll
      for (int j = 0; j < PW; ++j) *reinterpret_cast<f32x4*>(o + (i * PW + j) * plane) = v[j];
    }
  }
}

// ---- 3. output transform: one thread = one tile x 4 output channels; H axis first (A^T per column), then W -----------------
template <int MH, int MW>
__device__ __forceinline__ void wino_output_body(const float* Mw, int Cout, const WinoGeom& g, long plane_mt, const float* bias, const float* res,
                                                 long res_ld, int relu, float* out, long out_ld, long t, int c) {
  constexpr int PH = MH + 2, PW = MW + 2;
  if (t >= g.Mt) return;
  const int tw = (int)(t % g.TW);
  const long r = t / g.TW;
  const int th = (int)(r % g.TH);
  const int n = (int)(r / g.TH);
  const long plane = plane_mt * (long)Cout;
  const float* mp = Mw + t * (long)Cout + c;
  // load order only (register allocation, not arithmetic): F(2x2) loads the whole tile first, the 6-point forms column by column
  f32x4 mt[PH][PW];
  if constexpr (MH == 2) {
#pragma unroll
    for (int i = 0; i < PH; ++i)
#pragma unroll
      for (int j = 0; j < PW; ++j) mt[i][j] = *reinterpret_cast<const f32x4*>(mp + (i * PW + j) * plane);
  }
  f32x4 s[MH][PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    f32x4 m[PH], y[MH];
#pragma unroll
    for (int i = 0; i < PH; ++i) m[i] = MH == 2 ? mt[i][j] : *reinterpret_cast<const f32x4*>(mp + (i * PW + j) * plane);
    wino_at1<MH>(m, y);
#pragma unroll
    for (int a = 0; a < MH; ++a) s[a][j] = y[a];
  }
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (bias) b = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
  for (int a = 0; a < MH; ++a) {
    const int ho = MH * th + a;
    if (ho >= g.H) continue;
    f32x4 y[MW];
    wino_at1<MW>(s[a], y);
#pragma unroll
    for (int j = 0; j < MW; ++j) {
      const int wo = g.w0 + MW * tw + j;
      if (wo >= g.W) continue;
      const long pix = ((long)n * g.H + ho) * g.W + wo;
      f32x4 v = y[j] + b;
      if (res) v += *reinterpret_cast<const f32x4*>(res + pix * res_ld + c);
      if (relu) {
        v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
      }
      *reinterpret_cast<f32x4*>(out + pix * out_ld + c) = v;
    }
  }
}

// thread -> (tile, first of its 4 channels): gid = tile * (C / 4) + channel group
__device__ __forceinline__ long wino_thread_tile(int C, int* c) {
  const int cch = C >> 2;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long t = gid / cch;
  *c = (int)(gid - t * cch) << 2;
  return t;
}

// One kernel symbol per form and direction: profilers, bench.py and tools/ sort kernels into the convolution stage by these names.
#define WINO_TRANSFORM_KERNELS(PREFIX, MH, MW)                                                                                    \
  __global__ __launch_bounds__(256) void PREFIX##_input_kernel(const float* __restrict__ in, long sN, long sH, long sW, int C,   \
                                                               WinoGeom g, float* __restrict__ V) {                            \
    int c;                                                                                                                       \
    const long t = wino_thread_tile(C, &c);                                                                                      \
    wino_input_body<MH, MW>(in, sN, sH, sW, C, g, g.Mt, V, t, c);                                                                \
  }                                                                                                                              \
  __global__ __launch_bounds__(256) void PREFIX##_output_kernel(const float* __restrict__ Mw, int Cout, WinoGeom g,              \
                                                                const float* __restrict__ bias, const float* __restrict__ res,  \
                                                                long res_ld, int relu, float* __restrict__ out, long out_ld) {  \
    int c;                                                                                                                       \
    const long t = wino_thread_tile(Cout, &c);                                                                                   \
    wino_output_body<MH, MW>(Mw, Cout, g, g.Mt, bias, res, res_ld, relu, out, out_ld, t, c);                                     \
  }
WINO_TRANSFORM_KERNELS(wino, 2, 2)
WINO_TRANSFORM_KERNELS(wino42, 4, 2)
WINO_TRANSFORM_KERNELS(wino44, 4, 4)
#undef WINO_TRANSFORM_KERNELS

// Square tiles + tail column (W % 4 == 1): ONE launch per direction over the tiles of both passes, the square pass's first.  The tile
// index picks the body; with C / 4 >= 64 threads per tile the branch is uniform over a wave.  The names keep the wino44_ prefix:
// they are the square form's kernels as far as profilers, bench.py and tools/ are concerned.
__global__ __launch_bounds__(256) void wino44_input_kernel_coltail(const float* __restrict__ in, long sN, long sH, long sW, int C,
                                                                   WinoGeom g44, WinoGeom g41, float* __restrict__ V44,
                                                                   float* __restrict__ V41) {
  int c;
  const long t = wino_thread_tile(C, &c);
  if (t < g44.Mt) wino_input_body<4, 4>(in, sN, sH, sW, C, g44, g44.Mt, V44, t, c);
  else wino_input_body<4, 1>(in, sN, sH, sW, C, g41, g41.Mt, V41, t - g44.Mt, c);
}
__global__ __launch_bounds__(256) void wino44_output_kernel_coltail(const float* __restrict__ Mw44, const float* __restrict__ Mw41,
                                                                    int Cout, WinoGeom g44, WinoGeom g41,
                                                                    const float* __restrict__ bias, const float* __restrict__ res,
                                                                    long res_ld, int relu, float* __restrict__ out, long out_ld) {
  int c;
  const long t = wino_thread_tile(Cout, &c);
  if (t < g44.Mt) wino_output_body<4, 4>(Mw44, Cout, g44, g44.Mt, bias, res, res_ld, relu, out, out_ld, t, c);
  else wino_output_body<4, 1>(Mw41, Cout, g41, g41.Mt, bias, res, res_ld, relu, out, out_ld, t - g44.Mt, c);
}

// ---- per-crop kernels: the output transform of a square-form layer (with or without the tail column) into LDS ----------------------
// Where one image's map [H][W][C] f32 fits the LDS of a CU (TRBA's 4 x 13 x 512: 106 496 B), what follows the output transform of an SE
// block's convolution can read the map from there instead of from HBM.  One workgroup per image: phase 1 is the output bodies above on
// this image's rows of Mw, storing into the LDS crop through a one-image geometry (tile t of the image, the batch's plane stride);
// each thread takes (tile, 4 channels) pairs, looping where the image has more pairs than the workgroup has threads.  Then
//   wino44_output_kernel_chain  conv1 -> conv2 of a block: the input bodies read the crop and write this image's rows of the next
//                               convolution's V (Cin == Cout: the same plan, so V goes where this layer's V was, dead since its GEMM);
//   wino44_output_kernel_se     conv2 -> SE tail: the phases of se_tail.h with x read from the crop, in the f32 order of
//                               se_residual_kernel (1024 virtual threads).
// The same device functions on the same values in the same order as the kernels they replace: bit-identical results.  The names keep
// the wino44_output_kernel prefix (the convolution stage of profilers, bench.py and tools/).
constexpr int kCropThreads = 512;  // 4 x 13 x 512: 4 tiles x 128 channel groups = one pair per thread; LDS allows one workgroup per CU
constexpr int kCropLdsMax = 160 * 1024;  // the LDS of a CU: the kernels' dynamic-LDS limit is raised to it once, whatever the first crop's size

struct WinoCrop {
  WinoGeom a, b;                // one-image geometries of the square part and of the tail column (b.Mt == 0 without one)
  long mt44, mt41, row0_44, row0_41;  // the batch's tiles per plane of each part; this image's first tile row of each part, in floats
};
__device__ __forceinline__ WinoCrop wino_crop(const WinoGeom& g44, const WinoGeom& g41, int C) {
  WinoCrop k;
  k.a = g44; k.b = g41;
  k.a.N = k.b.N = 1;
  k.a.Mt = (long)g44.TH * g44.TW;
  k.b.Mt = g41.Mt ? (long)g41.TH * g41.TW : 0;
  k.mt44 = g44.Mt; k.mt41 = g41.Mt;
  k.row0_44 = blockIdx.x * k.a.Mt * C; k.row0_41 = blockIdx.x * k.b.Mt * C;
  return k;
}
// f44(t, c) / f41(t, c) for this thread's (tile of the image, first of 4 channels) pairs, the square part's tiles first
template <typename F44, typename F41>
__device__ __forceinline__ void wino_crop_pairs(const WinoCrop& k, int C, F44 f44, F41 f41) {
  const int cch = C >> 2, t44 = (int)k.a.Mt, pairs = (t44 + (int)k.b.Mt) * cch;
  for (int i = threadIdx.x; i < pairs; i += kCropThreads) {
    const int t = i / cch, c = (i - t * cch) << 2;
    if (t < t44) f44(t, c);
    else f41(t - t44, c);
  }
}
__device__ __forceinline__ void wino_crop_output(const WinoCrop& k, const float* Mw44, const float* Mw41, int C, const float* bias, int relu,
                                                 float* crop) {
  wino_crop_pairs(k, C,
                  [&](int t, int c) { wino_output_body<4, 4>(Mw44 + k.row0_44, C, k.a, k.mt44, bias, nullptr, 0, relu, crop, C, t, c); },
                  [&](int t, int c) { wino_output_body<4, 1>(Mw41 + k.row0_41, C, k.b, k.mt41, bias, nullptr, 0, relu, crop, C, t, c); });
  __syncthreads();
}

__global__ __launch_bounds__(kCropThreads) void wino44_output_kernel_chain(const float* __restrict__ Mw44, const float* __restrict__ Mw41,
                                                                            int C, WinoGeom g44, WinoGeom g41,
                                                                            const float* __restrict__ bias, int relu,
                                                                            float* __restrict__ V44, float* __restrict__ V41) {
  extern __shared__ __attribute__((aligned(16))) float crop[];  // [H][W][C]
  const WinoCrop k = wino_crop(g44, g41, C);
  wino_crop_output(k, Mw44, Mw41, C, bias, relu, crop);
  const long sW = C, sH = (long)g44.W * C;
  wino_crop_pairs(k, C,
                  [&](int t, int c) { wino_input_body<4, 4>(crop, 0, sH, sW, C, k.a, k.mt44, V44 + k.row0_44, t, c); },
                  [&](int t, int c) { wino_input_body<4, 1>(crop, 0, sH, sW, C, k.b, k.mt41, V41 + k.row0_41, t, c); });
}

__global__ __launch_bounds__(kCropThreads) void wino44_output_kernel_se(const float* __restrict__ Mw44, const float* __restrict__ Mw41,
                                                                         int C, WinoGeom g44, WinoGeom g41,
                                                                         const float* __restrict__ bias, const float* __restrict__ idt,
                                                                         const float* __restrict__ w1, const float* __restrict__ w2,
                                                                         float* __restrict__ gate_ws, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float crop[];  // [H][W][C] | the scratch of se_tail.h
  const int tid = threadIdx.x, HW = g44.H * g44.W;
  const long n = blockIdx.x;
  float* sm = crop + (long)HW * C;
  const WinoCrop k = wino_crop(g44, g41, C);
  wino_crop_output(k, Mw44, Mw41, C, bias, 0, crop);
  const float* is = idt + n * HW * C;
  float* os = out + n * HW * C;
  auto ldx = [&](int p, int c) { return *reinterpret_cast<const f32x4*>(crop + p * C + c); };
  se_partial_sums<1024, kCropThreads>(ldx, HW, C, sm, tid);
  const float* gate = se_gate<1024, kCropThreads>(sm, HW, C, w1, w2, gate_ws + n * C, tid);
  se_scale<1024, kCropThreads>(ldx, [&](int p, int c) { return *reinterpret_cast<const f32x4*>(is + (long)p * C + c); },
                               [&](int p, int c, f32x4 y) { *reinterpret_cast<f32x4*>(os + (long)p * C + c) = y; }, HW, C, gate, tid);
}

// ---- host side of the unfused forms --------------------------------------------------------------------------------------------
// Every entry point derives ONE plan from (d, form): the form's parts, each with its tile geometry, its transform points and its V and
// Mw blocks of the workspace.  2X2, 4X2 and 4X4 are one part, V | Mw.  4X4_COLTAIL is two, V44 | Mw44 | V41 | Mw41: the square pass
// over tile columns 0 ... W/4 - 1 (it reads input column W - 1 as the right halo of its last tile; these are the 4X4 form's own tiles, V
// rows and GEMM rows, so output columns 0 ... W - 2 are that form's bit for bit), then output column W - 1 as one F(4,3) x F(1,3) tile
// per tile row (TRBA's 4 x 13 maps: 108 + 18 point rows per crop where the padded fourth tile made it 144).
struct WinoPart {
  WinoGeom g;
  int P;       // transform points = batched GEMMs of this part
  long v, mw;  // V [P][g.Mt][Cin] and Mw [P][g.Mt][Cout] in the workspace, in floats
};
struct WinoPlan {
  int form, nparts;
  WinoPart part[2];
  long tiles, total;  // the tiles of all parts (the transform grids run over them); the workspace in floats
};

static const int kWinoTile[4][2] = {{2, 2}, {4, 2}, {4, 4}, {4, 4}};  // output tile (MH, MW) per MSOCR_WINO_* form (4X4_COLTAIL: of its square part)

static bool wino_plan(const msocr_conv_desc* d, int form, WinoPlan* pl) {
  if (form < MSOCR_WINO_2X2 || form > MSOCR_WINO_4X4_COLTAIL || !d || d->dtype != MSOCR_F32) return false;
  if (d->KH != 3 || d->KW != 3 || d->stride_h != 1 || d->stride_w != 1 || d->pad_h != 1 || d->pad_w != 1) return false;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Ho != d->H || d->Wo != d->W) return false;
  if (d->Cin <= 0 || d->Cin % 16 || d->Cout <= 0 || d->Cout % 32) return false;
  // every form: the F(2x2) tile count fits in 31 bits and the larger of V / Mw in 2^46 elements
  if ((long)d->N * ((d->H + 1) / 2) * ((d->W + 1) / 2) > 0x7fffffffL) return false;
  const int mh = kWinoTile[form][0], mw = kWinoTile[form][1];
  WinoGeom g;
  g.N = d->N; g.H = d->H; g.W = d->W;
  g.TH = (d->H + mh - 1) / mh; g.TW = (d->W + mw - 1) / mw;
  g.w0 = 0;
  g.Mt = (long)d->N * g.TH * g.TW;
  const int P = (mh + 2) * (mw + 2);
  if (P * g.Mt * (long)(d->Cin > d->Cout ? d->Cin : d->Cout) > 0x3fffffffffffL) return false;
  pl->form = form;
  pl->nparts = 1;
  pl->part[0].g = g; pl->part[0].P = P;
  if (form == MSOCR_WINO_4X4_COLTAIL) {  // the checks above were the 4X4 form's, on its padded tile count
    if (d->W < 5 || d->W % 4 != 1) return false;
    if (d->Cin % 32 || d->Cout % 64) return false;  // the split GEMMs
    pl->nparts = 2;
    WinoGeom& g44 = pl->part[0].g;
    g44.TW = d->W / 4; g44.Mt = (long)d->N * g.TH * g44.TW;
    WinoGeom& g41 = pl->part[1].g;
    g41 = g; g41.TW = 1; g41.w0 = d->W - 1; g41.Mt = (long)d->N * g.TH;
    pl->part[1].P = 18;
  }
  pl->tiles = pl->total = 0;
  for (int i = 0; i < pl->nparts; ++i) {
    WinoPart& p = pl->part[i];
    pl->tiles += p.g.Mt;
    p.v = pl->total;
    p.mw = p.v + p.P * p.g.Mt * d->Cin;
    pl->total = p.mw + p.P * p.g.Mt * d->Cout;
  }
  return true;
}

static bool wino_strides_ok(const msocr_conv_desc* d) { return !(d->in_sN % 4 || d->in_sH % 4 || d->in_sW % 4); }

static int wino_check(const msocr_conv_desc* d, int form, WinoPlan* pl) {
  if (!wino_plan(d, form, pl) || !wino_strides_ok(d) || d->out_ld % 4 || d->out_ld < d->Cout) return MSOCR_E_ARG;
  return MSOCR_OK;
}

// the (form, split) pairs that have GEMM kernels: 2X2 exact, 4X2 exact or split, 4X4 with or without the tail column split
static bool wino_gemm_ok(int form, int split) {
  if (split != 0 && split != 1) return false;
  return form == MSOCR_WINO_4X2 || (form == MSOCR_WINO_2X2 && !split) || ((form == MSOCR_WINO_4X4 || form == MSOCR_WINO_4X4_COLTAIL) && split);
}

extern "C" int64_t msocr_winograd_workspace_bytes(const msocr_conv_desc* d, int form) {
  WinoPlan pl;
  if (!wino_plan(d, form, &pl)) return -1;
  return pl.total * (int64_t)sizeof(float);
}

// the transform grids: one thread per tile and 4 channels, the tiles of all parts
static bool wino_grid(const WinoPlan& pl, int C, dim3* grid) {
  const long nb = (pl.tiles * (C / 4) + 255) / 256;
  if (nb > 0x7fffffffL) return false;
  *grid = dim3((unsigned)nb);
  return true;
}

static int wino_launch_input(const msocr_conv_desc* d, const WinoPlan& pl, const void* in, void* workspace, void* stream) {
  if (!in || !workspace || (((uintptr_t)in | (uintptr_t)workspace) & 15)) return MSOCR_E_ARG;
  dim3 grid;
  if (!wino_grid(pl, d->Cin, &grid)) return MSOCR_E_ARG;
  const dim3 blk(256);
  hipStream_t st = (hipStream_t)stream;
  const float* x = (const float*)in;
  float* ws = (float*)workspace;
  const long sN = d->in_sN, sH = d->in_sH, sW = d->in_sW;
  const WinoPart& a = pl.part[0];
  if (pl.nparts == 2) MSOCR_LAUNCH(wino44_input_kernel_coltail, grid, blk, 0, st, x, sN, sH, sW, d->Cin, a.g, pl.part[1].g, ws + a.v, ws + pl.part[1].v);
  else if (pl.form == MSOCR_WINO_2X2) MSOCR_LAUNCH(wino_input_kernel, grid, blk, 0, st, x, sN, sH, sW, d->Cin, a.g, ws + a.v);
  else if (pl.form == MSOCR_WINO_4X2) MSOCR_LAUNCH(wino42_input_kernel, grid, blk, 0, st, x, sN, sH, sW, d->Cin, a.g, ws + a.v);
  else MSOCR_LAUNCH(wino44_input_kernel, grid, blk, 0, st, x, sN, sH, sW, d->Cin, a.g, ws + a.v);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

// The three stages of msocr_conv3x3_winograd as separate entry points (same kernels): tests and the per-kernel roofline of
// bench.py time them one by one.
extern "C" int msocr_winograd_input_transform(const msocr_conv_desc* d, int form, const void* in, void* workspace, void* stream) {
  WinoPlan pl;
  if (wino_check(d, form, &pl) != MSOCR_OK) return MSOCR_E_ARG;
  return wino_launch_input(d, pl, in, workspace, stream);
}

// One batched GEMM launch per part, in part order.  split = 0: u = [P][Cout][Cin] f32 (exact-f32 MFMA); split = 1: u = K-tile-major bf16
// planes [3][P][Cin/32][Cout][32], the P GEMMs on the bf16 matrix pipes with exactly split operands (conv_split.hip / conv_split_pp.hip;
// V is split in registers).  Two parts: u = the first part's array, then the second's, each with its own plane stride (4X4_COLTAIL:
// the split of the 4X4 form's [36][Cout][Cin], then the split of the tail tile's [18][Cout][Cin]).
extern "C" int msocr_winograd_gemm(const msocr_conv_desc* d, int form, int split, const void* u, void* workspace, void* stream) {
  WinoPlan pl;
  if (!wino_gemm_ok(form, split) || wino_check(d, form, &pl) != MSOCR_OK || !u || !workspace) return MSOCR_E_ARG;
  if (split && (d->Cin % 32 || d->Cout % 64)) return MSOCR_E_ARG;
  float* ws = (float*)workspace;
  long uoff = 0;  // in elements of u: a multiple of Cin, so 16-byte aligned in either format
  for (int i = 0; i < pl.nparts; ++i) {
    const WinoPart& p = pl.part[i];
    const int rc = split ? msocr_internal_gemm_split_batched(ws + p.v, (const uint16_t*)u + uoff, ws + p.mw, p.g.Mt, d->Cout, d->Cin, p.P, (hipStream_t)stream)
                         : msocr_internal_gemm_f32_batched(ws + p.v, (const float*)u + uoff, ws + p.mw, p.g.Mt, d->Cout, d->Cin, p.P, (hipStream_t)stream);
    if (rc != MSOCR_OK) return rc;
    uoff += (split ? 3L : 1L) * p.P * d->Cout * d->Cin;
  }
  return MSOCR_OK;
}

extern "C" int msocr_winograd_output_transform(const msocr_conv_desc* d, int form, const void* workspace, const float* bias,
                                               const void* residual, void* out, void* stream) {
  WinoPlan pl;
  if (wino_check(d, form, &pl) != MSOCR_OK || !out || !workspace) return MSOCR_E_ARG;
  if (((uintptr_t)out | (uintptr_t)workspace) & 15) return MSOCR_E_ARG;
  const bool has_res = (d->flags & MSOCR_CONV_RESIDUAL) != 0;
  if (has_res && (!residual || d->res_ld % 4 || d->res_ld < d->Cout || ((uintptr_t)residual & 15))) return MSOCR_E_ARG;
  if (bias && ((uintptr_t)bias & 15)) return MSOCR_E_ARG;
  dim3 grid;
  if (!wino_grid(pl, d->Cout, &grid)) return MSOCR_E_ARG;
  const dim3 blk(256);
  hipStream_t st = (hipStream_t)stream;
  const float* ws = (const float*)workspace;
  const float* rp = has_res ? (const float*)residual : nullptr;
  const long res_ld = d->res_ld, out_ld = d->out_ld;
  const int relu = (d->flags & MSOCR_CONV_RELU) ? 1 : 0;
  float* o = (float*)out;
  const WinoPart& a = pl.part[0];
  if (pl.nparts == 2) MSOCR_LAUNCH(wino44_output_kernel_coltail, grid, blk, 0, st, ws + a.mw, ws + pl.part[1].mw, d->Cout, a.g, pl.part[1].g, bias, rp, res_ld, relu, o, out_ld);
  else if (pl.form == MSOCR_WINO_2X2) MSOCR_LAUNCH(wino_output_kernel, grid, blk, 0, st, ws + a.mw, d->Cout, a.g, bias, rp, res_ld, relu, o, out_ld);
  else if (pl.form == MSOCR_WINO_4X2) MSOCR_LAUNCH(wino42_output_kernel, grid, blk, 0, st, ws + a.mw, d->Cout, a.g, bias, rp, res_ld, relu, o, out_ld);
  else MSOCR_LAUNCH(wino44_output_kernel, grid, blk, 0, st, ws + a.mw, d->Cout, a.g, bias, rp, res_ld, relu, o, out_ld);
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

// ---- host side of the per-crop kernels -------------------------------------------------------------------------------------------
// Dynamic LDS of a per-crop kernel on d's layer: the crop, and with se the SE tail's scratch behind it; -1 where the kernels do not
// apply: a form without square tiles, Cin != Cout for the chain, a channel count the SE tail does not take, out not dense, or more
// than the 160 KB of a CU.
static long wino_crop_lds(const msocr_conv_desc* d, const WinoPlan& pl, bool se) {
  if (pl.form != MSOCR_WINO_4X4 && pl.form != MSOCR_WINO_4X4_COLTAIL) return -1;
  const int C = d->Cout;
  if (se ? (C < 64 || C > 1024 || (C & (C - 1)) || d->out_ld != C) : d->Cin != C) return -1;
  const long bytes = ((long)d->H * d->W * C + (se ? se_scratch_floats(1024, C) : 0)) * (long)sizeof(float);
  return bytes <= kCropLdsMax ? bytes : -1;
}

extern "C" int64_t msocr_winograd_crop_lds_bytes(const msocr_conv_desc* d, int form, int se) {
  WinoPlan pl;
  if (!wino_plan(d, form, &pl)) return -1;
  return wino_crop_lds(d, pl, se != 0);
}

// the parts of a square-form plan as the per-crop kernels take them: without a tail column the second part is empty
struct WinoCropParts {
  WinoGeom g44, g41;
  long v44, v41, mw44, mw41;
};
static WinoCropParts wino_crop_parts(const WinoPlan& pl) {
  const WinoPart& a = pl.part[0];
  const WinoPart& b = pl.part[pl.nparts - 1];
  WinoCropParts k = {a.g, b.g, a.v, b.v, a.mw, b.mw};
  if (pl.nparts == 1) k.g41.Mt = 0;
  return k;
}

extern "C" int msocr_winograd_output_chain(const msocr_conv_desc* d, int form, void* workspace, const float* bias, void* stream) {
  WinoPlan pl;
  if (!wino_plan(d, form, &pl) || !workspace || ((uintptr_t)workspace & 15) || (bias && ((uintptr_t)bias & 15))) return MSOCR_E_ARG;
  const long lds = wino_crop_lds(d, pl, false);
  if (lds < 0 || (d->flags & MSOCR_CONV_RESIDUAL)) return MSOCR_E_ARG;
  if (msocr_internal_lds_limit(reinterpret_cast<const void*>(wino44_output_kernel_chain), kCropLdsMax) != MSOCR_OK) return MSOCR_E_LAUNCH;
  const WinoCropParts k = wino_crop_parts(pl);
  float* ws = (float*)workspace;
  MSOCR_LAUNCH(wino44_output_kernel_chain, dim3((unsigned)d->N), dim3(kCropThreads), (size_t)lds, (hipStream_t)stream, ws + k.mw44, ws + k.mw41,
               d->Cout, k.g44, k.g41, bias, (d->flags & MSOCR_CONV_RELU) ? 1 : 0, ws + k.v44, ws + k.v41);
  return LAUNCH_OK();
}

extern "C" int msocr_winograd_output_se(const msocr_conv_desc* d, int form, const void* workspace, const float* bias, const void* identity,
                                        const float* w1, const float* w2, float* gate_ws, void* out, void* stream) {
  WinoPlan pl;
  if (!wino_plan(d, form, &pl) || !workspace || !identity || !w1 || !w2 || !gate_ws || !out) return MSOCR_E_ARG;
  if (((uintptr_t)workspace | (uintptr_t)identity | (uintptr_t)out) & 15 || (bias && ((uintptr_t)bias & 15))) return MSOCR_E_ARG;
  const long lds = wino_crop_lds(d, pl, true);
  if (lds < 0 || (d->flags & (MSOCR_CONV_RESIDUAL | MSOCR_CONV_RELU))) return MSOCR_E_ARG;
  if (msocr_internal_lds_limit(reinterpret_cast<const void*>(wino44_output_kernel_se), kCropLdsMax) != MSOCR_OK) return MSOCR_E_LAUNCH;
  const WinoCropParts k = wino_crop_parts(pl);
  const float* ws = (const float*)workspace;
  MSOCR_LAUNCH(wino44_output_kernel_se, dim3((unsigned)d->N), dim3(kCropThreads), (size_t)lds, (hipStream_t)stream, ws + k.mw44, ws + k.mw41,
               d->Cout, k.g44, k.g41, bias, (const float*)identity, w1, w2, gate_ws, (float*)out);
  return LAUNCH_OK();
}

extern "C" int msocr_conv3x3_winograd(const msocr_conv_desc* d, int form, int split, const void* in, const void* u, const float* bias,
                                      const void* residual, void* out, void* workspace, void* stream) {
  if (!u || !wino_gemm_ok(form, split)) return MSOCR_E_ARG;
  int rc = msocr_winograd_input_transform(d, form, in, workspace, stream);
  if (rc != MSOCR_OK) return rc;
  rc = msocr_winograd_gemm(d, form, split, u, workspace, stream);
  if (rc != MSOCR_OK) return rc;
  return msocr_winograd_output_transform(d, form, workspace, bias, residual, out, stream);
}

// =====================================================================================================================
// Cin == 64: the tall form with the 24 GEMMs AND the output transform in ONE kernel (Mw never reaches HBM).
// With 64 input channels the transform-domain GEMMs have K = 64 and the unfused form is HBM-bound on Mw (3x the layer's output:
// TRBA conv0b would move 132 GB per step against 19 GB for the direct convolution).  Here a workgroup owns 32 tiles x 32 output
// channels: for each of the 24 points it stages V[p][32 tiles][64] and U[p][32 couts][64] through LDS (double-buffered, 16-B chunks
// XOR-swizzled by row), one 16x16 accumulator tile per wave and point (v_mfma_f32_16x16x4_f32, k = 64 -> 16 MFMAs); after the 24th
// point every lane holds all 24 transform-domain values of its 4 (tile, cout) positions and applies A6^T . A4 in registers, then
// bias / residual / ReLU and — MSOCR_CONV_POOL2 — the 2x2/2 max-pool that closes conv0 in SE-ResNet31 (seresnet31.py:81-89: ... ReLU,
// MaxPool2d(2, 2)), so the pooled map is the only thing written.  HBM traffic: V once (3x the input) + the (pooled) output.
// =====================================================================================================================
typedef unsigned int u32x4w __attribute__((ext_vector_type(4)));
#ifndef WINO_FUSED_PFD
#define WINO_FUSED_PFD 3
#endif

// SPLIT = true (round 3): the 24 K = 64 GEMMs on the bf16 matrix pipes with exactly split operands (conv_split.hip has the
// arithmetic): V is split in registers on the way into LDS, U arrives as three bf16 planes [3][24][Cout][64]; per point and wave
// 12 x v_mfma_f32_16x16x32_bf16 (192 cycles) replace 16 x v_mfma_f32_16x16x4_f32 (512 cycles).  Same accumulator layout, so the
// output transform below is shared.
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2w __attribute__((ext_vector_type(2)));
template <bool POOL, bool SPLIT = false>
__global__ __launch_bounds__(256, 3) void wino42_fused64_kernel(const float* __restrict__ V, const void* __restrict__ Uv, int Cout,
                                                                 WinoGeom g, const float* __restrict__ bias,
                                                                 const float* __restrict__ res, long res_ld, int relu,
                                                                 float* __restrict__ out, long out_ld) {
  constexpr int K = 64, BM = 32, BN = 32, ROWB = K * 4;  // exact form: 256-byte tile rows, 16 chunks of 16 B
  constexpr int ROWS = 128, PLANE = BM * ROWS;           // split form: six [32 rows][64 bf16 = 128 B] planes per stage
  constexpr int STAGE_BYTES = SPLIT ? 6 * PLANE : (BM + BN) * ROWB;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = wave >> 1, nj = wave & 1;
  const int r16 = lane & 15, kg = lane >> 4;
  // XCD-aware order: blocks b, b+8, ... share an XCD (its L2): give each XCD a contiguous range of logical blocks, cout blocks
  // fastest, so the Cout/32 workgroups that read one V tile run on the same L2
  const int nbn = Cout / BN;
  const long bid = xcd_tile<long>(blockIdx.x, gridDim.x);
  const int nb = (int)(bid % nbn);
  const long m0 = (bid / nbn) * BM;
  const int n0 = nb * BN;
  f32x4 acc[24];

  if constexpr (SPLIT) {
    const unsigned short* U = reinterpret_cast<const unsigned short*>(Uv);
    // staging: V as the exact form (row = tid / 16 (+16), 16-B chunk of 4 f32 = tid % 16); U planes: row = tid / 8, 16-B chunk of 8 bf16 = tid % 8
    const int chunk = tid & 15, row0 = tid >> 4;
    const int bchunk = tid & 7, brow = tid >> 3;
    const long planeV = g.Mt * (long)K, planeU = (long)Cout * K, uplane = 24 * planeU;
    const float* pa[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      long m = m0 + row0 + 16 * i;
      if (m >= g.Mt) m = g.Mt - 1;  // valid memory; the rows are never stored
      pa[i] = V + m * K + chunk * 4;
    }
    const unsigned short* pb = U + (long)(n0 + brow) * K + bchunk * 8;
    constexpr int PFD = 2;
    u32x4w ra[PFD][2], rb[PFD][3];
    auto gload = [&](int p) {
#pragma unroll
      for (int i = 0; i < 2; ++i) ra[p % PFD][i] = *reinterpret_cast<const u32x4w*>(pa[i] + p * planeV);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) rb[p % PFD][pl] = *reinterpret_cast<const u32x4w*>(pb + pl * uplane + p * planeU);
    };
    auto sstore = [&](int p) {
      unsigned char* st = &smem[p & 1][0];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = row0 + 16 * i;
        float x0 = __uint_as_float(ra[p % PFD][i][0]), x1 = __uint_as_float(ra[p % PFD][i][1]);
        float x2 = __uint_as_float(ra[p % PFD][i][2]), x3 = __uint_as_float(ra[p % PFD][i][3]);
        unsigned char* dst = st + row * ROWS + (((chunk >> 1) ^ (row & 7)) << 4) + ((chunk & 1) << 3);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          u32x2w v;
          v[0] = split_step(x0, x1);
          v[1] = split_step(x2, x3);
          *reinterpret_cast<u32x2w*>(dst + pl * PLANE) = v;
        }
      }
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        *reinterpret_cast<u32x4w*>(st + (3 + pl) * PLANE + brow * ROWS + ((bchunk ^ (brow & 7)) << 4)) = rb[p % PFD][pl];
    };
#pragma unroll
    for (int q = 0; q < PFD; ++q) gload(q);
    sstore(0);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 24; ++p) {
      if (p + PFD < 24) gload(p + PFD);
      const unsigned char* st = &smem[p & 1][0];
      const int rowa = mi * 16 + r16, rowb = nj * 16 + r16;
      f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {  // two k32 steps; lane (r16, kg) takes k = 32 ks + 8 kg + 0..7 of its row for both operands
        const int c = 4 * ks + kg;
        bf16x8w fa[3], fb[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          fa[pl] = *reinterpret_cast<const bf16x8w*>(st + pl * PLANE + rowa * ROWS + ((c ^ (rowa & 7)) << 4));
          fb[pl] = *reinterpret_cast<const bf16x8w*>(st + (3 + pl) * PLANE + rowb * ROWS + ((c ^ (rowb & 7)) << 4));
        }
        mma6(fa, fb, c4);
      }
      acc[p] = c4;
      if (p + 1 < 24) sstore(p + 1);
      __syncthreads();
    }
  } else {
  const float* U = reinterpret_cast<const float*>(Uv);
  // staging coordinates: thread -> (row = tid / 16 (+16 on the second pass), 16-B chunk = tid % 16)
  const int chunk = tid & 15, row0 = tid >> 4;
  const long planeV = g.Mt * (long)K, planeU = (long)Cout * K;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    long m = m0 + row0 + 16 * i;
    if (m >= g.Mt) m = g.Mt - 1;  // valid memory; the rows are never stored
    pa[i] = V + m * K + chunk * 4;
    pb[i] = U + (long)(n0 + row0 + 16 * i) * K + chunk * 4;
  }
  // register prefetch PFD points ahead (slot = point % PFD): one point's MFMAs (16 per wave) are shorter than an HBM round trip
  constexpr int PFD = WINO_FUSED_PFD;
  u32x4w ra[PFD][2], rb[PFD][2];
  auto gload = [&](int p) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[p % PFD][i] = *reinterpret_cast<const u32x4w*>(pa[i] + p * planeV);
      rb[p % PFD][i] = *reinterpret_cast<const u32x4w*>(pb[i] + p * planeU);
    }
  };
  auto sstore = [&](int p) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = row0 + 16 * i;
      *reinterpret_cast<u32x4w*>(&smem[p & 1][row * ROWB + ((chunk ^ (row & 15)) << 4)]) = ra[p % PFD][i];
      *reinterpret_cast<u32x4w*>(&smem[p & 1][(BM + row) * ROWB + ((chunk ^ (row & 15)) << 4)]) = rb[p % PFD][i];
    }
  };
#pragma unroll
  for (int q = 0; q < PFD; ++q) gload(q);
  sstore(0);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 24; ++p) {
    if (p + PFD < 24) gload(p + PFD);  // slot p % PFD held point p, stored to LDS at the end of point p - 1
    const unsigned char* sa = &smem[p & 1][0];
    const unsigned char* sb = sa + BM * ROWB;
    // lane (r16, kg) takes k = 16 * kg + 0..15 of its row for BOTH operands (a consistent permutation of the reduction index)
    const int rowa = mi * 16 + r16, rowb = nj * 16 + r16;
    u32x4w fa[4], fb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = kg * 4 + q;
      fa[q] = *reinterpret_cast<const u32x4w*>(sa + rowa * ROWB + ((c ^ (rowa & 15)) << 4));
      fb[q] = *reinterpret_cast<const u32x4w*>(sb + rowb * ROWB + ((c ^ (rowb & 15)) << 4));
    }
    // one dependent accumulation chain per point (two chains double the live registers: measured, dropped; the U fragments straight
    // from L2 instead of LDS: 1.5x slower)
    f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(fa[q][e]), __uint_as_float(fb[q][e]), c4, 0, 0, 0);
    acc[p] = c4;
    if (p + 1 < 24) sstore(p + 1);
    __syncthreads();
  }

  }

  // ---- output transform in registers: lane holds rows (tiles) 4 * kg + e, column (cout) r16 of its wave's 16x16 block ----
  const int co = n0 + nj * 16 + r16;
  const float b = bias ? bias[co] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long t = m0 + mi * 16 + 4 * kg + e;
    if (t >= g.Mt) continue;
    const int tw = (int)(t % g.TW);
    const long r = t / g.TW;
    const int th = (int)(r % g.TH);
    const int n = (int)(r / g.TH);
    float s[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m0_ = acc[0 * 4 + j][e], m1 = acc[1 * 4 + j][e], m2 = acc[2 * 4 + j][e], m3 = acc[3 * 4 + j][e], m4 = acc[4 * 4 + j][e],
                  m5 = acc[5 * 4 + j][e];
      const float p12 = m1 + m2, d12 = m1 - m2, p34 = m3 + m4, d34 = m3 - m4;   // A^T of wino44_at, scalar
      s[0][j] = (m0_ + p12) + p34;
      s[1][j] = fmaf(1.5f, d12, (2.0f / 3.0f) * d34);
      s[2][j] = fmaf(2.25f, p12, (4.0f / 9.0f) * p34);
      s[3][j] = fmaf(3.375f, d12, (8.0f / 27.0f) * d34) + m5;
    }
    float y[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i][0] = ((s[i][0] + s[i][1]) + s[i][2]) + b;
      y[i][1] = ((s[i][1] - s[i][2]) - s[i][3]) + b;
    }
    if constexpr (POOL) {
      // H and W are even (host check): the 2x2 windows are (rows 4th+{0,1} | 4th+{2,3}) x (cols 2tw+{0,1})
      const int Hp = g.H >> 1, Wp = g.W >> 1;
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const int hp = 2 * th + i2;
        if (hp >= Hp || tw >= Wp) continue;
        float v0 = y[2 * i2][0], v1 = y[2 * i2][1], v2 = y[2 * i2 + 1][0], v3 = y[2 * i2 + 1][1];
        if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        out[(((long)n * Hp + hp) * Wp + tw) * out_ld + co] = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ho = 4 * th + i;
        if (ho >= g.H) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int wo = 2 * tw + j;
          if (wo >= g.W) continue;
          const long pix = ((long)n * g.H + ho) * g.W + wo;
          float v = y[i][j];
          if (res) v += res[pix * res_ld + co];
          if (relu) v = fmaxf(v, 0.f);
          out[pix * out_ld + co] = v;
        }
      }
    }
  }
}

// ---- fused Cin = 64 layer, second form (round 3, split operands, Cout % 64 == 0) --------------------------------------------------
// The kernel above holds the 24 products of a (tile, cout) pair in 24 accumulators and transforms them at the end, which pins a
// wave to one 16 x 16 block (96 accumulator registers) and a workgroup to 32 tiles x 32 couts: per point 12 short MFMAs between two
// barriers, and every workgroup pulls all of U for its 32 couts (288 KB) from L2 for 32 tiles (PMC: matrix pipes 0.25 busy on conv0b,
// 13 ms per step).  The output transform is linear in the 24 products, so this form accumulates it on the fly:
//   Y[a][b] += AT6[a][i] * AT4[b][j] * M[i][j]   right after point (i, j) is multiplied
// (8 output accumulators + the current product; 108 FMAs per element and kernel instead of 24 x 64 MACs on the pipes).  A wave then
// owns a 32 x 32 block (v_mfma_f32_32x32x16_bf16, 24 per point), a workgroup 64 tiles x 64 couts: 4x the matrix work per barrier and
// half the L2 traffic per MAC.  Same V / U layouts, same epilogue semantics (bias, residual, ReLU, MaxPool2d(2, 2)).
template <bool POOL>
__global__ __launch_bounds__(256, 2) void wino42_fused64_v2_kernel(const float* __restrict__ V, const unsigned short* __restrict__ U, int Cout,
                                                                    WinoGeom g, const float* __restrict__ bias,
                                                                    const float* __restrict__ res, long res_ld, int relu,
                                                                    float* __restrict__ out, long out_ld) {
  constexpr int K = 64, BM = 64, BN = 64, ROWS = 128, PLANE = BM * ROWS;  // six [64 rows][64 bf16 = 128 B] planes, one stage
  typedef float f32x16w __attribute__((ext_vector_type(16)));
  __shared__ __attribute__((aligned(16))) unsigned char smem[6 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, half = lane >> 5;
  const int nbn = Cout / BN;
  const long bid = xcd_tile<long>(blockIdx.x, gridDim.x);  // XCD-aware order, cout blocks fastest (the workgroups that read one V tile share an L2)
  const int nb = (int)(bid % nbn);
  const long m0 = (bid / nbn) * BM;
  const int n0 = nb * BN;

  // staging: V rows = tid / 16 + 16 i, 16-B chunk of 4 f32 = tid % 16; U planes: rows = tid / 8 + 32 j, 16-B chunk of 8 bf16 = tid % 8
  const int chunk = tid & 15, row0 = tid >> 4;
  const int bchunk = tid & 7, brow = tid >> 3;
  const long planeV = g.Mt * (long)K, planeU = (long)Cout * K, uplane = 24 * planeU;
  const float* pa[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long m = m0 + row0 + 16 * i;
    if (m >= g.Mt) m = g.Mt - 1;  // valid memory; the rows are never stored
    pa[i] = V + m * K + chunk * 4;
  }
  const unsigned short* pb = U + (long)(n0 + brow) * K + bchunk * 8;
  u32x4w ra[4], rb[3][2];
  auto gload = [&](int p) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const u32x4w*>(pa[i] + p * planeV);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j) rb[pl][j] = *reinterpret_cast<const u32x4w*>(pb + pl * uplane + p * planeU + (long)j * 32 * K);
  };
  auto sstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 16 * i;
      float x0 = __uint_as_float(ra[i][0]), x1 = __uint_as_float(ra[i][1]), x2 = __uint_as_float(ra[i][2]), x3 = __uint_as_float(ra[i][3]);
      unsigned char* dst = smem + row * ROWS + (((chunk >> 1) ^ (row & 7)) << 4) + ((chunk & 1) << 3);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        u32x2w v;
        v[0] = split_step(x0, x1);
        v[1] = split_step(x2, x3);
        *reinterpret_cast<u32x2w*>(dst + pl * PLANE) = v;
      }
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = brow + 32 * j;
        *reinterpret_cast<u32x4w*>(smem + (3 + pl) * PLANE + row * ROWS + ((bchunk ^ (row & 7)) << 4)) = rb[pl][j];
      }
  };

  f32x16w Y[8];
#pragma unroll
  for (int o = 0; o < 8; ++o)
#pragma unroll
    for (int e = 0; e < 16; ++e) Y[o][e] = 0.f;

  gload(0);
  sstore();
  __syncthreads();
  // coefficient of point p = 4 i + j in output o = 2 a + b: AT6[a][i] * AT4[b][j], AT6 = A^T of wino44_at (the points
  // {0, +-3/2, +-2/3, inf} since round 4), AT4 = [[1,1,1,0],[0,1,-1,-1]] — a run-time table and a ROLLED loop over the points: unrolled, the 24 points'
  // loads and products are hoisted across each other and the kernel spills (375 registers fully unrolled, 128 with four points
  // per iteration); the price is 8 FMAs per element and point including the 84 zero coefficients (192 instead of 108)
  __shared__ float s_cf[24][8];
  if (tid < 192) {
    const float t6[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1.5f, -1.5f, 2.0f / 3.0f, -2.0f / 3.0f, 0}, {0, 2.25f, 2.25f, 4.0f / 9.0f, 4.0f / 9.0f, 0},
                            {0, 3.375f, -3.375f, 8.0f / 27.0f, -8.0f / 27.0f, 1}};   // A^T on the points {0, +-3/2, +-2/3, inf}
    const float t4[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
    const int pp = tid >> 3, o = tid & 7;
    s_cf[pp][o] = t6[o >> 1][pp >> 2] * t4[o & 1][pp & 3];
  }
  __syncthreads();
  const int rowa = wm * 32 + r32, rowb = wn * 32 + r32;
#pragma unroll 1
  for (int p = 0; p < 24; ++p) {
    if (p + 1 < 24) gload(p + 1);  // in flight under this point's MFMAs
    f32x16w m;
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {  // k16 steps; lane (r32, half) takes k = 16 ks + 8 half + 0..7 of its row for both operands
      const int c = 2 * ks + half;
      bf16x8w fa[3], fb[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        fa[pl] = *reinterpret_cast<const bf16x8w*>(smem + pl * PLANE + rowa * ROWS + ((c ^ (rowa & 7)) << 4));
        fb[pl] = *reinterpret_cast<const bf16x8w*>(smem + (3 + pl) * PLANE + rowb * ROWS + ((c ^ (rowb & 7)) << 4));
      }
      mma6(fa, fb, m);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const float cf = s_cf[p][o];
#pragma unroll
      for (int e = 0; e < 16; ++e) Y[o][e] = fmaf(cf, m[e], Y[o][e]);
    }
    __syncthreads();  // every wave has read the stage
    if (p + 1 < 24) sstore();
    __syncthreads();
  }

  // ---- epilogue: element e of this lane = tile m0 + 32 wm + acc_row(e, half), cout n0 + 32 wn + r32 ----
  const int co = n0 + wn * 32 + r32;
  const float bv = bias ? bias[co] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long t = m0 + wm * 32 + acc_row(e, half);
    if (t >= g.Mt) continue;
    const int tw = (int)(t % g.TW);
    const long r = t / g.TW;
    const int th = (int)(r % g.TH);
    const int n = (int)(r / g.TH);
    if constexpr (POOL) {
      const int Hp = g.H >> 1, Wp = g.W >> 1;
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const int hp = 2 * th + i2;
        if (hp >= Hp || tw >= Wp) continue;
        float v0 = Y[4 * i2 + 0][e] + bv, v1 = Y[4 * i2 + 1][e] + bv, v2 = Y[4 * i2 + 2][e] + bv, v3 = Y[4 * i2 + 3][e] + bv;
        if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        out[(((long)n * Hp + hp) * Wp + tw) * out_ld + co] = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
      }
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int ho = 4 * th + a;
        if (ho >= g.H) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int wo = 2 * tw + b;
          if (wo >= g.W) continue;
          const long pix = ((long)n * g.H + ho) * g.W + wo;
          float v = Y[a * 2 + b][e] + bv;
          if (res) v += res[pix * res_ld + co];
          if (relu) v = fmaxf(v, 0.f);
          out[pix * out_ld + co] = v;
        }
      }
    }
  }
}

static int wino_fused64_check(const msocr_conv_desc* d, WinoPlan* pl) {
  if (!wino_plan(d, MSOCR_WINO_4X2, pl) || d->Cin != 64 || !wino_strides_ok(d) || d->out_ld < d->Cout) return MSOCR_E_ARG;
  if (d->flags & MSOCR_CONV_POOL2) {
    if ((d->H & 1) || (d->W & 1) || (d->flags & MSOCR_CONV_RESIDUAL)) return MSOCR_E_ARG;
  }
  return MSOCR_OK;
}

extern "C" int64_t msocr_winograd_fused64_workspace_bytes(const msocr_conv_desc* d) {
  WinoPlan pl;
  if (wino_fused64_check(d, &pl) != MSOCR_OK) return -1;
  return 24 * pl.part[0].g.Mt * (int64_t)d->Cin * (int64_t)sizeof(float);
}

// stage 2 of msocr_conv3x3_winograd_fused64 (stage 1 is msocr_winograd_input_transform of the 4X2 form): V in the workspace -> out.
// split = 0: u = [24][Cout][64] f32; split = 1: u = three bf16 planes [3][24][Cout][64] (msocr_split_bf16x3_host), the GEMMs on the
// bf16 matrix pipes with exactly split operands
extern "C" int msocr_winograd_fused64_gemm_output(const msocr_conv_desc* d, int split, const void* u, const void* workspace,
                                                  const float* bias, const void* residual, void* out, void* stream) {
  WinoPlan pl;
  if ((split != 0 && split != 1) || wino_fused64_check(d, &pl) != MSOCR_OK || !u || !workspace || !out) return MSOCR_E_ARG;
  const WinoGeom& g = pl.part[0].g;
  if (((uintptr_t)workspace | (uintptr_t)u) & 15) return MSOCR_E_ARG;
  const bool has_res = (d->flags & MSOCR_CONV_RESIDUAL) != 0;
  if (has_res && (!residual || d->res_ld < d->Cout)) return MSOCR_E_ARG;
  const long nblk = ((g.Mt + 31) / 32) * (long)(d->Cout / 32);
  if (nblk <= 0 || nblk > 0x7fffffffL) return MSOCR_E_ARG;
  const int relu = (d->flags & MSOCR_CONV_RELU) ? 1 : 0;
  const float* rp = has_res ? (const float*)residual : nullptr;
  const dim3 grid((unsigned)nblk), blk(256);
  hipStream_t st = (hipStream_t)stream;
  const float* ws = (const float*)workspace;
  // split operands and Cout % 64 == 0: the on-the-fly output transform with 64 x 64 workgroup tiles; the 24-accumulator kernel
  // takes exact operands and split ones with Cout % 64 != 0
  if (split && d->Cout % 64 == 0) {
    const long nblk2 = ((g.Mt + 63) / 64) * (long)(d->Cout / 64);
    if (nblk2 <= 0 || nblk2 > 0x7fffffffL) return MSOCR_E_ARG;
    const dim3 grid2((unsigned)nblk2);
    const unsigned short* up = (const unsigned short*)u;
    if (d->flags & MSOCR_CONV_POOL2)
      MSOCR_LAUNCH((wino42_fused64_v2_kernel<true>), grid2, blk, 0, st, ws, up, d->Cout, g, bias, (const float*)nullptr, 0L, relu, (float*)out, (long)d->out_ld);
    else
      MSOCR_LAUNCH((wino42_fused64_v2_kernel<false>), grid2, blk, 0, st, ws, up, d->Cout, g, bias, rp, (long)d->res_ld, relu, (float*)out, (long)d->out_ld);
    return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
  }
  if (d->flags & MSOCR_CONV_POOL2) {
    if (split) MSOCR_LAUNCH((wino42_fused64_kernel<true, true>), grid, blk, 0, st, ws, u, d->Cout, g, bias, (const float*)nullptr, 0L, relu, (float*)out, (long)d->out_ld);
    else MSOCR_LAUNCH((wino42_fused64_kernel<true, false>), grid, blk, 0, st, ws, u, d->Cout, g, bias, (const float*)nullptr, 0L, relu, (float*)out, (long)d->out_ld);
  } else {
    if (split) MSOCR_LAUNCH((wino42_fused64_kernel<false, true>), grid, blk, 0, st, ws, u, d->Cout, g, bias, rp, (long)d->res_ld, relu, (float*)out, (long)d->out_ld);
    else MSOCR_LAUNCH((wino42_fused64_kernel<false, false>), grid, blk, 0, st, ws, u, d->Cout, g, bias, rp, (long)d->res_ld, relu, (float*)out, (long)d->out_ld);
  }
  return hipGetLastError() == hipSuccess ? MSOCR_OK : MSOCR_E_LAUNCH;
}

extern "C" int msocr_conv3x3_winograd_fused64(const msocr_conv_desc* d, int split, const void* in, const void* u, const float* bias,
                                              const void* residual, void* out, void* workspace, void* stream) {
  WinoPlan pl;
  if ((split != 0 && split != 1) || wino_fused64_check(d, &pl) != MSOCR_OK || !u) return MSOCR_E_ARG;
  const int rc = wino_launch_input(d, pl, in, workspace, stream);
  if (rc != MSOCR_OK) return rc;
  return msocr_winograd_fused64_gemm_output(d, split, u, workspace, bias, residual, out, stream);
}

static const double kWinoG4[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};  // F(2,3) on {0, 1, -1, inf}
static const double kWinoG6[6][3] = {{1.0, 0.0, 0.0},                                                      // F(4,3): wino44_bt's points
                                     {8.0 / 65, 12.0 / 65, 18.0 / 65},     {8.0 / 65, -12.0 / 65, 18.0 / 65},
                                     {-81.0 / 130, -27.0 / 65, -18.0 / 65}, {-81.0 / 130, 27.0 / 65, -18.0 / 65},
                                     {0.0, 0.0, 1.0}};
static const double kWinoG3[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};                    // F(1,3): the taps themselves

static const double (*wino_g(int points))[3] { return points == 6 ? kWinoG6 : points == 4 ? kWinoG4 : kWinoG3; }

// U[xi*PW+nu][co][c] = sum_{kh,kw} Gh[xi][kh] Gw[nu][kw] w[co][kh][kw][c] (xi on the kernel's H axis), evaluated in f64 (G g over kh
// first, then over kw) and rounded once to f32, [PH*PW][Cout][Cin]: one tile's planes per call.  4X4_COLTAIL: its tail tile's,
// F(4,3) x F(1,3) with Gw = the identity, [18][Cout][Cin]; its square tiles' planes are the 4X4 form's call.  u_out carries no size,
// and no call writes more than the 36 planes of the largest tile.  HOST function (runs at weight-load time): w_khwc and u_out are
// host pointers.
extern "C" int msocr_winograd_weights_host(int form, const float* w_khwc, int Cout, int Cin, float* u_out) {
  if (form < MSOCR_WINO_2X2 || form > MSOCR_WINO_4X4_COLTAIL || !w_khwc || !u_out || Cout <= 0 || Cin <= 0) return MSOCR_E_ARG;
  const int PH = kWinoTile[form][0] + 2, PW = form == MSOCR_WINO_4X4_COLTAIL ? 1 + 2 : kWinoTile[form][1] + 2;  // the tail tile is 4 x 1
  const double(*Gh)[3] = wino_g(PH);
  const double(*Gw)[3] = wino_g(PW);
  const long plane = (long)Cout * Cin;
  for (int co = 0; co < Cout; ++co) {
    const float* w = w_khwc + (long)co * 9 * Cin;
    for (int c = 0; c < Cin; ++c) {
      double gw[6][3];  // Gh g
      for (int xi = 0; xi < PH; ++xi)
        for (int kw = 0; kw < 3; ++kw)
          gw[xi][kw] = Gh[xi][0] * w[(0 * 3 + kw) * Cin + c] + Gh[xi][1] * w[(1 * 3 + kw) * Cin + c] + Gh[xi][2] * w[(2 * 3 + kw) * Cin + c];
      for (int xi = 0; xi < PH; ++xi)
        for (int nu = 0; nu < PW; ++nu)
          u_out[(xi * PW + nu) * plane + (long)co * Cin + c] =
              (float)(gw[xi][0] * Gw[nu][0] + gw[xi][1] * Gw[nu][1] + gw[xi][2] * Gw[nu][2]);
    }
  }
  return MSOCR_OK;
}
