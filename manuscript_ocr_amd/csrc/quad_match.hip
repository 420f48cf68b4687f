// quad_match.hip — msocr_quad_match: greedy one-to-one matching of predicted to ground-truth quads by fp64 IoU, per page and per IoU
// threshold (include/msocr.h, "detection quality").  The geometry and the host twin are csrc/quad_iou.h.
//
// Three kernels (the first only zeroes the candidate counters; every node of a captured call is a kernel):
//   pair phase   one thread per (prediction, ground truth) pair over QM_TILE x QM_TILE tiles of one page.  A workgroup stages the
//                canonical f64 quads, boxes and validity of its two tiles in LDS; a thread holds one ground truth in registers and
//                walks QM_TILE / 4 predictions.  The box shortcut comes first, the register-resident clip runs for the survivors, and
//                every IoU > 0 is appended to its prediction's candidate list (QM_CAND_CAP slots and a counter per prediction).
//   match phase  one wave (a workgroup of its own) per page and threshold.  A wave walks the predictions in order, 64 at a time:
//                invalid ones and those without a candidate are settled by their lanes at once; for each of the others the wave gathers the
//                candidates, drops the ground truths already used at its threshold (a bitmap in LDS), and reduces to the best one
//                under the total order (IoU descending, j ascending), which restates the reference's ascending scan with a strict
//                ">" whatever order the pair phase appended in.  A prediction whose counter passed QM_CAND_CAP is recomputed by the
//                wave against every ground truth of the page with the same functions: the result does not depend on the cap.
#include "internal.h"
#include "quad_iou.h"

namespace {

constexpr int QM_TILE = 64;        // predictions and ground truths per workgroup of the pair phase
constexpr int QM_PAIR_T = 256;     // its threads: 64 ground truths x 4 prediction rows
constexpr int QM_CAND_CAP = 8;     // candidate slots per prediction; a row with more takes the recompute path of the match phase

struct QmThresholds {
  double t[MSOCR_QM_MAX_T];
};

struct QmWs {
  double* cand_iou;   // [N][max_pred][QM_CAND_CAP]
  int32_t* cand_j;    // [N][max_pred][QM_CAND_CAP]
  int32_t* cand_n;    // [N][max_pred] offers made (may exceed the cap)
  int64_t bytes;
};
inline QmWs qm_ws(void* base, int N, int max_pred) {
  const int64_t rows = (int64_t)N * max_pred;
  char* p = (char*)base;
  QmWs w;
  w.cand_iou = (double*)p;
  w.cand_j = (int32_t*)(p + rows * QM_CAND_CAP * 8);
  w.cand_n = (int32_t*)(p + rows * QM_CAND_CAP * 12);
  w.bytes = rows * (QM_CAND_CAP * 12 + 4) + 16;
  return w;
}

__device__ __forceinline__ int qm_clamp_count(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

struct QmStaged {  // one quad of a tile in LDS
  double v[8];
  QiBox box;
  int valid;
};

__device__ __forceinline__ void qm_stage(QmStaged& s, const float* q, bool present) {
  s.valid = 0;
  if (present && qi_canonical(q, s.v)) {
    s.valid = 1;
    s.box = qi_box(s.v);
  }
}

__global__ __launch_bounds__(256) void quad_zero_kernel(int32_t* __restrict__ cand_n, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) cand_n[i] = 0;
}

__global__ __launch_bounds__(QM_PAIR_T) void quad_pair_kernel(const float* __restrict__ pred, const int32_t* __restrict__ n_pred, int max_pred,
                                                              const float* __restrict__ gt, const int32_t* __restrict__ n_gt, int max_gt,
                                                              QmWs ws) {
  const int p = blockIdx.x;
  const int np = qm_clamp_count(n_pred[p], max_pred), ng = qm_clamp_count(n_gt[p], max_gt);
  const int i0 = blockIdx.y * QM_TILE, j0 = blockIdx.z * QM_TILE;
  if (i0 >= np || j0 >= ng) return;  // uniform over the workgroup
  __shared__ QmStaged sp[QM_TILE], sg[QM_TILE];
  const int tid = threadIdx.x;
  if (tid < QM_TILE) {
    const int i = i0 + tid;
    qm_stage(sp[tid], pred + ((size_t)p * max_pred + (i < np ? i : 0)) * 8, i < np);
  } else if (tid < 2 * QM_TILE) {
    const int j = j0 + tid - QM_TILE;
    qm_stage(sg[tid - QM_TILE], gt + ((size_t)p * max_gt + (j < ng ? j : 0)) * 8, j < ng);
  }
  __syncthreads();
  const int gl = tid & (QM_TILE - 1);
  if (!sg[gl].valid) return;
  double g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = sg[gl].v[k];
  const QiBox gb = sg[gl].box;
  for (int r = tid / QM_TILE; r < QM_TILE; r += QM_PAIR_T / QM_TILE) {
    const QmStaged& s = sp[r];  // the same for every lane of the wave: an LDS broadcast
    if (!s.valid) continue;
    if (qi_far_apart(s.box, gb)) continue;
    double iou;
    if (!qi_polygon_iou_fast(s.v, g, &iou)) iou = qi_polygon_iou_general(s.v, g);
    if (iou > 0) {
      const size_t row = (size_t)p * max_pred + i0 + r;
      const int slot = atomicAdd(&ws.cand_n[row], 1);
      if (slot < QM_CAND_CAP) {
        ws.cand_iou[row * QM_CAND_CAP + slot] = iou;
        ws.cand_j[row * QM_CAND_CAP + slot] = j0 + gl;
      }
    }
  }
}

// the wave's best offer under (IoU descending, j ascending); every lane returns it
__device__ __forceinline__ void qm_wave_best(double& iou, int& j) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double oi = __shfl_xor(iou, m, 64);
    const int oj = __shfl_xor(j, m, 64);
    if (oj >= 0 && qi_better(oi, oj, iou, j)) {
      iou = oi;
      j = oj;
    }
  }
}

__global__ __launch_bounds__(64) void quad_match_kernel(const float* __restrict__ pred, const int32_t* __restrict__ n_pred, int max_pred,
                                                        const float* __restrict__ gt, const int32_t* __restrict__ n_gt, int max_gt,
                                                        QmThresholds thr, int T, QmWs ws, int32_t* __restrict__ match_out,
                                                        double* __restrict__ iou_out, int32_t* __restrict__ counts_out) {
  extern __shared__ uint32_t qm_used[];  // [words]: ground truths taken at this threshold
  const int p = blockIdx.x;
  const int t = blockIdx.y, lane = threadIdx.x;
  const int np = qm_clamp_count(n_pred[p], max_pred), ng = qm_clamp_count(n_gt[p], max_gt);
  const int words = (max_gt + 31) >> 5;
  volatile uint32_t* used = qm_used;  // one wave: its LDS accesses complete in order, no barrier anywhere
  for (int w = lane; w < words; w += 64) used[w] = 0u;
  const double th = thr.t[t];
  const float* P = pred + (size_t)p * max_pred * 8;
  const float* Q = gt + (size_t)p * max_gt * 8;
  const size_t row0 = (size_t)p * max_pred;
  int32_t* mo = match_out + ((size_t)p * T + t) * max_pred;
  double* io = iou_out + ((size_t)p * T + t) * max_pred;
  int tp = 0, fp = 0;
  for (int i0 = 0; i0 < np; i0 += 64) {
    const int i = i0 + lane;
    bool valid = false;
    int offers = 0;
    if (i < np) {
      double v[8];
      valid = qi_canonical(P + (size_t)i * 8, v);
      offers = valid && ng > 0 ? ws.cand_n[row0 + i] : 0;  // a page without ground truth made no offer (and may have no counters)
      if (offers <= 0) {  // settled without looking at a ground truth
        mo[i] = valid ? -1 : -2;
        io[i] = 0.0;
      }
    }
    fp += __popcll(__ballot(i < np && offers <= 0));
    unsigned long long todo = __ballot(offers > 0);
    while (todo) {
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int ii = i0 + l;
      const int n = __shfl(offers, l, 64);
      double best_iou = 0.0;
      int bj = -1;
      if (n <= QM_CAND_CAP) {
        if (lane < n) {
          const double ci = ws.cand_iou[(row0 + ii) * QM_CAND_CAP + lane];
          const int cj = ws.cand_j[(row0 + ii) * QM_CAND_CAP + lane];
          if (cj >= 0 && cj < ng && !((used[cj >> 5] >> (cj & 31)) & 1u)) {
            best_iou = ci;
            bj = cj;
          }
        }
      } else {  // more offers than slots: this prediction against every ground truth of the page
        double v[8];
        qi_canonical(P + (size_t)ii * 8, v);
        const QiBox vb = qi_box(v);
        for (int j = lane; j < ng; j += 64) {
          if ((used[j >> 5] >> (j & 31)) & 1u) continue;
          double g[8];
          if (!qi_canonical(Q + (size_t)j * 8, g)) continue;
          const double iou = qi_iou(v, vb, g, qi_box(g));
          if (iou > 0 && qi_better(iou, j, best_iou, bj)) {
            best_iou = iou;
            bj = j;
          }
        }
      }
      qm_wave_best(best_iou, bj);
      const bool hit = bj >= 0 && best_iou >= th;
      if (hit) {
        ++tp;
        if (lane == 0) used[bj >> 5] = used[bj >> 5] | (1u << (bj & 31));
      } else {
        ++fp;
      }
      if (lane == 0) {
        mo[ii] = hit ? bj : -1;
        io[ii] = bj >= 0 ? best_iou : 0.0;
      }
    }
  }
  if (lane == 0) {
    int32_t* c = counts_out + ((size_t)p * T + t) * 3;
    c[0] = tp;
    c[1] = fp;
    c[2] = ng - tp;
  }
}

bool qm_pointers_ok(const void* pred, const void* n_pred, const void* gt, const void* n_gt, const void* match_out, const void* iou_out,
                    const void* counts_out) {
  return pred && n_pred && gt && n_gt && match_out && iou_out && counts_out;
}

}  // namespace

extern "C" int64_t msocr_quad_match_ws_bytes(int N, int max_pred, int max_gt) {
  if (N < 0 || max_pred < 0 || max_pred > MSOCR_QM_MAX_QUADS || max_gt < 0 || max_gt > MSOCR_QM_MAX_QUADS) return MSOCR_E_ARG;
  return qm_ws(nullptr, N, max_pred).bytes;
}

extern "C" int msocr_quad_match(const float* pred, const int32_t* n_pred, int max_pred, const float* gt, const int32_t* n_gt, int max_gt,
                                int N, const double* thresholds, int T, int32_t* match_out, double* iou_out, int32_t* counts_out,
                                void* workspace, void* stream) {
  if (!qm_pointers_ok(pred, n_pred, gt, n_gt, match_out, iou_out, counts_out) || !workspace) return MSOCR_E_ARG;
  if (!qm_shape_ok(N, max_pred, max_gt, thresholds, T)) return MSOCR_E_ARG;
  if (N == 0) return MSOCR_OK;
  const QmWs ws = qm_ws(workspace, N, max_pred);
  hipStream_t s = (hipStream_t)stream;
  QmThresholds thr;
  for (int t = 0; t < MSOCR_QM_MAX_T; ++t) thr.t[t] = t < T ? thresholds[t] : 1.0;
  const int tiles_p = (max_pred + QM_TILE - 1) / QM_TILE, tiles_g = (max_gt + QM_TILE - 1) / QM_TILE;
  if (tiles_p > 0 && tiles_g > 0) {
    const long rows = (long)N * max_pred;
    if ((rows + 255) / 256 > 0x7fffffffL) return MSOCR_E_ARG;
    MSOCR_LAUNCH(quad_zero_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, ws.cand_n, rows);
    int rc = LAUNCH_OK();
    if (rc != MSOCR_OK) return rc;
    MSOCR_LAUNCH(quad_pair_kernel, dim3(N, tiles_p, tiles_g), dim3(QM_PAIR_T), 0, s, pred, n_pred, max_pred, gt, n_gt, max_gt, ws);
    rc = LAUNCH_OK();
    if (rc != MSOCR_OK) return rc;
  }
  // with max_pred == 0 or max_gt == 0 the match phase reads no counter: no prediction, or every count clamped to "no ground truth"
  const int lds = ((max_gt + 31) / 32) * (int)sizeof(uint32_t);
  MSOCR_LAUNCH(quad_match_kernel, dim3(N, T), dim3(64), lds, s, pred, n_pred, max_pred, gt, n_gt, max_gt, thr, T, ws, match_out, iou_out,
               counts_out);
  return LAUNCH_OK();
}

extern "C" int msocr_quad_match_host(const float* pred, const int32_t* n_pred, int max_pred, const float* gt, const int32_t* n_gt,
                                     int max_gt, int N, const double* thresholds, int T, int32_t* match_out, double* iou_out,
                                     int32_t* counts_out) {
  if (!qm_pointers_ok(pred, n_pred, gt, n_gt, match_out, iou_out, counts_out)) return MSOCR_E_ARG;
  if (!qm_shape_ok(N, max_pred, max_gt, thresholds, T)) return MSOCR_E_ARG;
  for (int p = 0; p < N; ++p)
    if (n_pred[p] < 0 || n_pred[p] > max_pred || n_gt[p] < 0 || n_gt[p] > max_gt) return MSOCR_E_ARG;
  qm_match_host(pred, n_pred, max_pred, gt, n_gt, max_gt, N, thresholds, T, match_out, iou_out, counts_out);
  return MSOCR_OK;
}
