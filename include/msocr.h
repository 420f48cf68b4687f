/* msocr.h — C ABI of libmsocr.so, the MI355X (gfx950) hot path of manuscript-ocr.
 *
 * The reference (olegiy/manuscript-ocr) has no FFI: its boundary is the Python
 * plugin API (Pipeline / EAST / TRBA).  This header is the INNER native boundary
 * that the Python host in manuscript_ocr_amd/ binds with ctypes; every entry
 * point names the reference code it replaces (paths relative to
 * /root/reference/src/manuscript/).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and
 *     stream-ordered, allocates nothing and never synchronises (graph-capturable);
 *   - activations are NHWC; `dtype` selects the storage/MFMA input type
 *     (MSOCR_F32: v_mfma_f32_32x32x2_f32, exact f32; MSOCR_BF16:
 *     v_mfma_f32_32x32x16_bf16, f32 accumulate);
 *   - return value: 0 = ok, negative = MSOCR_E_* (nothing was launched).
 */
#ifndef MSOCR_H
#define MSOCR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSOCR_F32 0
#define MSOCR_BF16 1

#define MSOCR_OK 0
#define MSOCR_E_ARG (-1)     /* bad argument / unsupported shape */
#define MSOCR_E_LAUNCH (-2)  /* hipLaunch failed */
#define MSOCR_E_NOGPU (-3)

/* flags for msocr_conv2d */
#define MSOCR_CONV_RELU 1u
#define MSOCR_CONV_RESIDUAL 2u /* out = act(conv + bias + residual) */
#define MSOCR_CONV_POOL2 4u    /* msocr_*winograd_fused64* only: out = maxpool2x2/2(act(conv + bias)), out is [N][H/2][W/2] */

typedef struct msocr_conv_desc {
  int32_t dtype;                 /* MSOCR_F32 | MSOCR_BF16 (input, weight, residual, output) */
  int32_t N, H, W, Cin;          /* input extent; Cin = channels reduced per tap (multiple of 32 f32 / 32 bf16) */
  int64_t in_sN, in_sH, in_sW;   /* input strides in ELEMENTS (channel stride is 1) */
  int32_t KH, KW, stride_h, stride_w, pad_h, pad_w;
  int32_t Ho, Wo, Cout;          /* Cout multiple of 32 */
  int64_t out_ld;                /* elements between consecutive output pixels (>= Cout) */
  int64_t res_ld;                /* same for the residual tensor */
  uint32_t flags;
} msocr_conv_desc;

/* Implicit-GEMM convolution on MFMA: out[n,ho,wo,co] = act(sum_{kh,kw,c} in[n,ho*sh-ph+kh,wo*sw-pw+kw,c] *
 * w[co,kh,kw,c] + bias[co] (+ residual)).  weight layout [Cout][KH][KW][Cin] (dtype), bias f32 with BatchNorm
 * folded in by the host.  Replaces every nn.Conv2d+BatchNorm2d(+ReLU)(+add) of
 *   detectors/_east/east.py:13-30,56-67,96-105 (torchvision ResNet-50 Bottlenecks, DecoderBlock) and
 *   recognizers/_trba/model/seresnet31.py:37-45,81-89,129-136,150-155. */
int msocr_conv2d(const msocr_conv_desc* d, const void* in, const void* weight, const float* bias,
                 const void* residual, void* out, void* stream);

/* The same convolution for KH=KW=3, stride 1, pad 1, MSOCR_F32, as Winograd in one of four tile forms (`form`):
 *   MSOCR_WINO_2X2  F(2x2,3x3): 16 transform points per 2x2 output tile, 4 multiplies per output (direct: 9);
 *   MSOCR_WINO_4X2  the TALL form F(4,3) x F(2,3): 24 points per 4x2 tile, 3 multiplies per output, V / Mw 3x the layer's arrays;
 *   MSOCR_WINO_4X4  the square form F(4,3) x F(4,3): 36 points per 4x4 tile, 2.25 multiplies and workspace words per output;
 *   MSOCR_WINO_4X4_COLTAIL  the square form + tail column, for maps with W % 4 == 1 (W >= 5), without the 4X4 form's padded last tile:
 *                   output columns 0 ... W-2 are W/4 square tiles per tile row, bit for bit what the 4X4 form stores there; column W-1 is
 *                   one F(4,3) x F(1,3) tile per tile row (the 6-point transform along H, the three taps along W summed directly: 18
 *                   points).  36 * (W/4) + 18 point rows per tile row instead of 36 * (W/4 + 1).  The one form of two parts: one
 *                   transform launch per direction over the tiles of both, one batched GEMM launch per part.
 * The 6-point axes run on the interpolation points {0, +-3/2, +-2/3, inf} (round 4): the tall form at half the rounding error of the
 * textbook points {0, +-1, +-2}, the square form at the tall form's error on those (the textbook points would cost 4.7x; DESIGN.md
 * section 4.4).  Input transform (HBM-bound) -> P GEMMs [tiles x Cin] x [Cin x Cout] in one MFMA launch -> output transform +
 * bias/residual/ReLU (HBM-bound); all arithmetic f32 (differs from msocr_conv2d by rounding order only).
 * u = the transform-domain weight U = G g G^T on the DEVICE, from msocr_winograd_weights_host (a HOST function: both of its pointers
 * are host memory; evaluates G g G^T in f64, rounds once) of the BatchNorm-folded [Cout][3][3][Cin] weight, [P][Cout][Cin] f32
 * — one tile's planes per call.  4X4_COLTAIL: U is [54][Cout][Cin], the 4X4 form's 36 planes (that form's call), then the 18 of the
 * tail tile, which the call with this form gives: [18][Cout][Cin], U[xi*3+kw][co][c] = sum_kh G6[xi][kh] w[co][kh][kw][c].  The
 * output pointer carries no size; no call writes more than the 36 planes of the largest tile.
 *   split = 0: u as that f32 array, the GEMMs on exact-f32 MFMA;
 *   split = 1: u = K-tile-major bf16 planes [3][P][Cin/32][Cout][32] (msocr_split_bf16x3_ktile_host of it), the GEMMs with split
 *              operands on the bf16 matrix pipes (see msocr_conv1x1_split; Cin % 32 == 0, Cout % 64 == 0).
 *              4X4_COLTAIL: ONE buffer, the 4X4 form's planes [3][36][Cin/32][Cout][32] immediately followed by the tail tile's planes
 *              [3][18][Cin/32][Cout][32] (the second GEMM reads u + 3*36*Cout*Cin elements, 16-byte aligned as Cin % 32 == 0).  Each
 *              group keeps its own plane stride: the concatenation of the splits of U[0:36] and U[36:54], NOT the split of the
 *              [54][Cout][Cin] array as one.
 * GEMMs exist for 2X2 exact, 4X2 exact and split, and 4X4 and 4X4_COLTAIL split; any other (form, split) is MSOCR_E_ARG.
 * workspace: msocr_winograd_workspace_bytes(d, form) bytes, 16-B aligned, linear in N = V [P][tiles][Cin] f32 + Mw [P][tiles][Cout] f32;
 * 4X4_COLTAIL: V44 [36][Mt44][Cin] | Mw44 [36][Mt44][Cout] | V41 [18][Mt41][Cin] | Mw41 [18][Mt41][Cout], Mt44 = N ceil(H/4) (W/4),
 * Mt41 = N ceil(H/4)  (-1 = shape not supported: Cin % 16, Cout % 32, not 3x3/1/1; 4X4_COLTAIL also W % 4 != 1, W < 5, Cin % 32,
 * Cout % 64).  The three stages are also callable one by one (identical kernels, identical results when called in this order on
 * one stream with the same workspace): V = B^T d B into the workspace;
 * Mw[p] = V[p] U[p]^T; out = act(A^T Mw A + bias (+ residual)) — for tests and for the per-kernel rooflines of bench.py.
 * Same reference code as msocr_conv2d (every 3x3/1/1 conv of SE-ResNet31, ResNet-50 and the EAST decoder). */
#define MSOCR_WINO_2X2 0
#define MSOCR_WINO_4X2 1
#define MSOCR_WINO_4X4 2
#define MSOCR_WINO_4X4_COLTAIL 3
int64_t msocr_winograd_workspace_bytes(const msocr_conv_desc* d, int form);
int msocr_winograd_weights_host(int form, const float* w_khwc_host, int Cout, int Cin, float* u_out_host);
int msocr_conv3x3_winograd(const msocr_conv_desc* d, int form, int split, const void* in, const void* u, const float* bias,
                           const void* residual, void* out, void* workspace, void* stream);
int msocr_winograd_input_transform(const msocr_conv_desc* d, int form, const void* in, void* workspace, void* stream);
int msocr_winograd_gemm(const msocr_conv_desc* d, int form, int split, const void* u, void* workspace, void* stream);
int msocr_winograd_output_transform(const msocr_conv_desc* d, int form, const void* workspace, const float* bias, const void* residual,
                                    void* out, void* stream);

/* Per-crop forms of the output transform for the SE blocks of SE-ResNet31 (seresnet31.py:37-66), forms 4X4 and 4X4_COLTAIL, where
 * one image's map [H][W][Cout] f32 fits the LDS of a CU: one workgroup per image transforms its rows of Mw into LDS and goes on
 * from there, so the map makes no round trip through HBM.  Same arithmetic in the same order as the calls they replace: bit-identical.
 *   msocr_winograd_crop_lds_bytes: the dynamic LDS such a kernel takes for d's layer (se != 0: with the SE tail's scratch), or -1 where
 *     it does not apply: another form, more than 160 KB, Cin != Cout (chain), Cout not a power of two in [64, 1024] or out_ld != Cout (se).
 *   msocr_winograd_output_chain: conv1 -> conv2.  act(A^T Mw A + bias) of d's layer (flags: ReLU), then the INPUT transform of a
 *     following 3x3/1/1 layer of the same shape (Cin == Cout), written over V of the same workspace (dead since d's GEMM):
 *     msocr_winograd_gemm of that layer comes next.  Replaces msocr_winograd_output_transform + msocr_winograd_input_transform.
 *   msocr_winograd_output_se: conv2 -> SE tail.  x = A^T Mw A + bias (no flags), then msocr_se_residual on it:
 *     out = relu(x * sigmoid(W2 relu(W1 mean_hw(x))) + identity); identity and out [N][H][W][Cout] dense, gate_ws [N][Cout] f32. */
int64_t msocr_winograd_crop_lds_bytes(const msocr_conv_desc* d, int form, int se);
int msocr_winograd_output_chain(const msocr_conv_desc* d, int form, void* workspace, const float* bias, void* stream);
int msocr_winograd_output_se(const msocr_conv_desc* d, int form, const void* workspace, const float* bias, const void* identity,
                             const float* w1, const float* w2, float* gate_ws, void* out, void* stream);

/* ---- split-operand f32 ("bf16x3"): the default arithmetic of the f32 1x1 convolutions and Winograd-domain GEMMs --------------
 * gfx950 runs exact-f32 MFMA at 1/16 of the bf16 rate.  An f32 value is the exact sum of three bf16 values (round-to-nearest
 * residual chain); of the nine cross products of two such sums the six largest are accumulated in f32 on the bf16 matrix pipes,
 * the three dropped ones are <= 2^-25 of the product (below the rounding of the f32 accumulation itself).  The activation operand
 * is split in registers inside the kernel; the WEIGHT operand is split once at load time:
 *   msocr_split_bf16x3_host(w, n, planes)   HOST: w [n] f32 -> planes [3][n] bf16 (uint16), w == p0 + p1 + p2 exactly.
 *   msocr_split_bf16x3_ktile_host(w, nb, rows, k, planes)   HOST: the same split of w [nb][rows][k] (k % 32 == 0) written
 *     K-TILE-MAJOR, planes [3][nb][k/32][rows][32]: the 32-element pieces of all rows for one K-tile are contiguous (64 bytes per row),
 *     so a workgroup's weight tile of one K-tile is ONE dense block — whole 128-byte lines, every byte used.  (Row-major planes
 *     gave 64-byte pieces at a stride of 2 k bytes: half of every fetched line belonged to the NEXT K-tile and was fetched again —
 *     TCP -> L2 read requests 2x the algorithmic count, profiles/r04_pp_ablations.txt.)  This is the layout the two GEMM entry
 *     points below and msocr_winograd_gemm with split = 1 take ("weight_planes" / "u"; k = KH * KW * Cin in the weight's own
 *     [KH][KW][Cin] order).
 * msocr_conv1x1_split: msocr_conv2d for KH = KW = 1 / stride 1 / no padding / MSOCR_F32 over a dense pixel sequence
 *   (in_sH == W * in_sW, in_sN == H * in_sH), Cin % 32 == 0, Cout % 64 == 0; weight_planes = K-tile-major planes of [1][Cout][Cin] on the device.
 *   Same flags, epilogue and reference layers as msocr_conv2d (torchvision Bottleneck conv1 / conv3 / downsample, DecoderBlock
 *   conv1x1, SEBasicBlock downsample, the BiLSTM input projections and linears).
 * msocr_conv2d_split: msocr_conv2d for MSOCR_F32 with any kernel size / stride / padding (the strided 3x3 and 1x1 convolutions of
 *   the two ResNet trunks, which have no Winograd form), weight_planes = K-tile-major planes of [1][Cout][KH*KW*Cin]; Cin % 32 == 0, Cout % 64 == 0.
 * msocr_conv3x3_winograd with split = 1: the Winograd-domain GEMMs in this arithmetic.
 * Results differ from the exact-f32 entry points by rounding only (tests/test_gpu_ops.py bounds both against an f64 reference). */
int msocr_split_bf16x3_host(const float* w_host, int64_t n, uint16_t* planes_out_host);
int msocr_split_bf16x3_ktile_host(const float* w_host, int64_t nbatch, int64_t rows, int64_t k, uint16_t* planes_out_host);
int msocr_conv1x1_split(const msocr_conv_desc* d, const void* in, const void* weight_planes, const float* bias,
                        const void* residual, void* out, void* stream);
int msocr_conv2d_split(const msocr_conv_desc* d, const void* in, const void* weight_planes, const float* bias,
                       const void* residual, void* out, void* stream);

/* Cin == 64: the tall form (MSOCR_WINO_4X2) with the 24 transform-domain GEMMs (K = 64) and the output transform fused in one
 * kernel, so Mw never reaches HBM (unfused, a 64-channel layer is HBM-bound on Mw).  workspace holds V only
 * (msocr_winograd_fused64_workspace_bytes; -1 = unsupported: Cin != 64, Cout % 32, or POOL2 with odd H / W or a residual).
 * split = 0: u = [24][Cout][64] f32 from msocr_winograd_weights_host(MSOCR_WINO_4X2, ...); split = 1: u = its three bf16 planes
 * [3][24][Cout][64] (msocr_split_bf16x3_host), the GEMMs in the split-operand arithmetic (see msocr_conv1x1_split).
 * With MSOCR_CONV_POOL2 in d->flags the kernel also applies the 2x2 / stride-2 max-pool that closes conv0 of SE-ResNet31
 * (recognizers/_trba/model/seresnet31.py:81-89: conv3x3 64->128, BN, ReLU, MaxPool2d(2, 2)) and writes the pooled
 * [N][H/2][W/2][Cout] map (d->out_ld = its channel stride).  msocr_winograd_fused64_gemm_output is stage 2 alone (stage 1 =
 * msocr_winograd_input_transform(d, MSOCR_WINO_4X2, ...) into the same workspace). */
int64_t msocr_winograd_fused64_workspace_bytes(const msocr_conv_desc* d);
int msocr_conv3x3_winograd_fused64(const msocr_conv_desc* d, int split, const void* in, const void* u, const float* bias,
                                   const void* residual, void* out, void* workspace, void* stream);
int msocr_winograd_fused64_gemm_output(const msocr_conv_desc* d, int split, const void* u, const void* workspace, const float* bias,
                                       const void* residual, void* out, void* stream);

/* u8 RGB images (N x H x W x 3) -> normalised NHWC with C padded 3->cpad (4 or 8) inside a zero canvas
 * out[N][Hp][Wp][cpad], image origin at (pad_t, pad_l); the zero border is the stem convolution's padding.
 *   mode 0: EAST ToTensor+Normalize, detectors/_east/infer.py:127-132,305  -> (x/255 - .5)/.5
 *   mode 1: TRBA A.Normalize(.5,.5,max 255), recognizers/_trba/data/transforms.py:185-193 -> (x-127.5)*f32(1/127.5) */
int msocr_normalize_u8(const uint8_t* src, int N, int H, int W, int pad_t, int pad_l, int Hp, int Wp, int cpad,
                       int mode, int dtype, void* out, void* stream);

/* cv2.resize(img,(dw,dh)) INTER_LINEAR for u8 HxWx3 (OpenCV 11-bit fixed point), batched.
 * Replaces detectors/_east/infer.py:304 (restated from OpenCV, parity unpinned). */
int msocr_resize_linear_u8(const uint8_t* src, int N, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream);

/* MaxPool2d(k, stride=s, padding=p) on NHWC.  (torchvision resnet maxpool 3/2/1; seresnet31.py:88 2/2/0)
 * As torch: 2p <= k, a NaN in a window gives NaN.  in_ld, out_ld >= C: pixel strides in elements. */
int msocr_maxpool2d(const void* in, int N, int H, int W, int C, int64_t in_ld, int k, int s, int p, int dtype,
                    void* out, int Ho, int Wo, int64_t out_ld, void* stream);

/* F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) written into the first C channels of a
 * concat buffer (out_ld >= C): fuses the torch.cat of detectors/_east/east.py:87-92. */
int msocr_upsample2x_bilinear(const void* in, int N, int H, int W, int C, int64_t in_ld, int dtype, void* out,
                              int64_t out_ld, void* stream);

/* OutputHead (east.py:96-105): score = sigmoid(w_s . x + b_s), geo = W_g x + b_g from the 32-channel h1.
 * w9 = [9][32] f32 (row 0 score, rows 1..8 geo), b9 = [9] f32.  score_out [N][H][W] f32, geo_out [N][H][W][8] f32.
 * h1 is read and geo_out written by 16-byte vectors: h1 and geo_out 16-byte aligned, in_ld a multiple of 4 (f32) / 8 (bf16). */
int msocr_east_head(const void* h1, int64_t npix, int64_t in_ld, int dtype, const float* w9, const float* b9,
                    float* score_out, float* geo_out, void* stream);

/* decode_quads_from_maps (detectors/_east/utils.py:328-381), batched over pages: threshold (strict >),
 * quantise to q x q cells, unique in (y,x) order, decode 4 vertices + score at the cell centre.
 * cand_out [N][max_cand][9] f32, count_out [N] int32 (clamped to max_cand; overflow flag in bit 31). */
int msocr_east_decode(const float* score, const float* geo, int N, int H, int W, float thresh, float scale,
                      int quant, float* cand_out, int32_t* count_out, int max_cand, void* stream);

/* locality_aware_nms (detectors/_east/lanms.py:156-207 incl. standard_nms :133-153 and the fp64 geometry :7-130),
 * batched over pages.  cand [N][max_cand][9] f32 + counts from msocr_east_decode; boxes_out [N][max_cand][9] f32,
 * nbox_out [N] int32.  workspace: msocr_lanms_workspace_bytes(N, max_cand) bytes. */
int64_t msocr_lanms_workspace_bytes(int N, int max_cand);
int msocr_east_lanms(const float* cand, const int32_t* counts, int N, int max_cand, double iou_thr, float* boxes_out,
                     int32_t* nbox_out, void* workspace, void* stream);

/* The box filters of EAST.predict after the NMS (infer.py:340-356): expand_boxes (utils.py:384-422), scale to the original
 * page (infer.py:134-147), removal of fully contained boxes (infer.py:174-214, cv2.pointPolygonTest restated), area anomalies
 * (infer.py:216-233, np.mean / np.std with NumPy's f32 pairwise summation) and axis-aligned conversion (infer.py:149-172), with
 * NumPy's f32 operation order: bit-identical to the host implementation.  expand_w/h, scale_x = orig_w / target_w,
 * scale_y = orig_h / target_h and sigma are the Python floats of the reference (rounded to f32 where NumPy does).
 * msocr_east_box_tail: one workgroup per page on boxes [N][max_cand][9] / nbox [N] from msocr_east_lanms ->
 * out [N][max_cand][9], n_out [N] (-1 for a page with more than min(max_cand, 16384) boxes: use the host path; pages above
 * 2048 boxes keep their per-box arrays in the workspace instead of LDS); workspace:
 * msocr_east_box_tail_workspace_bytes(N, max_cand) bytes.
 * msocr_east_box_tail_host: HOST twin running the same code on the CPU (quads_host [M][9] -> out_host [<=M][9], *n_out_host). */
int64_t msocr_east_box_tail_workspace_bytes(int N, int max_cand);
int msocr_east_box_tail(const float* boxes, const int32_t* nbox, int N, int max_cand, double expand_w, double expand_h,
                        double scale_x, double scale_y, int axis_aligned_output, int remove_anomalies, double sigma, int min_count,
                        float* out, int32_t* n_out, void* workspace, void* stream);
int msocr_east_box_tail_host(const float* quads_host, int M, double expand_w, double expand_h, double scale_x, double scale_y,
                             int axis_aligned_output, int remove_anomalies, double sigma, int min_count, float* out_host,
                             int32_t* n_out_host);

/* ---- TRBA ---------------------------------------------------------------------------------------------- */

/* SELayer (recognizers/_trba/model/seresnet31.py:5-20) fused with the residual tail of SEBasicBlock.forward
 * (:61-66): out = relu(x * sigmoid(W2 relu(W1 mean_hw(x))) + identity).  x, identity, out: [N][HW][C] (ld = C).
 * w1 [C/16][C] f32, w2 [C][C/16] f32.  gate_ws: [N][C] f32 scratch. */
int msocr_se_residual(const void* x, const void* identity, int N, int HW, int C, int dtype, const float* w1,
                      const float* w2, float* gate_ws, void* out, void* stream);

/* AdaptiveAvgPool2d((1,None)) + squeeze + permute (recognizers/_trba/model/model.py:388-390):
 * [N][H][W][C] (dtype) -> [N][W][C] f32. */
int msocr_mean_over_h(const void* in, int N, int H, int W, int C, int dtype, float* out, void* stream);

/* One bidirectional LSTM layer + Linear (BidirectionalLSTM.forward, model/model.py:9-21).
 * xproj [B][T][2][4H] f32 = x W_ih^T + b_ih + b_hh for both directions (an msocr_conv2d 1x1 / GEMM);
 * w_hh_t [2][H][H][4] f32 = weight_hh^T with the 4 gates (i,f,g,o) of unit j interleaved: [dir][k][j][gate];
 * hcat_out [B][T][2H] f32. */
int msocr_bilstm_recurrent(const float* xproj, const float* w_hh_t, int B, int T, int H, float* hcat_out,
                           void* stream);
/* The same recurrence (H == 256) with the step's product h W_hh^T on the bf16 matrix pipes in the split-operand form, 32 crops per
 * workgroup (csrc/bilstm_mfma.hip).  whh_planes (device): two blocks (forward, reverse) of msocr_attn_pack_split_elems(4 H)
 * uint16 each, packed on the host by msocr_attn_pack_split_host(w_hh_t + dir * H * 4 H, 4 H, 1, .). */
int msocr_bilstm_recurrent_split(const float* xproj, const uint16_t* whh_planes, int B, int T, int H, float* hcat_out,
                                 void* stream);

typedef struct msocr_attn_weights {
  const float* h2h_wt;   /* [H][H]   h2h.weight^T */
  const float* h2h_b;    /* [H] */
  const float* score_w;  /* [H] */
  const float* wih_ctx_t;/* [H][H][4]  rnn.weight_ih[:, :H]^T, gates of unit j interleaved: [k][j][gate] */
  const float* wih_tok;  /* [V][H][4]  rnn.weight_ih[:, H:]^T (one-hot matmul == row gather): [token][j][gate] */
  const float* whh_t;    /* [H][H][4]  rnn.weight_hh^T: [k][j][gate] */
  const float* b_gates;  /* [H][4]     b_ih + b_hh: [j][gate] */
  const float* gen_wt;   /* [H][V]  generator.weight^T */
  const float* gen_b;    /* [V] */
} msocr_attn_weights;

/* Attention decode (model/model.py:34-46 cell, :227-259 greedy, :92-225 beam): the whole step loop in ONE launch
 * (rows are independent).  batch_H, proj_H: [B][T][H] f32 with proj_H = i2h(batch_H) hoisted out of the loop (the
 * reference recomputes it every step); H a multiple of 64 in 64..512, V <= 512, T <= 64, steps <= 64, beam <= 16
 * with beam * H <= 4096.  Every decode is one call, msocr_attn_decode, of a descriptor (msocr_attn_desc, below the two beam
 * options); this comment and the ones that follow say what the modes and options compute.
 * Kernel family: ctx_gates == NULL runs the general kernels (csrc/attn_general.hip, one workgroup per batch row, exact f32) for
 * every shape of the envelope.  ctx_gates given runs the matrix-core kernels (csrc/attn_beam_mfma.hip: greedy and forced 32 crops
 * per workgroup, beam 4 rows x 8 beams) with the context half of the LSTMCell input product hoisted out of the step loop:
 * H == 256, V <= 256, T <= 48, beam <= 8, other shapes MSOCR_E_ARG.  ctx_gates [B][T][H][4] f32 = batch_H x
 * rnn.weight_ih[:, :H]^T with the four gates of a unit adjacent (row j*4+g of the product), computed once per call by a GEMM
 * (msocr_conv1x1_split), 16-byte aligned.  W_ih[:, :H] (sum_t alpha_t batch_H_t) == sum_t alpha_t (W_ih[:, :H] batch_H_t): same
 * result up to f32 summation order, half the matrix work per step.  ws (msocr_attn_split_weights) given: the split-operand
 * products; ws == NULL: exact-f32 MFMA in beam mode, MSOCR_E_ARG in greedy and forced mode.
 * greedy (Attention._greedy_decode, model.py:227-259): steps = max_len+1; logits_out [B][steps][V] f32, ids_out [B][steps] i32 for
 *         ALL steps.
 * beam  : steps = max_len; per step the kernel stores every beam's temperature-scaled logits, back-pointers,
 *         tokens and the arg-max beam into `workspace`, and fin_step_out[b] = number of steps after which every
 *         beam of row b is finished (or steps).  lp[steps] = f32 length-penalty factors
 *         ((5+t+1)^alpha / 6^alpha, computed by the host exactly as model.py:160) or NULL when alpha <= 0.
 *         Optional early exit (all three pointers non-NULL): chunk_id[B] = index of the reference chunk (the slice of
 *         batch_size crops one model call sees) of every row, chunk_size[nchunks] = rows per chunk, all of them inside
 *         this call; chunk_state[2*nchunks] int32 zeroed by the caller.  The matrix-core kernel
 *         then leaves the step loop once every chunk its rows belong to is completely finished (model.py:215), so steps >=
 *         the chunk's run length are skipped; the general kernel runs every step (same outputs for t < the run length).
 * The reference stops the loop for the whole batch chunk (model.py:215,254); the host derives each row's run length
 * t_run from ids/fin_step and msocr_attn_beam_finalize walks the back-pointers from (t_run-1, best beam at t_run-1):
 * logits_out [B][steps][V] (rows t < t_run valid), ids_out [B][steps] (-1 beyond t_run).
 * Attention weights (the softmax over the encoder frames that AttentionCell.forward returns, model.py:40-46, and its callers
 * drop): alpha_out keeps them for every step; every other output is bit-identical with it on or off, and the beam workspace
 * layout is unchanged.
 * greedy: alpha_out [B][steps][T] f32, every step written.
 * beam  : alpha_out is a workspace of its own, [B][steps][beam][T] f32 (msocr_attn_beam_alpha_bytes; 16-byte aligned), slot-
 *         indexed exactly like the logits trace: the weights of step s at slot k belong to the hypothesis that occupies slot k
 *         WHEN step s is computed, the one whose logits are stored at [b][s][k].  Steps skipped by the chunk early exit are not
 *         written.  Given that trace as alpha_ws (with T as in the decode, and alpha_out [B][steps][T]) the finalize step also
 *         gathers the best path's weights, alpha_out[b][t][:] = alpha_ws[b][t][path[t]][:] for t < t_run, and writes zeros for
 *         t >= t_run; alpha_ws NULL, T 0, alpha_out NULL: off. */
int64_t msocr_attn_beam_workspace_bytes(int B, int steps, int beam, int V);
int64_t msocr_attn_beam_alpha_bytes(int B, int steps, int beam, int T);
int msocr_attn_beam_finalize(const void* workspace, int B, int V, int steps, int beam, const int32_t* trun_dev, float* logits_out,
                             int32_t* ids_out, const void* alpha_ws, int T, float* alpha_out, void* stream);
/* Optional split form of the three per-step weight matrices (device pointers, each packed by msocr_attn_pack_split_host and
 * copied to the device by the caller): with it the matrix-core kernel forms every f32 product from three bf16 terms per
 * operand on the bf16 matrix pipe (six partial products, f32 accumulation: f32 result up to 2^-25 relative per product and the
 * order of summation) instead of the 1/16-rate exact-f32 MFMA.  NULL = exact-f32 products. */
typedef struct msocr_attn_split_weights {
  const uint16_t* h2h_p;  /* from h2h_wt, N = H */
  const uint16_t* whh_p;  /* from whh_t,  N = 4 H, gate_interleaved */
  const uint16_t* gen_p;  /* from gen_wt, N = V */
} msocr_attn_split_weights;
/* Packing of a decoder weight for the fields of msocr_attn_split_weights; HOST memory in and out.  wt: [256][N] f32 row-major (h2h_wt,
 * gen_wt) or, with gate_interleaved != 0, [256][N/4][4] (whh_t).  out: msocr_attn_pack_split_elems(N) = 3 * 256 * ceil32(N)
 * uint16 (bf16 bit patterns), laid out [plane][k / 16][column][k % 16] with wt == plane0 + plane1 + plane2 exactly. */
int64_t msocr_attn_pack_split_elems(int N);
int msocr_attn_pack_split_host(const float* wt_host, int N, int gate_interleaved, uint16_t* out_host);

/* Recognition confidence (recognizers/_trba/__init__.py:413-431): mean over the t_run generated positions of
 * exp(log_softmax(logits)[id]).  logits [B][steps][V] f32, ids [B][steps] i32 (must be valid for t < trun[b]),
 * trun_dev [B] i32 -> conf_out [B] f32 (0 when t_run == 0). */
int msocr_seq_confidence(const float* logits, const int32_t* ids, const int32_t* trun_dev, int B, int V, int steps,
                         float* conf_out, void* stream);

/* Per-symbol details of a decoded batch, all [B][steps]: prob_out = exp(log_softmax(logits[b][t])[ids[b][t]]) (the quantity whose
 * mean over t < t_run is the confidence above), centre_out = sum_j alpha[b][t][j] * (j + 0.5) in encoder frames, peak_out =
 * the arg-max frame (int32, the smaller index on ties).  Entries t >= trun[b]: 0, 0 and -1.  alpha [B][steps][T] f32 from the
 * decodes' alpha_out, T <= 64; everything stays on the device. */
int msocr_seq_char_details(const float* logits, const int32_t* ids, const float* alpha, const int32_t* trun_dev, int B, int V,
                           int steps, int T, float* prob_out, float* centre_out, int32_t* peak_out, void* stream);

/* N-best readings: the final hypotheses of a row's beam search, read out of the workspace a beam decode left behind (any of the
 * beam decodes; the decode itself is untouched).  The workspace is logits [B][steps][beam][V] f32 | back
 * [B][steps][beam] i32 | tokv [B][steps][beam] i32 | best_at [B][steps] i32, and the beam kernels fill the slots of every step in
 * rank order (best score first), so the r-th best hypothesis of a row is the back-trace from slot r of step t_run-1.
 * Rank rule: rank 0 is the slot best_at[b][t_run-1] — the walk of msocr_attn_beam_finalize, the same ids — and ranks 1 .. n_best-1
 * are the remaining slots in slot order.  Outputs, for b < B and r < n_best <= beam:
 *   ids_out  [B][n_best][steps] i32: the path's tokens, -1 for t >= t_run;
 *   prob_out [B][n_best][steps] f32: exp(log_softmax(logits[b][t][parent slot])[token]) of every step, 0 for t >= t_run;
 *   conf_out [B][n_best] f32: the mean of prob over t < t_run, summed in f32 in step order: for rank 0 bit-equal to
 *            msocr_seq_confidence of the finalized path;
 *   logp_out [B][n_best] f32: the hypothesis's summed log-probability, the score the search ranks by (before the length penalty):
 *            log_softmax(...)[token] over the steps up to and including the path's first eos_id (later steps add 0, as the search
 *            extends a finished hypothesis), accumulated in f64 in step order and rounded once.
 * V <= 512, steps <= 64, beam <= 16, 1 <= n_best <= beam, otherwise MSOCR_E_ARG.  trun_dev [B] i32 as for the finalize step; a value
 * outside [1, steps] is clamped into it.  The _host twin takes host copies of the workspace and of t_run and writes host arrays:
 * the same walk and the same order of every sum; ids equal the device's, floats up to expf / logf of the host's libm. */
int msocr_attn_beam_nbest(const void* workspace, int B, int V, int steps, int beam, int n_best, int eos_id, const int32_t* trun_dev,
                          int32_t* ids_out, float* prob_out, float* conf_out, float* logp_out, void* stream);
int msocr_attn_beam_nbest_host(const void* workspace_host, int B, int V, int steps, int beam, int n_best, int eos_id,
                               const int32_t* trun_host, int32_t* ids_out_host, float* prob_out_host, float* conf_out_host,
                               float* logp_out_host);

/* Forced (teacher-forced) decode: score and align a GIVEN transcription.  Attention.forward(is_train=True) of the reference
 * (model.py:287-320) with sampling_prob 0 in eval(): step s is fed tok_in[b][s] (i32 [B][steps]: column 0 = sos_id, then the
 * transcription's ids, the layout of the reference's pack_attention_targets, data/transforms.py:123-157) instead of the arg-max of
 * step s-1, and the logits of every step are returned with the attention weights: logits_out [B][steps][V] f32 (blank_id masked to
 * -1e4 as in the greedy decode; -1 = no blank), alpha_out [B][steps][T] f32 (required).  Every step of every row is written; no ids
 * are. A row fed the ids of a greedy decode with alpha_out reproduces that decode's logits and weights bit for bit.  An id outside
 * [0, V) is replaced by sos_id inside the kernel before it is used as an index (callers who want an error check their ids first:
 * msocr_seq_logp reports such an id as NaN).  Forced mode of msocr_attn_decode; the kernel families and their shapes are the greedy
 * decode's (csrc/attn_general_forced.hip, csrc/attn_forced_mfma.hip). */

/* Log-probability of given ids under a decode's logits: logp_steps_out [B][steps] f32 = log_softmax(logits[b][t] / temperature)[ids[b][t]]
 * in f32 with max subtraction (a true f32 division, skipped when temperature == 1) for t < trun[b] and 0 behind; logp_out [B] f32 =
 * their sum over t < trun[b], accumulated in f64 in step order and rounded once (the convention of msocr_attn_beam_nbest's logp_out).
 * With ids = the targets of a forced decode (the transcription's ids, then EOS) and trun = length + 1 this is the summed
 * log-probability of the transcription including its EOS.  An id outside [0, V) at a step t < trun[b] makes that step's value and
 * the row's sum NaN; nothing is read through it.  trun is clamped into [0, steps].  V <= 512, steps <= 64, otherwise MSOCR_E_ARG.
 * The _host twin takes host arrays: the same lane partials, the same order of every sum; it differs from the device by what
 * expf / logf differ between the device and the host's libm. */
int msocr_seq_logp(const float* logits, const int32_t* ids, const int32_t* trun_dev, int B, int V, int steps, float temperature,
                   float* logp_steps_out, float* logp_out, void* stream);
int msocr_seq_logp_host(const float* logits_host, const int32_t* ids_host, const int32_t* trun_host, int B, int V, int steps,
                        float temperature, float* logp_steps_out_host, float* logp_out_host);

/* Lexicon-constrained beam decode (beam mode with lexicon set): the search restricted to the words of a closed vocabulary, held as a prefix tree
 * (trie) in device memory.  msocr_lexicon: CSR arrays, nodes in breadth-first order (root = node 0, child > parent): edge_begin
 * [n_nodes + 1] i32, edge_tok [n_edges] i32 (strictly ascending inside a node), edge_child [n_edges] i32, terminal [n_nodes] u8 (1 where
 * a word ends).  The decode is the beam loop with two additions:
 *   state: every beam slot carries a trie node (i32; all slots start at the root; -1 = a dead slot);
 *   mask : where the candidates are formed, token v of a slot that is not finished is allowed if v is a child token of the slot's
 *          node, or v == eos_id and the node is terminal; every other candidate is -inf, and so is every candidate of a dead slot.
 *          Finished slots keep the plain rule (EOS alone, log-probability 0).
 * There is NO renormalisation: the log-sum-exp stays over the full row of V logits, so a path's score is the model's own joint
 * log-probability of that text (the number msocr_seq_logp gives for a forced decode of it).  Temperature, length penalty, the blank
 * column and the tie rule (larger value, then smaller flat index) are the plain decode's.  After the top-K a new slot's node is its
 * source's node when the source was finished or the token is eos_id, else the child of the source's node along the token (-1 when
 * there is none), and -1 whenever the winning candidate's value is not finite; a slot whose node is -1 counts as finished, so
 * fin_step and the chunk early exit fire as before.  The workspace layout and fin_step are unchanged: msocr_attn_beam_finalize,
 * msocr_attn_beam_nbest and msocr_seq_confidence read a constrained decode's workspace as they read a plain one's.  One more output:
 * node_out [B][steps][beam] i32 (msocr_attn_beam_slots_bytes), the node of every slot after step s (steps the early exit skips stay
 * unwritten).  alpha_out is required (there is one constrained kernel per family, with the weight output on:
 * csrc/attn_general_lexicon.hip, csrc/attn_lexicon_mfma.hip).
 * A null member of the lexicon, n_nodes < 1, n_edges < 0, a null node_out or alpha_out and shapes outside the kernel's envelope return
 * MSOCR_E_ARG before any launch.  The entry point receives device pointers and cannot validate the trie; the kernels clamp every
 * edge range into [0, n_edges], ignore an edge token outside [0, V) and treat a child outside [0, n_nodes) as none, so a malformed
 * trie can yield a wrong word but no out-of-bounds read.  msocr_lexicon_check_host validates HOST copies of the arrays: begins
 * monotone from 0 to n_edges, tokens strictly ascending per node and inside [0, V), parent < child < n_nodes, every node but the
 * root with exactly one parent, every childless node terminal, depth <= max_depth; MSOCR_OK or MSOCR_E_ARG. */
typedef struct {
  const int32_t *edge_begin, *edge_tok, *edge_child;
  const uint8_t* terminal;
  int n_nodes, n_edges;
} msocr_lexicon; /* device pointers */
int msocr_lexicon_check_host(const int32_t* edge_begin_host, const int32_t* edge_tok_host, const int32_t* edge_child_host,
                             const uint8_t* terminal_host, int n_nodes, int n_edges, int V, int max_depth);

/* Beam decode with a character n-gram language model fused in (shallow fusion), for open-vocabulary text: nothing is forbidden, every
 * candidate of a live hypothesis gains lm_weight * log P_lm(token | its last order - 1 tokens).
 * msocr_charlm: a dense table [n_ctx][V] f32 of natural-log probabilities in device memory, n_ctx = V^(order - 1), order 1..3.  Row ctx is
 * the context made of a hypothesis' last order - 1 tokens, the most recent one least significant (order 3: ctx = t[-2] * V + t[-1]);
 * positions before the start of the word count as sos_id, so every slot starts at ctx0 = sum_{i < order - 1} sos_id * V^i.  Order 1:
 * n_ctx 1, ctx always 0.  n_ctx * V <= 2^26 elements (256 MiB; order 3 up to V 406), so every index fits 32 bits.
 * The decode (beam mode with lm set) is the beam loop with alpha_out on, with one piece of state and one addend:
 *   state : every beam slot carries ctx (i32).  After the top-K, with ended = done[src] | (token == eos_id):
 *           ctx_new = ended ? ctx[src] : (ctx[src] * V + token) mod n_ctx.  ctx stays inside [0, n_ctx) and the token inside [0, V) by
 *           construction, and no index is formed from a table value: arbitrary table contents cause no out-of-bounds read.
 *   addend: where the candidates are formed, after the log-softmax (its log-sum-exp stays over the full temperature-scaled row), a slot
 *           that is not finished gets logp = fma(lm_weight, table[ctx * V + v], logit - lse) for every v, eos_id included (the model's
 *           end-of-word is fused with the LM's).  Finished slots keep the plain rule (EOS alone, log-probability 0, no LM term).
 * Temperature, the length-penalty division, the blank column, the tie rule, done / fin_step, the chunk early exit and the workspace
 * layout are unchanged.  The logits trace holds the MODEL's logits, not fused values: msocr_attn_beam_finalize,
 * msocr_attn_beam_nbest and msocr_seq_confidence read the workspace as they read a plain one's, and their log-probabilities and
 * confidences are the model's own numbers; the slots are in fused-score order.  lm_weight is a finite f32 >= 0; with lm_weight == 0
 * and a finite table the decode is bit-identical to the plain beam decode with alpha_out (workspace, fin_step, weight trace).  A table
 * with non-finite values is the caller's error (a NaN candidate is treated as in the plain decode).  One more output: ctx_out
 * [B][steps][beam] i32 (msocr_attn_beam_slots_bytes), the context of every slot after step s (steps the early exit skips stay unwritten).
 * The kernels: csrc/attn_general_lm.hip (general), csrc/attn_lm_mfma.hip (matrix cores).
 * A null table, ctx_out or alpha_out, order outside 1..3, lm->V != V, n_ctx != V^(order - 1), n_ctx * V > 2^26, lm_weight negative or
 * not finite, sos_id outside [0, V) and shapes outside the kernel's envelope return MSOCR_E_ARG before any launch.  A language model
 * and a lexicon in one decode are not provided. */
typedef struct {
  const float* table; /* device pointer */
  int32_t order;
  int32_t V;
  int64_t n_ctx;
} msocr_charlm;
/* the size of node_out and of ctx_out: [B][steps][beam] i32; 0 for a non-positive dimension */
int64_t msocr_attn_beam_slots_bytes(int B, int steps, int beam);

/* The one attention decode call.  The caller zeroes a descriptor, sets struct_bytes and mode, and fills the fields its mode reads
 * (G greedy, B beam, F forced); a pointer field the mode does not read must stay NULL, so a descriptor that mixes modes is
 * refused.  Null required pointers, shapes outside the envelope of the kernel family (above) and every other violation named in
 * this header return MSOCR_E_ARG before any launch.  All pointers but w, ws, lexicon and lm are device memory.  (The constants
 * carry _MODE_ because the kernel units use MSOCR_ATTN_FORCED and its like as their own compile-time switches.) */
#define MSOCR_ATTN_MODE_GREEDY 0
#define MSOCR_ATTN_MODE_BEAM 1
#define MSOCR_ATTN_MODE_FORCED 2
typedef struct msocr_attn_desc {
  int32_t struct_bytes;  /* GBF  sizeof(msocr_attn_desc); any other value: MSOCR_E_ARG before anything else is read */
  int32_t mode;          /* GBF  MSOCR_ATTN_MODE_GREEDY, MSOCR_ATTN_MODE_BEAM or MSOCR_ATTN_MODE_FORCED */
  int32_t B, T, H, V;    /* GBF  rows, encoder frames, hidden size, tokens */
  int32_t steps;         /* GBF  greedy max_len + 1, beam max_len, forced the columns of tok_in */
  int32_t beam;          /* B    beam width, 1..16 (matrix cores: <= 8) */
  int32_t sos_id;        /* GBF  inside [0, V) */
  int32_t eos_id;        /* GB   forced mode ends no row: it runs with -1 */
  int32_t blank_id;      /* GBF  column masked to -1e4; -1 = none */
  float temperature;     /* B    greedy and forced run with 1 */
  const float* batch_H;  /* GBF  [B][T][H] f32 */
  const float* proj_H;   /* GBF  [B][T][H] f32 = i2h(batch_H) */
  const float* ctx_gates;                /* GBF  [B][T][H][4] f32, 16-byte aligned: the matrix-core kernels; NULL: the general kernels */
  const msocr_attn_weights* w;           /* GBF */
  const msocr_attn_split_weights* ws;    /* GBF  with ctx_gates only (NULL without); G and F require it there, B: NULL = exact f32 */
  const float* lp;       /* B    [steps] f32 length-penalty factors, or NULL */
  const int32_t* tok_in; /* F    [B][steps] i32 */
  float* logits_out;     /* GF   [B][steps][V] f32 */
  int32_t* ids_out;      /* G    [B][steps] i32 */
  void* workspace;       /* B    msocr_attn_beam_workspace_bytes, 16-byte aligned */
  int32_t* fin_step_out; /* B    [B] i32 */
  const int32_t* chunk_id;   /* B    [B] i32          the early exit: all three or none */
  const int32_t* chunk_size; /* B    [nchunks] i32 */
  int32_t* chunk_state;      /* B    [2*nchunks] i32, zeroed by the caller */
  float* alpha_out;      /* GBF  attention weights: G, F [B][steps][T]; B [B][steps][beam][T], 16-byte aligned.  NULL = off (G, B);
                          *      F requires it */
  const msocr_lexicon* lexicon; /* B    non-NULL: the lexicon-constrained kernels; needs node_out and alpha_out; not with lm */
  int32_t* node_out;            /* B    [B][steps][beam] i32, with lexicon only */
  const msocr_charlm* lm;       /* B    non-NULL: the language-model kernels; needs ctx_out and alpha_out; not with lexicon */
  float lm_weight;              /* B    with lm: finite, >= 0 */
  int32_t* ctx_out;             /* B    [B][steps][beam] i32, with lm only */
} msocr_attn_desc;
int msocr_attn_decode(const msocr_attn_desc* d, void* stream);

/* Approximate dictionary lookup (csrc/lexicon_nearest.hip, csrc/edit_distance.h): for every recognised row the
 * k words of a lexicon with the smallest Levenshtein distance (unit costs for insertion, deletion and substitution), and the same
 * distance between pairs of rows.  Exact integers; the host twins run the same header.
 * A row's text is what TRBA.texts decodes: the ids before the first eos_id among the first min(max(trun, 0), steps) steps (all of them
 * if there is none), pad_id and blank_id removed; blank_id = -1 means none.  An id outside [0, V) in a row is a symbol that equals no
 * token: it costs a substitution or deletion like any mismatch and is never an index; so is a word token outside [0, V).
 * msocr_wordlist: the lexicon's encoded words as CSR arrays in device memory, word_begin [n_words + 1] i32 and word_tok [n_tok] i32; word
 * i is entry i of the lexicon.  The device entry points cannot validate it: a begin is clamped into [0, n_tok] (lo <= hi) and a word
 * longer than 63 tokens is read up to 63, so a corrupt list can give a wrong distance, not an out-of-bounds read.
 * msocr_wordlist_check_host validates HOST copies: begins monotone from 0 to n_tok, every word 1..max_word_len (<= 63) tokens, every
 * token in [0, V); MSOCR_OK or MSOCR_E_ARG.
 * by_length is for a second, kernel-friendly copy of the same list: the words stored in ascending (length, index) order, position p of
 * word_begin / word_tok holding the word whose index in the lexicon is by_length[p].  The lanes of a wave then hold words of one length
 * in adjacent memory (no wave waits for its longest word, and a length the bound rules out is skipped by whole waves).  Results and the
 * tie rule are in the ORIGINAL index and do not change with it: the key of a word is (distance, by_length[p]) whatever position it was
 * met at; any order of storage is accepted.  An entry outside [0, n_words) is skipped; an array that is no permutation gives a wrong
 * result (a word twice, or never), no out-of-bounds read.  The host twin reads it the same way.
 *   msocr_lexicon_nearest: for row b the k words with the smallest key (distance, index), ascending; equal distances go to the smaller
 *     index, a total order, so the result does not depend on how the lexicon is cut over workgroups.  max_distance >= 0 drops words
 *     further away, -1 = no bound.  Unfilled ranks hold index = -1, dist = -1.  workspace: msocr_lexicon_nearest_ws_bytes(B, n_words,
 *     k) bytes of device memory (0 when one workgroup per row covers the lexicon: then it may be NULL), 8-byte aligned, contents
 *     irrelevant.  Two launches at most (per-slice top-k, merge), no allocation, no synchronisation, capturable.
 *   msocr_edit_distance_pairs: row r of a against row r of b, both under the text rule: dist, and the two text lengths.
 * Envelope: 1 <= k <= 16, 1 <= steps (steps_a, steps_b) <= 64, 1 <= V <= 512, B >= 0 (B == 0: MSOCR_OK, no launch).  Null pointers,
 * n_words < 1, eos_id or pad_id outside [0, V), blank_id outside [-1, V), max_distance < -1 and shapes outside the envelope return
 * MSOCR_E_ARG before any launch; msocr_lexicon_nearest_ws_bytes returns MSOCR_E_ARG for B < 0, n_words < 1 or k outside 1..16. */
typedef struct {
  const int32_t *word_begin, *word_tok;
  int n_words, n_tok;
  const int32_t* by_length; /* optional (NULL = none): [n_words] i32; the arrays then hold word by_length[p] at position p */
} msocr_wordlist; /* device pointers (host pointers for the _host twin) */
int64_t msocr_lexicon_nearest_ws_bytes(int B, int n_words, int k);
int msocr_lexicon_nearest(const int32_t* ids, const int32_t* trun_dev, int B, int steps, int V, int eos_id, int pad_id, int blank_id,
                          const msocr_wordlist* wl, int k, int max_distance, int32_t* index_out, int32_t* dist_out, void* workspace,
                          void* stream);
int msocr_lexicon_nearest_host(const int32_t* ids_host, const int32_t* trun_host, int B, int steps, int V, int eos_id, int pad_id,
                               int blank_id, const msocr_wordlist* wl_host, int k, int max_distance, int32_t* index_out,
                               int32_t* dist_out);
int msocr_edit_distance_pairs(const int32_t* a_ids, const int32_t* a_trun, int steps_a, const int32_t* b_ids, const int32_t* b_trun,
                              int steps_b, int B, int V, int eos_id, int pad_id, int blank_id, int32_t* dist_out, int32_t* len_a_out,
                              int32_t* len_b_out, void* stream);
int msocr_edit_distance_pairs_host(const int32_t* a_ids, const int32_t* a_trun, int steps_a, const int32_t* b_ids, const int32_t* b_trun,
                                   int steps_b, int B, int V, int eos_id, int pad_id, int blank_id, int32_t* dist_out,
                                   int32_t* len_a_out, int32_t* len_b_out);
int msocr_wordlist_check_host(const int32_t* word_begin_host, const int32_t* word_tok_host, int n_words, int n_tok, int V,
                              int max_word_len);

/* The same lookup under confusion-weighted costs (csrc/lexicon_nearest.hip, csrc/edit_distance_weighted.h): the
 * distance is what it costs to turn the recognised ROW into the lexicon WORD, the textbook dynamic programme in exact integers.
 * msocr_edit_costs, device pointers (host pointers for the _host twin):
 *   sub [V][V] u8: sub[a * V + b] = reading recognised symbol a as lexicon symbol b; diagonal 0; need not be symmetric.
 *   del [V] u8: dropping recognised symbol a (the recogniser added it).  ins [V] u8: supplying lexicon symbol b (it dropped it).
 *   unknown, 1..255: any edit that involves a symbol outside [0, V), in the row or in the word; such a symbol matches nothing, itself
 *     included (the unit-cost rule above).
 *   min_ins, min_del: the minima of the two vectors, computed by the host; read only for the length bound: a word of n tokens costs a
 *     row of m symbols at least (n - m) * min_ins or (m - n) * min_del, and is skipped where that exceeds what could still be kept;
 *     the entry point takes min(min_ins, unknown) and min(min_del, unknown) for it, since a symbol outside [0, V) costs `unknown`.
 *     Minima larger than the true ones make the lookup miss words; they cause no out-of-bounds read.
 *   Every off-diagonal sub and every ins and del is 1..255, so distance 0 still means "the row is in the lexicon"; the largest
 *   distance is (64 + 63) * 255 = 32 385.  The device entry point cannot validate the tables: msocr_edit_costs_check_host does, for
 *   HOST copies (zero diagonal, nothing else zero, the minima, unknown in 1..255, 1 <= V <= 512, no null pointer): MSOCR_OK or
 *   MSOCR_E_ARG.  A table that breaks these rules gives other distances, no out-of-bounds read.
 * msocr_lexicon_nearest_weighted(_host): the contract of msocr_lexicon_nearest(_host) in every other respect: index / dist [B][k]
 *   ascending in (distance, index), -1 / -1 in unfilled ranks, max_distance in cost units (-1 = no bound), 1 <= k <= 16, the same
 *   envelope and rejections, and MSOCR_E_ARG also for costs == NULL, a null table, costs->V != V, unknown outside 1..255 or a minimum
 *   outside 1..255.  workspace: msocr_lexicon_nearest_weighted_ws_bytes(B, n_words, k), the number msocr_lexicon_nearest_ws_bytes
 *   returns.  Two launches at most, no allocation, no synchronisation, capturable. */
typedef struct {
  const uint8_t *sub, *del, *ins;
  int V, unknown, min_ins, min_del;
} msocr_edit_costs;
int msocr_edit_costs_check_host(const uint8_t* sub_host, const uint8_t* del_host, const uint8_t* ins_host, int V, int unknown, int min_ins,
                                int min_del);
int64_t msocr_lexicon_nearest_weighted_ws_bytes(int B, int n_words, int k);
int msocr_lexicon_nearest_weighted(const int32_t* ids, const int32_t* trun_dev, int B, int steps, int V, int eos_id, int pad_id,
                                   int blank_id, const msocr_wordlist* wl, const msocr_edit_costs* costs, int k, int max_distance,
                                   int32_t* index_out, int32_t* dist_out, void* workspace, void* stream);
int msocr_lexicon_nearest_weighted_host(const int32_t* ids_host, const int32_t* trun_host, int B, int steps, int V, int eos_id,
                                        int pad_id, int blank_id, const msocr_wordlist* wl_host, const msocr_edit_costs* costs_host,
                                        int k, int max_distance, int32_t* index_out, int32_t* dist_out);

/* ---- detection quality: predicted quads matched to ground truth (an extension beyond the reference's inference code:
 * EAST.evaluate, Pipeline.evaluate, detectors.match_detections) ----
 * The matching rule of the reference's compute_f1 (detectors/_east/utils.py:435-474) with one change: the IoU is the reference's own
 * lanms.polygon_iou (lanms.py:60-91; csrc/quad_iou.h restates it bit for bit), not shapely's.
 * Inputs: quads [n][4][2] f32; all arithmetic is f64 on the converted values.
 * Validity: a quad is valid iff its eight coordinates are finite and the four turn cross products (v[i+1]-v[i]) x (v[i+2]-v[i+1])
 *   are all > 0 or all < 0 (strictly convex).  This stands in for shapely's is_valid: self-intersecting and degenerate quads are
 *   invalid under both rules; a concave simple quad is valid for shapely and INVALID here (stated deviation).
 * Canonical winding: a valid quad whose cross products are negative is read as [v0, v3, v2, v1], predictions and ground truth alike.
 *   polygon_iou takes the left of the clip polygon's edges as inside (polygon_iou(q, q reversed) is 0.0, polygon_iou(q, q) is 1.0);
 *   shapely is winding-blind and annotations come in either winding.
 * IoU: polygon_iou(prediction, ground truth), prediction as subject, ground truth as clip.  The function is not bitwise symmetric:
 *   the argument order is part of the definition.
 * Matching, per page and per threshold t independently:
 *   predictions in the given order; an invalid prediction is a false positive (match -2, iou 0);
 *   a valid prediction starts at best_iou = 0, bj = -1 and scans the ground truths j ascending that are valid and unused at this t,
 *   taking j when iou > best_iou (strict: the smallest j wins a tie); best_iou >= t: true positive, match = bj, used[bj] set;
 *   otherwise false positive, match = -1, nothing marked.  iou_out holds best_iou as it stood at the decision (0 when no unused
 *   ground truth overlapped).  An invalid ground truth is never matched but counts: fn = n_gt - tp.  counts = {tp, fp, fn}.
 * Thresholds: T f64 values in (0, 1], read from HOST memory by both entry points and handed to the kernel as an argument (a
 *   threshold <= 0 would mark used[-1] in the reference).
 * Envelope: 0 <= n_pred[p] <= max_pred <= 16384, 0 <= n_gt[p] <= max_gt <= 16384, 1 <= T <= 16, N >= 0 (N == 0: MSOCR_OK, no launch).
 *   Null pointers (the workspace included), a threshold outside (0, 1] or not finite and shapes outside the envelope return MSOCR_E_ARG
 *   before any launch; the ws_bytes query returns MSOCR_E_ARG for them.  The host twin also refuses a count outside [0, max]; the
 *   device entry point cannot read its counts and the kernels clamp them into [0, max].
 * Outputs: match_out [N][T][max_pred] i32, iou_out [N][T][max_pred] f64: entries i < n_pred[p] are written, the others are left as
 *   they were; counts_out [N][T][3] i32.  workspace: msocr_quad_match_ws_bytes bytes of device memory, 8-byte aligned, contents
 *   irrelevant (candidate lists of 8 slots per prediction; a prediction with more overlaps is recomputed against the whole page, the
 *   result does not depend on the slot count).  Three launches, no allocation, no synchronisation, capturable. */
int64_t msocr_quad_match_ws_bytes(int N, int max_pred, int max_gt);
int msocr_quad_match(const float* pred, const int32_t* n_pred, int max_pred, const float* gt, const int32_t* n_gt, int max_gt, int N,
                     const double* thresholds_host, int T, int32_t* match_out, double* iou_out, int32_t* counts_out, void* workspace,
                     void* stream);
int msocr_quad_match_host(const float* pred_host, const int32_t* n_pred_host, int max_pred, const float* gt_host,
                          const int32_t* n_gt_host, int max_gt, int N, const double* thresholds_host, int T, int32_t* match_out,
                          double* iou_out, int32_t* counts_out);

/* ---- page-level error rates: the edit distance of long sequences (an extension beyond the reference's inference code:
 * recognizers.sequence_edit_distances / text_error_rates, Pipeline.evaluate_text; csrc/edit_distance_long.hip,
 * csrc/edit_distance_long.h) ----
 * The exact Levenshtein distance (unit costs for insertion, deletion and substitution) between N pairs of int32 token sequences of
 * 0 .. 16384 tokens each (MSOCR_EDL_MAX_LEN): a page's running text against its transcription, as characters or as words.
 * Integers; the host twin runs the same header block by block.
 * Tokens: CSR arrays.  a_tok holds the patterns, b_tok the texts, pair p being a_tok[a_off[p] .. a_off[p + 1]) against
 * b_tok[b_off[p] .. b_off[p + 1]); device memory for msocr_edit_distance_long, host memory for the twin.  The offset arrays
 * a_off [N + 1], b_off [N + 1] and the alphabet sizes v [N] are HOST memory on both routes.  The token arrays hold at least
 * a_off[N] / b_off[N] elements; a pointer to an array without elements must still be non-null.
 * v[p]: tokens of pair p in [0, v[p]) compare by equality; a token outside it, on either side, equals nothing (the rule of
 * msocr_edit_distance_pairs) and is never an index.  The distance is symmetric, so either side may be the pattern; the pattern's
 * side decides the workspace.
 * m == 0 gives n, n == 0 gives m; N == 0: MSOCR_OK, nothing launched.  dist_out [N] i32; nothing behind it is written.
 * workspace (device route): device memory, 8-byte aligned, contents irrelevant, of at least msocr_edit_distance_long_ws_bytes =
 *   32 N + sum over the pairs of v[p] * ceil(m_p / 64) * 8 bytes: the uploaded heads (one 32-byte record per pair) and the pairs'
 *   match-mask tables [v][ceil(m / 64)] of 64-bit words, which a small kernel builds before the distance kernel runs.
 * Refused with MSOCR_E_ARG before any launch: N < 0, a null pointer, an offset array that does not start at a value >= 0 or
 *   decreases, a length above the cap, v[p] < 0, a workspace that is misaligned or smaller than required (workspace_bytes); the
 *   ws_bytes query returns MSOCR_E_ARG for the same arrays.  The host twin also returns MSOCR_E_ARG when it cannot allocate a table.
 * The entry point uploads the heads from a buffer of its own and waits for that copy on `stream`; three launches follow, which
 *   the host does not wait for.  Not capturable: this is an evaluation call.  One wave per pair: a batch of a few long pairs is
 *   bound by latency, not by the chip (measured: profiles/edit_distance_long.txt). */
int64_t msocr_edit_distance_long_ws_bytes(const int32_t* a_off_host, const int32_t* b_off_host, const int32_t* v_host, int N);
int msocr_edit_distance_long(const int32_t* a_tok, const int32_t* a_off_host, const int32_t* b_tok, const int32_t* b_off_host,
                             const int32_t* v_host, int N, int32_t* dist_out, void* workspace, int64_t workspace_bytes, void* stream);
int msocr_edit_distance_long_host(const int32_t* a_tok_host, const int32_t* a_off_host, const int32_t* b_tok_host,
                                  const int32_t* b_off_host, const int32_t* v_host, int N, int32_t* dist_out);

/* ---- alignment behind the error rates: one optimal edit script of long sequences (an extension beyond the reference's inference
 * code: recognizers.sequence_alignments / error_breakdown / text_error_rates(breakdown=True), Pipeline.evaluate_text(breakdown=True),
 * Pipeline.transfer_text; csrc/edit_alignment.hip, csrc/edit_alignment.h) ----
 * Which pattern token pairs with which text token under the distance of msocr_edit_distance_long, and how many hits,
 * substitutions, deletions and insertions that makes.  Of the optimal alignments the one this tie rule fixes: from
 * (i, j) = (m, n), while i > 0 and j > 0, the first of
 *   1. a[i-1] equals b[j-1]: hit, paired, to (i-1, j-1);      2. D[i-1][j-1] + 1 == D[i][j]: substitution, paired, to (i-1, j-1);
 *   3. D[i-1][j] + 1 == D[i][j]: deletion, a[i-1] unpaired, to (i-1, j);      4. otherwise insertion, b[j-1] unpaired, to (i, j-1);
 * then the rest of the pattern is deletions or the rest of the text insertions (D: the Levenshtein table).  Integers; the host
 * twin applies the same header's rule to the same trace, so the two routes agree bit for bit.  The rule is NOT symmetric: the
 * caller decides which side is the pattern (recognizers.sequence_alignments: always the reference).
 * Tokens, offsets, v and the equality rule: as for msocr_edit_distance_long above.
 * Outputs (device memory; host memory for the twin): dist_out [N] i32; a_map_out [a_off[N] - a_off[0]] i32, for the token at
 * a_tok[a_off[p] + i] the element a_off[p] - a_off[0] + i = the index of its partner within pair p's text, or -1;
 * b_map_out [b_off[N] - b_off[0]] i32 likewise, indices within the pair's pattern; counts_out [N][4] i32 = {hits, substitutions,
 * deletions, insertions}: substitutions + deletions + insertions = dist, hits + substitutions + deletions = m,
 * hits + substitutions + insertions = n.  Every element is written exactly once; nothing behind the stated extents is written.
 * A map without elements must still be a non-null pointer.  m == 0: all insertions; n == 0: all deletions; N == 0: MSOCR_OK,
 * nothing launched.
 * workspace (device route): device memory, 16-byte aligned, contents irrelevant, of at least msocr_edit_alignment_ws_bytes =
 *   40 N + sum v[p] * ceil(m_p / 64) * 8, rounded up to a multiple of 16, + sum 16 * ceil(m_p / 64) * n_p bytes: the heads, one
 *   trace offset per pair, the match-mask tables, and the trace: per pattern block and text column the two 64-bit words of the
 *   block recurrence that decide every cell of that block and column.  2.9 MB for a page of 3400 characters against itself, 64 MiB
 *   for a pair at the cap on both sides (a linear-memory traceback is not provided).
 * Refused with MSOCR_E_ARG before any launch: what msocr_edit_distance_long refuses (a workspace not 16-byte aligned included);
 *   the ws_bytes query returns MSOCR_E_ARG for the same arrays.  The host twin also returns MSOCR_E_ARG when it cannot allocate a
 *   table or a trace.
 * The entry point uploads the heads from a buffer of its own and waits for that copy on `stream`; four launches follow (tables,
 *   the distance kernel's sweep with the trace stores, and the traceback in a launch of its own: one wave per pair walks back
 *   through windows of 64 x 64 cells held in registers), which the host does not wait for.  Not capturable: an evaluation call.
 *   Measured: profiles/edit_alignment.txt. */
int64_t msocr_edit_alignment_ws_bytes(const int32_t* a_off_host, const int32_t* b_off_host, const int32_t* v_host, int N);
int msocr_edit_alignment(const int32_t* a_tok, const int32_t* a_off_host, const int32_t* b_tok, const int32_t* b_off_host,
                         const int32_t* v_host, int N, int32_t* dist_out, int32_t* a_map_out, int32_t* b_map_out, int32_t* counts_out,
                         void* workspace, int64_t workspace_bytes, void* stream);
int msocr_edit_alignment_host(const int32_t* a_tok_host, const int32_t* a_off_host, const int32_t* b_tok_host,
                              const int32_t* b_off_host, const int32_t* v_host, int N, int32_t* dist_out, int32_t* a_map_out,
                              int32_t* b_map_out, int32_t* counts_out);

/* ---- approximate text search: where do Q short patterns occur in T texts, with up to k errors each (an extension beyond the
 * reference's inference code: recognizers.TextCorpus / search_texts, PageCorpus, Pipeline.search; csrc/text_search.hip,
 * csrc/text_search.h) ----
 * Sellers' semi-global form of the Levenshtein table, unit costs, integers.
 * Tokens: int32.  A call has one alphabet size v, 1 <= v <= MSOCR_SEARCH_MAX_ALPHABET.  Tokens in [0, v) compare by equality; any
 *   other token, on either side, equals nothing and is never used as an index (the rule of msocr_edit_distance_long).
 * Inputs: patterns q = 0 .. Q-1 as CSR (pat_tok, pat_off [Q + 1]), each of length 1 <= m_q <= MSOCR_SEARCH_MAX_PATTERN (64) with an
 *   error bound k_q = max_dist[q], 0 <= k_q < m_q (with k >= m the empty substring would match everywhere); texts t = 0 .. T-1 as
 *   CSR (txt_tok, txt_off [T + 1]), each of any length n_t >= 0, at most 2^31 - 1 tokens in all.  The token arrays are device memory
 *   for the device entry point and host memory for the twin; pat_off, max_dist and txt_off are HOST memory on both routes.
 * Scores: for a pattern a[0..m) and a text b[0..n), s_0 = m and s_j = min over 0 <= l <= j of ed(a, b[j-l .. j)) for 1 <= j <= n:
 *   the bottom row of Sellers' table, which has D[0][j] = 0 and D[i][0] = i.
 * Hits: every (q, t, j) with s_j <= k_q is a hit; all end positions are reported, not local minima.  Its record:
 *   end = j, exclusive, counted inside its text; distance = s_j; start = j - l*, l* the SMALLEST l with ed(a, b[j-l .. j)) == s_j,
 *   the shortest substring that attains the score (m - s_j <= l* <= min(j, m + s_j)).  It is computed by the global recurrence of
 *   the reversed pattern over b[j-1], b[j-2], ..: the first l at which that distance equals s_j.
 * Order and capacity: the canonical order is ascending (pattern, text, end); the key is unique.  The host twin writes the first
 *   `capacity` hits in canonical order; the device route writes hits in no particular order.  On both routes count_out (int64) is
 *   the EXACT number of hits, also when it exceeds `capacity`: then exactly `capacity` records are written, each a true, distinct
 *   hit, and nothing is written behind hits_out[capacity].
 * Selection (a host function on read-back hits, for both routes, which therefore agree bit for bit after it): sorts the n records
 *   into canonical order; per (pattern, text) it walks the hits by (distance, end) ascending and keeps one iff [start, end)
 *   intersects no kept hit of the same (pattern, text); the kept hits are compacted to the front in canonical order and their
 *   number is returned.  MSOCR_E_ARG for n < 0 or a null pointer with n > 0.
 * workspace (device route): device memory, 8-byte aligned, contents irrelevant, of at least the ws_bytes query's
 *   16 Q v + 8 (T + 1) + 4 (T + 1) + 4 (Q + 1) + 4 Q bytes, rounded up to a multiple of 8: the match-mask tables [Q][2][v] of 64-bit
 *   words (the patterns' masks and the reversed patterns'), which a small kernel builds, and the uploaded heads: per text the
 *   number of segments before it and its offset, per pattern its offset and bound.  A text is cut into segments of
 *   MSOCR_SEARCH_SEGMENT tokens; one lane scans one (pattern, segment), from m + k tokens before it.
 * Refused with MSOCR_E_ARG before any launch: a null pointer (an array without elements is never read, its pointer must still be
 *   non-null; Q == 0 / T == 0 do not read the pattern / text offsets), Q < 0 or T < 0, offsets that do not start at a value >= 0 or
 *   decrease, m_q outside 1..64, k_q outside [0, m_q), v outside 1..2048, capacity < 0, a workspace that is misaligned or smaller
 *   than required; the ws_bytes query returns MSOCR_E_ARG for the same arrays.  Q == 0 or T == 0: MSOCR_OK with count 0 (ws_bytes: 0;
 *   the device route needs no workspace then and launches the one kernel that clears the count).
 * The device entry point uploads the heads from a buffer of its own and waits for that copy on `stream`; four launches follow
 *   (clear, masks, scan, starts), which the host does not wait for.  Not capturable.  Measured: profiles/text_search.txt. */
#define MSOCR_SEARCH_MAX_ALPHABET 2048
#define MSOCR_SEARCH_MAX_PATTERN 64
#define MSOCR_SEARCH_SEGMENT 64
typedef struct msocr_search_hit {
  int32_t pattern, text, start, end, distance;
} msocr_search_hit;
int64_t msocr_text_search_ws_bytes(const int32_t* pat_off_host, const int32_t* max_dist_host, int Q, const int32_t* txt_off_host, int T,
                                   int v);
int msocr_text_search(const int32_t* pat_tok, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q, const int32_t* txt_tok,
                      const int32_t* txt_off_host, int T, int v, msocr_search_hit* hits_out, int64_t capacity, int64_t* count_out,
                      void* workspace, int64_t workspace_bytes, void* stream);
int msocr_text_search_host(const int32_t* pat_tok_host, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                           const int32_t* txt_tok_host, const int32_t* txt_off_host, int T, int v, msocr_search_hit* hits_out,
                           int64_t capacity, int64_t* count_out);
int64_t msocr_text_search_select_host(msocr_search_hit* hits, int64_t n);

/* The same search under confusion-weighted costs (csrc/text_search_weighted.hip, csrc/text_search_weighted.h):
 * the semi-global form of the weighted table of msocr_lexicon_nearest_weighted, in exact integers.  Everything not said here is the
 * contract of msocr_text_search(_host): the CSR inputs, which arrays are host memory, the record, the canonical order, the capacity
 * and count protocol, Q == 0 / T == 0, and msocr_text_search_select_host on the read-back records.
 * Direction: the TEXT is the recognised side, the PATTERN the true word (msocr_edit_costs' own direction).
 * Classes: tok_class [v] int32 (device memory; host memory for the twin) gives the cost class in [0, costs->V) of corpus token c, any
 *   other value (-1 by convention) where c has none.  cls(t) = tok_class[t] for t in [0, v) if that lies in [0, V), else none.
 *   w_sub(t, p), reading text token t as pattern token p: 0 if t == p and both lie in [0, v) (equal corpus characters match even
 *     where the charset lacks them); else sub[cls(t) * V + cls(p)] if both have a class (two tokens of one class cost the diagonal);
 *     else `unknown`.  A token outside [0, v), on either side, matches nothing, itself included.
 *   w_del(t) = del[cls(t)] or `unknown`: dropping a text token.  w_ins(p) = ins[cls(p)] or `unknown`: supplying a pattern token.
 * Table: D[0][j] = 0; D[i][0] = the sum of w_ins over a[0..i); D[i][j] = min(D[i-1][j-1] + w_sub(b[j-1], a[i-1]),
 *   D[i][j-1] + w_del(b[j-1]), D[i-1][j] + w_ins(a[i-1])).
 * Hits: every end j >= 1 with D[m][j] <= k' = min(k_q, D[m][0] - 1), so the empty substring never matches; k_q = max_dist[q] >= 0
 *   is in cost units.  distance = D[m][j]; start = the LARGEST s whose weighted global distance between the pattern and b[s .. j)
 *   equals it: the shortest substring that attains the score, the tie rule of the unit search.
 * Window: W_q = m_q + k_q / dmin tokens, dmin = min(costs->min_del, costs->unknown), must not exceed MSOCR_SEARCH_W_MAX_WINDOW: an
 *   alignment of cost <= k drops at most k / dmin text tokens, so it spans at most W_q of them, and the device scans a segment from
 *   that far before it (from m_q + k' / dmin, which is no more).  The check takes k_q as given, since D[m][0] is device data.  A
 *   min_del above the true minimum makes the device route miss hits; it causes no out-of-bounds read.
 * With every cost 1 (and unknown 1) the records are those of msocr_text_search on the same arrays, whether the tokens have a class
 *   or not, as long as no two tokens share one (those would match at the diagonal's 0).
 * workspace (device route): 8-byte aligned, at least the ws_bytes query's 8 (T + 1) + 4 (T + 1) + 4 (Q + 1) + 4 Q bytes rounded up
 *   to a multiple of 8 (the uploaded heads; there are no mask tables).
 * MSOCR_E_ARG before any launch, beyond the cases of msocr_text_search: k_q < 0 (k_q >= m_q is allowed), W_q above the cap, v
 *   outside 1..MSOCR_SEARCH_W_MAX_ALPHABET, tok_class or costs NULL, a null table, costs->V outside 1..512, unknown, min_ins or
 *   min_del outside 1..255.  The device entry point cannot validate the tables or the classes (msocr_edit_costs_check_host does
 *   the former): whatever they hold, no index leaves them.
 * The device entry point uploads the heads and waits for that copy on `stream`; two launches follow (clear the count, scan), which
 *   the host does not wait for.  A workgroup builds its pattern's cost profile, (v + 1) rows of 72 bytes, in dynamic LDS (at most
 *   57 KB); a lane keeps its column in 64 registers, the start packed under the cost.  Not capturable.  Measured:
 *   profiles/text_search_weighted.txt. */
#define MSOCR_SEARCH_W_MAX_ALPHABET 768
#define MSOCR_SEARCH_W_MAX_WINDOW 256
int64_t msocr_text_search_weighted_ws_bytes(const int32_t* pat_off_host, const int32_t* max_dist_host, int Q, const int32_t* txt_off_host,
                                            int T, int v, const msocr_edit_costs* costs);
int msocr_text_search_weighted(const int32_t* pat_tok, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                               const int32_t* txt_tok, const int32_t* txt_off_host, int T, int v, const int32_t* tok_class,
                               const msocr_edit_costs* costs, msocr_search_hit* hits_out, int64_t capacity, int64_t* count_out,
                               void* workspace, int64_t workspace_bytes, void* stream);
int msocr_text_search_weighted_host(const int32_t* pat_tok_host, const int32_t* pat_off_host, const int32_t* max_dist_host, int Q,
                                    const int32_t* txt_tok_host, const int32_t* txt_off_host, int T, int v,
                                    const int32_t* tok_class_host, const msocr_edit_costs* costs_host, msocr_search_hit* hits_out,
                                    int64_t capacity, int64_t* count_out);

/* ---- word spotting: query-by-example search over encoder features, Q query words against N indexed words by a dynamic-time-warping
 * distance between their frame sequences (an extension beyond the reference's inference code: TRBA.embed, WordIndex,
 * Pipeline.index_words / spot; csrc/word_spotting.hip, csrc/word_spotting.h) ----
 * Sequences: a sequence is x[0..L) of frames in R^H, stored as row n of a dense [N][T][H] f32 array with its length len[n],
 *   1 <= len <= T.  Frames t >= len are never read by any function here.
 * Unit frames (msocr_frame_normalize): u_t = x_t / ||x_t||, the squared norm accumulated in f32 in this order: 64 partial sums,
 *   partial l takes the elements l, l + 64, l + 128, .. ascending, each by one fmaf; the partials are folded by a butterfly over the
 *   masks 32, 16, 8, 4, 2, 1 (p[l] += p[l ^ mask]); the root and the quotient x / root are correctly rounded f32 operations.  If the
 *   squared norm is not finite (an Inf or NaN element, or an overflow) or below FLT_MIN, u_t = 0: such a frame costs 1 against
 *   everything, and no NaN leaves this step.  Frames t >= len are WRITTEN as zeros (and not read); a length outside [0, T] is
 *   clamped into it.  unit_out may be feat itself.  | ||u|| - 1 | <= (H + 4) 2^-24.
 * Local cost: c(i, j) = 1 - <u_i, v_j>.
 * Distance (msocr_dtw_distances): symmetric steps, unit weights: D(0,0) = c(0,0); D(i,j) = c(i,j) + min(D(i-1,j-1), D(i-1,j),
 *   D(i,j-1)), absent neighbours +inf; d = D(Lq-1, Ln-1) / (Lq + Ln).  dist [Q][N] f32.
 * Length gate: query q carries integer bounds len_lo[q] <= len_hi[q]; a pair whose word length lies outside them gets d = +inf and
 *   costs no arithmetic.  On the device route a query or word length outside [1, T] gates its pairs out the same way (the lengths
 *   are device memory there and cannot be refused); the host twin refuses them, and len_lo > len_hi.
 * Arithmetic: the device forms <u_i, v_j> with the exact f32 matrix instruction (one f32 rounding per product and per addition, K
 *   order documented in the kernel), the table and the division in f32: | d - d_f64 | <= (H + 2 (Lq + Ln) + 16) 2^-24 for the
 *   same unit frames (DESIGN.md section 4.25 has the derivation).
 *   The host twin forms every product, sum and table entry in f64 and rounds to f32 once.
 * Subsequence distance (msocr_dtw_subsequence): "which words CONTAIN this".  The same sequences, unit frames
 *   and local cost; the query may start and end anywhere on the word's axis.  S(0, j) = c(0, j) for every j (a free start: row 0
 *   takes no left step); S(i, j) = c(i, j) + min(S(i-1, j-1), S(i-1, j), S(i, j-1)) for i >= 1, absent neighbours +inf;
 *   d = min_j S(Lq-1, j) / Lq.  Every cell carries the column at which its path left row 0: start(0, j) = j, otherwise the start of
 *   the chosen predecessor; among equal predecessors the diagonal one wins, then the upper, then the left.  The end e is the
 *   SMALLEST j that attains the minimum.  Per pair: dist [Q][N] f32 = d and span [Q][N][2] int32 = [start(Lq-1, e), e + 1), in word
 *   frames.  Lq > Ln is legal (the path then takes vertical steps).  There is no slope constraint and no minimum span: a query may
 *   collapse onto one word frame.  The length gate is msocr_dtw_distances' (same two arguments); a gated-out pair, and on the device
 *   route a query or word length outside [1, T], gets d = +inf and span (-1, -1) and costs no arithmetic; the host twin refuses such
 *   lengths, and len_lo > len_hi.  Arithmetic as for the distance: the device's table and division are f32,
 *   | d - d_f64 | <= (3 H + 2 (Lq + Ln) + 16) 2^-24 (Lq + Ln) / Lq from the same raw frames (tests/test_gpu_word_spotting_partial.py
 *   has the derivation); its span is a span whose best pinned path costs at most that much more than the f64 optimum (near-ties may
 *   fall differently).  The host twin forms every product, sum and table entry in f64 and rounds d to f32 once.
 *   The encoder's frames carry context (a BiLSTM), so a stem cut alone and the same stem inside a longer word need not embed alike:
 *   what is defined and tested is the arithmetic, nothing about retrieval quality.
 * Selection (msocr_topk_smallest): per row of dist the k smallest FINITE values in ascending order, equal values (as floats:
 *   -0.0 == +0.0) by ascending index; +inf, -inf and NaN are never returned; unused slots hold index -1 and value +inf.  A value is
 *   copied as stored.  The host twin returns the same bits as the device.
 * Envelope: 1 <= T <= MSOCR_SPOT_MAX_T (64); H a multiple of 64 in 64 .. MSOCR_SPOT_MAX_H (512); Q, N >= 0; Q T H and N T H below
 *   2^31; 1 <= k <= MSOCR_SPOT_MAX_K (256); q_unit and c_unit 16-byte aligned on the device route.  Anything else, and a null
 *   pointer, is MSOCR_E_ARG before any launch.  Q == 0 or N == 0 launches nothing that reads features (the selection still fills its
 *   Q rows with -1 / +inf).
 * The device entry points take device pointers, allocate nothing, wait for nothing and launch one kernel each on `stream`; they
 *   are not meant for graph capture.  A workgroup of msocr_dtw_distances or msocr_dtw_subsequence owns MSOCR_SPOT_TILE words.
 *   Measured: profiles/word_spotting.txt, profiles/word_spotting_partial.txt. */
#define MSOCR_SPOT_MAX_T 64
#define MSOCR_SPOT_MAX_H 512
#define MSOCR_SPOT_MAX_K 256
#define MSOCR_SPOT_TILE 4
int msocr_frame_normalize(const float* feat, const int32_t* len, int N, int T, int H, float* unit_out, void* stream);
int msocr_frame_normalize_host(const float* feat, const int32_t* len, int N, int T, int H, float* unit_out);
int msocr_dtw_distances(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                        const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, void* stream);
int msocr_dtw_distances_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                             const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist);
int msocr_dtw_subsequence(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                          const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, int32_t* span, void* stream);
int msocr_dtw_subsequence_host(const float* q_unit, const int32_t* q_len, const int32_t* len_lo, const int32_t* len_hi, int Q,
                               const float* c_unit, const int32_t* c_len, int N, int T, int H, float* dist, int32_t* span);
int msocr_topk_smallest(const float* dist, int Q, int N, int k, int32_t* idx, float* val, void* stream);
int msocr_topk_smallest_host(const float* dist, int Q, int N, int k, int32_t* idx, float* val);

/* Word crops -> recogniser canvases on the device: clamped AABB crop (Pipeline._extract_word_image,
 * _pipeline.py:204-221) + ResizeAndPadA (recognizers/_trba/data/transforms.py:85-120: aspect-preserving resize,
 * INTER_AREA if any axis shrinks else INTER_LINEAR, pasted at x=0 / vertically centred on a 255 canvas).
 * pages [N][H][W][3] u8; descriptor per crop = 8 x int32 {page, x1, y1, x2, y2, new_w, new_h, y0} (the host
 * evaluates Python's banker's rounding of the new size); desc_host is the same array in host memory, used only
 * to validate bounds before the launch, or NULL when the descriptors were produced on the device
 * (msocr_reading_order_crops): the kernel then checks every descriptor itself and emits a white canvas for an
 * invalid one.  canvases [M][img_h][img_w][3] u8.  (cv2 restated: parity unpinned.) */
int msocr_crop_resize_pad(const uint8_t* pages, int N, int H, int W, const int32_t* desc_dev,
                          const int32_t* desc_host, int M, int img_h, int img_w, uint8_t* canvases, void* stream);

/* HOST function (plain C++, all pointers host memory): reading order of a page's word boxes, i.e. the Python glue between
 * detector and recogniser: resolve_intersections + sort_boxes_reading_order(+_with_resolutions)
 * (detectors/_east/utils.py:500-644) and the "first word with an equal box" re-match of _pipeline.py:113-121, with the
 * reference's integer / double arithmetic.  boxes_host [n][4] int32 (x_min, y_min, x_max, y_max);
 * order_out_host [n] int32: entry k = index of the input box at position k of the reading order (duplicates as the
 * reference's dict semantics produce them). */
int msocr_reading_order_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio,
                             int32_t* order_out_host);

/* HOST function: the same order together with the TEXT LINES it is built from (sort_boxes_reading_order groups the shrunk boxes
 * into lines, sorts the lines by mean centre y and the words of a line by x, and returns only the flattened list).
 * line_out_host [n]: 0-based index of the line of every position of order_out_host; lines are numbered in reading order, so the
 * values start at 0, never decrease and step by 0 or 1.  lines_out_host [n][6]: one record {first, count, x0, y0, x1, y1} per line:
 * first / count = the line's span of positions, x0..y1 = the union of the input boxes of the words written at those positions
 * (boxes_host[order_out_host[pos]]).  *nlines_out_host: the number of lines, 0 for n = 0.  Rows past the line count stay untouched. */
int msocr_reading_lines_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio, int32_t* order_out_host,
                             int32_t* line_out_host, int32_t* lines_out_host, int32_t* nlines_out_host);

/* The same glue ON THE DEVICE, one workgroup per page, fed by msocr_east_box_tail's output, plus what follows it on the way to the
 * recogniser: word AABBs with np.int32 truncation and the min_text_size filter (_pipeline.py:100-133), the clamped crop window
 * (_pipeline.py:204-221) and ResizeAndPadA's size arithmetic (recognizers/_trba/data/transforms.py:91-95,114-117) -> descriptors in
 * the format of msocr_crop_resize_pad.  boxes [N][max_cand][9] f32, nbox [N] (negative: page skipped, ncrop = -1).
 * order_out [N][max_cand]: entry k = index of the word at reading-order position k; keep_out [N][max_cand]: 1 where position k
 * yields a crop; desc_out [N][max_cand][8]: the page's crop descriptors in order, compacted (page field = page_base + n);
 * ncrop_out [N]: crops of the page, or -1 = take the host path for this page (more than min(max_cand, 16384) boxes, more than
 * 4096 text lines, or more intersecting box pairs than the pair buffer holds).  Bit-identical to msocr_reading_order_host + the
 * host descriptor arithmetic.  workspace: msocr_reading_order_workspace_bytes(N, max_cand) bytes, 16-B aligned. */
int64_t msocr_reading_order_workspace_bytes(int N, int max_cand);
int msocr_reading_order_crops(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                              int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio, int page_base,
                              int32_t* order_out, int32_t* keep_out, int32_t* desc_out, int32_t* ncrop_out, void* workspace,
                              void* stream);

/* msocr_reading_order_crops with the page's text lines as three more outputs (an extension beyond the reference, off by default:
 * Pipeline.group_lines).  Same arguments, same workspace, the same order_out / keep_out / desc_out / ncrop_out bit for bit.
 * line_out [N][max_cand]: for every position pos < n of order_out the 0-based index of its line, lines numbered in reading order.
 * lines_out [N][rows][6], rows = msocr_reading_order_line_rows(max_cand) = min(max_cand, 4096): one record
 * {first, count, x0, y0, x1, y1} per line, first / count = its span of positions in order_out, x0..y1 = the union of the integer
 * word boxes (np.int32 truncation of the quad, min / max) of the words written at those positions.  nlines_out [N]: lines of the
 * page, 0 for a page without boxes, -1 exactly where ncrop_out is -1 (then nothing else of the three is defined; rows of such a
 * page and rows past a page's counts stay untouched).  Bit-identical to msocr_reading_lines_host. */
int msocr_reading_order_line_rows(int max_cand);
int msocr_reading_order_lines(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                              int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio, int page_base,
                              int32_t* order_out, int32_t* keep_out, int32_t* desc_out, int32_t* ncrop_out, int32_t* line_out,
                              int32_t* lines_out, int32_t* nlines_out, void* workspace, void* stream);

/* ---- skew-aware reading order (an extension beyond the reference, off by default: Pipeline.deskew) ----
 * The page's skew is estimated from the detected quads, and the boxes that the reading order shrinks, groups and sorts are those of
 * the corners rotated back about the page centre.  Integer arithmetic, or IEEE f64 in the order written here without contraction and
 * without a transcendental, so the kernel and the HOST twins give the same bytes.
 * A word votes when its corners are finite, its quad passes the convexity test of the canonical corner order (below, rectified
 * crops), and with d = (P1 - P0) + (P2 - P3), r = (P3 - P0) + (P2 - P1) of the canonical corners (f64), qx = (int64)rint(8 d.x),
 * qy, px, py likewise: 0 < qx < 2^23, |qy| <= qx, qx^2 + qy^2 >= px^2 + py^2 (wider than tall).  S1 = the int64 sum of (qx, qy)
 * over the voting words; S2 and the count m over those of them with 4 |S1x qy - S1y qx| <= S1x qx + S1y qy (within atan(1/4) of
 * S1).  The rotation is applied iff m >= 8, S2x > 0, |S2y| <= S2x and 256 |S2y| > S2x; then nrm = sqrt(S2x S2x + S2y S2y),
 * c = S2x / nrm, s = S2y / nrm, else c = 1, s = 0.  Ordering box of a word, rotation applied and all corners finite: per corner
 * u = x - 0.5 page_w, v = y - 0.5 page_h, x' = (c u + s v) + 0.5 page_w, y' = (c v - s u) + 0.5 page_h, box = floor of the min / max
 * of x' and y'; otherwise the word's integer box as msocr_reading_order_crops forms it (truncation).
 * msocr_page_skew_host (HOST): quads_host [n][8] f32, n <= 65536 -> skew_out_host [4] = {S2x, S2y, m, applied}, cs_out_host [2] = {c, s}.
 * msocr_deskew_boxes_host (HOST): the ordering boxes [n][4] int32 for a skew / cs pair from it.
 * msocr_reading_order_deskew (DEVICE): msocr_reading_order_lines with these boxes as the ones shrunk and ordered, and as the unshrunk
 * copy of the duplicate dictionary and the re-match; crop windows, keep_out, desc_out and the line records' x0..y1 stay those of the
 * original boxes of the words at the positions.  Order and lines are those of msocr_reading_lines_host on the ordering boxes.
 * line_out / lines_out / nlines_out: all three or none (NULL).  skew_out [N][4] int64 and cs_out [N][2] f64 as above ({0, 0, 0, 0},
 * {1, 0} for a page without boxes); the rows of a page with ncrop_out = -1 stay untouched.  A page whose rotation is not applied
 * gives the outputs of msocr_reading_order_lines bit for bit.  workspace: msocr_reading_order_deskew_workspace_bytes(N, max_cand)
 * bytes, 16-B aligned. */
int msocr_page_skew_host(const float* quads_host, int n, int64_t* skew_out_host, double* cs_out_host);
int msocr_deskew_boxes_host(const float* quads_host, int n, int page_h, int page_w, const int64_t* skew_host, const double* cs_host,
                            int32_t* boxes_out_host);
int64_t msocr_reading_order_deskew_workspace_bytes(int N, int max_cand);
int msocr_reading_order_deskew(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                               int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio, int page_base,
                               int32_t* order_out, int32_t* keep_out, int32_t* desc_out, int32_t* ncrop_out, int32_t* line_out,
                               int32_t* lines_out, int32_t* nlines_out, int64_t* skew_out, double* cs_out, void* workspace,
                               void* stream);

/* ---- column-aware reading order (an extension beyond the reference, off by default: Pipeline.columns) ----
 * An XY-cut ahead of the line rule: the page is cut at its wide empty vertical and horizontal bands into regions, the regions are
 * read in order and sort_boxes_reading_order runs inside every region.  Integer arithmetic, or IEEE f64 in the order written here
 * without contraction, so the kernel and the HOST twin give the same bytes.
 * S[i] = the shrunk boxes after resolve_intersections over the whole page (with deskew: of the ordering boxes of the deskewed
 * frame).  avg_h = (exact integer sum of y1 - y0 over all n shrunk boxes) / n, gx = col_gap_ratio * avg_h, gy = row_gap_ratio * avg_h,
 * mh = col_min_height_ratio * avg_h.  Differences of coordinates are formed in int64 and converted to f64 for the comparison.
 * A region is a set of words; the root holds all words at depth 0.  A region at depth 6 or with one word is a leaf.  Otherwise the
 * vertical attempt, allowed only when (double)(max y1 - min y0 over the region) >= mh: walk the region's words in the order
 * (x0, index) with the running maximum of x1 over the words before the current one; a word starts a new segment iff
 * (double)(x0 - running maximum) >= gx; more than one segment: the segments, left to right, are the children at depth + 1.  Not
 * allowed, or one segment: the horizontal attempt, the same walk with (y0, index), y1 and gy, children top to bottom.  No cut by
 * either: a leaf.  The leaves in depth-first order are the regions in reading order.  Inside a leaf, order and lines are
 * sort_boxes_reading_order's on the leaf's shrunk boxes in ascending word index, with the LEAF's mean height behind y_tol_ratio and
 * x_gap_ratio.  Lines are numbered region-major; a line never spans two regions.  The dictionary from shrunk box to original box
 * and the first-equal-word re-match stay page-wide.  A ratio may be +inf (never cuts); NaN or a negative ratio: MSOCR_E_ARG.
 * msocr_reading_regions_host (HOST): msocr_reading_lines_host with the three ratios, and region_out_host [n]: the region of every
 * position; regions_out_host [n][6]: one record {first, count, x0, y0, x1, y1} per region, its span of positions and the union of the
 * input boxes of the words written there; *nregions_out_host (0 for n = 0).  No cap on the regions.  A page that ends as one leaf
 * gives msocr_reading_lines_host's outputs.
 * msocr_reading_order_regions (DEVICE): msocr_reading_order_deskew's arguments with the three ratios and `deskew` (1: the cut and
 * the order run in the deskewed frame; 0: on the words' own boxes, and skew_out / cs_out may be NULL and stay untouched).
 * line_out / lines_out / nlines_out: all three or none.  region_out [N][max_cand], regions_out [N][rows][6] with
 * rows = msocr_reading_order_region_rows(max_cand) = min(max_cand, 256) (the box is the union of the words' own integer boxes, as
 * in the line records), nregions_out [N]: -1 exactly where ncrop_out is -1, 0 for a page without boxes.  More than 256 regions flag
 * the page (ncrop_out = -1) like the other capacities; rows of a flagged page and rows past a page's counts stay untouched.  A page
 * that ends as one region gives the outputs of msocr_reading_order_lines (deskew = 1: of msocr_reading_order_deskew) bit for bit.
 * workspace: msocr_reading_order_regions_workspace_bytes(N, max_cand) bytes, 16-B aligned. */
int msocr_reading_regions_host(const int32_t* boxes_host, int n, double y_tol_ratio, double x_gap_ratio, double col_gap_ratio,
                               double row_gap_ratio, double col_min_height_ratio, int32_t* order_out_host, int32_t* line_out_host,
                               int32_t* lines_out_host, int32_t* nlines_out_host, int32_t* region_out_host, int32_t* regions_out_host,
                               int32_t* nregions_out_host);
int msocr_reading_order_region_rows(int max_cand);
int64_t msocr_reading_order_regions_workspace_bytes(int N, int max_cand);
int msocr_reading_order_regions(const float* boxes, const int32_t* nbox, int N, int max_cand, int page_h, int page_w,
                                int min_text_size, int img_h, int img_w, double y_tol_ratio, double x_gap_ratio, int page_base,
                                double col_gap_ratio, double row_gap_ratio, double col_min_height_ratio, int deskew,
                                int32_t* order_out, int32_t* keep_out, int32_t* desc_out, int32_t* ncrop_out, int32_t* line_out,
                                int32_t* lines_out, int32_t* nlines_out, int64_t* skew_out, double* cs_out, int32_t* region_out,
                                int32_t* regions_out, int32_t* nregions_out, void* workspace, void* stream);

/* ---- rectified word crops (an extension beyond the reference, off by default: Pipeline.rectify_crops) -----------------------
 * The canvas of a word is cut ALONG its detected quadrilateral instead of from the quad's axis-aligned window.  All arithmetic is
 * IEEE f64 in the order written here, without contraction, so the device kernels and the HOST twins give the same bytes.
 * Canonical corner order: the four cross products of consecutive edges of the polygon as stored ((P[i+1] - P[i]) x (P[i+2] - P[i+1]),
 * f64) must be non-zero and of one sign, else the quad is unusable.  Negative (counter-clockwise on screen, y pointing down): the
 * corners are walked backwards (3, 2, 1, 0).  Of the four cyclic rotations the one whose edge P0 -> P1 has the largest x1 - x0
 * wins, on equality the one whose start corner has the smallest index in the stored order: (tl, tr, br, bl) for a tilt below 45
 * degrees.  No transcendental is used.
 * Size: w = max(|P1 - P0|, |P2 - P3|), h = max(|P3 - P0|, |P2 - P1|) (sqrt of the f64 sum of squares), then ResizeAndPadA's
 * arithmetic: scale = min(img_h / h, img_w / w), new_w = max(1, rint(w * scale)), new_h likewise, both clipped to the canvas,
 * y0 = max(0, min((img_h - new_h) / 2, img_h - new_h)).
 * Fallback: an unusable quad, a non-finite corner, or w < 1 or h < 1 takes the corners (x1, y1), (x2, y1), (x2, y2), (x1, y2) of
 * the word's clamped AABB window instead, so every word that has an AABB crop has a rectified one.
 * Descriptor = 12 x int32 {page, x0, y0, x1, y1, x2, y2, x3, y3 as f32 bit patterns in canonical order, new_w, new_h, y0}.
 * Sampling: canvas pixel (cx, cy) with dx = cx < new_w and 0 <= dy = cy - y0 < new_h is the mean of Sx x Sy sub-samples,
 * Sx = clamp(ceil(w / new_w), 1, 4), Sy likewise from h / new_h (w, h recomputed from the descriptor's corners), j outer, i inner:
 * u = (dx + (i + 0.5) / Sx) / new_w, v = (dy + (j + 0.5) / Sy) / new_h,
 * p = (1-u)(1-v) P0 + u(1-v) P1 + u v P2 + (1-u) v P3, the page read at p - 0.5 with 4 taps whose indices are clamped to the page:
 * (1-fy) ((1-fx) a + fx b) + fy ((1-fx) c + fx d); value = rint(sum / (Sx Sy)) clamped to 0..255.  Every other pixel is 255.
 * An axis-aligned quad with integer corners and new_w == w, new_h == h reproduces the page window byte for byte.
 *
 * msocr_quad_crop_descriptors (DEVICE, one workgroup per page): boxes / nbox as given to msocr_reading_order_crops and its
 * order_out / keep_out / desc_out / ncrop_out -> qdesc_out [N][max_cand][12], the page's quad descriptors compacted in exactly the
 * order of desc_out (page field copied from it).  A page with ncrop < 0 is skipped: its rows stay untouched.
 * msocr_quad_crop_descriptors_host (HOST, all pointers host memory): the same arithmetic for quads_host [M][8] f32 (corners as
 * stored) and their AABB descriptors desc_host [M][8].  natural != 0: the region at its own size (new_w = max(1, rint(w)), new_h
 * likewise, y0 = 0; img_h / img_w unused) for a caller that resizes afterwards. */
int msocr_quad_crop_descriptors(const float* boxes, const int32_t* nbox, int N, int max_cand, int img_h, int img_w,
                                const int32_t* order, const int32_t* keep, const int32_t* desc, const int32_t* ncrop,
                                int32_t* qdesc_out, void* stream);
int msocr_quad_crop_descriptors_host(const float* quads_host, const int32_t* desc_host, int M, int img_h, int img_w, int natural,
                                     int32_t* qdesc_out_host);

/* pages [N][H][W][3] u8 + M quad descriptors -> canvases [M][img_h][img_w][3] u8, one workgroup per crop.  qdesc_host is the same
 * array in host memory, used only to refuse invalid descriptors before the launch (MSOCR_E_ARG), or NULL when they were produced
 * on the device: the kernel checks every descriptor itself and writes a white canvas for an invalid one.  Invalid: page outside
 * [0, N), a non-finite corner, new_w / new_h outside [1, img_w] / [1, img_h], y0 < 0 or y0 + new_h > img_h.  Corners may lie
 * anywhere (the taps are clamped to the page).  msocr_quad_crop_host is the HOST twin (all pointers host memory; an invalid
 * descriptor gives a white canvas). */
int msocr_quad_crop(const uint8_t* pages, int N, int H, int W, const int32_t* qdesc_dev, const int32_t* qdesc_host, int M,
                    int img_h, int img_w, uint8_t* canvases, void* stream);
int msocr_quad_crop_host(const uint8_t* pages_host, int N, int H, int W, const int32_t* qdesc_host, int M, int img_h, int img_w,
                         uint8_t* canvases_host);

/* ---- tiled detection of large pages (EAST(tile_size=...); an extension beyond the reference, off by default) ----------
 * A page too large for one run of the network is cut into overlapping tiles at its own resolution; the network runs on the tiles
 * as a batch and the tiles' maps are stitched into one page-sized map, behind which msocr_east_decode (scale 4), msocr_east_lanms
 * and msocr_east_box_tail (scale_x = scale_y = 1) run unchanged.  The geometry map holds offsets relative to the map pixel
 * itself, so stitching is pure data movement: both calls are bit-exact.
 * Grid of one axis of `len` pixels (detectors/_east/tiles.py::tile_grid): L32 = round_up(len, 32); n tile origins, multiples of
 * 32, ascending from 0 without gaps, the last tile ending at max(L32, tile): a page smaller than the tile has one tile, otherwise
 * the last tile is pulled back to end at L32.  Tile index = ty * nx + tx.  Every origin list is given twice, on the device for the
 * kernel and in host memory (_host) for the argument check; so are the owner tables.  The check is the one that keeps every read in
 * bounds (multiples of 32, from 0, ascending, no gap, last tile ending at max(L32, tile)); it does not hold the overlap to
 * tile / 2, which is tile_grid's own rule.
 *
 * msocr_east_tile_gather: pages [N][H][W][3] u8 -> tiles [N][ny*nx][tile_h][tile_w][3] u8 (16-byte aligned).  Tile pixel (y, x) of
 * tile (ty, tx) is page pixel (min(oy[ty] + y, H - 1), min(ox[tx] + x, W - 1)): rows and columns past the page repeat its edge
 * (at most 31 of them unless the tile is larger than the page), never a black frame.
 * msocr_east_stitch_maps: tile maps score [N][ny*nx][tile_h/4][tile_w/4] f32 and geometry [...][8] f32 -> page maps
 * score_out [N][Hm][Wm], geo_out [N][Hm][Wm][8] with Hm = round_up(H, 32) / 4, Wm likewise (all four 16-byte aligned).
 * row_tile [Hm] / col_tile [Wm] int32 name the tile row / column that OWNS each map row / column (tiles.py::owner_table: tile i
 * owns the page pixels between the middles of its overlaps with its neighbours; those cuts are multiples of 16 page pixels, so the
 * tables are constant over every 4 map pixels and a 16-byte vector of scores has one owner).  Page-map pixel (y, x) is the owner's
 * pixel (y - oy[row_tile[y]] / 4, x - ox[col_tile[x]] / 4); one whose page position (4 y, 4 x) lies outside the page (4 y >= H or
 * 4 x >= W) is 0.0f in score and geometry, so the padding never yields a box.
 * Both refuse with MSOCR_E_ARG, before any launch: a null pointer, N, H, W, ny, nx <= 0, tile_h / tile_w not a positive multiple
 * of 32, origins that are not such a grid, a table entry outside [0, n), one that changes inside a group of 4 map pixels or whose
 * map pixel lies outside its tile, a misaligned tensor (16 bytes; `pages` may start at any byte), 2^31 or more 16-byte vectors in the output, a
 * page row of 2^30 or more bytes. */
int msocr_east_tile_gather(const uint8_t* pages, int N, int H, int W, const int32_t* oy_dev, const int32_t* ox_dev,
                           const int32_t* oy_host, const int32_t* ox_host, int ny, int nx, int tile_h, int tile_w, uint8_t* tiles,
                           void* stream);
int msocr_east_stitch_maps(const float* tile_score, const float* tile_geo, int N, int H, int W, int ny, int nx, int tile_h,
                           int tile_w, const int32_t* oy_dev, const int32_t* ox_dev, const int32_t* row_tile_dev,
                           const int32_t* col_tile_dev, const int32_t* oy_host, const int32_t* ox_host, const int32_t* row_tile_host,
                           const int32_t* col_tile_host, float* score_out, float* geo_out, void* stream);

/* ---- image ingest: JPEG -> RGB on the device -------------------------------------------------------------------------
 * Replaces the file decode of read_image (detectors/_east/utils.py:477-497: cv2.imread / PIL = libjpeg-turbo defaults).
 * 8-bit baseline / extended-sequential Huffman JPEG, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart
 * markers.  msocr_jpeg_parse_host fills `info`; the Huffman stage has three forms that give the same bits: on the HOST
 * msocr_jpeg_entropy_decode_host (the serial decoder and the judge of every stream; writes the quantised coefficients, natural
 * order, component after component: [blocks_h][blocks_w][64] int16 at coef_off[c]); on the DEVICE one thread per restart interval
 * for streams WITH a restart interval (msocr_jpeg_scan_prepare_host + msocr_jpeg_entropy_decode_device below); and on the DEVICE the
 * self-synchronising decode of a serial segment, parallel inside it, for streams WITHOUT restart markers and for long intervals
 * (msocr_jpeg_sync_prepare_host + msocr_jpeg_entropy_decode_sync_device below);
 * dequantisation + inverse DCT (libjpeg "islow"), fancy chroma upsampling and YCbCr->RGB run on the DEVICE
 * (msocr_jpeg_reconstruct: coef_dev = the same array in device memory, workspace = msocr_jpeg_workspace_bytes(info) bytes,
 * rgb_out [height][width][3] u8).  msocr_jpeg_reconstruct_host is the HOST twin of the device stage (same code; all pointers
 * host memory).  Unsupported or corrupt streams: MSOCR_E_ARG / info.supported = 0 -> use the host decoder.  The reconstruction
 * entries take the sampling forms a parse produces and no other (first component 1x1, 2x1 or 2x2, every other one 1x1): an
 * `info` with anything else, h1v2 for one, is MSOCR_E_ARG and nothing is launched or written.
 * Exif orientation (tag 0x0112 of IFD0 in an APP1 "Exif" segment), which the reference's reader applies: msocr_jpeg_parse_host
 * refuses a stream whose orientation is 2..8 (msocr_jpeg_reconstruct writes upright pages only).  msocr_jpeg_parse_oriented_host is
 * the same marker walk that reports the orientation instead: *orientation_out = 1..8 (1 for an absent tag, a value outside 2..8 or
 * an unreadable Exif block); `info` is the same either way (width / height as stored in the frame header).  It refuses a stream
 * with more than one Exif APP1 segment (readers differ on which one wins: host reader).  The entropy entries below take the `info` of
 * either parse entry.  msocr_jpeg_reconstruct_oriented = msocr_jpeg_reconstruct with the orientation applied in the last write of
 * the colour stage (no extra pass over the page): source pixel (X, Y) of the W x H frame goes to
 *     orientation   2       3       4       5    6       7       8
 *     row           Y       H-1-Y   H-1-Y   X    X       W-1-X   W-1-X
 *     column        W-1-X   W-1-X   X       Y    H-1-Y   H-1-Y   Y
 * rgb_out is [height][width][3] for orientations 1..4 and [width][height][3] for 5..8; orientation 1 IS msocr_jpeg_reconstruct;
 * anything outside 1..8: MSOCR_E_ARG.  Same workspace.  msocr_jpeg_reconstruct_oriented_host is its HOST twin. */
typedef struct msocr_jpeg_info {
  int32_t width, height, ncomp;   /* ncomp 1 (grayscale) or 3 (YCbCr) */
  int32_t hs[3], vs[3];           /* sampling factors per component */
  int32_t blocks_w[3], blocks_h[3]; /* component planes in 8x8 blocks, padded to whole MCUs */
  int32_t supported;
  int64_t coef_off[3];            /* int16 elements */
  int64_t coef_total;
  uint16_t quant[3][64];          /* natural order */
} msocr_jpeg_info;
int msocr_jpeg_parse_host(const uint8_t* data_host, int64_t len, msocr_jpeg_info* info_out);
int msocr_jpeg_parse_oriented_host(const uint8_t* data_host, int64_t len, msocr_jpeg_info* info_out, int32_t* orientation_out);
int msocr_jpeg_entropy_decode_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int16_t* coef_out_host);
/* Device-side entropy decode of a BATCH of streams with restart intervals (DRI): the intervals between RSTn markers are independent
 * byte-aligned bit streams.  Host, per page (thread-safe; no state): msocr_jpeg_scan_prepare_host walks the markers of a stream
 * msocr_jpeg_parse_host accepted and writes (a) the page's descriptor — msocr_jpeg_scan_desc_bytes() opaque bytes: frame geometry,
 * Huffman tables, bytes_base = where the file's first byte sits in the batch byte buffer — and (b) one (begin, end) pair of uint32
 * byte offsets INTO THE FILE per interval.  Returns the number of intervals, or MSOCR_E_ARG (no restart interval / corrupt marker
 * sequence / more than bounds_cap intervals: use msocr_jpeg_entropy_decode_host).
 * Device: msocr_jpeg_entropy_decode_device(bytes_dev = the files' bytes as they are on disk, descs_dev [n_pages] descriptors (8-byte
 * aligned), max_intervals = the largest interval count of a page, bounds_dev = the pages' pairs one page after the other,
 * page_base_dev [n_pages][2] int64 = {where the page's coefficient array starts in coef_dev (int16 elements), index of the page's
 * first pair in bounds_dev}, coef_dev [coef_total] int16 (zero-filled by this call), status_dev [n_pages]: 0, or 1 = the page's
 * stream is bad (same verdict as msocr_jpeg_entropy_decode_host: take the host reader)).  Bit-identical coefficients to
 * msocr_jpeg_entropy_decode_host.  msocr_jpeg_entropy_decode_intervals_host is the HOST twin of the kernel (same per-interval
 * decoder; all pointers host memory). */
int64_t msocr_jpeg_scan_desc_bytes(void);
int64_t msocr_jpeg_scan_prepare_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int64_t bytes_base,
                                     void* desc_out, uint32_t* bounds_out, int64_t bounds_cap);
int msocr_jpeg_entropy_decode_device(const uint8_t* bytes_dev, const void* descs_dev, int32_t n_pages, int32_t max_intervals,
                                     const uint32_t* bounds_dev, const int64_t* page_base_dev, int16_t* coef_dev, int64_t coef_total,
                                     int32_t* status_dev, void* stream);
int msocr_jpeg_entropy_decode_intervals_host(const uint8_t* bytes_host, const void* descs_host, int32_t n_pages,
                                             const uint32_t* bounds_host, const int64_t* page_base_host, int16_t* coef_host,
                                             int64_t coef_total, int32_t* status_host);
/* Self-synchronising device entropy decode of a BATCH of streams, with or without restart intervals: every interval (a stream
 * without DRI = one interval of all its MCUs) is cut into subsequences of subseq_bytes bytes, one thread each; max_rounds rounds
 * bring their entry states to the fixed point (entry of i == exit of i - 1; a page that stands costs nothing in later rounds), a
 * prefix sum places them, a write pass scatters the coefficients with DC differences and a per-component prefix sum turns those
 * into values.  Host, per page: msocr_jpeg_sync_prepare_host = msocr_jpeg_scan_prepare_host that also takes streams without DRI
 * (one pair: first byte of the scan, first marker) and refuses files above 0x1ff00000 bytes (bit positions are 32-bit).  The caller
 * lays the subsequences out: interval k of a page has max(1, ceil((end - begin) / subseq_bytes)) of them, sub_first [one uint32 per
 * interval, the pages' one after the other like the pairs] = index inside the PAGE of the interval's first subsequence, and
 * page_base [n_pages][4] int64 = {where the page's coefficient array starts in coef (int16 elements), index of the page's first
 * pair / sub_first entry, index of the page's first subsequence in the batch, number of subsequences of the page}; max_subseq = the
 * largest of those numbers, total_subseq their sum.  workspace_dev: msocr_jpeg_sync_workspace_bytes(total_subseq, n_pages,
 * max_rounds) bytes, 8-byte aligned.  16 <= subseq_bytes <= 65536, 2 <= max_rounds <= 65536.
 * coef_dev [coef_total] is zero-filled by the call.  status_dev [n_pages]: 0 = decoded, bit-identical to
 * msocr_jpeg_entropy_decode_host; 1 = the stream is bad (exactly when msocr_jpeg_entropy_decode_host refuses it: the verdict comes
 * from the decode along the true chain of states, never from a speculative one); 2 = not decoded here, stream not judged (no fixed
 * point within max_rounds, or the data ends with more than 64 blocks of an interval outstanding, i.e. a truncated stream): decode
 * it with msocr_jpeg_entropy_decode_host.  rounds_dev [n_pages] (may be NULL): rounds that decoded something.  One launch sequence
 * per batch on `stream`, no host wait.  msocr_jpeg_entropy_decode_sync_host is the HOST twin (same functions, same rounds; all
 * pointers host memory; no workspace). */
int64_t msocr_jpeg_sync_prepare_host(const uint8_t* data_host, int64_t len, const msocr_jpeg_info* info, int64_t bytes_base,
                                     void* desc_out, uint32_t* bounds_out, int64_t bounds_cap);
int64_t msocr_jpeg_sync_workspace_bytes(int64_t total_subseq, int32_t n_pages, int32_t max_rounds);
int msocr_jpeg_entropy_decode_sync_device(const uint8_t* bytes_dev, const void* descs_dev, int32_t n_pages,
                                          const uint32_t* bounds_dev, const uint32_t* sub_first_dev, const int64_t* page_base_dev,
                                          int32_t max_subseq, int64_t total_subseq, int32_t subseq_bytes, int32_t max_rounds,
                                          int16_t* coef_dev, int64_t coef_total, int32_t* status_dev, int32_t* rounds_dev,
                                          void* workspace_dev, void* stream);
int msocr_jpeg_entropy_decode_sync_host(const uint8_t* bytes_host, const void* descs_host, int32_t n_pages,
                                        const uint32_t* bounds_host, const uint32_t* sub_first_host, const int64_t* page_base_host,
                                        int32_t subseq_bytes, int32_t max_rounds, int16_t* coef_host, int64_t coef_total,
                                        int32_t* status_host, int32_t* rounds_host);
int64_t msocr_jpeg_workspace_bytes(const msocr_jpeg_info* info);
int msocr_jpeg_reconstruct(const msocr_jpeg_info* info, const int16_t* coef_dev, void* workspace_dev, uint8_t* rgb_out_dev,
                           void* stream);
int msocr_jpeg_reconstruct_host(const msocr_jpeg_info* info, const int16_t* coef_host, uint8_t* rgb_out_host);
int msocr_jpeg_reconstruct_oriented(const msocr_jpeg_info* info, int32_t orientation, const int16_t* coef_dev, void* workspace_dev,
                                    uint8_t* rgb_out_dev, void* stream);
int msocr_jpeg_reconstruct_oriented_host(const msocr_jpeg_info* info, int32_t orientation, const int16_t* coef_host,
                                         uint8_t* rgb_out_host);

/* f32 <-> bf16 / layout helpers */
int msocr_nchw_f32_to_nhwc(const float* in, int N, int C, int H, int W, int dtype, void* out, int64_t out_ld,
                           void* stream);
int msocr_nhwc_to_nchw_f32(const void* in, int N, int C, int H, int W, int64_t in_ld, int dtype, float* out,
                           void* stream);

const char* msocr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSOCR_H */
