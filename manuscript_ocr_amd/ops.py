"""Thin tensor-level wrappers over the C ABI (device pointers + current HIP stream).

PyTorch owns memory and streams only; all arithmetic happens in libmsocr.so.
Activations are NHWC tensors [N, H, W, C] (possibly channel-slice views of a wider
concat buffer: the kernels take explicit strides / leading dimensions).
"""
import ctypes
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _native as nat


# When set to a list, the wrappers below append one record per kernel launch: (start_event, end_event, kind, work, tag), with
# the events recorded on the launch stream (torch's current stream).  bench.py turns them into the live HIP-event rooflines.
#   kind "conv_gemm": work = (algorithmic direct-convolution FLOP, FLOP the MFMAs execute, direct-form layer bytes: input + output
#                     (+ residual) + weights at the tensor dtype), tag = (M, N, K, "direct"|"winograd")
#   kind "wino_in" / "wino_out" / "se_residual" / "maxpool" / ...: work = algorithmic HBM bytes (bytes in + bytes out)
#                     ("wino_out" of a per-crop kernel of se_block: tag = (tiles, C, "chain" | "se"))
#   kind "bilstm" / "attn_beam": work = (algorithmic bytes per SURVEY.md 8d, recurrent steps of the launch)
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_end(e0, kind, work, tag=None):
    if e0 is None or PROFILE is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.append((e0, e1, kind, work, tag))


def _dt(t):
    if t.dtype == torch.float32:
        return nat.F32
    if t.dtype == torch.bfloat16:
        return nat.BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise nat.NativeError("native ops need device tensors (no CPU fallback)")


def _pixel_dense_ld(t):
    """Leading dimension (elements per pixel) of an NHWC tensor/view whose pixels are dense."""
    N, H, W, C = t.shape
    ld = t.stride(2)
    if t.stride(3) != 1 or t.stride(1) != W * ld or (N > 1 and t.stride(0) != H * W * ld) or ld < C:
        raise ValueError(f"tensor is not pixel-dense NHWC: shape {tuple(t.shape)} strides {t.stride()}")
    return ld


# Winograd F(2x2,3x3) for f32 3x3/1/1 convolutions with at least this many input channels (0 disables it).  Below 128
# channels the 16 transform-domain GEMMs have K < 128 and become HBM-bound themselves.
WINOGRAD_MIN_CIN = int(os.environ.get("MSOCR_WINOGRAD_MIN_CIN", "128"))


# Winograd workspace (V and Mw, 16 * tiles * (Cin + Cout) f32): ONE reusable arena per launch stream, grown lazily to the
# largest layer seen — calls on a stream are stream-ordered, so consecutive layers reuse the same bytes.  (A fresh torch.empty
# per call left every layer's high-water block cached in every one of the 32 stream pools: 279 GB reserved at 3072x4096.)
# Calls whose workspace would exceed WINO_WS_LIMIT are split over the batch dimension.
WINO_WS_LIMIT = int(os.environ.get("MSOCR_WINO_WS_LIMIT", str(1 << 30)))
_WINO_ARENA = {}


def _wino_workspace(nbytes, device):
    if torch.cuda.is_current_stream_capturing():  # a hipGraph capture owns its allocations (private pool)
        return torch.empty((nbytes,), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    buf = _WINO_ARENA.get(key)
    if buf is None or buf.numel() < nbytes:
        # the old block returns to the caching allocator on the stream it was allocated on: kernels already queued there
        # finish with it before any later allocation of that stream can reuse it
        buf = None
        _WINO_ARENA.pop(key, None)
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        _WINO_ARENA[key] = buf
    return buf


# Tall Winograd form F(4,3) x F(2,3) (csrc/winograd.hip, wino42_*): 24 transform points per 4x2 outputs = 3 multiplies per output
# instead of 4, V / Mw 3x instead of 4x.  Taken when it is cheaper for the map height: 24 * ceil(H/4) < 16 * ceil(H/2)
# (H = 4, 7, 8, 11, 12, >= 15 ...).  MSOCR_WINO_TALL=0 keeps every layer on F(2x2,3x3).
WINOGRAD_TALL = int(os.environ.get("MSOCR_WINO_TALL", "1"))


def _tall_pays(H):
    return 24 * (-(-H // 4)) < 16 * (-(-H // 2))


# Square form F(4,3) x F(4,3) on the points {0, +-3/2, +-2/3, inf} (csrc/winograd.hip, wino44_*; round 4): 36 points per 4x4 outputs =
# 2.25 multiplies and workspace words per output instead of 3.  Split-operand GEMMs only (precision="fp32" default); taken where it is
# cheaper than the tall form for the map width: 36 * ceil(W/4) < 24 * ceil(W/2) (_square_pays below; for W % 4 == 1 at the price of
# square tiles + tail column).  MSOCR_WINO_SQUARE=0 keeps the tall form.
# Which layers: per layer the square form's rounding error is 1.1-1.3x the tall form's on the textbook points and 2.2-2.5x the tall
# form's on the new points; end to end (tests/test_gpu_f64.py, device error against f64 relative to the reference's own f32 error,
# bound 2.0, three weight sets) the recogniser reads 1.47-1.60 all tall, 1.79-1.91 with the square form on its Cin = 512 layers
# (+4.0 % pages/s on one box: 81.6 -> 84.9) and 1.71-2.24 with it on every eligible layer (+5.9 %: 86.4) — the default is the
# largest set that holds the bound on all three: Cin >= 512 (MSOCR_WINO_SQUARE_MIN_CIN=256 takes the rest).
WINOGRAD_SQUARE = int(os.environ.get("MSOCR_WINO_SQUARE", "1"))
WINOGRAD_SQUARE_MIN_CIN = int(os.environ.get("MSOCR_WINO_SQUARE_MIN_CIN", "512"))


# Square tiles + tail column (csrc/winograd.hip, wino44_*_coltail): on a map with W % 4 == 1 the last of the ceil(W/4) square tiles holds
# one real output column and three that are thrown away (TRBA's 4 x 13 maps pay for 16 columns).  There the square pass covers the
# W // 4 full tiles and column W - 1 is one F(4,3) x F(1,3) tile per tile row, 18 points: 36 * (W // 4) + 18 point rows instead of
# 36 * (W // 4 + 1), the other columns bit for bit the same.  MSOCR_WINO_COLTAIL=0 keeps the padded tile.
WINOGRAD_COLTAIL = int(os.environ.get("MSOCR_WINO_COLTAIL", "1"))


def _coltail(W):
    return bool(WINOGRAD_COLTAIL) and W % 4 == 1 and W >= 5


def _square_pays(W):
    points = 36 * (W // 4) + 18 if _coltail(W) else 36 * (-(-W // 4))
    return points < 24 * (-(-W // 2))


# The Winograd tile forms (csrc/winograd.hip, include/msocr.h MSOCR_WINO_*): form id -> (PROFILE tag stem, transform points, output tile);
# the square form + tail column is a square-form layer to the profile: 36 points of the square tiles, then 18 of the tail column's
WINO_FORMS = {nat.WINO_2X2: ("winograd", 16, (2, 2)), nat.WINO_4X2: ("winograd42", 24, (4, 2)), nat.WINO_4X4: ("winograd44", 36, (4, 4)),
              nat.WINO_4X4_COLTAIL: ("winograd44", 36 + 18, (4, 4))}


def _wino_rows(form, nn, H, W):
    """(point rows, tiles) of nn H x W images in a form: the rows of V and of Mw, and the tiles the transform kernels run over."""
    _, npts, (mh, mw) = WINO_FORMS[form]
    TH = -(-H // mh)
    if form == nat.WINO_4X4_COLTAIL:  # 36 per square tile + 18 per tail tile
        mt44, mt41 = nn * TH * (W // 4), nn * TH
        return 36 * mt44 + 18 * mt41, mt44 + mt41
    mt = nn * TH * -(-W // mw)
    return npts * mt, mt


def _wino_weights(wh, form):
    """Host [Cout,3,3,Cin] f32 weight -> U [points, Cout, Cin] f32 (msocr_winograd_weights_host: f64, rounded once, one tile's planes
    per call); WINO_4X4_COLTAIL: [54, Cout, Cin], the WINO_4X4 form's 36 planes, then the 18 of its tail tile."""
    Cout, _, _, Cin = wh.shape
    u = torch.empty((WINO_FORMS[form][1], Cout, Cin), dtype=torch.float32)
    calls = [(nat.WINO_4X4, u[:36]), (form, u[36:])] if form == nat.WINO_4X4_COLTAIL else [(form, u)]
    for f, planes in calls:
        nat.check(nat.lib().msocr_winograd_weights_host(f, wh.data_ptr(), Cout, Cin, planes.data_ptr()), "winograd_weights_host")
    return u


# Cin == 64 layers (TRBA conv0b, the 3x3s of ResNet-50 layer1): tall Winograd with the 24 GEMMs (K = 64) and the output transform
# fused in one kernel (csrc/winograd.hip, wino42_fused64_kernel) — unfused, such a layer is HBM-bound on Mw.  conv2d(pool2=True)
# folds the following 2x2/2 max-pool into the same kernel.  MSOCR_WINO_FUSED64=0 keeps these layers on the direct kernel.
WINOGRAD_FUSED64 = int(os.environ.get("MSOCR_WINO_FUSED64", "1"))


# Split-operand f32 ("bf16x3", csrc/conv_split.hip): the f32 1x1 convolutions and the Winograd-domain GEMMs of the tall form run on
# the bf16 matrix pipes with each operand split EXACTLY into three bf16 terms (six products per f32 product, f32 accumulate; the
# dropped terms are <= 2^-25 of a product).  The weight operand is split once, here, at load time.  0 = exact-f32 MFMA everywhere
# (precision="fp32-exact" of EAST / TRBA).
SPLIT_BF16X3 = int(os.environ.get("MSOCR_SPLIT", "1"))


def split_planes(t):
    """f32 tensor (any device) -> bf16 tensor [3, *t.shape] on t's device with t == p0 + p1 + p2 exactly (msocr_split_bf16x3_host)."""
    th = t.detach().float().cpu().contiguous()
    planes = torch.empty((3,) + tuple(th.shape), dtype=torch.int16)
    nat.check(nat.lib().msocr_split_bf16x3_host(th.data_ptr(), th.numel(), planes.data_ptr()), "split_bf16x3_host")
    return planes.view(torch.bfloat16).to(t.device)


def split_planes_ktile(t, nbatch, rows):
    """f32 tensor viewed as [nbatch][rows][k] -> bf16 planes [3, nbatch, k/32, rows, 32] on t's device: the K-tile-major layout the
    split-operand GEMM kernels read (msocr_split_bf16x3_ktile_host; include/msocr.h says why)."""
    th = t.detach().float().cpu().contiguous()
    k = th.numel() // (nbatch * rows)
    assert k % 32 == 0 and nbatch * rows * k == th.numel()
    planes = torch.empty((3, nbatch, k // 32, rows, 32), dtype=torch.int16)
    nat.check(nat.lib().msocr_split_bf16x3_ktile_host(th.data_ptr(), nbatch, rows, k, planes.data_ptr()), "split_bf16x3_ktile_host")
    return planes.view(torch.bfloat16).to(t.device)


def unsplit_planes_ktile(planes):
    """Inverse of split_planes_ktile for tests: planes [3, nb, k/32, rows, 32] -> f32 [nb, rows, k] = p0 + p1 + p2."""
    nb, kt, rows = planes.shape[1:4]
    return planes.float().sum(0).permute(0, 2, 1, 3).reshape(nb, rows, kt * 32)


# Below this reduction length (KH * KW * Cin) a convolution stays on the exact-f32 kernel: the split kernel's K-tiles of 32 with two
# barriers each lose to the exact lean kernel's K-tiles of 16 at K = 64 (55 against 64 TFLOP/s, profiles/r03_conv_layers_split_all.txt;
# these layers sit at 0.78 of their HBM roofline anyway).  Whole pipeline, same box, after the split kernel lost its spill:
# 70.4 / 70.9 / 71.2 pages/s with the threshold at 256 / 192 / 128.
SPLIT_MIN_K = int(os.environ.get("MSOCR_SPLIT_MIN_K", "128"))


def _split_eligible(w):
    Cout, KH, KW, Cin = w.shape
    return w.dtype == torch.float32 and Cin % 32 == 0 and Cout % 64 == 0 and KH * KW * Cin >= SPLIT_MIN_K


def attach_split(w, split=None):
    """Load-time: give a [Cout,1,1,Cin] f32 device weight its three bf16 planes (conv2d() then takes the split-operand kernels);
    split=False marks the weight as exact-f32 only (precision="fp32-exact").  Weights of other kernel sizes get their planes on
    first use as a strided / non-Winograd convolution (conv2d), so a 3x3 weight that only ever runs as Winograd holds none."""
    if split is False:
        w._msocr_nosplit = True
        return w
    Cout, KH, KW, Cin = w.shape
    if (SPLIT_BF16X3 if split is None else split) and KH == 1 and KW == 1 and _split_eligible(w):
        w._msocr_split = split_planes_ktile(w, 1, Cout)
    return w


def attach_winograd(w, split=None, square=True):
    """Load-time: give a [Cout,3,3,Cin] f32 device weight its transform-domain twins U = G g G^T ([16,Cout,Cin] f32 for F(2x2,3x3),
    [24,Cout,Cin] for the tall form F(4,3) x F(2,3), planes of [36,Cout,Cin] for the square form; computed on the host in f64 by
    msocr_winograd_weights_host).  conv2d() then takes the Winograd path for 3x3/1/1 calls."""
    Cout, KH, KW, Cin = w.shape
    if (WINOGRAD_MIN_CIN and WINOGRAD_FUSED64 and WINOGRAD_TALL and w.dtype == torch.float32 and KH == 3 and KW == 3 and Cin == 64
            and Cin < WINOGRAD_MIN_CIN and Cout % 32 == 0):
        u42 = _wino_weights(w.detach().cpu().contiguous(), nat.WINO_4X2)
        w._msocr_wino42_fused = u42.to(w.device)
        # the K = 64 GEMMs on the bf16 pipes pay only for the wide layer (TRBA conv0b, 64 -> 128 + pool: 2.43 -> 2.21 ms per 960 crops);
        # with 64 output channels the kernel is bound by staging and barriers either way (0.84 -> 0.86 ms) and stays exact.
        # Cout % 64 == 0 takes wino42_fused64_v2_kernel, which is split whatever Cout.
        if (SPLIT_BF16X3 if split is None else split) and (Cout % 64 == 0 or Cout >= 128):
            w._msocr_wino42_fused_split = split_planes(u42).to(w.device)  # [3][24][Cout][64] bf16
        return w
    if not (WINOGRAD_MIN_CIN and w.dtype == torch.float32 and KH == 3 and KW == 3 and Cin >= WINOGRAD_MIN_CIN and Cin % 16 == 0
            and Cout % 32 == 0):
        return w
    wh = w.detach().cpu().contiguous()
    w._msocr_wino = _wino_weights(wh, nat.WINO_2X2).to(w.device)
    u42 = _wino_weights(wh, nat.WINO_4X2)
    w._msocr_wino42 = u42.to(w.device)
    if (SPLIT_BF16X3 if split is None else split) and Cin % 32 == 0 and Cout % 64 == 0:
        w._msocr_wino42_split = split_planes_ktile(u42, 24, Cout).to(w.device)  # [3][24][Cin/32][Cout][32] bf16
        if WINOGRAD_SQUARE and square and Cin >= WINOGRAD_SQUARE_MIN_CIN:  # square=False: the caller keeps this layer on the tall form (half the rounding error)
            # ONE buffer, as the 4X4_COLTAIL form reads it: the split of the square form's 36 planes, then the split of the tail column's 18;
            # the 4X4 form reads the first group alone
            u54 = _wino_weights(wh, nat.WINO_4X4_COLTAIL)
            p44, p41 = split_planes_ktile(u54[:36], 36, Cout), split_planes_ktile(u54[36:], 18, Cout)
            w._msocr_wino44ct_split = torch.cat([p44.reshape(-1), p41.reshape(-1)]).to(w.device)
            w._msocr_wino44_split = w._msocr_wino44ct_split[:p44.numel()].view(p44.shape)  # [3][36][Cin/32][Cout][32] bf16
            w._msocr_wino41_split = w._msocr_wino44ct_split[p44.numel():].view(p41.shape)  # [3][18][Cin/32][Cout][32] bf16: the tail column
    return w


def _wino_stage_in(d, form, xp, ws, what):
    """The input transform of d's images at xp into the workspace, as one "wino_in" record."""
    rows, mt = _wino_rows(form, d.N, d.H, d.W)
    e = _prof_begin()
    nat.check(nat.lib().msocr_winograd_input_transform(ctypes.byref(d), form, xp, ws.data_ptr(), _stream()), what)
    _prof_end(e, "wino_in", 4.0 * (d.N * d.H * d.W * d.Cin + rows * d.Cin), (mt, d.Cin))


def _wino_stage_gemm(d, form, split, u, ws, what, alg, name, out_px, res_io, fused_tail=None):
    """The transform-domain GEMMs of d's images as one "conv_gemm" record (alg: the algorithmic FLOP of these images); fused_tail =
    (bias, residual, out) pointers: the Cin = 64 kernel, which holds the output transform too."""
    rows, _ = _wino_rows(form, d.N, d.H, d.W)
    e = _prof_begin()
    if fused_tail is not None:
        rc = nat.lib().msocr_winograd_fused64_gemm_output(ctypes.byref(d), int(split), u.data_ptr(), ws.data_ptr(), *fused_tail, _stream())
    else:
        rc = nat.lib().msocr_winograd_gemm(ctypes.byref(d), form, int(split), u.data_ptr(), ws.data_ptr(), _stream())
    nat.check(rc, what)
    io = 4 * (d.N * d.H * d.W * d.Cin + d.N * out_px * d.Cout * res_io + d.Cout * 9 * d.Cin)
    _prof_end(e, "conv_gemm", (alg, 2.0 * rows * d.Cin * d.Cout, io), (d.N * d.H * d.W, d.Cout, 9 * d.Cin, name))


def _winograd(d, x, w, u, form, split, bias, residual, out, alg, fused=False, pool2=False):
    """One Winograd convolution described by d (3x3/1/1, f32) in the given form: the workspace from the per-stream arena, the batch cut
    so that it stays under WINO_WS_LIMIT, and per part either the one-call entry point or — with PROFILE on — the stages one by one,
    one event pair each.  fused: the Cin = 64 tall form with the GEMMs and the output transform (+ the 2x2 max-pool) in one kernel.
    The square form + tail column is still ONE conv_gemm record, spanning both GEMM launches."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    name = WINO_FORMS[form][0] + ("_fused" if fused else "") + ("_split" if split else "")
    L = nat.lib()
    nbytes = L.msocr_winograd_fused64_workspace_bytes(ctypes.byref(d)) if fused else L.msocr_winograd_workspace_bytes(ctypes.byref(d), form)
    if nbytes < 0:
        raise nat.NativeError(f"{name}: unsupported shape {tuple(x.shape)} * {tuple(w.shape)} pool2={pool2}")
    parts = min(N, -(-nbytes // WINO_WS_LIMIT))  # images per call such that the workspace stays under the limit
    per = -(-N // parts)
    ws = _wino_workspace(nbytes if parts == 1 else (nbytes // N) * per, x.device)
    bp = bias.data_ptr() if bias is not None else None
    what = f"msocr_conv3x3_{name} {tuple(x.shape)} * {tuple(w.shape)}"
    out_px = H * W // (4 if pool2 else 1)
    res_io = 2 if residual is not None else 1
    for n0 in range(0, N, per):
        n1 = min(N, n0 + per)
        d.N = n1 - n0
        xp, rp, op = x[n0:n1].data_ptr(), (residual[n0:n1].data_ptr() if residual is not None else None), out[n0:n1].data_ptr()
        if PROFILE is None:
            if fused:
                rc = L.msocr_conv3x3_winograd_fused64(ctypes.byref(d), int(split), xp, u.data_ptr(), bp, rp, op, ws.data_ptr(), _stream())
            else:
                rc = L.msocr_conv3x3_winograd(ctypes.byref(d), form, int(split), xp, u.data_ptr(), bp, rp, op, ws.data_ptr(), _stream())
            nat.check(rc, what)
            continue
        nn = n1 - n0
        rows, mt = _wino_rows(form, nn, H, W)
        _wino_stage_in(d, form, xp, ws, what)
        _wino_stage_gemm(d, form, split, u, ws, what, alg * nn / N, name, out_px, res_io, (bp, rp, op) if fused else None)
        if not fused:
            e = _prof_begin()
            nat.check(L.msocr_winograd_output_transform(ctypes.byref(d), form, ws.data_ptr(), bp, rp, op, _stream()), what)
            _prof_end(e, "wino_out", 4.0 * (rows * Cout + nn * H * W * Cout * res_io), (mt, Cout))
    d.N = N


def _wino_form(w, H, W):
    """(form, U, split) of the unfused Winograd path for a 3x3/1/1 call of weight w (attach_winograd) on H x W maps."""
    form, u, split = nat.WINO_2X2, w._msocr_wino, False
    if WINOGRAD_TALL and _tall_pays(H) and getattr(w, "_msocr_wino42", None) is not None:
        form, u = nat.WINO_4X2, w._msocr_wino42
        up = getattr(w, "_msocr_wino42_split", None)
        if up is not None and SPLIT_BF16X3:  # the 24 GEMMs on the bf16 pipes with exactly split operands
            u, split = up, True
        up44 = getattr(w, "_msocr_wino44ct_split", None)  # the 4X4 form reads the first 36 planes of the buffer, the composite all 54
        if up44 is not None and SPLIT_BF16X3 and WINOGRAD_SQUARE and _square_pays(W):
            form, u, split = nat.WINO_4X4_COLTAIL if _coltail(W) else nat.WINO_4X4, up44, True
    return form, u, split


def conv2d(x, w, bias, stride=(1, 1), pad=(0, 0), relu=False, residual=None, out=None, out_hw=None, alg_k=None, pool2=False):
    """x [N,H,W,Cin] (any N/H/W strides, channel stride 1), w [Cout,KH,KW,Cin], bias f32 [Cout] or None.
    alg_k: algorithmic reduction length when the packed K is padded (stem), for FLOP accounting only.
    pool2: return maxpool2x2/2 of the result (fused into the convolution where the fused Cin = 64 kernel applies, else a second
    kernel)."""
    _need_cuda(x, w, bias, residual, out)
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cw = w.shape
    assert Cw == Cin and w.is_contiguous() and w.dtype == x.dtype and x.stride(3) == 1
    sh, sw = stride
    ph, pw = pad
    Ho, Wo = out_hw if out_hw else ((H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1)
    wino = (sh, sw, ph, pw) == (1, 1, 1, 1) and (Ho, Wo) == (H, W)
    fused = (getattr(w, "_msocr_wino42_fused", None) is not None and WINOGRAD_FUSED64 and WINOGRAD_TALL and wino and _tall_pays(H)
             and (not pool2 or (H % 2 == 0 and W % 2 == 0 and residual is None)))
    if pool2 and not fused:
        return maxpool2d(conv2d(x, w, bias, stride, pad, relu, residual, None, out_hw, alg_k), 2, 2, 0, out=out)
    u = getattr(w, "_msocr_wino", None)
    use_wino = u is not None and wino
    oh, ow = (Ho // 2, Wo // 2) if pool2 else (Ho, Wo)
    if out is None:
        out = torch.empty((N, oh, ow, Cout), dtype=x.dtype, device=x.device)
    assert out.shape == (N, oh, ow, Cout) and out.dtype == x.dtype
    d = nat.ConvDesc()
    d.dtype = _dt(x)
    d.N, d.H, d.W, d.Cin = N, H, W, Cin
    d.in_sN, d.in_sH, d.in_sW = x.stride(0), x.stride(1), x.stride(2)
    d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = KH, KW, sh, sw, ph, pw
    d.Ho, d.Wo, d.Cout = Ho, Wo, Cout
    d.out_ld = _pixel_dense_ld(out)
    flags = (nat.CONV_RELU if relu else 0) | (nat.CONV_POOL2 if pool2 else 0)
    rp = None
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == x.dtype
        d.res_ld = _pixel_dense_ld(residual)
        flags |= nat.CONV_RESIDUAL
        rp = residual.data_ptr()
    d.flags = flags
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == Cout and bias.is_contiguous()
    bp = bias.data_ptr() if bias is not None else None
    alg = 2.0 * N * Ho * Wo * Cout * (alg_k if alg_k else KH * KW * Cin)  # ALGORITHMIC direct-convolution FLOP (2 * MACs)
    if fused:  # Cin == 64: the 24 GEMMs (on the bf16 pipes with exactly split operands where the planes exist) + output transform
        up = getattr(w, "_msocr_wino42_fused_split", None) if SPLIT_BF16X3 else None
        u = w._msocr_wino42_fused if up is None else up
        _winograd(d, x, w, u, nat.WINO_4X2, up is not None, bias, residual, out, alg, fused=True, pool2=pool2)
    elif use_wino:
        form, u, split = _wino_form(w, H, W)
        _winograd(d, x, w, u, form, split, bias, residual, out, alg)
    else:
        wp = getattr(w, "_msocr_split", None)
        if (wp is None and SPLIT_BF16X3 and not getattr(w, "_msocr_nosplit", False) and _split_eligible(w)
                and not torch.cuda.is_current_stream_capturing()):
            wp = w._msocr_split = split_planes_ktile(w, 1, Cout)  # first use of this weight outside the Winograd path: split once, keep
        split = wp is not None and SPLIT_BF16X3 and KH * KW * Cin >= SPLIT_MIN_K and all(v % 4 == 0 for v in x.stride()[:3])
        lean = (split and (KH, KW, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0) and (Ho, Wo) == (H, W)
                and (H == 1 or x.stride(1) == W * x.stride(2)) and (N == 1 or x.stride(0) == H * W * x.stride(2)))
        e = _prof_begin()
        if split:
            fn = nat.lib().msocr_conv1x1_split if lean else nat.lib().msocr_conv2d_split
            rc = fn(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), bp, rp, out.data_ptr(), _stream())
            nat.check(rc, f"msocr_conv{'1x1' if lean else '2d'}_split {tuple(x.shape)} * {tuple(w.shape)}")
        else:
            rc = nat.lib().msocr_conv2d(ctypes.byref(d), x.data_ptr(), w.data_ptr(), bp, rp, out.data_ptr(), _stream())
            nat.check(rc, f"msocr_conv2d {tuple(x.shape)} * {tuple(w.shape)}")
        io = x.element_size() * (N * H * W * Cin + N * Ho * Wo * Cout * (2 if residual is not None else 1) + Cout * KH * KW * Cin)
        _prof_end(e, "conv_gemm", (alg, 2.0 * N * Ho * Wo * Cout * KH * KW * Cin, io),
                  (N * Ho * Wo, Cout, KH * KW * Cin, "direct_split" if split else "direct"))
    return out


def normalize_u8(imgs_u8, pad_t, pad_l, Hp, Wp, mode, dtype, cpad=4):
    """imgs [N,H,W,3] u8 (device) -> [N,Hp,Wp,cpad] normalised, zero canvas (mode 0 EAST, 1 TRBA)."""
    _need_cuda(imgs_u8)
    N, H, W, C = imgs_u8.shape
    assert C == 3 and imgs_u8.dtype == torch.uint8 and imgs_u8.is_contiguous()
    out = torch.empty((N, Hp, Wp, cpad), dtype=dtype, device=imgs_u8.device)
    nat.check(nat.lib().msocr_normalize_u8(imgs_u8.data_ptr(), N, H, W, pad_t, pad_l, Hp, Wp, cpad, mode, _dt(out), out.data_ptr(),
                                           _stream()),
              "normalize_u8")
    return out


def resize_linear_u8(src, dh, dw):
    _need_cuda(src)
    N, sh, sw, C = src.shape
    assert C == 3 and src.dtype == torch.uint8 and src.is_contiguous()
    dst = torch.empty((N, dh, dw, 3), dtype=torch.uint8, device=src.device)
    nat.check(nat.lib().msocr_resize_linear_u8(src.data_ptr(), N, sh, sw, dst.data_ptr(), dh, dw, _stream()), "resize_linear_u8")
    return dst


def maxpool2d(x, k, s, p, out=None):
    _need_cuda(x, out)
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    e = _prof_begin()
    nat.check(nat.lib().msocr_maxpool2d(x.data_ptr(), N, H, W, C, _pixel_dense_ld(x), k, s, p, _dt(x), out.data_ptr(), Ho, Wo,
                                        _pixel_dense_ld(out), _stream()), "maxpool2d")
    _prof_end(e, "maxpool", float(x.element_size()) * N * C * (H * W + Ho * Wo))
    return out


def upsample2x_into(x, out):
    """Bilinear x2 of x [N,H,W,C] into out[..., :C] (out is [N,2H,2W,Ctot] or a channel-slice view)."""
    _need_cuda(x, out)
    N, H, W, C = x.shape
    assert out.shape[0] == N and out.shape[1] == 2 * H and out.shape[2] == 2 * W and out.dtype == x.dtype
    nat.check(nat.lib().msocr_upsample2x_bilinear(x.data_ptr(), N, H, W, C, _pixel_dense_ld(x), _dt(x), out.data_ptr(),
                                                  _pixel_dense_ld(out), _stream()), "upsample2x")
    return out


def east_head(h1, w9, b9, score=None, geo=None):
    _need_cuda(h1, w9, b9)
    N, H, W, C = h1.shape
    assert C == 32 and w9.shape == (9, 32) and w9.dtype == torch.float32
    if score is None:
        score = torch.empty((N, H, W), dtype=torch.float32, device=h1.device)
    if geo is None:
        geo = torch.empty((N, H, W, 8), dtype=torch.float32, device=h1.device)
    nat.check(nat.lib().msocr_east_head(h1.data_ptr(), N * H * W, _pixel_dense_ld(h1), _dt(h1), w9.data_ptr(), b9.data_ptr(),
                                        score.data_ptr(), geo.data_ptr(), _stream()), "east_head")
    return score, geo


def east_decode(score, geo, thresh, scale, quant, max_cand):
    """score [N,H,W] f32, geo [N,H,W,8] f32 -> cand [N,max_cand,9] f32, counts [N] int32."""
    _need_cuda(score, geo)
    N, H, W = score.shape
    assert score.dtype == torch.float32 and geo.shape == (N, H, W, 8) and score.is_contiguous() and geo.is_contiguous()
    cand = torch.empty((N, max_cand, 9), dtype=torch.float32, device=score.device)
    counts = torch.empty((N,), dtype=torch.int32, device=score.device)
    nat.check(nat.lib().msocr_east_decode(score.data_ptr(), geo.data_ptr(), N, H, W, float(thresh), float(scale), int(quant),
                                          cand.data_ptr(), counts.data_ptr(), max_cand, _stream()), "east_decode")
    return cand, counts


def east_lanms(cand, counts, iou_thr, workspace=None):
    _need_cuda(cand, counts)
    N, max_cand, _ = cand.shape
    if workspace is None:
        nbytes = nat.lib().msocr_lanms_workspace_bytes(N, max_cand)
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=cand.device)
    boxes = torch.empty_like(cand)
    nbox = torch.empty((N,), dtype=torch.int32, device=cand.device)
    nat.check(nat.lib().msocr_east_lanms(cand.data_ptr(), counts.data_ptr(), N, max_cand, float(iou_thr), boxes.data_ptr(),
                                         nbox.data_ptr(), workspace.data_ptr(), _stream()), "east_lanms")
    return boxes, nbox


def east_box_tail(boxes, nbox, expand_w, expand_h, scale_x, scale_y, axis_aligned, remove_anomalies, sigma, min_count, workspace=None):
    """boxes [N,max_cand,9] f32 + nbox [N] i32 (device, from east_lanms) -> (final boxes [N,max_cand,9], counts [N] i32; -1 = page
    with more than min(max_cand, 16384) boxes, to be finished by the host path).  expand / scale / contained / anomalies / axis-aligned."""
    _need_cuda(boxes, nbox)
    N, max_cand, _ = boxes.shape
    ws = workspace
    if ws is None:
        ws = torch.empty((nat.lib().msocr_east_box_tail_workspace_bytes(N, max_cand),), dtype=torch.uint8, device=boxes.device)
    out = torch.empty_like(boxes)
    n_out = torch.empty((N,), dtype=torch.int32, device=boxes.device)
    nat.check(nat.lib().msocr_east_box_tail(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, float(expand_w), float(expand_h),
                                            float(scale_x), float(scale_y), int(bool(axis_aligned)), int(bool(remove_anomalies)),
                                            float(sigma), int(min_count), out.data_ptr(), n_out.data_ptr(), ws.data_ptr(), _stream()),
              "east_box_tail")
    return out, n_out


# ------------------------------------------------------------------------------------------- tiled detection
class TileTables(NamedTuple):
    """A tile grid (detectors/_east/tiles.py::PageGrid) with its four int32 arrays also on the device."""
    grid: tuple          # the PageGrid: host arrays, read by the argument checks of the C ABI
    oy: torch.Tensor
    ox: torch.Tensor
    row_tile: torch.Tensor
    col_tile: torch.Tensor


def east_tile_tables(grid, device):
    host = [np.ascontiguousarray(a, dtype=np.int32) for a in (grid.oy, grid.ox, grid.row_tile, grid.col_tile)]
    grid = grid._replace(oy=host[0], ox=host[1], row_tile=host[2], col_tile=host[3])
    return TileTables(grid, *[torch.from_numpy(a).to(device) for a in host])


def east_tile_gather(pages_u8, tables):
    """pages [N,H,W,3] u8 device + the tables of the grid of an H x W page -> tiles [N, ny*nx, tile_h, tile_w, 3] u8, clamped to
    the page's edge (msocr_east_tile_gather)."""
    _need_cuda(pages_u8)
    g = tables.grid
    N, H, W, C = pages_u8.shape
    assert C == 3 and pages_u8.dtype == torch.uint8 and pages_u8.is_contiguous() and (H, W) == (g.H, g.W)
    tiles = torch.empty((N, g.ntiles, g.tile_h, g.tile_w, 3), dtype=torch.uint8, device=pages_u8.device)
    nat.check(nat.lib().msocr_east_tile_gather(pages_u8.data_ptr(), N, H, W, tables.oy.data_ptr(), tables.ox.data_ptr(),
                                               g.oy.ctypes.data, g.ox.ctypes.data, g.ny, g.nx, g.tile_h, g.tile_w, tiles.data_ptr(),
                                               _stream()), "east_tile_gather")
    return tiles


def east_stitch_maps(tile_score, tile_geo, tables):
    """Tile maps score [N,T,th/4,tw/4] f32 + geo [N,T,th/4,tw/4,8] f32 -> page maps score [N,Hm,Wm], geo [N,Hm,Wm,8]: every pixel
    from the tile that owns it, zeros outside the page (msocr_east_stitch_maps)."""
    _need_cuda(tile_score, tile_geo)
    g = tables.grid
    N = int(tile_score.shape[0])
    assert tile_score.dtype == torch.float32 and tile_geo.dtype == torch.float32 and tile_score.is_contiguous() and tile_geo.is_contiguous()
    assert tuple(tile_score.shape) == (N, g.ntiles, g.tile_h // 4, g.tile_w // 4) and tuple(tile_geo.shape) == tuple(tile_score.shape) + (8,)
    Hm, Wm = g.map_hw
    score = torch.empty((N, Hm, Wm), dtype=torch.float32, device=tile_score.device)
    geo = torch.empty((N, Hm, Wm, 8), dtype=torch.float32, device=tile_score.device)
    nat.check(nat.lib().msocr_east_stitch_maps(tile_score.data_ptr(), tile_geo.data_ptr(), N, g.H, g.W, g.ny, g.nx, g.tile_h, g.tile_w,
                                               tables.oy.data_ptr(), tables.ox.data_ptr(), tables.row_tile.data_ptr(),
                                               tables.col_tile.data_ptr(), g.oy.ctypes.data, g.ox.ctypes.data, g.row_tile.ctypes.data,
                                               g.col_tile.ctypes.data, score.data_ptr(), geo.data_ptr(), _stream()), "east_stitch_maps")
    return score, geo


class ReadingOrder(NamedTuple):
    """Result of `reading_order_crops`, per page, on the device."""
    order: torch.Tensor  # [N,max_cand] i32: the words in reading order
    keep: torch.Tensor   # [N,max_cand] i32: which positions of that order yield a crop
    desc: torch.Tensor   # [N,max_cand,8] i32: the kept words' crop descriptors, compacted
    ncrop: torch.Tensor  # [N] i32: crops per page; -1 = the page takes the host path


def reading_order_crops(boxes, nbox, page_hw, min_text_size, img_h, img_w, page_base=0, y_tol_ratio=0.6, x_gap_ratio=float("inf"),
                        workspace=None):
    """Final boxes [N,max_cand,9] f32 + counts [N] i32 (device, from east_box_tail) -> per page, on the device: reading order of
    the words, which positions yield a crop, and the crop descriptors for crop_resize_pad (msocr_reading_order_crops).
    Returns a ReadingOrder."""
    _need_cuda(boxes, nbox)
    N, max_cand, _ = boxes.shape
    dev = boxes.device
    ws = workspace
    if ws is None:
        ws = torch.empty((nat.lib().msocr_reading_order_workspace_bytes(N, max_cand),), dtype=torch.uint8, device=dev)
    order = torch.empty((N, max_cand), dtype=torch.int32, device=dev)
    keep = torch.empty((N, max_cand), dtype=torch.int32, device=dev)
    desc = torch.empty((N, max_cand, 8), dtype=torch.int32, device=dev)
    ncrop = torch.empty((N,), dtype=torch.int32, device=dev)
    nat.check(nat.lib().msocr_reading_order_crops(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, int(page_hw[0]), int(page_hw[1]),
                                                  int(min_text_size), int(img_h), int(img_w), float(y_tol_ratio), float(x_gap_ratio),
                                                  int(page_base), order.data_ptr(), keep.data_ptr(), desc.data_ptr(), ncrop.data_ptr(),
                                                  ws.data_ptr(), _stream()), "reading_order_crops")
    return ReadingOrder(order, keep, desc, ncrop)


class ReadingLines(NamedTuple):
    """The text lines behind a ReadingOrder (`reading_order_lines`), per page, on the device."""
    line: torch.Tensor    # [N,max_cand] i32: the line of every position of `order`, lines numbered in reading order
    lines: torch.Tensor   # [N,rows,6] i32: per line {first, count, x0, y0, x1, y1}: its span of positions and the union of its words' boxes
    nlines: torch.Tensor  # [N] i32: lines per page; -1 exactly where ncrop is -1


def reading_order_lines(boxes, nbox, page_hw, min_text_size, img_h, img_w, page_base=0, y_tol_ratio=0.6, x_gap_ratio=float("inf"),
                        workspace=None):
    """reading_order_crops that also returns the text lines the order is built from (msocr_reading_order_lines): the same
    ReadingOrder bit for bit, and a ReadingLines.  Returns (ReadingOrder, ReadingLines)."""
    _need_cuda(boxes, nbox)
    N, max_cand, _ = boxes.shape
    dev = boxes.device
    ws = workspace
    if ws is None:
        ws = torch.empty((nat.lib().msocr_reading_order_workspace_bytes(N, max_cand),), dtype=torch.uint8, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    ro = ReadingOrder(i32(N, max_cand), i32(N, max_cand), i32(N, max_cand, 8), i32(N))
    rl = ReadingLines(i32(N, max_cand), i32(N, nat.lib().msocr_reading_order_line_rows(max_cand), 6), i32(N))
    nat.check(nat.lib().msocr_reading_order_lines(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, int(page_hw[0]), int(page_hw[1]),
                                                  int(min_text_size), int(img_h), int(img_w), float(y_tol_ratio), float(x_gap_ratio),
                                                  int(page_base), *[t.data_ptr() for t in ro + rl], ws.data_ptr(), _stream()),
              "reading_order_lines")
    return ro, rl


def reading_lines_host(aabbs_i32, y_tol_ratio=0.6, x_gap_ratio=float("inf")):
    """Integer word boxes [n,4] (x_min, y_min, x_max, y_max) -> (order [n], line [n], lines [L,6]) as numpy int32, through the host
    twin msocr_reading_lines_host: the reading order, the line of every position and per line {first, count, x0, y0, x1, y1}."""
    boxes = np.ascontiguousarray(aabbs_i32, dtype=np.int32).reshape(-1, 4)
    n = len(boxes)
    order, line, lines = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((n, 6), dtype=np.int32)
    nlines = np.zeros(1, dtype=np.int32)
    nat.check(nat.lib().msocr_reading_lines_host(boxes.ctypes.data, n, float(y_tol_ratio), float(x_gap_ratio), order.ctypes.data,
                                                 line.ctypes.data, lines.ctypes.data, nlines.ctypes.data), "reading_lines_host")
    return order, line, lines[:int(nlines[0])].copy()


class PageSkew(NamedTuple):
    """The skew estimate behind a deskewed ReadingOrder (`reading_order_deskew`), per page, on the device."""
    skew: torch.Tensor  # [N,4] i64 {S2x, S2y, m, applied}: the summed word directions in 1/16 px, the words in the sum, 1 = rotated
    cs: torch.Tensor    # [N,2] f64 {c, s}: the rotation the ordering boxes were formed with; {1, 0} where none was applied


def reading_order_deskew(boxes, nbox, page_hw, min_text_size, img_h, img_w, page_base=0, y_tol_ratio=0.6, x_gap_ratio=float("inf"),
                         workspace=None, lines=True):
    """reading_order_lines in the deskewed frame (msocr_reading_order_deskew): the page's skew is estimated
    from the quads and the order and lines are those of the rotated corners' boxes; keep, desc and the line records' boxes stay those
    of the original boxes.  The rows of `skew` / `cs` of a page with ncrop = -1 are undefined.  lines=False: without the three line
    outputs.  Returns (ReadingOrder, ReadingLines or None, PageSkew)."""
    _need_cuda(boxes, nbox)
    N, max_cand, _ = boxes.shape
    dev = boxes.device
    ws = workspace
    if ws is None:
        ws = torch.empty((nat.lib().msocr_reading_order_deskew_workspace_bytes(N, max_cand),), dtype=torch.uint8, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    ro = ReadingOrder(i32(N, max_cand), i32(N, max_cand), i32(N, max_cand, 8), i32(N))
    rl = ReadingLines(i32(N, max_cand), i32(N, nat.lib().msocr_reading_order_line_rows(max_cand), 6), i32(N)) if lines else None
    sk = PageSkew(torch.empty((N, 4), dtype=torch.int64, device=dev), torch.empty((N, 2), dtype=torch.float64, device=dev))
    nat.check(nat.lib().msocr_reading_order_deskew(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, int(page_hw[0]), int(page_hw[1]),
                                                   int(min_text_size), int(img_h), int(img_w), float(y_tol_ratio), float(x_gap_ratio),
                                                   int(page_base), *[t.data_ptr() for t in ro], *([t.data_ptr() for t in rl] if lines else [None] * 3),
                                                   sk.skew.data_ptr(), sk.cs.data_ptr(), ws.data_ptr(), _stream()), "reading_order_deskew")
    return ro, rl, sk


def page_skew_host(quads):
    """Word quads [n,4,2] or [n,8] (x, y per corner as stored) -> (skew int64 [4] = {S2x, S2y, m, applied}, cs f64 [2] = {c, s}) through
    the host twin msocr_page_skew_host.  skew_deg = degrees(atan2(S2y, S2x)) is the caller's, for reporting."""
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    skew, cs = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.float64)
    nat.check(nat.lib().msocr_page_skew_host(q.ctypes.data, len(q), skew.ctypes.data, cs.ctypes.data), "page_skew_host")
    return skew, cs


def deskew_boxes_host(quads, page_hw, skew, cs):
    """Word quads [n,4,2] or [n,8] + a (skew, cs) of page_skew_host -> the ordering boxes int32 [n,4] of the deskewed frame through the
    host twin msocr_deskew_boxes_host: the words' integer boxes themselves where the rotation is not applied (skew[3] = 0)."""
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    skew, cs = np.ascontiguousarray(skew, dtype=np.int64), np.ascontiguousarray(cs, dtype=np.float64)
    assert skew.shape == (4,) and cs.shape == (2,)
    out = np.empty((len(q), 4), dtype=np.int32)
    nat.check(nat.lib().msocr_deskew_boxes_host(q.ctypes.data, len(q), int(page_hw[0]), int(page_hw[1]), skew.ctypes.data, cs.ctypes.data,
                                                out.ctypes.data), "deskew_boxes_host")
    return out


COLUMN_PARAMS = {"col_gap_ratio": 2.0, "row_gap_ratio": 1.5, "col_min_height_ratio": 3.0}  # placeholders, not tuned values


def column_ratios(params=None):
    """The three ratios of the column-aware reading order as floats, (col_gap_ratio, row_gap_ratio, col_min_height_ratio), from a
    mapping that may leave any of them out (COLUMN_PARAMS then).  +inf is taken (never cuts); NaN or a negative ratio is refused."""
    p = {**COLUMN_PARAMS, **(params or {})}
    if set(p) != set(COLUMN_PARAMS):
        raise ValueError(f"column_params takes {sorted(COLUMN_PARAMS)}, got {sorted(p)}")
    r = tuple(float(p[k]) for k in COLUMN_PARAMS)
    if not all(v >= 0.0 for v in r):
        raise ValueError(f"column_params: a ratio must be >= 0 (+inf = never cut), got {p}")
    return r


class ReadingRegions(NamedTuple):
    """The regions behind a column-aware ReadingOrder (`reading_order_regions`), per page, on the device."""
    region: torch.Tensor    # [N,max_cand] i32: the region of every position of `order`, regions numbered in reading order
    regions: torch.Tensor   # [N,rows,6] i32: per region {first, count, x0, y0, x1, y1}: its span of positions and the union of its words' boxes
    nregions: torch.Tensor  # [N] i32: regions per page; -1 exactly where ncrop is -1


def reading_order_regions(boxes, nbox, page_hw, min_text_size, img_h, img_w, page_base=0, y_tol_ratio=0.6, x_gap_ratio=float("inf"),
                          col_gap_ratio=COLUMN_PARAMS["col_gap_ratio"], row_gap_ratio=COLUMN_PARAMS["row_gap_ratio"],
                          col_min_height_ratio=COLUMN_PARAMS["col_min_height_ratio"], workspace=None, lines=True, deskew=False):
    """The column-aware reading order (msocr_reading_order_regions): the page is cut into regions at its wide
    empty bands, and reading_order_lines' rule runs inside every region.  deskew=True: in the deskewed frame, as reading_order_deskew.
    lines=False: without the three line outputs.  Returns (ReadingOrder, ReadingLines or None, PageSkew or None, ReadingRegions)."""
    _need_cuda(boxes, nbox)
    N, max_cand, _ = boxes.shape
    dev = boxes.device
    ws = workspace
    if ws is None:
        ws = torch.empty((nat.lib().msocr_reading_order_regions_workspace_bytes(N, max_cand),), dtype=torch.uint8, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    ro = ReadingOrder(i32(N, max_cand), i32(N, max_cand), i32(N, max_cand, 8), i32(N))
    rl = ReadingLines(i32(N, max_cand), i32(N, nat.lib().msocr_reading_order_line_rows(max_cand), 6), i32(N)) if lines else None
    sk = PageSkew(torch.empty((N, 4), dtype=torch.int64, device=dev), torch.empty((N, 2), dtype=torch.float64, device=dev)) if deskew else None
    rg = ReadingRegions(i32(N, max_cand), i32(N, nat.lib().msocr_reading_order_region_rows(max_cand), 6), i32(N))
    nat.check(nat.lib().msocr_reading_order_regions(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, int(page_hw[0]), int(page_hw[1]),
                                                    int(min_text_size), int(img_h), int(img_w), float(y_tol_ratio), float(x_gap_ratio),
                                                    int(page_base), float(col_gap_ratio), float(row_gap_ratio), float(col_min_height_ratio),
                                                    1 if deskew else 0, *[t.data_ptr() for t in ro],
                                                    *([t.data_ptr() for t in rl] if lines else [None] * 3),
                                                    *([t.data_ptr() for t in sk] if deskew else [None] * 2),
                                                    *[t.data_ptr() for t in rg], ws.data_ptr(), _stream()), "reading_order_regions")
    return ro, rl, sk, rg


def reading_regions_host(aabbs_i32, y_tol_ratio=0.6, x_gap_ratio=float("inf"), col_gap_ratio=COLUMN_PARAMS["col_gap_ratio"],
                         row_gap_ratio=COLUMN_PARAMS["row_gap_ratio"], col_min_height_ratio=COLUMN_PARAMS["col_min_height_ratio"]):
    """Integer word boxes [n,4] -> (order [n], line [n], lines [L,6], region [n], regions [R,6]) as numpy int32 through the host twin
    msocr_reading_regions_host: reading_lines_host behind an XY-cut of the page, with the region of every position and per region
    {first, count, x0, y0, x1, y1}."""
    boxes = np.ascontiguousarray(aabbs_i32, dtype=np.int32).reshape(-1, 4)
    n = len(boxes)
    order, line, lines = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((n, 6), dtype=np.int32)
    region, regions = np.empty(n, dtype=np.int32), np.empty((n, 6), dtype=np.int32)
    nlines, nregions = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    nat.check(nat.lib().msocr_reading_regions_host(boxes.ctypes.data, n, float(y_tol_ratio), float(x_gap_ratio), float(col_gap_ratio),
                                                   float(row_gap_ratio), float(col_min_height_ratio), order.ctypes.data, line.ctypes.data,
                                                   lines.ctypes.data, nlines.ctypes.data, region.ctypes.data, regions.ctypes.data,
                                                   nregions.ctypes.data), "reading_regions_host")
    return order, line, lines[:int(nlines[0])].copy(), region, regions[:int(nregions[0])].copy()


def nchw_to_nhwc(x_f32, dtype, out=None):
    _need_cuda(x_f32)
    N, C, H, W = x_f32.shape
    assert x_f32.dtype == torch.float32 and x_f32.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C), dtype=dtype, device=x_f32.device)
    nat.check(nat.lib().msocr_nchw_f32_to_nhwc(x_f32.data_ptr(), N, C, H, W, _dt(out), out.data_ptr(), _pixel_dense_ld(out), _stream()),
              "nchw_to_nhwc")
    return out


def nhwc_to_nchw_f32(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    nat.check(nat.lib().msocr_nhwc_to_nchw_f32(x.data_ptr(), N, C, H, W, _pixel_dense_ld(x), _dt(x), out.data_ptr(), _stream()),
              "nhwc_to_nchw")
    return out


# ------------------------------------------------------------------------------------------- TRBA
def se_residual(x, identity, w1, w2, out=None, gate=None):
    """relu(x * sigmoid(W2 relu(W1 mean_hw(x))) + identity); x, identity [N,H,W,C] contiguous.  gate: optional [N,C] f32 tensor that
    receives the sigmoid gates (scratch otherwise)."""
    _need_cuda(x, identity, w1, w2)
    N, H, W, C = x.shape
    assert x.is_contiguous() and identity.is_contiguous() and identity.shape == x.shape and identity.dtype == x.dtype
    assert w1.shape == (C // 16, C) and w2.shape == (C, C // 16) and w1.dtype == torch.float32
    if out is None:
        out = torch.empty_like(x)
    if gate is None:
        gate = torch.empty((N, C), dtype=torch.float32, device=x.device)
    assert gate.shape == (N, C) and gate.dtype == torch.float32 and gate.is_contiguous()
    e = _prof_begin()
    nat.check(nat.lib().msocr_se_residual(x.data_ptr(), identity.data_ptr(), N, H * W, C, _dt(x), w1.data_ptr(), w2.data_ptr(),
                                          gate.data_ptr(), out.data_ptr(), _stream()), "se_residual")
    _prof_end(e, "se_residual", 3.0 * x.element_size() * N * H * W * C, (N, H * W, C))  # x + identity in, out (x re-read from cache)
    return out


# SE blocks whose map fits the LDS of a CU (TRBA layer3 / layer4: 4 x 13 x 512 f32 = 106 496 B) on square-form Winograd convolutions:
# the output transform of conv1 hands the map to the input transform of conv2 through LDS (wino44_output_kernel_chain), and the output
# transform of conv2 hands it to the SE tail (wino44_output_kernel_se), instead of a round trip through HBM each.  The same device
# functions in the same order: bit-identical.  MSOCR_SE_BLOCK_FUSED=0 keeps the three separate calls.
SE_BLOCK_FUSED = int(os.environ.get("MSOCR_SE_BLOCK_FUSED", "1"))


def _square_desc(dtype, N, H, W, w, stride, relu):
    """(descriptor, form, U) where conv2d runs a dense [N,H,W,Cin] -> [N,H,W,Cout] 3x3 / pad 1 call of weight w as split-operand square-form
    Winograd (with or without the tail column), else None."""
    Cout, KH, KW, Cin = w.shape
    if (dtype != torch.float32 or (KH, KW) != (3, 3) or tuple(stride) != (1, 1) or getattr(w, "_msocr_wino", None) is None
            or getattr(w, "_msocr_wino42_fused", None) is not None):
        return None
    form, u, split = _wino_form(w, H, W)
    if form not in (nat.WINO_4X4, nat.WINO_4X4_COLTAIL) or not split:
        return None
    d = nat.ConvDesc()
    d.dtype = nat.F32
    d.N, d.H, d.W, d.Cin = N, H, W, Cin
    d.in_sN, d.in_sH, d.in_sW = H * W * Cin, W * Cin, Cin
    d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = 3, 3, 1, 1, 1, 1
    d.Ho, d.Wo, d.Cout = H, W, Cout
    d.out_ld = Cout
    d.flags = nat.CONV_RELU if relu else 0
    return d, form, u


def se_block(x, conv1, conv2, identity, se, stride=(1, 1), gate=None):
    """SEBasicBlock (seresnet31.py:37-66) in one call: relu(se(conv2(relu(conv1(x)))) + identity), conv1 / conv2 = (weight, bias) of the
    BatchNorm-folded 3x3 / pad 1 convolutions (conv1 with the block's stride), se = (w1, w2) of the SE layer, identity [N,Ho,Wo,C]
    contiguous (x itself or the downsample branch).  gate: as se_residual.
    With SE_BLOCK_FUSED the per-crop kernels take what they can: conv2 -> SE tail where conv2 is a square-form Winograd layer whose
    map and SE scratch fit LDS, and conv1 -> conv2 where conv1 is one too, of the same shape (Cin == Cout).  Everything else — larger
    maps, bf16, exact f32, a strided conv1 — takes conv2d, conv2d, se_residual as before; the results are the same bit for bit."""
    (w1, b1), (w2, b2), (s1, s2) = conv1, conv2, se
    _need_cuda(x, w1, b1, w2, b2, identity, s1, s2, gate)
    N, H, W, _ = x.shape
    Ho, Wo = (H - 1) // stride[0] + 1, (W - 1) // stride[1] + 1
    C = w2.shape[0]
    L = nat.lib()
    q2 = _square_desc(x.dtype, N, Ho, Wo, w2, (1, 1), False) if SE_BLOCK_FUSED and SPLIT_BF16X3 else None
    if q2 is None or L.msocr_winograd_crop_lds_bytes(ctypes.byref(q2[0]), q2[1], 1) < 0:
        o = conv2d(x, w1, b1, stride=stride, pad=(1, 1), relu=True)
        o = conv2d(o, w2, b2, pad=(1, 1))
        return se_residual(o, identity, s1, s2, gate=gate)
    d2, form, u2 = q2
    assert identity.shape == (N, Ho, Wo, C) and identity.dtype == x.dtype and identity.is_contiguous()
    assert s1.shape == (C // 16, C) and s2.shape == (C, C // 16) and s1.dtype == torch.float32
    assert b1.dtype == b2.dtype == torch.float32 and b1.is_contiguous() and b2.is_contiguous() and b2.numel() == C
    assert w2.shape[3] == w1.shape[0] == b1.numel() and w1.shape[3] == x.shape[3]
    q1 = _square_desc(x.dtype, N, H, W, w1, stride, True) if x.stride(3) == 1 else None
    if q1 is not None and (q1[1] != form or L.msocr_winograd_crop_lds_bytes(ctypes.byref(q1[0]), form, 0) < 0):
        q1 = None
    if q1 is not None:  # conv1 -> conv2 through LDS: conv1's output is never written
        d1, _, u1 = q1
        d1.in_sN, d1.in_sH, d1.in_sW = x.stride(0), x.stride(1), x.stride(2)
        o1 = None
    else:
        o1 = conv2d(x, w1, b1, stride=stride, pad=(1, 1), relu=True)
    out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    if gate is None:
        gate = torch.empty((N, C), dtype=torch.float32, device=x.device)
    assert gate.shape == (N, C) and gate.dtype == torch.float32 and gate.is_contiguous()
    # one cut of the batch for the whole block: conv1 and conv2 have the same plan where they chain
    nbytes = L.msocr_winograd_workspace_bytes(ctypes.byref(d2), form)
    parts = min(N, -(-nbytes // WINO_WS_LIMIT))
    per = -(-N // parts)
    ws = _wino_workspace(nbytes if parts == 1 else (nbytes // N) * per, x.device)
    name = WINO_FORMS[form][0] + "_split"
    what = f"se_block {tuple(x.shape)} * {tuple(w1.shape)} * {tuple(w2.shape)}"
    alg = 2.0 * Ho * Wo * C * 9  # algorithmic FLOP of a convolution per image and input channel
    for n0 in range(0, N, per):
        n1 = min(N, n0 + per)
        nn = d2.N = n1 - n0
        rows, mt = _wino_rows(form, nn, Ho, Wo)
        if q1 is not None:
            d1.N = nn
            _wino_stage_in(d1, form, x[n0:n1].data_ptr(), ws, what)
            _wino_stage_gemm(d1, form, True, u1, ws, what, alg * d1.Cin * nn, name, Ho * Wo, 1)
            e = _prof_begin()
            nat.check(L.msocr_winograd_output_chain(ctypes.byref(d1), form, ws.data_ptr(), b1.data_ptr(), _stream()), what)
            _prof_end(e, "wino_out", 4.0 * 2 * rows * C, (mt, C, "chain"))  # Mw read, V written
        else:
            _wino_stage_in(d2, form, o1[n0:n1].data_ptr(), ws, what)
        _wino_stage_gemm(d2, form, True, u2, ws, what, alg * d2.Cin * nn, name, Ho * Wo, 1)
        e = _prof_begin()
        nat.check(L.msocr_winograd_output_se(ctypes.byref(d2), form, ws.data_ptr(), b2.data_ptr(), identity[n0:n1].data_ptr(), s1.data_ptr(),
                                             s2.data_ptr(), gate[n0:n1].data_ptr(), out[n0:n1].data_ptr(), _stream()), what)
        _prof_end(e, "wino_out", 4.0 * (rows * C + 2 * nn * Ho * Wo * C), (mt, C, "se"))  # Mw + identity read, out written
    return out


def mean_over_h(x):
    """[N,H,W,C] (dtype) -> [N,W,C] f32."""
    _need_cuda(x)
    N, H, W, C = x.shape
    assert x.is_contiguous()
    out = torch.empty((N, W, C), dtype=torch.float32, device=x.device)
    nat.check(nat.lib().msocr_mean_over_h(x.data_ptr(), N, H, W, C, _dt(x), out.data_ptr(), _stream()), "mean_over_h")
    return out


def bilstm_recurrent(xproj, whh_t, B, T, H, whh_planes=None):
    """xproj [B*T, 2*4H] f32 (= [B][T][2][4H]), whh_t [2,H,H,4] f32 (gate-interleaved) -> hcat [B,T,2H] f32.
    whh_planes (H == 256): W_hh of both directions in the packed split form -> the matrix-core kernel (csrc/bilstm_mfma.hip)."""
    _need_cuda(xproj, whh_t)
    assert xproj.is_contiguous() and xproj.numel() == B * T * 8 * H and whh_t.shape == (2, H, H, 4) and whh_t.is_contiguous()
    out = torch.empty((B, T, 2 * H), dtype=torch.float32, device=xproj.device)
    e = _prof_begin()
    if whh_planes is not None and H == 256 and SPLIT_BF16X3 and B * T * 8 * H < 2 ** 32:
        nat.check(nat.lib().msocr_bilstm_recurrent_split(xproj.data_ptr(), whh_planes.data_ptr(), B, T, H, out.data_ptr(), _stream()),
                  "bilstm_recurrent_split")
    else:
        nat.check(nat.lib().msocr_bilstm_recurrent(xproj.data_ptr(), whh_t.data_ptr(), B, T, H, out.data_ptr(), _stream()), "bilstm_recurrent")
    # per step per direction W_hh (4H x H f32) + B * (h + c + 4H pre-gates) * 4 B * 2
    _prof_end(e, "bilstm", (2.0 * T * (4.0 * H * H * 4 + B * (H + H + 4 * H) * 4 * 2), T), (B, T, H))
    return out


def crop_descriptors(boxes, page_ids, page_hw, img_h, img_w):
    """Host side of the device crop: clamped AABB (reference _pipeline.py:211-217) and ResizeAndPadA's size
    arithmetic (transforms.py:91-95,114-117; Python round = banker's = np.rint on the same doubles).  boxes: iterable of
    (x_min,y_min,x_max,y_max) ints.  Returns (int32 [M,8] descriptors, keep mask) — empty crops are dropped like the
    reference does.  Vectorised; `_crop_descriptors_loop` is the literal per-box form it is tested against."""
    H, W = page_hw
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    pg = np.asarray(page_ids, dtype=np.int64).reshape(-1)
    a_, b_ = np.maximum(0, b[:, 0]), np.maximum(0, b[:, 1])
    c_, d_ = np.minimum(W, b[:, 2]), np.minimum(H, b[:, 3])
    c_ = np.where(c_ < 0, np.maximum(W + c_, 0), c_)  # Python slice semantics of image[y1:y2, x1:x2] with a negative stop
    d_ = np.where(d_ < 0, np.maximum(H + d_, 0), d_)
    keep = (c_ > a_) & (d_ > b_)
    a_, b_, c_, d_, pg = a_[keep], b_[keep], c_[keep], d_[keep], pg[keep]
    h, w = d_ - b_, c_ - a_
    scale = np.minimum(img_h / np.maximum(h, 1), img_w / np.maximum(w, 1))  # float64, as Python's min of two true divisions
    nw = np.maximum(1, np.rint(w * scale).astype(np.int64))
    nh = np.maximum(1, np.rint(h * scale).astype(np.int64))
    yy = np.maximum(0, np.minimum((img_h - nh) // 2, img_h - nh))
    desc = np.stack([pg, a_, b_, c_, d_, nw, nh, yy], axis=1).astype(np.int32) if len(pg) else np.zeros((0, 8), dtype=np.int32)
    return desc, keep


def _crop_descriptors_loop(boxes, page_ids, page_hw, img_h, img_w):
    """DIAGNOSTIC, not on any product path: the literal per-box form of `crop_descriptors`, kept only as the second implementation
    of the differential CPU test (tests/test_host_cpu.py::test_vectorised_crop_descriptors_equal_the_loop)."""
    H, W = page_hw
    desc, keep = [], []
    for (x0, y0, x1, y1), pg in zip(boxes, page_ids):
        a, b = max(0, int(x0)), max(0, int(y0))
        c, d = min(W, int(x1)), min(H, int(y1))
        if c < 0:
            c = max(W + c, 0)
        if d < 0:
            d = max(H + d, 0)
        if c <= a or d <= b:
            keep.append(False)
            continue
        h, w = d - b, c - a
        scale = min(img_h / max(h, 1), img_w / max(w, 1))
        nw, nh = max(1, int(round(w * scale))), max(1, int(round(h * scale)))
        yy = max(0, min((img_h - nh) // 2, img_h - nh))
        desc.append((pg, a, b, c, d, nw, nh, yy))
        keep.append(True)
    return np.asarray(desc, dtype=np.int32).reshape(-1, 8), np.asarray(keep, dtype=bool)


def _crop(symbol, width, pages_u8, desc_host, img_h, img_w, desc_dev):
    """The body of `crop_resize_pad` (msocr_crop_resize_pad, descriptors [M,8]) and `quad_crop` (msocr_quad_crop, [M,12])."""
    _need_cuda(pages_u8, desc_dev)
    N, H, W, C = pages_u8.shape
    assert C == 3 and pages_u8.dtype == torch.uint8 and pages_u8.is_contiguous()
    hp = None
    if desc_host is not None:
        desc_host = desc_host.astype("int32", copy=False)
        hp = desc_host.ctypes.data
    M = len(desc_host) if desc_host is not None else int(desc_dev.shape[0])
    if desc_dev is None:
        desc_dev = torch.from_numpy(desc_host).to(pages_u8.device)
    else:
        assert desc_dev.dtype == torch.int32 and desc_dev.is_contiguous() and desc_dev.shape == (M, width)
        desc_dev.record_stream(torch.cuda.current_stream())
    out = torch.empty((M, img_h, img_w, 3), dtype=torch.uint8, device=pages_u8.device)
    nat.check(getattr(nat.lib(), symbol)(pages_u8.data_ptr(), N, H, W, desc_dev.data_ptr(), hp, M, img_h, img_w, out.data_ptr(), _stream()),
              symbol[len("msocr_"):])
    return out


def crop_resize_pad(pages_u8, desc_host, img_h, img_w, desc_dev=None):
    """pages [N,H,W,3] u8 device, desc_host int32 [M,8] (numpy) -> canvases [M,img_h,img_w,3] u8 device.
    desc_dev: the same descriptors already on the device (uploaded by the caller on another stream); desc_host may be None
    when they were produced on the device (reading_order_crops): the kernel then validates every descriptor itself."""
    return _crop("msocr_crop_resize_pad", 8, pages_u8, desc_host, img_h, img_w, desc_dev)


# ------------------------------------------------------------------------------------------- rectified crops
def quad_crop_descriptors(boxes, nbox, ro, img_h, img_w, out=None):
    """Device form of the quad descriptors (msocr_quad_crop_descriptors): boxes [N,max_cand,9] f32 + counts [N] as given to
    `reading_order_crops` and its result `ro` = (order, keep, desc, ncrop) -> qdesc [N,max_cand,12] i32 on the device, per page the
    quad descriptors of the kept words, compacted in exactly the order of `desc`.  Rows of a page with ncrop < 0 (host route) and
    rows past a page's ncrop are not written (zeros, or what `out` held)."""
    ro = ReadingOrder(*ro)  # any (order, keep, desc, ncrop) will do
    _need_cuda(boxes, nbox, *ro)
    N, max_cand, _ = boxes.shape
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and ro.desc.shape == (N, max_cand, 8) and ro.desc.is_contiguous()
    qdesc = out if out is not None else torch.zeros((N, max_cand, 12), dtype=torch.int32, device=boxes.device)
    assert qdesc.shape == (N, max_cand, 12) and qdesc.dtype == torch.int32 and qdesc.is_contiguous() and qdesc.is_cuda
    nat.check(nat.lib().msocr_quad_crop_descriptors(boxes.data_ptr(), nbox.data_ptr(), N, max_cand, int(img_h), int(img_w),
                                                    ro.order.data_ptr(), ro.keep.data_ptr(), ro.desc.data_ptr(), ro.ncrop.data_ptr(),
                                                    qdesc.data_ptr(), _stream()), "quad_crop_descriptors")
    return qdesc


def quad_descriptors(polygons, desc, img_h=0, img_w=0, natural=False):
    """Host form through the host twin (msocr_quad_crop_descriptors_host): polygons [M,4,2] (corners as the detector stored them, taken
    as f32) + the words' AABB descriptors `desc` int32 [M,8] (`crop_descriptors`) -> quad descriptors int32 [M,12] (numpy).
    natural=True: the regions at their own size (new_w = rint(w), new_h = rint(h), y0 = 0) instead of the fit to img_h x img_w."""
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 8)
    M = len(desc)
    quads = np.ascontiguousarray(np.asarray(polygons, dtype=np.float32).reshape(M, 8))
    out = np.zeros((M, 12), dtype=np.int32)
    nat.check(nat.lib().msocr_quad_crop_descriptors_host(quads.ctypes.data, desc.ctypes.data, M, int(img_h), int(img_w), int(bool(natural)),
                                                         out.ctypes.data), "quad_crop_descriptors_host")
    return out


def quad_crop_host(pages_u8, qdesc, img_h, img_w):
    """The CPU twin of `quad_crop` (msocr_quad_crop_host): pages [N,H,W,3] u8 numpy + quad descriptors int32 [M,12] -> canvases
    [M,img_h,img_w,3] u8 numpy, the same bytes as the kernel's."""
    pages_u8 = np.ascontiguousarray(pages_u8, dtype=np.uint8)
    qdesc = np.ascontiguousarray(qdesc, dtype=np.int32).reshape(-1, 12)
    N, H, W, C = pages_u8.shape
    assert C == 3
    out = np.empty((len(qdesc), img_h, img_w, 3), dtype=np.uint8)
    nat.check(nat.lib().msocr_quad_crop_host(pages_u8.ctypes.data, N, H, W, qdesc.ctypes.data, len(qdesc), int(img_h), int(img_w),
                                             out.ctypes.data), "quad_crop_host")
    return out


def quad_crop(pages_u8, qdesc_host, img_h, img_w, qdesc_dev=None):
    """pages [N,H,W,3] u8 device, qdesc_host int32 [M,12] (numpy) -> canvases [M,img_h,img_w,3] u8 device, cut along the words'
    quadrilaterals (msocr_quad_crop).  Mirrors `crop_resize_pad`: qdesc_dev = the same descriptors already on the device;
    qdesc_host may be None when they were produced there (quad_crop_descriptors): the kernel then validates every descriptor itself."""
    return _crop("msocr_quad_crop", 12, pages_u8, qdesc_host, img_h, img_w, qdesc_dev)


# ------------------------------------------------------------------------------------------- detection quality
def _thresholds(thresholds):
    th = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
    if th.ndim != 1:
        raise ValueError("thresholds must be a scalar or a one-dimensional sequence")
    return th


def quad_match_workspace_bytes(N, max_pred, max_gt):
    n = nat.lib().msocr_quad_match_ws_bytes(int(N), int(max_pred), int(max_gt))
    nat.check(min(n, 0), "quad_match_ws_bytes")
    return int(n)


def quad_match(pred, n_pred, gt, n_gt, thresholds, workspace=None, out=None):
    """pred [N,max_pred,4,2] f32, n_pred [N] i32, gt [N,max_gt,4,2] f32, n_gt [N] i32 (device), thresholds: T f64 values in (0, 1]
    (host) -> (match [N,T,max_pred] i32, iou [N,T,max_pred] f64, counts [N,T,3] i32 = tp, fp, fn), all on the device
    (msocr_quad_match: the matching rule of include/msocr.h, "detection quality").  Entries behind a page's n_pred are not written.
    out: the three tensors to write into."""
    _need_cuda(pred, n_pred, gt, n_gt)
    th = _thresholds(thresholds)
    N, max_pred, max_gt, T = int(pred.shape[0]), int(pred.shape[1]), int(gt.shape[1]), len(th)
    if tuple(pred.shape[2:]) != (4, 2) or tuple(gt.shape[2:]) != (4, 2) or gt.shape[0] != N or n_pred.numel() != N or n_gt.numel() != N:
        raise ValueError("quads are [N,max,4,2] with one count per page")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or n_pred.dtype != torch.int32 or n_gt.dtype != torch.int32:
        raise TypeError("quads are float32, counts int32")
    if not (pred.is_contiguous() and gt.is_contiguous() and n_pred.is_contiguous() and n_gt.is_contiguous()):
        raise ValueError("quad_match takes dense tensors")
    dev = pred.device
    if workspace is None:
        workspace = torch.empty((quad_match_workspace_bytes(N, max_pred, max_gt),), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty((N, T, max_pred), dtype=torch.int32, device=dev), torch.empty((N, T, max_pred), dtype=torch.float64, device=dev),
               torch.empty((N, T, 3), dtype=torch.int32, device=dev))
    match, iou, counts = out
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    ptr = [t.data_ptr() or workspace.data_ptr() for t in (pred, n_pred, gt, n_gt, match, iou, counts)]
    nat.check(nat.lib().msocr_quad_match(ptr[0], ptr[1], max_pred, ptr[2], ptr[3], max_gt, N, th.ctypes.data, T, ptr[4], ptr[5], ptr[6],
                                         workspace.data_ptr(), _stream()), "quad_match")
    return match, iou, counts


def quad_match_host(pred, n_pred, gt, n_gt, thresholds):
    """The CPU twin of `quad_match` (msocr_quad_match_host) on numpy arrays: the same three arrays, bit for bit.  Entries behind a
    page's n_pred hold match -3 and iou NaN (the entry point leaves them unwritten)."""
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    gt = np.ascontiguousarray(gt, dtype=np.float32)
    n_pred = np.ascontiguousarray(n_pred, dtype=np.int32).reshape(-1)
    n_gt = np.ascontiguousarray(n_gt, dtype=np.int32).reshape(-1)
    th = _thresholds(thresholds)
    N, T = len(n_pred), len(th)
    if pred.ndim != 4 or gt.ndim != 4 or pred.shape[0] != N or gt.shape[0] != N or pred.shape[2:] != (4, 2) or gt.shape[2:] != (4, 2) \
            or len(n_gt) != N:
        raise ValueError("quads are [N,max,4,2] with one count per page")
    max_pred, max_gt = pred.shape[1], gt.shape[1]
    match = np.full((N, T, max_pred), -3, dtype=np.int32)
    iou = np.full((N, T, max_pred), np.nan, dtype=np.float64)
    counts = np.zeros((N, T, 3), dtype=np.int32)
    pad = np.zeros(8, dtype=np.float64)  # an address for arrays without elements
    ptr = [a.ctypes.data if a.size else pad.ctypes.data for a in (pred, n_pred, gt, n_gt, match, iou, counts)]
    nat.check(nat.lib().msocr_quad_match_host(ptr[0], ptr[1], max_pred, ptr[2], ptr[3], max_gt, N, th.ctypes.data, T, ptr[4], ptr[5],
                                              ptr[6]), "quad_match_host")
    return match, iou, counts


# ------------------------------------------------------------------------------------------- page-level error rates
EDL_MAX_LEN = 16384  # msocr.h MSOCR_EDL_MAX_LEN: tokens of either side of a pair


def _edl_heads(a_off, b_off, v):
    a_off = np.ascontiguousarray(a_off, dtype=np.int32).reshape(-1)
    b_off = np.ascontiguousarray(b_off, dtype=np.int32).reshape(-1)
    v = np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
    N = len(v)
    if len(a_off) != N + 1 or len(b_off) != N + 1:
        raise ValueError("offsets are [N + 1] for v [N]")
    return a_off, b_off, v, N


def edit_distance_long_workspace_bytes(a_off, b_off, v):
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    n = nat.lib().msocr_edit_distance_long_ws_bytes(a_off.ctypes.data, b_off.ctypes.data, v.ctypes.data, N)
    nat.check(min(n, 0), "edit_distance_long_ws_bytes")
    return int(n)


def edit_distance_long(a_tok, a_off, b_tok, b_off, v, workspace=None, out=None):
    """Levenshtein distance of N pairs of token sequences of up to EDL_MAX_LEN tokens each (msocr_edit_distance_long; include/msocr.h,
    "page-level error rates").  a_tok, b_tok: int32 device tensors, the patterns and the texts one after the other; a_off, b_off
    [N + 1] and v [N]: host arrays (numpy), pair p = a_tok[a_off[p]:a_off[p + 1]] against b_tok[b_off[p]:b_off[p + 1]], tokens in
    [0, v[p]) compare by equality and every other token equals nothing.  -> dist [N] i32 on the device (out: the tensor to write into)."""
    _need_cuda(a_tok, b_tok)
    if a_tok.dtype != torch.int32 or b_tok.dtype != torch.int32 or a_tok.dim() != 1 or b_tok.dim() != 1:
        raise TypeError("tokens are one-dimensional int32 tensors")
    if not (a_tok.is_contiguous() and b_tok.is_contiguous()):
        raise ValueError("edit_distance_long takes dense tensors")
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    if N and (int(a_off[-1]) > a_tok.numel() or int(b_off[-1]) > b_tok.numel()):
        raise ValueError("offsets reach past the token tensors")
    dev = a_tok.device
    need = edit_distance_long_workspace_bytes(a_off, b_off, v)
    if workspace is None:
        workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((N,), dtype=torch.int32, device=dev)
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    ptr = [t.data_ptr() or workspace.data_ptr() for t in (a_tok, b_tok, out)]
    nat.check(nat.lib().msocr_edit_distance_long(ptr[0], a_off.ctypes.data, ptr[1], b_off.ctypes.data, v.ctypes.data, N, ptr[2],
                                                 workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()),
              "edit_distance_long")
    return out


def edit_distance_long_host(a_tok, a_off, b_tok, b_off, v):
    """The CPU twin of `edit_distance_long` (msocr_edit_distance_long_host) on numpy arrays -> dist [N] int32."""
    a_tok = np.ascontiguousarray(a_tok, dtype=np.int32).reshape(-1)
    b_tok = np.ascontiguousarray(b_tok, dtype=np.int32).reshape(-1)
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    if N and (int(a_off[-1]) > a_tok.size or int(b_off[-1]) > b_tok.size):
        raise ValueError("offsets reach past the token arrays")
    out = np.empty(N, dtype=np.int32)
    pad = np.zeros(2, dtype=np.int32)  # an address for arrays without elements
    ptr = [x.ctypes.data if x.size else pad.ctypes.data for x in (a_tok, b_tok, out)]
    nat.check(nat.lib().msocr_edit_distance_long_host(ptr[0], a_off.ctypes.data, ptr[1], b_off.ctypes.data, v.ctypes.data, N, ptr[2]),
              "edit_distance_long_host")
    return out


# ------------------------------------------------------------------------------------------- alignment behind the error rates
def edit_alignment_workspace_bytes(a_off, b_off, v):
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    n = nat.lib().msocr_edit_alignment_ws_bytes(a_off.ctypes.data, b_off.ctypes.data, v.ctypes.data, N)
    nat.check(min(n, 0), "edit_alignment_ws_bytes")
    return int(n)


def edit_alignment(a_tok, a_off, b_tok, b_off, v, workspace=None, out=None):
    """One optimal alignment of N pairs of token sequences of up to EDL_MAX_LEN tokens each (msocr_edit_alignment; include/msocr.h,
    "alignment behind the error rates": the tie rule is stated there).  Arguments as for `edit_distance_long`; the pattern side a is
    the side whose unpaired tokens count as deletions.  -> (dist [N], a_map [a_off[N] - a_off[0]], b_map [b_off[N] - b_off[0]],
    counts [N, 4] = hits, substitutions, deletions, insertions), int32 on the device; a map holds, for each token, the index of its
    partner within its pair's other side, or -1.  out: the four tensors to write into.  workspace: uint8, 16-byte aligned, at least
    `edit_alignment_workspace_bytes` (16 bytes per pattern block and text column for the trace: 64 MiB for a pair at the cap)."""
    _need_cuda(a_tok, b_tok)
    if a_tok.dtype != torch.int32 or b_tok.dtype != torch.int32 or a_tok.dim() != 1 or b_tok.dim() != 1:
        raise TypeError("tokens are one-dimensional int32 tensors")
    if not (a_tok.is_contiguous() and b_tok.is_contiguous()):
        raise ValueError("edit_alignment takes dense tensors")
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    if N and (int(a_off[-1]) > a_tok.numel() or int(b_off[-1]) > b_tok.numel()):
        raise ValueError("offsets reach past the token tensors")
    dev = a_tok.device
    need = edit_alignment_workspace_bytes(a_off, b_off, v)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    if out is None:
        na, nb = (int(a_off[-1]) - int(a_off[0]), int(b_off[-1]) - int(b_off[0])) if N else (0, 0)
        out = (torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((na,), dtype=torch.int32, device=dev),
               torch.empty((nb,), dtype=torch.int32, device=dev), torch.empty((N, 4), dtype=torch.int32, device=dev))
    dist, a_map, b_map, counts = out
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    ptr = [t.data_ptr() or workspace.data_ptr() for t in (a_tok, b_tok, dist, a_map, b_map, counts)]
    nat.check(nat.lib().msocr_edit_alignment(ptr[0], a_off.ctypes.data, ptr[1], b_off.ctypes.data, v.ctypes.data, N, ptr[2], ptr[3],
                                             ptr[4], ptr[5], workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                             _stream()), "edit_alignment")
    return dist, a_map, b_map, counts


def edit_alignment_host(a_tok, a_off, b_tok, b_off, v):
    """The CPU twin of `edit_alignment` (msocr_edit_alignment_host) on numpy arrays -> (dist, a_map, b_map, counts) int32, bit for bit."""
    a_tok = np.ascontiguousarray(a_tok, dtype=np.int32).reshape(-1)
    b_tok = np.ascontiguousarray(b_tok, dtype=np.int32).reshape(-1)
    a_off, b_off, v, N = _edl_heads(a_off, b_off, v)
    if N and (int(a_off[-1]) > a_tok.size or int(b_off[-1]) > b_tok.size):
        raise ValueError("offsets reach past the token arrays")
    na, nb = (int(a_off[-1]) - int(a_off[0]), int(b_off[-1]) - int(b_off[0])) if N else (0, 0)
    out = (np.empty(N, dtype=np.int32), np.empty(na, dtype=np.int32), np.empty(nb, dtype=np.int32), np.empty((N, 4), dtype=np.int32))
    pad = np.zeros(4, dtype=np.int32)  # an address for arrays without elements
    ptr = [x.ctypes.data if x.size else pad.ctypes.data for x in (a_tok, b_tok) + out]
    nat.check(nat.lib().msocr_edit_alignment_host(ptr[0], a_off.ctypes.data, ptr[1], b_off.ctypes.data, v.ctypes.data, N, ptr[2], ptr[3],
                                                  ptr[4], ptr[5]), "edit_alignment_host")
    return out


# ------------------------------------------------------------------------------------------- approximate text search
SEARCH_MAX_ALPHABET = 2048  # msocr.h MSOCR_SEARCH_MAX_ALPHABET
SEARCH_MAX_PATTERN = 64     # msocr.h MSOCR_SEARCH_MAX_PATTERN: tokens of a pattern
SEARCH_SEGMENT = 64         # msocr.h MSOCR_SEARCH_SEGMENT: tokens of a text that one lane of the scan kernel reports
SEARCH_CAPACITY = 65536     # records of the first pass of `text_search`


def _ts_heads(pat_off, max_dist, txt_off):
    pat_off = np.ascontiguousarray(pat_off, dtype=np.int32).reshape(-1)
    max_dist = np.ascontiguousarray(max_dist, dtype=np.int32).reshape(-1)
    txt_off = np.ascontiguousarray(txt_off, dtype=np.int32).reshape(-1)
    Q, T = len(max_dist), len(txt_off) - 1
    if len(pat_off) != Q + 1 or T < 0:
        raise ValueError("offsets are [Q + 1] for max_dist [Q], and [T + 1]")
    return pat_off, max_dist, txt_off, Q, T


def text_search_workspace_bytes(pat_off, max_dist, txt_off, v):
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    n = nat.lib().msocr_text_search_ws_bytes(pat_off.ctypes.data, max_dist.ctypes.data, Q, txt_off.ctypes.data, T, int(v))
    nat.check(min(n, 0), "text_search_ws_bytes")
    return int(n)


def text_search_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, hits, count, workspace=None):
    """One call of msocr_text_search (include/msocr.h, "approximate text search"): every end position at which pattern q
    = pat_tok[pat_off[q]:pat_off[q + 1]] matches a substring of text t = txt_tok[txt_off[t]:txt_off[t + 1]] with at most max_dist[q]
    errors.  pat_tok, txt_tok: int32 device tensors; pat_off [Q + 1], max_dist [Q], txt_off [T + 1]: host arrays (numpy); tokens in
    [0, v) compare by equality and every other token equals nothing.  hits: int32 device tensor [capacity, 5], rows (pattern, text,
    start, end, distance), written in no particular order up to its capacity; count: int64 device tensor [1], the exact number of
    hits.  Nothing is read back and nothing is waited for but the upload of the offsets."""
    _need_cuda(pat_tok, txt_tok, hits, count)
    if pat_tok.dtype != torch.int32 or txt_tok.dtype != torch.int32 or pat_tok.dim() != 1 or txt_tok.dim() != 1:
        raise TypeError("tokens are one-dimensional int32 tensors")
    if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 5 or count.dtype != torch.int64 or count.numel() != 1:
        raise TypeError("hits is int32 [capacity, 5], count is int64 [1]")
    if not (pat_tok.is_contiguous() and txt_tok.is_contiguous() and hits.is_contiguous()):
        raise ValueError("text_search takes dense tensors")
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    if (Q and int(pat_off[-1]) > pat_tok.numel()) or (T and int(txt_off[-1]) > txt_tok.numel()):
        raise ValueError("offsets reach past the token tensors")
    need = text_search_workspace_bytes(pat_off, max_dist, txt_off, v)
    if workspace is None:
        workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=txt_tok.device)
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    ptr = [t.data_ptr() or workspace.data_ptr() for t in (pat_tok, txt_tok, hits)]
    nat.check(nat.lib().msocr_text_search(ptr[0], pat_off.ctypes.data, max_dist.ctypes.data, Q, ptr[1], txt_off.ctypes.data, T, int(v),
                                          ptr[2], hits.shape[0], count.data_ptr(), workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(), _stream()), "text_search")


def text_search(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, capacity=SEARCH_CAPACITY):
    """All hits of `text_search_into`, read back: int32 numpy [count, 5], rows (pattern, text, start, end, distance) in no particular
    order (`text_search_select` or a sort makes them canonical).  The overflow protocol lives here: the first pass has room for
    `capacity` records; if there are more hits than that, the search runs once more with room for all of them, so the result is
    complete whatever the capacity."""
    capacity = int(capacity)
    if capacity < 0:
        raise ValueError("capacity >= 0")
    dev = txt_tok.device
    with torch.cuda.device(dev):
        count = torch.zeros((1,), dtype=torch.int64, device=dev)
        hits = torch.empty((capacity, 5), dtype=torch.int32, device=dev)
        text_search_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, hits, count)
        n = int(count.item())
        if n > capacity:
            hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
            text_search_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, hits, count)
            if int(count.item()) != n:
                raise nat.NativeError("text_search: the second pass counted other hits than the first")
        return hits[:n].cpu().numpy()


def text_search_host(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, capacity=None):
    """The CPU twin of `text_search` (msocr_text_search_host) on numpy arrays -> (hits int32 [min(count, capacity), 5] in canonical
    order (pattern, text, end ascending), count).  capacity None: room for every hit (a first call counts them)."""
    pat_tok = np.ascontiguousarray(pat_tok, dtype=np.int32).reshape(-1)
    txt_tok = np.ascontiguousarray(txt_tok, dtype=np.int32).reshape(-1)
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    if (Q and int(pat_off[-1]) > pat_tok.size) or (T and int(txt_off[-1]) > txt_tok.size):
        raise ValueError("offsets reach past the token arrays")
    pad = np.zeros(8, dtype=np.int32)  # an address for arrays without elements
    count = np.zeros(1, dtype=np.int64)

    def run(cap):
        hits = np.empty((cap, 5), dtype=np.int32)
        ptr = [x.ctypes.data if x.size else pad.ctypes.data for x in (pat_tok, txt_tok, hits)]
        nat.check(nat.lib().msocr_text_search_host(ptr[0], pat_off.ctypes.data, max_dist.ctypes.data, Q, ptr[1], txt_off.ctypes.data, T,
                                                   int(v), ptr[2], cap, count.ctypes.data), "text_search_host")
        return hits[:min(cap, int(count[0]))]

    if capacity is None:
        run(0)
        capacity = int(count[0])
    elif capacity < 0:
        raise ValueError("capacity >= 0")
    return run(int(capacity)), int(count[0])


def text_search_select(hits):
    """msocr_text_search_select_host on hits int32 [n, 5] (numpy): sorted into canonical order, then per (pattern, text) the hits are
    walked by (distance, end) ascending and one is kept iff [start, end) intersects none kept before -> the kept rows, canonical."""
    hits = np.array(hits, dtype=np.int32).reshape(-1, 5)  # a copy: the C function works in place
    n = nat.lib().msocr_text_search_select_host(hits.ctypes.data if len(hits) else None, len(hits))
    nat.check(min(n, 0), "text_search_select_host")
    return hits[:int(n)]


# ------------------------------------------------------------------------------- text search under confusion-weighted costs
SEARCH_W_MAX_ALPHABET = 768  # msocr.h MSOCR_SEARCH_W_MAX_ALPHABET
SEARCH_W_MAX_WINDOW = 256    # msocr.h MSOCR_SEARCH_W_MAX_WINDOW: m + max_dist // min(min_del, unknown) of a pattern


def text_search_weighted_workspace_bytes(pat_off, max_dist, txt_off, v, costs):
    """costs: a recognizers.EditCosts; only its scalars are read"""
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    n = nat.lib().msocr_text_search_weighted_ws_bytes(pat_off.ctypes.data, max_dist.ctypes.data, Q, txt_off.ctypes.data, T, int(v),
                                                      costs.struct(None))
    nat.check(min(n, 0), "text_search_weighted_ws_bytes")
    return int(n)


def text_search_weighted_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, tok_class, costs, hits, count, workspace=None):
    """One call of msocr_text_search_weighted (include/msocr.h, "The same search under confusion-weighted costs"): `text_search_into`
    with max_dist in cost units under costs (a recognizers.EditCosts; the text is the recognised side, the pattern the true word).
    tok_class: int32 device tensor [v], the cost class of corpus token c or -1.  hits, count and the workspace: as there."""
    _need_cuda(pat_tok, txt_tok, tok_class, hits, count)
    if pat_tok.dtype != torch.int32 or txt_tok.dtype != torch.int32 or pat_tok.dim() != 1 or txt_tok.dim() != 1:
        raise TypeError("tokens are one-dimensional int32 tensors")
    if tok_class.dtype != torch.int32 or tok_class.dim() != 1 or tok_class.numel() != int(v) or not tok_class.is_contiguous():
        raise TypeError("tok_class is a dense int32 tensor [v]")
    if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 5 or count.dtype != torch.int64 or count.numel() != 1:
        raise TypeError("hits is int32 [capacity, 5], count is int64 [1]")
    if not (pat_tok.is_contiguous() and txt_tok.is_contiguous() and hits.is_contiguous()):
        raise ValueError("text_search_weighted takes dense tensors")
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    if (Q and int(pat_off[-1]) > pat_tok.numel()) or (T and int(txt_off[-1]) > txt_tok.numel()):
        raise ValueError("offsets reach past the token tensors")
    need = text_search_weighted_workspace_bytes(pat_off, max_dist, txt_off, v, costs)
    if workspace is None:
        workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=txt_tok.device)
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    ptr = [t.data_ptr() or workspace.data_ptr() for t in (pat_tok, txt_tok, hits)]
    nat.check(nat.lib().msocr_text_search_weighted(ptr[0], pat_off.ctypes.data, max_dist.ctypes.data, Q, ptr[1], txt_off.ctypes.data, T,
                                                   int(v), tok_class.data_ptr(), costs.struct(txt_tok.device), ptr[2], hits.shape[0],
                                                   count.data_ptr(), workspace.data_ptr(),
                                                   workspace.numel() * workspace.element_size(), _stream()), "text_search_weighted")


def text_search_weighted(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, tok_class, costs, capacity=SEARCH_CAPACITY):
    """All hits of `text_search_weighted_into`, read back: int32 numpy [count, 5] in no particular order; the two-pass overflow
    protocol of `text_search`."""
    capacity = int(capacity)
    if capacity < 0:
        raise ValueError("capacity >= 0")
    dev = txt_tok.device
    with torch.cuda.device(dev):
        count = torch.zeros((1,), dtype=torch.int64, device=dev)
        hits = torch.empty((capacity, 5), dtype=torch.int32, device=dev)
        text_search_weighted_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, tok_class, costs, hits, count)
        n = int(count.item())
        if n > capacity:
            hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
            text_search_weighted_into(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, tok_class, costs, hits, count)
            if int(count.item()) != n:
                raise nat.NativeError("text_search_weighted: the second pass counted other hits than the first")
        return hits[:n].cpu().numpy()


def text_search_weighted_host(pat_tok, pat_off, max_dist, txt_tok, txt_off, v, tok_class, costs, capacity=None):
    """The CPU twin of `text_search_weighted` (msocr_text_search_weighted_host) on numpy arrays -> (hits in canonical order, count).
    capacity None: room for every hit (a first call counts them)."""
    pat_tok = np.ascontiguousarray(pat_tok, dtype=np.int32).reshape(-1)
    txt_tok = np.ascontiguousarray(txt_tok, dtype=np.int32).reshape(-1)
    tok_class = np.ascontiguousarray(tok_class, dtype=np.int32).reshape(-1)
    if tok_class.size != int(v):
        raise ValueError("tok_class is [v]")
    pat_off, max_dist, txt_off, Q, T = _ts_heads(pat_off, max_dist, txt_off)
    if (Q and int(pat_off[-1]) > pat_tok.size) or (T and int(txt_off[-1]) > txt_tok.size):
        raise ValueError("offsets reach past the token arrays")
    pad = np.zeros(8, dtype=np.int32)  # an address for arrays without elements
    count = np.zeros(1, dtype=np.int64)

    def run(cap):
        hits = np.empty((cap, 5), dtype=np.int32)
        ptr = [x.ctypes.data if x.size else pad.ctypes.data for x in (pat_tok, txt_tok, hits, tok_class)]
        nat.check(nat.lib().msocr_text_search_weighted_host(ptr[0], pat_off.ctypes.data, max_dist.ctypes.data, Q, ptr[1],
                                                            txt_off.ctypes.data, T, int(v), ptr[3], costs.struct(None), ptr[2], cap,
                                                            count.ctypes.data), "text_search_weighted_host")
        return hits[:min(cap, int(count[0]))]

    if capacity is None:
        run(0)
        capacity = int(count[0])
    elif capacity < 0:
        raise ValueError("capacity >= 0")
    return run(int(capacity)), int(count[0])


# ------------------------------------------------------------------------------------------- word spotting
SPOT_MAX_T = 64    # msocr.h MSOCR_SPOT_MAX_T: frames of a sequence
SPOT_MAX_H = 512   # msocr.h MSOCR_SPOT_MAX_H: elements of a frame, a multiple of 64
SPOT_MAX_K = 256   # msocr.h MSOCR_SPOT_MAX_K: neighbours of one selection
SPOT_TILE = 4      # msocr.h MSOCR_SPOT_TILE: corpus words of one workgroup of the distance kernel


def _ws_feat_dev(x, what):
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise TypeError(f"{what} is a dense float32 device tensor [N, T, H]")
    return x


def _ws_i32_dev(x, n, like, what):
    _need_cuda(x)
    if x.dtype != torch.int32 or x.dim() != 1 or x.numel() != n or not x.is_contiguous() or x.device != like.device:
        raise TypeError(f"{what} is a dense int32 tensor [{n}] on the features' device")
    return x


def _ws_ptr(t, pad):
    # a tensor without elements has no address: the entry point wants one and then reads or writes nothing through it
    return t.data_ptr() or pad.data_ptr()


def frame_normalize(feat, lengths, out=None):
    """msocr_frame_normalize (include/msocr.h, "word spotting"): feat f32 [N, T, H] and lengths int32 [N] on the device -> unit frames
    f32 [N, T, H]; frames at or beyond a word's length are zeros, a frame without a finite norm of at least sqrt(FLT_MIN) too."""
    _ws_feat_dev(feat, "feat")
    N, T, H = feat.shape
    _ws_i32_dev(lengths, N, feat, "lengths")
    if out is None:
        out = torch.empty_like(feat)
    elif out.shape != feat.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != feat.device:
        raise TypeError("out is a dense float32 tensor of feat's shape and device")
    with torch.cuda.device(feat.device):
        pad = torch.empty(4, dtype=torch.float32, device=feat.device)
        nat.check(nat.lib().msocr_frame_normalize(_ws_ptr(feat, pad), _ws_ptr(lengths, pad), N, T, H, _ws_ptr(out, pad), _stream()),
                  "frame_normalize")
    return out


def dtw_distances(q_unit, q_len, len_lo, len_hi, c_unit, c_len, out=None):
    """msocr_dtw_distances: the normalised DTW distance of every query (q_unit f32 [Q, T, H], q_len, len_lo, len_hi int32 [Q]) to every
    indexed word (c_unit f32 [N, T, H], c_len int32 [N]), all on one device -> f32 [Q, N]; +inf where the word's length lies outside
    [len_lo[q], len_hi[q]].  Nothing is read back or waited for."""
    _ws_feat_dev(q_unit, "q_unit")
    _ws_feat_dev(c_unit, "c_unit")
    Q, T, H = q_unit.shape
    N = c_unit.shape[0]
    if tuple(c_unit.shape[1:]) != (T, H) or c_unit.device != q_unit.device:
        raise ValueError("queries and corpus share T, H and the device")
    for x, n, what in ((q_len, Q, "q_len"), (len_lo, Q, "len_lo"), (len_hi, Q, "len_hi"), (c_len, N, "c_len")):
        _ws_i32_dev(x, n, q_unit, what)
    if out is None:
        out = torch.empty((Q, N), dtype=torch.float32, device=q_unit.device)
    elif tuple(out.shape) != (Q, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q_unit.device:
        raise TypeError("out is a dense float32 tensor [Q, N] on the features' device")
    with torch.cuda.device(q_unit.device):
        pad = torch.empty(4, dtype=torch.float32, device=q_unit.device)
        p = [_ws_ptr(t, pad) for t in (q_unit, q_len, len_lo, len_hi, c_unit, c_len, out)]
        nat.check(nat.lib().msocr_dtw_distances(p[0], p[1], p[2], p[3], Q, p[4], p[5], N, T, H, p[6], _stream()), "dtw_distances")
    return out


def dtw_subsequence(q_unit, q_len, len_lo, len_hi, c_unit, c_len, out=None, span_out=None):
    """msocr_dtw_subsequence: the subsequence DTW distance of every query to every indexed word (arguments as `dtw_distances`): the
    query may start and end anywhere inside the word -> (d f32 [Q, N], the path's cost divided by the QUERY's length; span int32
    [Q, N, 2], the word frames [start, end) it matched).  +inf and (-1, -1) where the word's length lies outside [len_lo[q],
    len_hi[q]].  Nothing is read back or waited for."""
    _ws_feat_dev(q_unit, "q_unit")
    _ws_feat_dev(c_unit, "c_unit")
    Q, T, H = q_unit.shape
    N = c_unit.shape[0]
    if tuple(c_unit.shape[1:]) != (T, H) or c_unit.device != q_unit.device:
        raise ValueError("queries and corpus share T, H and the device")
    for x, n, what in ((q_len, Q, "q_len"), (len_lo, Q, "len_lo"), (len_hi, Q, "len_hi"), (c_len, N, "c_len")):
        _ws_i32_dev(x, n, q_unit, what)
    if out is None:
        out = torch.empty((Q, N), dtype=torch.float32, device=q_unit.device)
    elif tuple(out.shape) != (Q, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q_unit.device:
        raise TypeError("out is a dense float32 tensor [Q, N] on the features' device")
    if span_out is None:
        span_out = torch.empty((Q, N, 2), dtype=torch.int32, device=q_unit.device)
    elif (tuple(span_out.shape) != (Q, N, 2) or span_out.dtype != torch.int32 or not span_out.is_contiguous()
          or span_out.device != q_unit.device):
        raise TypeError("span_out is a dense int32 tensor [Q, N, 2] on the features' device")
    with torch.cuda.device(q_unit.device):
        pad = torch.empty(4, dtype=torch.float32, device=q_unit.device)
        p = [_ws_ptr(t, pad) for t in (q_unit, q_len, len_lo, len_hi, c_unit, c_len, out, span_out)]
        nat.check(nat.lib().msocr_dtw_subsequence(p[0], p[1], p[2], p[3], Q, p[4], p[5], N, T, H, p[6], p[7], _stream()), "dtw_subsequence")
    return out, span_out


def topk_smallest(dist, k):
    """msocr_topk_smallest: per row of dist (f32 [Q, N] on the device) the k smallest finite values ascending, ties by ascending index
    -> (idx int32 [Q, k], val f32 [Q, k]) on the device; unused slots hold -1 / +inf."""
    _need_cuda(dist)
    if dist.dtype != torch.float32 or dist.dim() != 2 or not dist.is_contiguous():
        raise TypeError("dist is a dense float32 device tensor [Q, N]")
    Q, N = dist.shape
    idx = torch.empty((Q, int(k)), dtype=torch.int32, device=dist.device)
    val = torch.empty((Q, int(k)), dtype=torch.float32, device=dist.device)
    with torch.cuda.device(dist.device):
        pad = torch.empty(4, dtype=torch.float32, device=dist.device)
        nat.check(nat.lib().msocr_topk_smallest(_ws_ptr(dist, pad), Q, N, int(k), _ws_ptr(idx, pad), _ws_ptr(val, pad), _stream()),
                  "topk_smallest")
    return idx, val


def _ws_feat_host(x, what):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise TypeError(f"{what} is float32 [N, T, H]")
    return x


def _ws_i32_host(x, n, what):
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
    if x.size != n:
        raise TypeError(f"{what} is int32 [{n}]")
    return x


_WS_PAD = np.zeros(8, dtype=np.float32)  # an address for arrays without elements


def _ws_hptr(x):
    return x.ctypes.data if x.size else _WS_PAD.ctypes.data


def frame_normalize_host(feat, lengths):
    """The CPU twin of `frame_normalize` (msocr_frame_normalize_host) on numpy arrays, with the same order of the f32 sum."""
    feat = _ws_feat_host(feat, "feat")
    N, T, H = feat.shape
    lengths = _ws_i32_host(lengths, N, "lengths")
    out = np.empty_like(feat)
    nat.check(nat.lib().msocr_frame_normalize_host(_ws_hptr(feat), _ws_hptr(lengths), N, T, H, _ws_hptr(out)), "frame_normalize_host")
    return out


def dtw_distances_host(q_unit, q_len, len_lo, len_hi, c_unit, c_len):
    """The CPU twin of `dtw_distances` (msocr_dtw_distances_host): every product, sum and table entry in f64, one rounding to f32.
    It refuses lengths outside [1, T] and len_lo > len_hi."""
    q_unit, c_unit = _ws_feat_host(q_unit, "q_unit"), _ws_feat_host(c_unit, "c_unit")
    Q, T, H = q_unit.shape
    N = c_unit.shape[0]
    if tuple(c_unit.shape[1:]) != (T, H):
        raise ValueError("queries and corpus share T and H")
    q_len, len_lo, len_hi = (_ws_i32_host(x, Q, w) for x, w in ((q_len, "q_len"), (len_lo, "len_lo"), (len_hi, "len_hi")))
    c_len = _ws_i32_host(c_len, N, "c_len")
    out = np.empty((Q, N), dtype=np.float32)
    p = [_ws_hptr(x) for x in (q_unit, q_len, len_lo, len_hi, c_unit, c_len, out)]
    nat.check(nat.lib().msocr_dtw_distances_host(p[0], p[1], p[2], p[3], Q, p[4], p[5], N, T, H, p[6]), "dtw_distances_host")
    return out


def dtw_subsequence_host(q_unit, q_len, len_lo, len_hi, c_unit, c_len):
    """The CPU twin of `dtw_subsequence` (msocr_dtw_subsequence_host): every product, sum and table entry in f64, one rounding to
    f32 -> (d f32 [Q, N], span int32 [Q, N, 2]).  It refuses lengths outside [1, T] and len_lo > len_hi."""
    q_unit, c_unit = _ws_feat_host(q_unit, "q_unit"), _ws_feat_host(c_unit, "c_unit")
    Q, T, H = q_unit.shape
    N = c_unit.shape[0]
    if tuple(c_unit.shape[1:]) != (T, H):
        raise ValueError("queries and corpus share T and H")
    q_len, len_lo, len_hi = (_ws_i32_host(x, Q, w) for x, w in ((q_len, "q_len"), (len_lo, "len_lo"), (len_hi, "len_hi")))
    c_len = _ws_i32_host(c_len, N, "c_len")
    out = np.empty((Q, N), dtype=np.float32)
    span = np.empty((Q, N, 2), dtype=np.int32)
    p = [_ws_hptr(x) for x in (q_unit, q_len, len_lo, len_hi, c_unit, c_len, out, span)]
    nat.check(nat.lib().msocr_dtw_subsequence_host(p[0], p[1], p[2], p[3], Q, p[4], p[5], N, T, H, p[6], p[7]), "dtw_subsequence_host")
    return out, span


def topk_smallest_host(dist, k):
    """The CPU twin of `topk_smallest` (msocr_topk_smallest_host): the same bits as the device on the same array."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    if dist.ndim != 2:
        raise TypeError("dist is float32 [Q, N]")
    Q, N = dist.shape
    idx = np.empty((Q, int(k)), dtype=np.int32)
    val = np.empty((Q, int(k)), dtype=np.float32)
    nat.check(nat.lib().msocr_topk_smallest_host(_ws_hptr(dist), Q, N, int(k), _ws_hptr(idx), _ws_hptr(val)), "topk_smallest_host")
    return idx, val
