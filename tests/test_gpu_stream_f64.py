"""The streaming kernels of csrc/elementwise.hip against plain references over their envelope: normalize_u8_kernel<float|bf16, 4|8>,
resize_linear_u8_kernel, maxpool_kernel<float|bf16>, upsample2x_kernel<float|bf16>, east_head_kernel<float|bf16>,
nchw_to_nhwc_kernel<float|bf16>, nhwc_to_nchw_kernel<float|bf16> and crop_resize_pad_kernel (16 instances; every case names the
instance it reaches, and a rocprofv3 kernel trace of this module lists the same set).

References and bounds (u = 2^-24, gamma_n = n u / (1 - n u)):
  normalize_u8   exact.  mode 0 = (x / 255 - .5) / .5 in f32 (oracle.imgproc.east_preprocess), mode 1 = (x - 127.5) * f32(1 / 127.5);
                 bf16 = the round-to-nearest-even of that f32 (torch .to(bfloat16)), bit for bit.  Lanes 3 .. cpad-1 and the border 0.
  resize_linear  bit-equal to oracle.imgproc.resize_linear_u8 (which tests/test_oracle_resample.py checks against the definition).
  crop_resize    bit-equal to oracle.imgproc.resize_and_pad, on host and on device-only descriptors; an invalid device descriptor
                 (each breaking one condition of the kernel's check) gives a canvas of 255.
  maxpool        exact: torch.equal with torch-CPU F.max_pool2d on the same values, NaN positions equal.  Selection rounds nothing.
  upsample2x     ref = bilinear x2 (align_corners=False) in f64 of the same (bf16: bf16-rounded) inputs, A = the same interpolation of
                 |x|.  The kernel forms w_y0 (w_x0 a + w_x1 b) + w_y1 (w_x0 c + w_x1 d) in f32 without FMA (-ffp-contract=off): every
                 input passes 4 roundings (product, sum, product, sum), so f32: |dev - ref| <= gamma_4 A.  bf16: the f32 value is
                 rounded to nearest even once: |dev - ref| <= 2^-8 |ref| (1 + 1e-3) + 2 gamma_4 A; a truncating store reaches 2^-7 |ref|.
  east_head      geo: 32 FMAs then the bias, 33 roundings: |dev - ref| <= gamma_33 (sum |w||x| + |b|) = G per element.  score: the
                 logit carries at most G; sigmoid moves it by at most s(1 - s)(1 + G) G (s' = s(1 - s) varies by at most a factor
                 e^G ~ 1 + G over [o - G, o + G]); 1 / (1 + expf(-o)) adds expf's relative error (taken as 2 ulp = 4u) times 1 - s
                 and two roundings (2u) times s: |dev - ref| <= s(1 - s)(1 + G) G + s((1 - s) 4u + 2u) + 2^-126 (results below the
                 f32 normal range carry no relative precision).  Logits beyond +-95 give scores of exactly 1 and 0.
  layout         exact against a torch permute (bf16: round to nearest even), round trips included.
Every envelope case writes into a sentinel-filled buffer: a channel slice of a wider buffer (or a span inside a longer one where the
ABI writes dense rows) with channels before and after it and one extra image behind the last one; the sentinels must survive.
Each kernel has a case above 2048 x 256 = 524 288 work items, so that its grid-stride loop iterates; where the reference is sampled
(upsample2x) the sample holds the first and the last work item of every sweep.  The C ABI's argument checks are tested through
_native (they launch nothing).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_oracle_resample as env

pytestmark = pytest.mark.gpu

SEED = 20261016
U = 2.0 ** -24
SENTINEL = 7.25
SWEEP = 2048 * 256                       # grid_for caps every grid at 2048 blocks of 256 work items
# Bounds, with what the first MI355X run of this module measured (every case prints its figures with -s):
#   upsample2x f32: worst |dev - ref| / (gamma_4 A) 0 .. 0.79 (0 at 1 x 1: weights 1 and 0); bf16: worst / (2^-8 |ref| + 2 gamma_4 A)
#     0.995 in every case (round to nearest reaches its bound; each truncating mutant failed every bf16 case).
#   east_head: geo worst / G 0.012 .. 0.142; score worst / bound 0.004 .. 0.661.
#   normalize, maxpool, layout, resize, crop: 0 elements differ.
UP_GAMMA = 4
BF16_U, BF16_EPS = 2.0 ** -8, 1e-3
HEAD_GAMMA = 33
EXPF_REL = 4 * U
N_RANDOM = 2000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def nat(ops):
    from manuscript_ocr_amd import _native
    return _native


def _gamma(n):
    return n * U / (1 - n * U)


def _dt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _guarded(N, H, W, C, dtype, pre, post, fill=SENTINEL):
    buf = torch.full((N + 1, H, W, pre + C + post), fill, dtype=dtype, device="cuda")
    return buf, buf[:N, :, :, pre:pre + C]


def _check_guard(buf, N, pre, C, what):
    assert torch.all(buf[:, :, :, :pre] == SENTINEL), (what, "channels before the output were written")
    assert torch.all(buf[:, :, :, pre + C:] == SENTINEL), (what, "channels after the output were written")
    assert torch.all(buf[N:] == SENTINEL), (what, "the image behind the last one was written")


def _sweep_ends(total):
    """First and last work item of every grid sweep of a grid_for(total, 256) launch."""
    grid = min(max(-(-total // 256), 1), 2048) * 256
    ends = []
    for s in range(0, total, grid):
        ends += [s, min(s + grid, total) - 1]
    return ends


def _specials(x, g, frac=0.02):
    """Put NaN, +-inf and +-0 at seeded random positions of a CPU f32 tensor (in place)."""
    flat = x.view(-1)
    for v in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0):
        idx = torch.randint(0, flat.numel(), (max(1, int(frac * flat.numel())),), generator=g)
        flat[idx] = v
    return x


# ================================================================================================ normalize_u8
def _every_u8(N, H, W, seed):
    """N x H x W x 3 u8; with H * W >= 256 every value occurs in every channel (strides 1, 7, 13 are odd: full cycles mod 256)."""
    p = np.arange(N * H * W, dtype=np.int64).reshape(N, H, W) + seed
    return np.stack([p % 256, (p * 7 + 3) % 256, (p * 13 + 5) % 256], -1).astype(np.uint8)


def _norm_ref(img, mode):
    if mode == 0:
        from oracle import imgproc
        return np.stack([imgproc.east_preprocess(im, im.shape[1], im.shape[0])[0].transpose(1, 2, 0) for im in img])
    return (img.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)


# name, instance, N, H, W, pad_t, pad_l, Hp, Wp, cpad, mode, dtype
NORM_CASES = [
    ("f32-c4-east", "normalize_u8<float,4>", 2, 20, 13, 3, 3, 26, 21, 4, 0, "f32"),
    ("f32-c4-m1-1x1", "normalize_u8<float,4>", 3, 1, 1, 0, 0, 1, 1, 4, 1, "f32"),
    ("f32-c8-trba", "normalize_u8<float,8>", 3, 16, 17, 1, 1, 18, 21, 8, 1, "f32"),
    ("f32-c8-m0-wide", "normalize_u8<float,8>", 1, 1, 300, 0, 2, 3, 305, 8, 0, "f32"),
    ("bf16-c4-east", "normalize_u8<bf16,4>", 2, 16, 19, 3, 3, 22, 27, 4, 0, "bf16"),
    ("bf16-c4-m1-tall", "normalize_u8<bf16,4>", 2, 270, 1, 2, 0, 275, 3, 4, 1, "bf16"),
    ("bf16-c8-trba", "normalize_u8<bf16,8>", 3, 32, 9, 1, 1, 34, 13, 8, 1, "bf16"),
    ("bf16-c8-m0", "normalize_u8<bf16,8>", 2, 13, 20, 0, 0, 15, 20, 8, 0, "bf16"),
    # grid-stride: the detector's stem canvas of two 1536 x 2048 pages; 160 recogniser canvases (bf16, cpad 8)
    ("f32-c4-page", "normalize_u8<float,4>", 2, 1536, 2048, 3, 3, 1542, 2054, 4, 0, "f32"),
    ("bf16-c4-page", "normalize_u8<bf16,4>", 2, 1536, 2048, 3, 3, 1542, 2054, 4, 0, "bf16"),
    ("bf16-c8-crops", "normalize_u8<bf16,8>", 160, 32, 100, 1, 1, 34, 104, 8, 1, "bf16"),
    ("f32-c8-crops", "normalize_u8<float,8>", 160, 32, 100, 1, 1, 34, 104, 8, 1, "f32"),
]


@pytest.mark.parametrize("c", NORM_CASES, ids=lambda c: c[0])
def test_normalize_u8_envelope(ops, nat, c):
    name, inst, N, H, W, pt, pl, Hp, Wp, cpad, mode, dn = c
    dt = _dt(dn)
    img = _every_u8(N, H, W, sum(map(ord, name)))
    if H * W >= 256:
        assert all(len(np.unique(img[0, ..., ch])) == 256 for ch in range(3))
    n_out = N * Hp * Wp * cpad
    pre = 16 // dt.itemsize * 2                  # 32 bytes of sentinel before: keeps the 16-byte vector stores aligned
    post = Hp * Wp * cpad + 8                    # one image and a bit behind the last one
    buf = torch.full((pre + n_out + post,), SENTINEL, dtype=dt, device="cuda")
    src = torch.from_numpy(img).cuda()
    nat.check(nat.lib().msocr_normalize_u8(src.data_ptr(), N, H, W, pt, pl, Hp, Wp, cpad, mode, ops._dt(buf),
                                           buf[pre:].data_ptr(), ops._stream()), "normalize_u8")
    torch.cuda.synchronize()
    assert torch.all(buf[:pre] == SENTINEL) and torch.all(buf[pre + n_out:] == SENTINEL), name
    out = buf[pre:pre + n_out].view(N, Hp, Wp, cpad).cpu()
    ref = torch.from_numpy(_norm_ref(img, mode))
    exp = torch.zeros((N, Hp, Wp, cpad), dtype=torch.float32)
    exp[:, pt:pt + H, pl:pl + W, :3] = ref
    if dt == torch.bfloat16:
        exp = exp.to(torch.bfloat16)
        same = torch.equal(out.view(torch.int16), exp.view(torch.int16))
    else:
        same = torch.equal(out.view(torch.int32), exp.view(torch.int32))
    bad = (out.float() != exp.float()).sum().item()
    print(f"normalize {name} [{inst}] {N * Hp * Wp} work items ({-(-N * Hp * Wp // SWEEP)} sweeps): {bad} elements differ")
    assert same, (name, bad)


# ================================================================================================ maxpool2d
def _pool_ref(x_nhwc_cpu, k, s, p):
    r = F.max_pool2d(x_nhwc_cpu.permute(0, 3, 1, 2), k, s, p)
    return r.permute(0, 2, 3, 1)


def _assert_equal_nan(dev, ref, what):
    dn, rn = torch.isnan(dev), torch.isnan(ref)
    assert torch.equal(dn, rn), (what, "NaN positions differ", int((dn != rn).sum()))
    assert torch.equal(dev.masked_fill(dn, 0), ref.masked_fill(rn, 0)), what


# name, instance, dtype, N, H, W, C, k, s, p, in_extra (input read from a channel slice), pre, post
POOL_CASES = [
    ("f32-stem-yx", "maxpool<float>", "f32", 2, 17, 23, 64, 3, 2, 1, 0, 64, 0),       # out = yx[..., 64:] of net.py (out_ld 128)
    ("bf16-stem-yx", "maxpool<bf16>", "bf16", 2, 18, 21, 64, 3, 2, 1, 0, 64, 0),
    ("f32-2x2-odd", "maxpool<float>", "f32", 1, 9, 13, 12, 2, 2, 0, 8, 4, 8),
    ("bf16-2x2-odd", "maxpool<bf16>", "bf16", 2, 11, 7, 12, 2, 2, 0, 4, 8, 4),
    ("f32-3x1-1x3", "maxpool<float>", "f32", 2, 1, 3, 4, 3, 1, 1, 4, 4, 4),
    ("bf16-3x2-3x1", "maxpool<bf16>", "bf16", 1, 3, 1, 4, 3, 2, 1, 0, 4, 4),
    ("f32-3x1-2x2", "maxpool<float>", "f32", 1, 2, 2, 20, 3, 1, 1, 0, 0, 4),
    ("bf16-2x2-2x3", "maxpool<bf16>", "bf16", 3, 2, 3, 4, 2, 2, 0, 12, 4, 0),
    ("f32-3x2-5x5-c36", "maxpool<float>", "f32", 1, 5, 5, 36, 3, 2, 1, 4, 4, 4),
    # grid-stride: the detector's stem at half a 1536 x 2048 page (1.6M work items), and 16 channels at a full page (0.8M)
    ("f32-stem-big", "maxpool<float>", "f32", 2, 384, 512, 64, 3, 2, 1, 0, 64, 0),
    ("bf16-stem-c16", "maxpool<bf16>", "bf16", 1, 768, 1024, 16, 3, 2, 1, 16, 8, 8),
]


@pytest.mark.parametrize("c", POOL_CASES, ids=lambda c: c[0])
def test_maxpool2d_envelope(ops, c):
    name, inst, dn, N, H, W, C, k, s, p, in_extra, pre, post = c
    dt = _dt(dn)
    g = torch.Generator().manual_seed(SEED + sum(map(ord, name)))
    x = _specials(torch.randn(N, H, W, C, generator=g), g).to(dt)
    xin = torch.full((N, H, W, in_extra + C), -3.0, dtype=dt)
    xin[..., in_extra:] = x
    xd = xin.cuda()[..., in_extra:]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    buf, out = _guarded(N, Ho, Wo, C, dt, pre, post)
    ops.maxpool2d(xd, k, s, p, out=out)
    torch.cuda.synchronize()
    _check_guard(buf, N, pre, C, name)
    ref = _pool_ref(x, k, s, p)
    dev = out.cpu().contiguous()
    total = N * Ho * Wo * C // 4
    print(f"maxpool {name} [{inst}] {total} work items ({-(-total // SWEEP)} sweeps): NaN outputs {int(torch.isnan(ref).sum())}, "
          f"+-inf outputs {int(torch.isinf(ref).sum())}, zeros {int((ref == 0).sum())}")
    _assert_equal_nan(dev, ref, name)


def test_maxpool2d_nan_rules(ops):
    """A NaN anywhere in a window (first, middle or last tap, already held or new) gives NaN; -inf and +inf taps, and windows
    without a NaN, are exact."""
    for dt in (torch.float32, torch.bfloat16):
        x = torch.full((1, 3, 9, 4), 1.0)
        x[0, 0, 0, 0] = float("nan")      # the first tap of window 0
        x[0, 1, 4, 1] = float("nan")      # the middle tap of window (0, 1)/(0, 2) rows: last row of a window too
        x[0, 2, 8, 2] = float("nan")      # the last tap of the last window
        x[0, :, :, 3] = float("-inf")
        x[0, 1, 6, 3] = float("inf")
        x = x.to(dt)
        dev = ops.maxpool2d(x.cuda(), 3, 2, 1).cpu()
        _assert_equal_nan(dev, _pool_ref(x, 3, 2, 1), f"nan rules {dt}")


# ================================================================================================ upsample2x_into
def _up_axis(n_out, n_in):
    s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * 0.5 - 0.5).clamp_min(0)
    i0 = s.floor().long()
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    return i0, i1, s - i0


def _up_ref_pixels(x, n, yo, xo):
    """f64 bilinear x2 (align_corners=False) and the same interpolation of |x| at output pixels (n, yo, xo); x is CPU f64 NHWC."""
    H, W = x.shape[1:3]
    y0, y1, ly = _up_axis(2 * H, H)
    x0, x1, lx = _up_axis(2 * W, W)
    Y0, Y1, LY, X0, X1, LX = y0[yo], y1[yo], ly[yo][:, None], x0[xo], x1[xo], lx[xo][:, None]
    ref = A = 0
    for (yy, wy) in ((Y0, 1 - LY), (Y1, LY)):
        for (xx, wx) in ((X0, 1 - LX), (X1, LX)):
            v = x[n, yy, xx]
            ref = ref + wy * wx * v
            A = A + wy * wx * v.abs()
    return ref, A


# name, instance, dtype, N, H, W, C, in_extra, pre, post
UP_CASES = [
    ("f32-1x1", "upsample2x<float>", "f32", 2, 1, 1, 4, 0, 0, 4),
    ("bf16-1x7", "upsample2x<bf16>", "bf16", 1, 1, 7, 12, 4, 4, 8),
    ("f32-5x1", "upsample2x<float>", "f32", 2, 5, 1, 8, 8, 0, 8),
    ("bf16-9x13-slice", "upsample2x<bf16>", "bf16", 2, 9, 13, 64, 32, 0, 32),
    ("f32-7x11", "upsample2x<float>", "f32", 1, 7, 11, 32, 0, 8, 4),
    ("f32-cat3", "upsample2x<float>", "f32", 2, 3, 5, 512, 0, 0, 1024),    # h4 into cat3 [..., :512] (taps of layer3 behind it)
    ("bf16-cat2", "upsample2x<bf16>", "bf16", 1, 6, 9, 256, 0, 0, 512),    # h3 into cat2
    ("f32-cat1", "upsample2x<float>", "f32", 2, 12, 16, 128, 0, 0, 256),   # h2 into cat1
    # grid-stride: h2 into cat1 for two 1536 x 2048 pages (2 x 192 x 256 x 128 -> 2 x 384 x 512 x 128 of 384 channels)
    ("f32-cat1-page", "upsample2x<float>", "f32", 2, 192, 256, 128, 0, 0, 256),
    ("bf16-cat1-page", "upsample2x<bf16>", "bf16", 2, 192, 256, 128, 0, 0, 256),
]


def test_upsample_reference_is_torch_f64():
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(2, 5, 7, 4, generator=g, dtype=torch.float64)
    t = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    n, yo, xo = torch.meshgrid(torch.arange(2), torch.arange(10), torch.arange(14), indexing="ij")
    ref, _ = _up_ref_pixels(x, n.reshape(-1), yo.reshape(-1), xo.reshape(-1))
    assert (ref - t.reshape(-1, 4)).abs().max().item() <= 1e-15


@pytest.mark.parametrize("c", UP_CASES, ids=lambda c: c[0])
def test_upsample2x_envelope(ops, c):
    name, inst, dn, N, H, W, C, in_extra, pre, post = c
    dt = _dt(dn)
    g = torch.Generator().manual_seed(SEED + sum(map(ord, name)))
    x = torch.randn(N, H, W, C, generator=g).to(dt)
    xin = torch.full((N, H, W, in_extra + C), SENTINEL, dtype=dt)
    xin[..., in_extra:] = x
    buf, out = _guarded(N, 2 * H, 2 * W, C, dt, pre, post)
    ops.upsample2x_into(xin.cuda()[..., in_extra:], out)
    torch.cuda.synchronize()
    _check_guard(buf, N, pre, C, name)
    Ho, Wo, C4 = 2 * H, 2 * W, C // 4
    npx = N * Ho * Wo
    total = npx * C4
    if npx <= 50000:
        pix = torch.arange(npx)
    else:  # the first and last work item of every sweep, the first and last output row, random pixels
        items = torch.tensor(_sweep_ends(total))
        pix = torch.cat([items // C4, torch.arange(Wo), torch.arange(npx - Wo, npx),
                         torch.randint(0, npx, (N_RANDOM,), generator=g)]).unique()
    n, rem = pix // (Ho * Wo), pix % (Ho * Wo)
    yo, xo = rem // Wo, rem % Wo
    ref, A = _up_ref_pixels(x.double(), n, yo, xo)
    dev = out[n.cuda(), yo.cuda(), xo.cuda()].cpu().double()
    e = (dev - ref).abs()
    gam = _gamma(UP_GAMMA)
    if dt == torch.float32:
        lim = gam * A
        what = "gamma_4 A"
    else:
        lim = BF16_U * ref.abs() * (1 + BF16_EPS) + 2 * gam * A
        what = "(2^-8 |ref| + 2 gamma_4 A)"
    worst = (e / lim.clamp_min(1e-300)).max().item()
    print(f"upsample2x {name} [{inst}] {total} work items ({-(-total // SWEEP)} sweeps), pixels {len(pix)}/{npx}: "
          f"err {e.max().item():.2e}, worst / {what} {worst:.3f}")
    assert torch.all(e <= lim), (name, worst)


# ================================================================================================ east_head
def _head_ref(h1, w9, b9):
    """f64 logits o [P, 9], A = |w| |x| + |b| [P, 9]; h1 [P, 32] f64."""
    w, b = w9.double(), b9.double()
    return h1 @ w.t() + b, h1.abs() @ w.abs().t() + b.abs()


# name, instance, dtype, N, H, W, in_ld extra (h1 is h1buf[..., 8:40] when > 0), saturate
HEAD_CASES = [
    ("f32-npix1", "east_head<float>", "f32", 1, 1, 1, 0, False),
    ("bf16-npix1", "east_head<bf16>", "bf16", 1, 1, 1, 16, False),
    ("f32-npix255", "east_head<float>", "f32", 1, 15, 17, 16, False),
    ("bf16-npix255", "east_head<bf16>", "bf16", 1, 5, 51, 0, False),
    ("f32-npix257", "east_head<float>", "f32", 1, 1, 257, 0, True),
    ("bf16-npix257", "east_head<bf16>", "bf16", 1, 257, 1, 16, True),
    ("f32-2x10x14-slice", "east_head<float>", "f32", 2, 10, 14, 16, True),
    # grid-stride: h1 of three 1536 x 2048 pages (3 x 384 x 512 = 589 824 pixels)
    ("f32-pages", "east_head<float>", "f32", 3, 384, 512, 0, True),
    ("bf16-pages", "east_head<bf16>", "bf16", 3, 384, 512, 16, True),
]


@pytest.mark.parametrize("c", HEAD_CASES, ids=lambda c: c[0])
def test_east_head_envelope(ops, c):
    name, inst, dn, N, H, W, extra, saturate = c
    dt = _dt(dn)
    g = torch.Generator().manual_seed(SEED + sum(map(ord, name)))
    P = N * H * W
    h1 = torch.randn(P, 32, generator=g)
    w9, b9 = torch.randn(9, 32, generator=g) * 0.3, torch.randn(9, generator=g)
    sat = torch.zeros(P, dtype=torch.bool)
    if saturate:  # every third pixel: channel 0 is +-1 and carries a score weight of 100, so the logit lies near +-100
        w9[0] = 0.0
        w9[0, 0] = 100.0
        b9[0] = 0.0
        sat = torch.arange(P) % 3 == 0
        h1[sat, 0] = torch.where(torch.rand(int(sat.sum()), generator=g) < 0.5, -1.0, 1.0) * (1 + 0.02 * torch.rand(int(sat.sum()), generator=g))
        h1[~sat, 0] *= 0.02
    h1 = h1.to(dt)
    ld = 32 + 2 * extra
    h1buf = torch.full((P, ld), SENTINEL, dtype=dt)
    h1buf[:, extra:extra + 32] = h1
    h1d = h1buf.cuda().view(N, H, W, ld)[..., extra:extra + 32]
    sbuf = torch.full((P + 8,), SENTINEL, device="cuda")
    gbuf = torch.full((P * 8 + 16,), SENTINEL, device="cuda")
    score, geo = sbuf[4:4 + P].view(N, H, W), gbuf[8:8 + P * 8].view(N, H, W, 8)
    ops.east_head(h1d, w9.cuda(), b9.cuda(), score=score, geo=geo)
    torch.cuda.synchronize()
    assert torch.all(sbuf[:4] == SENTINEL) and torch.all(sbuf[4 + P:] == SENTINEL), name
    assert torch.all(gbuf[:8] == SENTINEL) and torch.all(gbuf[8 + P * 8:] == SENTINEL), name
    o, A = _head_ref(h1.double(), w9, b9)
    G = _gamma(HEAD_GAMMA) * A
    dg = geo.cpu().reshape(P, 8).double()
    eg = (dg - o[:, 1:]).abs()
    wg = (eg / G[:, 1:].clamp_min(1e-300)).max().item()
    s = torch.sigmoid(o[:, 0])
    ds = score.cpu().reshape(P).double()
    G0 = G[:, 0]
    lim = s * (1 - s) * (1 + G0) * G0 + s * ((1 - s) * EXPF_REL + 2 * U) + 2.0 ** -126
    es = (ds - s).abs()
    ws = (es / lim).max().item()
    print(f"east_head {name} [{inst}] npix {P} ({-(-P // SWEEP)} sweeps), in_ld {ld}: geo worst / G {wg:.3f}, "
          f"score worst / bound {ws:.3f}, saturated pixels {int(sat.sum())}")
    assert torch.all(eg <= G[:, 1:]), (name, wg)
    assert torch.all(es <= lim), (name, ws)
    assert not torch.isnan(ds).any() and not torch.isnan(dg).any()
    if saturate:
        assert torch.all(o[sat, 0].abs() >= 95)
        assert torch.equal(ds[sat], (o[sat, 0] > 0).double()), name


# ================================================================================================ layout helpers
def _tie_values(g, n):
    """f32 values whose low 16 bits are exactly 0x8000 (halfway between two bf16), with even and odd bf16 mantissas, and specials."""
    hi = torch.randint(0x3000, 0x4800, (n,), generator=g, dtype=torch.int32)
    v = ((hi << 16) | 0x8000).view(torch.float32).clone()
    v[::7] = -v[::7]
    v[:4] = torch.tensor([float("inf"), float("-inf"), 0.0, -0.0])
    return v


# name, instances, N, C, H, W, out/in extra channels (pre, post)
LAYOUT_CASES = [
    ("c3-1x1", 2, 3, 1, 1, 1, 2),
    ("c5-3x7", 1, 5, 3, 7, 3, 0),
    ("c32-9x1", 2, 32, 9, 1, 0, 8),
    ("c64-7x9", 1, 64, 7, 9, 8, 8),
    ("c32-pages", 2, 32, 192, 256, 0, 16),     # grid-stride: 3.1M work items
]


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("c", LAYOUT_CASES, ids=lambda c: c[0])
def test_layout_helpers_envelope(ops, nat, c, dn):
    name, N, C, H, W, pre, post = c
    dt = _dt(dn)
    g = torch.Generator().manual_seed(SEED + sum(map(ord, name)))
    x = torch.randn(N, C, H, W, generator=g)
    flat = x.view(-1)
    k = min(flat.numel(), 4096)
    flat[:k] = _tie_values(g, k)[torch.randperm(k, generator=g)]
    exp = x.permute(0, 2, 3, 1).contiguous().to(dt)
    # NCHW f32 -> NHWC dtype into a channel slice (out_ld = pre + C + post)
    buf, out = _guarded(N, H, W, C, dt, pre, post)
    ops.nchw_to_nhwc(x.cuda(), dt, out=out)
    torch.cuda.synchronize()
    _check_guard(buf, N, pre, C, name)
    bits = torch.int16 if dt == torch.bfloat16 else torch.int32
    same = torch.equal(out.cpu().contiguous().view(bits), exp.view(bits))
    total = N * C * H * W
    print(f"layout {name} {dn} [nchw_to_nhwc<{'bf16' if dn == 'bf16' else 'float'}>, nhwc_to_nchw<...>] {total} work items "
          f"({-(-total // SWEEP)} sweeps): nhwc bit-equal {same}")
    assert same, name
    # NHWC dtype (a channel slice, in_ld > C) -> NCHW f32, into a span of a sentinel buffer; then the round trip
    n = total
    obuf = torch.full((n + C * H * W + 16,), SENTINEL, device="cuda")   # one image and a bit behind the output
    nat.check(nat.lib().msocr_nhwc_to_nchw_f32(out.data_ptr(), N, C, H, W, out.stride(2), ops._dt(out), obuf[4:].data_ptr(),
                                               ops._stream()), "nhwc_to_nchw")
    torch.cuda.synchronize()
    assert torch.all(obuf[:4] == SENTINEL) and torch.all(obuf[4 + n:] == SENTINEL), name
    back = obuf[4:4 + n].view(N, C, H, W).cpu()
    assert torch.equal(back.view(torch.int32), exp.float().permute(0, 3, 1, 2).contiguous().view(torch.int32)), name
    if dt == torch.float32:
        assert torch.equal(back.view(torch.int32), x.view(torch.int32)), name


# ================================================================================================ resize_linear_u8
@pytest.mark.parametrize("size", env.LINEAR_SIZES + [env.LINEAR_BIG], ids=lambda s: "x".join(map(str, s)))
def test_resize_linear_u8_envelope(ops, size):
    from oracle import imgproc
    N, sh, sw, dh, dw = size
    rng = np.random.default_rng(SEED + sh * 7 + sw)
    imgs = np.stack([rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8) for _ in range(N)])
    got = ops.resize_linear_u8(torch.from_numpy(imgs).cuda(), dh, dw).cpu().numpy()
    total = N * dh * dw
    bad = 0
    for i in range(N):
        bad += int((got[i] != imgproc.resize_linear_u8(imgs[i], dw, dh)).sum())
    path = "area2x" if (sw, sh) == (2 * dw, 2 * dh) else "linear"
    print(f"resize_linear_u8 {sh}x{sw}->{dh}x{dw} N {N} [resize_linear_u8, {path}] {total} work items ({-(-total // SWEEP)} sweeps): "
          f"{bad} bytes differ from the oracle")
    assert bad == 0, size


# ================================================================================================ crop_resize_pad
def _crop_setup(rng, canvases_repeat=1):
    H, W = env.PAGE_HW
    pages = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    boxes = env.crop_boxes(rng) * canvases_repeat
    pids = [i % 2 for i in range(len(boxes))]
    return pages, boxes, pids


def _oracle_canvas(pages, d, ih, iw):
    """resize_and_pad's canvas for a descriptor with any new size (mixed up / down included): its branch rule and placement."""
    from oracle import imgproc
    pg, x1, y1, x2, y2, nw, nh, y0 = (int(v) for v in d)
    crop = pages[pg, y1:y2, x1:x2]
    r = imgproc.resize_area_u8(crop, nw, nh) if (nh < y2 - y1 or nw < x2 - x1) else imgproc.resize_linear_u8(crop, nw, nh)
    can = np.full((ih, iw, 3), 255, dtype=np.uint8)
    can[y0:y0 + nh, :nw] = r
    return can


def _guarded_pages(pages):
    """The pages as a contiguous view with one page of sentinel bytes before and after them (a descriptor outside the pages that
    got past a check would read there, not outside the allocation)."""
    N, H, W, _ = pages.shape
    buf = torch.full((N + 2, H, W, 3), 77, dtype=torch.uint8)
    buf[1:N + 1] = torch.from_numpy(pages)
    bd = buf.cuda()
    return bd, bd[1:N + 1]


@pytest.mark.parametrize("canvas", env.CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_crop_resize_pad_envelope(ops, canvas):
    from oracle import imgproc
    ih, iw = canvas
    rng = np.random.default_rng(SEED + ih + iw)
    rep = 2 if ih * iw > 10000 else 1       # 64 x 256: 62 crops = 1.0M canvas pixels (the block-stride loop of every workgroup runs 64x)
    pages, boxes, pids = _crop_setup(rng, rep)
    desc, keep = ops.crop_descriptors(boxes, pids, env.PAGE_HW, ih, iw)
    assert keep.all()
    # two crops the host descriptors cannot produce: one axis up and the other down (INTER_AREA falls back to linear)
    extra = np.array([[0, 10, 20, 40, 60, 80, 16, 3], [1, 100, 50, 300, 55, iw, 9, 0]], dtype=np.int32)
    desc = np.concatenate([desc, extra])
    _, pd = _guarded_pages(pages)
    got_h = ops.crop_resize_pad(pd, desc, ih, iw).cpu().numpy()
    got_d = ops.crop_resize_pad(pd, None, ih, iw, desc_dev=torch.from_numpy(desc).cuda()).cpu().numpy()
    seen, bad = set(), 0
    for k, d in enumerate(desc):
        exp = _oracle_canvas(pages, d, ih, iw)
        if k < len(boxes):
            (x1, y1, x2, y2), pg = boxes[k], pids[k]
            assert np.array_equal(exp, imgproc.resize_and_pad(pages[pg, y1:y2, x1:x2], ih, iw)), k
        w, h = int(d[3] - d[1]), int(d[4] - d[2])
        seen.add(env.branch(w, h, int(d[5]), int(d[6])))
        bad += int((got_h[k] != exp).sum()) + int((got_d[k] != exp).sum())
    total = len(desc) * ih * iw
    print(f"crop_resize_pad {ih}x{iw} [crop_resize_pad] {len(desc)} crops, {total} canvas pixels, branches {sorted(seen)}: "
          f"{bad} bytes differ from the oracle")
    assert bad == 0, canvas
    assert {"copy", "linear", "area"} <= seen


def test_crop_resize_pad_device_validation(ops):
    """desc_host=None: the kernel checks every descriptor itself.  Each invalid one (breaking one condition) gives a canvas of 255;
    valid neighbours stay equal to the oracle."""
    ih, iw = 32, 100
    rng = np.random.default_rng(SEED)
    pages, boxes, pids = _crop_setup(rng)
    N, (H, W) = 2, env.PAGE_HW
    good, _ = ops.crop_descriptors(boxes[:6], pids[:6], env.PAGE_HW, ih, iw)
    base = good[2].copy()                                   # a valid descriptor to break, one field at a time
    pg, x1, y1, x2, y2, nw, nh, y0 = (int(v) for v in base)
    broken = {
        "page < 0": (0, -1), "page >= N": (0, N), "x1 < 0": (1, -1), "y1 < 0": (2, -1), "x2 > W": (3, W + 1), "y2 > H": (4, H + 1),
        "x2 <= x1": (3, x1), "y2 <= y1": (4, y1), "new_w < 1": (5, 0), "new_w > img_w": (5, iw + 1), "new_h < 1": (6, 0),
        "new_h > img_h": (6, ih + 1), "y0 < 0": (7, -1), "y0 + new_h > img_h": (7, ih - nh + 1),
    }   # new_h > img_h also breaks y0 + new_h <= img_h: no y0 >= 0 keeps that one
    desc, names = [], []
    for i, (why, (f, v)) in enumerate(broken.items()):
        desc.append(good[i % len(good)])
        names.append("valid")
        b = base.copy()
        b[f] = v
        desc.append(b)
        names.append(why)
    desc.append(good[0])
    names.append("valid")
    desc = np.stack(desc).astype(np.int32)
    _, pd = _guarded_pages(pages)
    for k, d in enumerate(desc):   # the host check refuses each broken descriptor on its own
        if names[k] != "valid":
            with pytest.raises(ops.nat.NativeError):
                ops.crop_resize_pad(pd, desc[k:k + 1], ih, iw)
    got = ops.crop_resize_pad(pd, None, ih, iw, desc_dev=torch.from_numpy(desc).cuda()).cpu().numpy()
    for k, d in enumerate(desc):
        if names[k] == "valid":
            assert np.array_equal(got[k], _oracle_canvas(pages, d, ih, iw)), k
        else:
            assert np.all(got[k] == 255), (k, names[k])
    print(f"crop_resize_pad device validation: {len(broken)} invalid descriptors filled with 255, {names.count('valid')} valid ones exact")


# ================================================================================================ C-ABI rejections
def test_abi_rejections_launch_nothing(ops, nat):
    L = nat.lib()
    E_ARG = -1
    st = ops._stream()
    a = torch.full((4096,), SENTINEL, device="cuda")          # 16 KB: every call below would stay inside it if it launched
    o = torch.full((4096,), SENTINEL, device="cuda")
    ap, op_ = a.data_ptr(), o.data_ptr()
    w9 = torch.zeros(9 * 32 + 9, device="cuda")
    F32, BF16 = nat.F32, nat.BF16
    calls = {
        # maxpool (in, N, H, W, C, in_ld, k, s, p, dtype, out, Ho, Wo, out_ld)
        "maxpool 2p > k": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 3, 1, 2, F32, op_, 4, 4, 4, st),
        "maxpool 2p > k (k 2, p 2)": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 2, 2, 2, F32, op_, 2, 2, 4, st),
        "maxpool in_ld < C": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 8, 4, 2, 2, 0, F32, op_, 2, 2, 8, st),
        "maxpool out_ld < C": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 8, 8, 2, 2, 0, BF16, op_, 2, 2, 4, st),
        "maxpool C % 4": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 6, 8, 2, 2, 0, F32, op_, 2, 2, 8, st),
        "maxpool k 0": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 0, 1, 0, F32, op_, 2, 2, 4, st),
        "maxpool s 0": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 2, 0, 0, F32, op_, 2, 2, 4, st),
        "maxpool Ho 0": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 2, 2, 0, F32, op_, 0, 2, 4, st),
        "maxpool last window off the map": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 2, 2, 0, F32, op_, 3, 2, 4, st),
        "maxpool null in": lambda: L.msocr_maxpool2d(None, 1, 4, 4, 4, 4, 2, 2, 0, F32, op_, 2, 2, 4, st),
        "maxpool dtype": lambda: L.msocr_maxpool2d(ap, 1, 4, 4, 4, 4, 2, 2, 0, 7, op_, 2, 2, 4, st),
        # east_head (h1, npix, in_ld, dtype, w9, b9, score, geo)
        "east_head f32 in_ld % 4": lambda: L.msocr_east_head(ap, 8, 34, F32, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head bf16 in_ld % 8": lambda: L.msocr_east_head(ap, 8, 36, BF16, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head f32 h1 misaligned": lambda: L.msocr_east_head(ap + 4, 8, 32, F32, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head bf16 h1 misaligned": lambda: L.msocr_east_head(ap + 8, 8, 32, BF16, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head geo misaligned": lambda: L.msocr_east_head(ap, 8, 32, F32, w9.data_ptr(), w9.data_ptr(), op_, op_ + 260, st),
        "east_head in_ld < 32": lambda: L.msocr_east_head(ap, 8, 28, F32, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head npix 0": lambda: L.msocr_east_head(ap, 0, 32, F32, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        "east_head null w9": lambda: L.msocr_east_head(ap, 8, 32, F32, None, w9.data_ptr(), op_, op_ + 256, st),
        "east_head dtype": lambda: L.msocr_east_head(ap, 8, 32, 7, w9.data_ptr(), w9.data_ptr(), op_, op_ + 256, st),
        # normalize_u8 (src, N, H, W, pad_t, pad_l, Hp, Wp, cpad, mode, dtype, out)
        "normalize mode 2": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, 0, 0, 4, 4, 4, 2, F32, op_, st),
        "normalize cpad 5": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, 0, 0, 4, 4, 5, 0, F32, op_, st),
        "normalize Hp < H + pad_t": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, 1, 0, 4, 4, 4, 0, F32, op_, st),
        "normalize Wp < W + pad_l": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, 0, 1, 5, 4, 4, 0, F32, op_, st),
        "normalize pad_t < 0": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, -1, 0, 4, 4, 4, 0, F32, op_, st),
        "normalize N 0": lambda: L.msocr_normalize_u8(ap, 0, 4, 4, 0, 0, 4, 4, 4, 0, F32, op_, st),
        "normalize dtype": lambda: L.msocr_normalize_u8(ap, 1, 4, 4, 0, 0, 4, 4, 4, 0, 7, op_, st),
        # resize_linear_u8 (src, N, sh, sw, dst, dh, dw)
        "resize dh 0": lambda: L.msocr_resize_linear_u8(ap, 1, 4, 4, op_, 0, 4, st),
        "resize sw 0": lambda: L.msocr_resize_linear_u8(ap, 1, 4, 0, op_, 4, 4, st),
        "resize null dst": lambda: L.msocr_resize_linear_u8(ap, 1, 4, 4, None, 4, 4, st),
        # upsample2x (in, N, H, W, C, in_ld, dtype, out, out_ld)
        "upsample C % 4": lambda: L.msocr_upsample2x_bilinear(ap, 1, 2, 2, 6, 8, F32, op_, 8, st),
        "upsample in_ld < C": lambda: L.msocr_upsample2x_bilinear(ap, 1, 2, 2, 8, 4, F32, op_, 8, st),
        "upsample out_ld < C": lambda: L.msocr_upsample2x_bilinear(ap, 1, 2, 2, 8, 8, BF16, op_, 4, st),
        "upsample H 0": lambda: L.msocr_upsample2x_bilinear(ap, 1, 0, 2, 8, 8, F32, op_, 8, st),
        "upsample dtype": lambda: L.msocr_upsample2x_bilinear(ap, 1, 2, 2, 8, 8, 7, op_, 8, st),
        # layout (in, N, C, H, W, dtype, out, ld)
        "nchw_to_nhwc out_ld < C": lambda: L.msocr_nchw_f32_to_nhwc(ap, 1, 8, 2, 2, F32, op_, 4, st),
        "nchw_to_nhwc dtype": lambda: L.msocr_nchw_f32_to_nhwc(ap, 1, 8, 2, 2, 7, op_, 8, st),
        "nhwc_to_nchw in_ld < C": lambda: L.msocr_nhwc_to_nchw_f32(ap, 1, 8, 2, 2, 4, BF16, op_, st),
        "nhwc_to_nchw W 0": lambda: L.msocr_nhwc_to_nchw_f32(ap, 1, 8, 2, 0, 8, F32, op_, st),
        "nhwc_to_nchw dtype": lambda: L.msocr_nhwc_to_nchw_f32(ap, 1, 8, 2, 2, 8, 7, op_, st),
        # crop_resize_pad (pages, N, H, W, desc_dev, desc_host, M, img_h, img_w, canvases)
        "crop M 0": lambda: L.msocr_crop_resize_pad(ap, 1, 8, 8, op_, None, 0, 4, 4, op_, st),
        "crop null desc_dev": lambda: L.msocr_crop_resize_pad(ap, 1, 8, 8, None, None, 1, 4, 4, op_, st),
        "crop img_w 0": lambda: L.msocr_crop_resize_pad(ap, 1, 8, 8, op_, None, 1, 4, 0, op_, st),
    }
    torch.cuda.synchronize()
    for why, call in calls.items():
        assert call() == E_ARG, why
    torch.cuda.synchronize()
    assert torch.all(a == SENTINEL) and torch.all(o == SENTINEL), "a rejected call wrote"
    print(f"ABI: {len(calls)} rejected calls, nothing written")


def test_envelope_reaches_all_16_instances():
    inst = {c[1] for c in NORM_CASES} | {c[1] for c in POOL_CASES} | {c[1] for c in UP_CASES} | {c[1] for c in HEAD_CASES}
    inst |= {f"{k}<{t}>" for k in ("nchw_to_nhwc", "nhwc_to_nchw") for t in ("float", "bf16")}   # test_layout_helpers_envelope
    inst |= {"resize_linear_u8", "crop_resize_pad"}
    assert len(inst) == 16, sorted(inst)
