"""The shared epilogue of the 4-wave GEMM kernels (csrc/conv_common.h epilogue_lds: conv_split_kernel of csrc/conv_split.hip and
conv_igemm_kernel of csrc/conv_igemm.hip): accumulator, + bias, + residual, ReLU, conversion, 16-byte stores.  A tile whose BM rows
all lie below M takes the unrolled path (the residual rows of a pass loaded before its barrier, every row in its own registers), the
last, partial M-tile of a launch the guarded row-by-row path; the M sweep below has launches of either kind alone (M = 128, M < 128)
and of both (M = 129, 200, ...).

(a) Exact f32 identity, no tolerance: out(bias, residual, relu) == max(out(bias) + residual, 0), element for element, for
    msocr_conv1x1_split, msocr_conv2d_split and msocr_conv2d, with and without a bias.  out(bias) is taken from the SAME kernel: a
    split launch without a residual and with Cout % 128 == 0, K >= 64 is routed to conv_split_pp_kernel, whose K order differs, so
    there the base is the launch with a residual of zeros (x + 0 == x for every x the comparison can tell apart); where the routing
    keeps the kernel, the launch without a residual must equal that base too.
(b) Leading dimensions: out_ld = Cout + 8, res_ld = Cout + 4 (bf16: + 8, the 16-byte rule of the descriptor) into a buffer of NaN: the
    gap columns and the rows behind M stay NaN.
(c) General loader: 3x3 / 2 / 1 with a residual on 9x7x32 maps, split and exact, identity (a) and the per-element f64 bound of
    test_gpu_conv_f64.py; the same bound on 1x1 launches with whole tiles (split and the 16x16x4 exact instance), so that the row
    mapping of the unrolled path is checked against f64 in this file too.
(d) bf16 operands on the same M tails against f64 under test_gpu_conv_f64.py's bound (c), into the NaN buffer.
(e) The other instances of conv_igemm_kernel (narrow rows, 32-channel tiles; f32 and bf16) on whole and partial tiles: identity for
    f32, the f64 bounds for both.
(f) Batched path: the Winograd-domain GEMMs of one precision="fp32-exact" tall-form convolution under test_winograd_envelope's bound
    (2x8x6x128 as the smallest case: partial tiles only; 2x32x18x128 has whole tiles)."""
import pytest
import torch

import test_gpu_conv_f64 as f64

pytestmark = pytest.mark.gpu

SEED = 20261018
M_TAILS = (1, 63, 64, 65, 127, 128, 129, 200)
COUTS = (64, 128, 192, 256)
KS = (32, 64, 128)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


def _setup(ops, monkeypatch):
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)


def _weight(ops, entry, Cout, k, Cin, g, dtype=torch.float32):
    w = (torch.randn(Cout, k[0], k[1], Cin, generator=g, device="cuda") * (2.0 / (k[0] * k[1] * Cin)) ** 0.5).to(dtype).contiguous()
    return ops.attach_split(w, entry != "conv2d")


def _input(entry, M, K, g, dtype=torch.float32):
    """(x, stride) of a 1x1 convolution with M output pixels that reaches `entry`: the lean layout, or every second pixel of a row
    (stride 2 is no lean launch, so the split weight goes through the general loader of msocr_conv2d_split)."""
    if entry == "conv2d_split":
        return torch.randn(1, 1, 2 * M - 1, K, generator=g, device="cuda").to(dtype), (1, 2)
    return torch.randn(1, 1, M, K, generator=g, device="cuda").to(dtype), (1, 1)


def _launch(ops, entry, x, w, b, stride, pad=(0, 0), relu=False, res=None, out=None):
    ops.PROFILE = []
    try:
        o = ops.conv2d(x, w, b, stride, pad, relu, res, out=out)
        tags = [t[4][3] for t in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert tags == ["direct" if entry == "conv2d" else "direct_split"], (entry, tags)
    return o


def _same_kernel_without_residual(entry, Cout, K):
    return entry == "conv2d" or not (Cout % 128 == 0 and K >= 64)


def _identity(ops, entry, x, w, b, stride, pad, res, what):
    full = _launch(ops, entry, x, w, b, stride, pad, True, res)
    base = _launch(ops, entry, x, w, b, stride, pad, False, torch.zeros_like(res))
    assert torch.isfinite(base).all(), what
    assert torch.equal(full, (base + res).clamp_min(0)), what
    Cout, KH, KW, Cin = w.shape
    if _same_kernel_without_residual(entry, Cout, KH * KW * Cin):
        assert torch.equal(_launch(ops, entry, x, w, b, stride, pad, False, None), base), (what, "no residual")
    return full


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("entry", ["conv1x1_split", "conv2d_split", "conv2d"])
def test_epilogue_identity_f32(ops, entry, use_bias, monkeypatch):
    _setup(ops, monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(SEED + len(entry) + use_bias)
    hit = 0
    for Cout in COUTS:
        b = torch.randn(Cout, generator=g, device="cuda") * 0.5 if use_bias else None
        for K in KS:
            w = _weight(ops, entry, Cout, (1, 1), K, g)
            for M in M_TAILS:
                x, stride = _input(entry, M, K, g)
                res = torch.randn(1, 1, M, Cout, generator=g, device="cuda")
                full = _identity(ops, entry, x, w, b, stride, (0, 0), res, (entry, use_bias, M, Cout, K))
                hit += int((full == 0).any() and (full > 0).any())
    assert hit > len(COUTS) * len(KS) * len(M_TAILS) // 2   # the clamp is exercised


# ------------------------------------------------------------------------------------------------ (b), (d)
def _nan_out(M, Cout, gap, dtype):
    """A [M + 3][Cout + gap] buffer of NaN and the NHWC view [1, 1, M, Cout] of its first M rows and Cout columns."""
    buf = torch.full((M + 3, Cout + gap), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[:M].unsqueeze(0).unsqueeze(0)[..., :Cout]


def _check_nan_guard(buf, M, Cout, what):
    assert torch.isnan(buf[:, Cout:]).all(), (what, "gap columns were written")
    assert torch.isnan(buf[M:]).all(), (what, "rows behind M were written")
    assert torch.isfinite(buf[:M, :Cout]).all(), (what, "output rows were left unwritten")


@pytest.mark.parametrize("entry", ["conv1x1_split", "conv2d_split", "conv2d"])
def test_epilogue_leading_dimensions_f32(ops, entry, monkeypatch):
    _setup(ops, monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(SEED + 7 + len(entry))
    K = 64
    for Cout in (64, 128):
        b = torch.randn(Cout, generator=g, device="cuda") * 0.5
        w = _weight(ops, entry, Cout, (1, 1), K, g)
        for M in M_TAILS:
            x, stride = _input(entry, M, K, g)
            res = torch.randn(1, 1, M, Cout + 4, generator=g, device="cuda")[..., :Cout]
            buf, out = _nan_out(M, Cout, 8, torch.float32)
            assert ops._pixel_dense_ld(out) == Cout + 8 and ops._pixel_dense_ld(res) == Cout + 4
            _launch(ops, entry, x, w, b, stride, (0, 0), True, res, out=out)
            torch.cuda.synchronize()
            _check_nan_guard(buf, M, Cout, (entry, M, Cout))
            dense = _launch(ops, entry, x, w, b, stride, (0, 0), True, res.contiguous())
            assert torch.equal(out, dense), (entry, M, Cout)


def _bf16_check(ops, x, w, b, res, relu, out, stride, pad, what):
    Cout, KH, KW, Cin = w.shape
    N, Ho, Wo = out.shape[:3]
    rows = torch.arange(N * Ho * Wo)
    ref, A, _ = f64._reference(x, w, b, res, relu, rows, Ho, Wo, stride, pad)
    e = (f64._rows_of(out, rows, Ho, Wo) - ref).abs()
    lim = f64.BF16_U * ref.abs() * (1 + f64.BF16_EPS) + 2 * f64._gamma(KH * KW * Cin) * A
    worst = (e / lim.clamp_min(1e-300)).max().item()
    print(f"{what}: worst / (2^-8 |ref| + 2 gamma_K A) {worst:.3f}")
    assert torch.all(e <= lim), (what, worst)


def test_epilogue_bf16_tails_against_f64(ops, monkeypatch):
    _setup(ops, monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(SEED + 11)
    K = 64
    for Cout in (64, 128):
        b = torch.randn(Cout, generator=g, device="cuda") * 0.5
        w = _weight(ops, "conv2d", Cout, (1, 1), K, g, torch.bfloat16)
        for M in M_TAILS:
            x, stride = _input("conv2d", M, K, g, torch.bfloat16)
            res = torch.randn(1, 1, M, Cout + 8, generator=g, device="cuda").bfloat16()[..., :Cout]
            buf, out = _nan_out(M, Cout, 8, torch.bfloat16)
            _launch(ops, "conv2d", x, w, b, stride, (0, 0), True, res, out=out)
            torch.cuda.synchronize()
            _check_nan_guard(buf, M, Cout, ("bf16", M, Cout))
            _bf16_check(ops, x, w, b, res, True, out, stride, (0, 0), f"bf16 M={M} Cout={Cout}")


# ------------------------------------------------------------------------------------------------ (c)
def _f32_check(entry, x, w, b, res, relu, out, stride, pad, what):
    Cout, KH, KW, Cin = w.shape
    N, Ho, Wo = out.shape[:3]
    rows = torch.arange(N * Ho * Wo)
    ref, A, _ = f64._reference(x, w, b, res, relu, rows, Ho, Wo, stride, pad)
    e = (f64._rows_of(out, rows, Ho, Wo) - ref).abs()
    lim = (f64.SPLIT_GAMMA if entry != "conv2d" else 1.0) * f64._gamma(KH * KW * Cin) * A
    worst = (e / lim.clamp_min(1e-300)).max().item()
    print(f"{what}: worst / gamma_K A {worst:.3f}")
    assert torch.all(e <= lim), (what, worst)


@pytest.mark.parametrize("entry", ["conv2d_split", "conv2d"])
@pytest.mark.parametrize("Cout", [64, 128])
def test_epilogue_general_loader_3x3_stride2_residual(ops, entry, Cout, monkeypatch):
    _setup(ops, monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(SEED + 13 + Cout)
    N, H, W, Cin = 13, 9, 7, 32            # 13 x 5 x 4 = 260 output pixels: two whole tiles of 128 and a partial one
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = _weight(ops, entry, Cout, (3, 3), Cin, g)
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5
    res = torch.randn(N, 5, 4, Cout, generator=g, device="cuda")
    full = _identity(ops, entry, x, w, b, (2, 2), (1, 1), res, (entry, Cout))
    _f32_check(entry, x, w, b, res, True, full, (2, 2), (1, 1), f"3x3/2/1 {entry} Cout={Cout}")


@pytest.mark.parametrize("entry", ["conv1x1_split", "conv2d"])
@pytest.mark.parametrize("Cout", [64, 128, 256])
def test_epilogue_1x1_whole_tiles_against_f64(ops, entry, Cout, monkeypatch):
    """(a) takes both sides from one kernel; this pins the unrolled path's row mapping to f64: a 1x1 launch of M = 300 (two whole tiles
    and a partial one) with a residual, per-element bound of test_gpu_conv_f64.py, K = 128 (split) and 64 (the 16x16x4 instance)."""
    _setup(ops, monkeypatch)
    g = torch.Generator(device="cuda").manual_seed(SEED + 23 + Cout)
    M, K = 300, 128 if entry == "conv1x1_split" else 64
    x, stride = _input(entry, M, K, g)
    w = _weight(ops, entry, Cout, (1, 1), K, g)
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5
    res = torch.randn(1, 1, M, Cout, generator=g, device="cuda")
    out = _launch(ops, entry, x, w, b, stride, (0, 0), True, res)
    _f32_check(entry, x, w, b, res, True, out, stride, (0, 0), f"1x1 {entry} Cout={Cout} M={M}")


# ------------------------------------------------------------------------------------------------ (e)
OTHER_INSTANCES = [
    # mode, Cin, Cout: conv_igemm_kernel instances the sweeps above do not reach (BM = 128 or 256; M = 600 has whole and partial tiles)
    ("f32", 16, 128), ("f32", 16, 64), ("f32", 64, 96), ("f32", 16, 32),
    ("bf16", 64, 128), ("bf16", 32, 128), ("bf16", 64, 64), ("bf16", 32, 64), ("bf16", 64, 96), ("bf16", 32, 32),
]


@pytest.mark.parametrize("case", OTHER_INSTANCES, ids=lambda c: f"{c[0]}-cin{c[1]}-cout{c[2]}")
def test_epilogue_other_igemm_instances(ops, case, monkeypatch):
    _setup(ops, monkeypatch)
    mode, Cin, Cout = case
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(SEED + 17 + Cin * Cout)
    N, H, W = 2, 20, 15                    # 3x3 / 1 / 1: M = 600
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda").to(dt)
    w = _weight(ops, "conv2d", Cout, (3, 3), Cin, g, dt)
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5
    res = torch.randn(N, H, W, Cout, generator=g, device="cuda").to(dt)
    if mode == "f32":
        full = _identity(ops, "conv2d", x, w, b, (1, 1), (1, 1), res, case)
        _f32_check("conv2d", x, w, b, res, True, full, (1, 1), (1, 1), str(case))
    else:
        for r in (res, None):
            out = _launch(ops, "conv2d", x, w, b, (1, 1), (1, 1), True, r)
            _bf16_check(ops, x, w, b, r, True, out, (1, 1), (1, 1), f"{case} res={r is not None}")


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("shape", [(2, 8, 6), (2, 32, 18)], ids=["2x8x6", "2x32x18"])
def test_epilogue_batched_winograd_gemms_fp32_exact(ops, shape, monkeypatch):
    N, H, W = shape
    Cin = Cout = 128
    case = ("w42-exact-epilogue", "42", N, H, W, Cin, Cout, True, "slice", False)
    g = torch.Generator(device="cuda").manual_seed(SEED + 19 + H)
    x, w, b, r = f64._wino_inputs(case, g)
    wk, tag = f64._wino_weights(ops, w, "42", monkeypatch)
    assert tag == "winograd42"
    ops.PROFILE = []
    out = ops.conv2d(x, wk, b, (1, 1), (1, 1), True, r)
    tags = [t[4][3] for t in ops.PROFILE if t[2] == "conv_gemm"]
    ops.PROFILE = None
    assert tags == [tag], tags
    ref, cpu, full = f64._f64_conv3x3(x, w, b, r, True, False)
    scale = max(full.abs().max().item(), 1.0)
    err = (out.cpu().double() - ref).abs().max().item()
    direct = ops.conv2d(x, ops.attach_split(w.clone(), False), b, (1, 1), (1, 1), True, r)
    e_d = (direct.cpu().double() - ref).abs().max().item()
    e_cpu = (cpu - ref).abs().max().item()
    print(f"tall exact {shape}: err {err / scale:.2e}, / direct err {err / max(e_d, 1e-300):.2f}, / cpu-f32 err {err / max(e_cpu, 1e-300):.2f}")
    assert err <= 2e-5 * scale and err <= 8 * e_d + 1e-6 * scale, (err, e_d, scale)
    assert err <= f64.F32_CPU_FACTOR * e_cpu + f64.F32_CPU_SLACK * scale, (err, e_cpu, scale)
