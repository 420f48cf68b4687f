"""Square tiles + tail column (csrc/winograd.hip, wino44_*_coltail) through ops.conv2d, switch on against switch off.

On a map with W % 4 == 1 the square Winograd form computes output columns 0 ... W-2 as W // 4 square tiles per tile row and column
W-1 as one F(4,3) x F(1,3) tile per tile row instead of a fourth, padded square tile.  The square tiles are the padded form's own
(same tiles, same V rows, same order over K in the GEMM rows), so those columns are bit-identical with the switch off; the last
column is computed differently and is held to the project's bounds for the square form: 2e-5 * scale against an f64 convolution and
3 x the tall split form's error (here: on that column) + 1e-7 * scale.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 7.0

CASES = [
    # name, N, H, W, Cin, Cout, relu, residual
    ("pp128x256-both-mt-below-a-tile", 3, 4, 13, 128, 256, False, False),   # conv_split_pp_kernel's 128 x 256 tile; Mt44 = 9, Mt41 = 3
    ("split64", 2, 4, 13, 128, 64, False, False),                           # conv_split_kernel<64>
    ("partial-h-one-square-tile", 2, 9, 5, 128, 128, True, True),           # TH = 3 with one real row in the last; one square tile + tail
    ("tail-mt-129", 129, 4, 5, 128, 128, False, False),                     # Mt41 = Mt44 = 129: both cross an M-tile boundary
    ("six-tiles-th2", 2, 8, 25, 256, 256, False, True),                     # six square tiles + tail, TH = 2
]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


def _run(ops, x, w, b, relu, r, profile=False):
    """conv2d into a channel slice of a wider buffer with sentinel channels on both sides and a sentinel image behind."""
    N, H, W, _ = x.shape
    Cout = w.shape[0]
    buf = torch.full((N + 1, H, W, 4 + Cout + 4), SENTINEL, device="cuda")
    out = buf[:N, :, :, 4:4 + Cout]
    recs = None
    if profile:
        ops.PROFILE = []
    try:
        ops.conv2d(x, w, b, (1, 1), (1, 1), relu, r, out=out)
    finally:
        recs, ops.PROFILE = ops.PROFILE, None
    torch.cuda.synchronize()
    assert torch.all(buf[..., :4] == SENTINEL) and torch.all(buf[..., 4 + Cout:] == SENTINEL) and torch.all(buf[N:] == SENTINEL)
    return out, recs


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_coltail_vs_padded_tile_tall_form_and_f64(ops, case, monkeypatch):
    name, N, H, W, Cin, Cout, relu, use_res = case
    assert W % 4 == 1 and W >= 5
    monkeypatch.setattr(ops, "_tall_pays", lambda H_: True)
    monkeypatch.setattr(ops, "_square_pays", lambda W_: True)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE_MIN_CIN", 128)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 1)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    g = torch.Generator(device="cuda").manual_seed(4100 + sum(map(ord, name)))
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, 3, 3, Cin, generator=g, device="cuda") * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g, device="cuda") * 0.1
    r = torch.randn(N, H, W, Cout + 32, generator=g, device="cuda")[..., :Cout] if use_res else None   # a channel slice too
    wk = ops.attach_winograd(w.clone(), True)
    assert wk._msocr_wino44_split.shape == (3, 36, Cin // 32, Cout, 32) and wk._msocr_wino41_split.shape == (3, 18, Cin // 32, Cout, 32)

    ref = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.cpu().double().permute(0, 3, 1, 2), b.cpu().double(), padding=1)
    if use_res:
        ref = ref + r.cpu().double().permute(0, 3, 1, 2)
    if relu:
        ref = F.relu(ref)
    ref = ref.permute(0, 2, 3, 1)
    scale = max(ref.abs().max().item(), 1.0)
    TH = -(-H // 4)
    mt44, mt41 = N * TH * (W // 4), N * TH

    # switch on: staged (profiled) and one-call
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    staged, recs = _run(ops, x, wk, b, relu, r, profile=True)
    gemm = [t for t in recs if t[2] == "conv_gemm"]
    assert [t[4][3] for t in gemm] == ["winograd44_split"], [t[4] for t in gemm]
    assert gemm[0][3][1] == 2.0 * (36 * mt44 + 18 * mt41) * Cin * Cout, (gemm[0][3], mt44, mt41)
    assert [t[2] for t in recs] == ["wino_in", "conv_gemm", "wino_out"]
    rows, res_io = 36 * mt44 + 18 * mt41, 2 if use_res else 1
    assert recs[0][3] == 4.0 * (N * H * W * Cin + rows * Cin) and recs[2][3] == 4.0 * (rows * Cout + N * H * W * Cout * res_io)
    on, _ = _run(ops, x, wk, b, relu, r)
    assert torch.equal(on, staged), "one-call result differs from the staged one"

    # switch off: the padded tile; one conv_gemm of 36 * N TH ceil(W/4) rows
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 0)
    off, recs_off = _run(ops, x, wk, b, relu, r, profile=True)
    gemm_off = [t for t in recs_off if t[2] == "conv_gemm"]
    assert [t[4][3] for t in gemm_off] == ["winograd44_split"]
    assert gemm_off[0][3][1] == 2.0 * 36 * N * TH * (W // 4 + 1) * Cin * Cout
    assert torch.equal(on[:, :, :W - 1], off[:, :, :W - 1]), "columns 0 ... W-2 differ from the padded form's"

    # the last column: against f64, and against the tall split form's error on the same column
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 0)
    tall, recs_t = _run(ops, x, wk, b, relu, r, profile=True)
    assert [t[4][3] for t in recs_t if t[2] == "conv_gemm"] == ["winograd42_split"]
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 1)
    col = ref[:, :, W - 1]
    e_c = (on[:, :, W - 1].cpu().double() - col).abs().max().item()
    e_p = (off[:, :, W - 1].cpu().double() - col).abs().max().item()
    e_t = (tall[:, :, W - 1].cpu().double() - col).abs().max().item()
    print(f"coltail {name}: last column err / scale: column form {e_c / scale:.2e}, padded tile {e_p / scale:.2e}, tall {e_t / scale:.2e}; "
          f"column / tall {e_c / max(e_t, 1e-300):.2f}")
    assert e_c <= 2e-5 * scale and e_c <= 3.0 * e_t + 1e-7 * scale, (e_c, e_t, scale)

    # image n alone = image n inside the batch
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    for n in range(N):
        img = ops.conv2d(x[n:n + 1], wk, b, (1, 1), (1, 1), relu, r[n:n + 1] if use_res else None)
        assert torch.equal(img, on[n:n + 1]), (name, n)


def test_coltail_batch_cut_by_the_workspace_limit(ops, monkeypatch):
    """The workspace is linear in N, so conv2d's cut of the batch by WINO_WS_LIMIT gives the one-call result, staged or not."""
    monkeypatch.setattr(ops, "_square_pays", lambda W_: True)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE_MIN_CIN", 128)
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    N, H, W, Cin, Cout = 5, 4, 13, 128, 128
    g = torch.Generator(device="cuda").manual_seed(4177)
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, 3, 3, Cin, generator=g, device="cuda") * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g, device="cuda") * 0.1
    wk = ops.attach_winograd(w, True)
    one = ops.conv2d(x, wk, b, (1, 1), (1, 1), True)
    per_image = (36 * 3 + 18) * (Cin + Cout) * 4
    monkeypatch.setattr(ops, "WINO_WS_LIMIT", 2 * per_image + 1)   # parts of 2, 2 and 1 images
    for prof in (None, []):
        ops.PROFILE = prof
        try:
            cut = ops.conv2d(x, wk, b, (1, 1), (1, 1), True)
        finally:
            recs, ops.PROFILE = ops.PROFILE, None
        assert torch.equal(cut, one), prof is not None
        if prof is not None:
            assert [t[4][3] for t in recs if t[2] == "conv_gemm"] == ["winograd44_split"] * 3
