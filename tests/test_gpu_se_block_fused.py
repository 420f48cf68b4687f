"""The per-crop kernels of the SE blocks (csrc/winograd.hip, wino44_output_kernel_chain / wino44_output_kernel_se) through
ops.se_block, switch on against switch off.

Where one image's map fits LDS, the output transform of conv1 hands it to the input transform of conv2, and the output transform of
conv2 hands it to the SE tail, without a round trip through HBM.  The arithmetic is the device functions of the separate kernels in
the same order, so every comparison here is torch.equal: there is no tolerance.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    # N, H, W, C
    (1, 4, 13, 512),   # the workload's shape: 4 tiles x 128 channel groups = one pair per thread
    (3, 4, 13, 512),
    (3, 4, 5, 64),     # the smallest tail-column width; 16 threads per tile, 64 pixel groups for 20 pixels
    (2, 4, 12, 64),    # pure square form, no tail
    (2, 8, 9, 128),    # two tile rows
    (2, 8, 17, 256),   # 10 tiles x 64 channel groups = 640 pairs on 512 threads: the tile loop; 157 760 B of the 163 840 B of LDS
]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


def _square_everywhere(ops, monkeypatch):
    """Every 3x3 weight of at least 64 channels gets the square form's planes, and conv2d takes them on every map."""
    monkeypatch.setattr(ops, "WINOGRAD_MIN_CIN", 64)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE_MIN_CIN", 64)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 1)
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    monkeypatch.setattr(ops, "WINOGRAD_TALL", 1)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    monkeypatch.setattr(ops, "_tall_pays", lambda H_: True)
    monkeypatch.setattr(ops, "_square_pays", lambda W_: True)


def _block(ops, seed, N, H, W, Cin, C, stride=1):
    """Seeded inputs and weights of one SE block: x, an identity distinct from x, conv1 (Cin -> C, stride), conv2 (C -> C), SE."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = rn(N, H, W, Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    idt = rn(N, Ho, Wo, C)
    conv1 = (ops.attach_winograd(rn(C, 3, 3, Cin) * (2.0 / (Cin * 9)) ** 0.5, True), rn(C) * 0.1)
    conv2 = (ops.attach_winograd(rn(C, 3, 3, C) * (2.0 / (C * 9)) ** 0.5, True), rn(C) * 0.1)
    se = (rn(C // 16, C) * (1.0 / C) ** 0.5, rn(C, C // 16) * (16.0 / C) ** 0.5)
    return x, idt, conv1, conv2, se


def _run(ops, fused, x, conv1, conv2, idt, se, stride=1, profile=False):
    """(out, gates, wino_out tags) of ops.se_block with the switch set."""
    C = conv2[0].shape[0]
    gate = torch.full((x.shape[0], C), -1.0, device="cuda")
    old, ops.SE_BLOCK_FUSED = ops.SE_BLOCK_FUSED, int(fused)
    if profile:
        ops.PROFILE = []
    try:
        out = ops.se_block(x, conv1, conv2, idt, se, stride=(stride, stride), gate=gate)
    finally:
        recs, ops.PROFILE = ops.PROFILE, None
        ops.SE_BLOCK_FUSED = old
    torch.cuda.synchronize()
    return out, gate, [r[4] for r in recs if r[2] == "wino_out"] if profile else None


def _fused_tags(tags):
    return [t[2] for t in tags if len(t) > 2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_block_equals_the_three_calls(ops, shape, monkeypatch):
    """Both kernels on every shape, with an identity tensor of its own and with identity = x; profiled or not, the same launches."""
    _square_everywhere(ops, monkeypatch)
    N, H, W, C = shape
    x, idt, conv1, conv2, se = _block(ops, 9100 + H * W + C, N, H, W, C, C)
    for identity in (idt, x):
        ref, ref_gate, _ = _run(ops, False, x, conv1, conv2, identity, se)
        assert torch.isfinite(ref).all() and (ref > 0).any() and (ref_gate > 0).all() and (ref_gate < 1).all()
        out, gate, _ = _run(ops, True, x, conv1, conv2, identity, se)
        assert torch.equal(out, ref) and torch.equal(gate, ref_gate)
        out, gate, tags = _run(ops, True, x, conv1, conv2, identity, se, profile=True)
        assert torch.equal(out, ref) and torch.equal(gate, ref_gate)
        assert _fused_tags(tags) == ["chain", "se"]


def test_se_kernel_alone_behind_a_conv1_that_cannot_chain(ops, monkeypatch):
    """Cin != Cout: conv1 runs as any convolution, conv2 still hands its map to the SE tail in LDS."""
    _square_everywhere(ops, monkeypatch)
    x, idt, conv1, conv2, se = _block(ops, 9201, 2, 4, 13, 128, 256)
    ref, ref_gate, _ = _run(ops, False, x, conv1, conv2, idt, se)
    out, gate, tags = _run(ops, True, x, conv1, conv2, idt, se, profile=True)
    assert torch.equal(out, ref) and torch.equal(gate, ref_gate)
    assert _fused_tags(tags) == ["se"]


@pytest.mark.parametrize("case", [("too-large-for-lds", 2, 8, 25, 256, 256, 1), ("strided-conv1", 2, 8, 26, 128, 256, 2)], ids=lambda c: c[0])
def test_blocks_the_kernels_do_not_take(ops, case, monkeypatch):
    """A map of 204 800 B takes the three calls; behind a strided conv1 (4 x 13 x 256 after it) only the SE kernel runs."""
    _square_everywhere(ops, monkeypatch)
    _, N, H, W, Cin, C, stride = case
    x, idt, conv1, conv2, se = _block(ops, 9300 + stride, N, H, W, Cin, C, stride)
    ref, ref_gate, ref_tags = _run(ops, False, x, conv1, conv2, idt, se, stride, profile=True)
    out, gate, tags = _run(ops, True, x, conv1, conv2, idt, se, stride, profile=True)
    assert torch.equal(out, ref) and torch.equal(gate, ref_gate)
    assert _fused_tags(ref_tags) == [] and "chain" not in _fused_tags(tags)
    if stride == 1:
        assert _fused_tags(tags) == [] and len(tags) == len(ref_tags) == 2
    else:
        assert _fused_tags(tags) == ["se"]


def test_strided_conv1_at_a_map_too_large_launches_neither(ops, monkeypatch):
    """The first block of a TRBA layer on the larger maps: strided conv1 and 8 x 25 x 256 behind it — today's calls, nothing fused."""
    _square_everywhere(ops, monkeypatch)
    x, idt, conv1, conv2, se = _block(ops, 9400, 2, 16, 50, 128, 256, 2)
    ref, ref_gate, _ = _run(ops, False, x, conv1, conv2, idt, se, 2)
    out, gate, tags = _run(ops, True, x, conv1, conv2, idt, se, 2, profile=True)
    assert torch.equal(out, ref) and torch.equal(gate, ref_gate)
    assert _fused_tags(tags) == []


def test_block_cut_by_the_workspace_limit(ops, monkeypatch):
    """One cut of the batch for the whole block: N = 5 in parts of 3 and 2 images gives the uncut result, staged or not."""
    _square_everywhere(ops, monkeypatch)
    N, H, W, C = 5, 4, 13, 128
    x, idt, conv1, conv2, se = _block(ops, 9500, N, H, W, C, C)
    one, one_gate, tags = _run(ops, True, x, conv1, conv2, idt, se, profile=True)
    assert _fused_tags(tags) == ["chain", "se"]
    per_image = (36 * 3 + 18) * (C + C) * 4
    monkeypatch.setattr(ops, "WINO_WS_LIMIT", 3 * per_image + 1)
    for profile in (False, True):
        cut, cut_gate, tags = _run(ops, True, x, conv1, conv2, idt, se, profile=profile)
        assert torch.equal(cut, one) and torch.equal(cut_gate, one_gate)
        if profile:
            assert _fused_tags(tags) == ["chain", "se"] * 2
    ref, ref_gate, _ = _run(ops, False, x, conv1, conv2, idt, se)
    assert torch.equal(one, ref) and torch.equal(one_gate, ref_gate)


def test_trba_cnn_features_bit_identical(ops):
    """TrbaNet.cnn on 4 seeded canvases with the library's own dispatch: layer3 / layer4 take the kernels, the features do not change."""
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers._trba.net import TrbaNet
    net = TrbaNet(synth.trba_state_dict(194, 256, seed=20260128), 194, 256, torch.float32)
    cd = torch.from_numpy(synth.synth_crops(31, 4, 32, 100)).cuda()
    feats = {}
    for fused in (0, 1):
        old, ops.SE_BLOCK_FUSED = ops.SE_BLOCK_FUSED, fused
        ops.PROFILE = []
        try:
            feats[fused] = net.cnn(cd).clone()
        finally:
            recs, ops.PROFILE = ops.PROFILE, None
            ops.SE_BLOCK_FUSED = old
        torch.cuda.synchronize()
        tags = _fused_tags([r[4] for r in recs if r[2] == "wino_out"])
        # 8 blocks of layer3 / layer4 on 4 x 13 x 512 maps; layer3.0's conv1 has 256 input channels and does not chain
        assert tags == ([] if not fused else ["se"] + ["chain", "se"] * 7), tags
    assert torch.isfinite(feats[0]).all() and torch.equal(feats[0], feats[1])
