"""ops.se_block against float64 at the edges of the per-crop kernels (csrc/winograd.hip, wino44_output_kernel_chain /
wino44_output_kernel_se; csrc/se_tail.h).

test_gpu_se_block_fused.py holds the two paths of ops.se_block to each other bit for bit; nothing there would notice an error they
share (the wiring of se_block, _square_desc, the flags and the bias of each stage, the batch cut).  Here the whole block,
out = relu(y * gate + identity), y = conv2(relu(conv1 x + b1)) + b2, gate = sigmoid(W2 relu(W1 mean_hw(y))), is held to a float64
reference of the operation computed from the raw weights (`_block_ref64`), with the switch on and with it off, on

  - every partial tile of the crop: H % 4 in {1, 2, 3}, W % 4 in {2, 3}, H < 4, W < 4, W == 1, the tail column on a partial tile row
    (wino_output_body skips rows and columns of the LDS crop there, and wino_input_body must read zeros past the crop's edge from
    an LDS buffer that has live SE scratch right behind it);
  - C = 1024 (PG = 4 pixel groups) and the largest map that fits LDS at every channel count the SE tail takes, and one pixel more;
  - more images than the device has CUs (one workgroup per image);
  - conv1 with Cin != Cout and with stride 2 (only the SE kernel runs) onto partial maps;
  - x as a channel slice of a wider buffer and as the first columns of a wider map (the chain's input transform reads x strided).

Inputs.  An f64 tolerance only sees the SE tail if the gates move the result: the SE weights are scaled (W1 ~ N(0, 1 / C),
W2 ~ N(0, 1.2 / (C / 16))) and conv2's bias has a spread of 1, so that in every case, on the f64 reference (asserted, `_conditions`):
between 1/4 and 3/4 of the hidden units are active over the batch, the gates' standard deviation over channels is at least 0.1, no
gate is within 0.01 of 0 or 1, at least 1/4 of `out` is positive and at least 1/10 is clipped by the final ReLU.  A wrong `hid` or
`w2` index then moves gates by ~0.1 and the output by as much.  Inputs are drawn on the CPU, so the conditions can be checked
without a device; a case that misses them is reseeded (its `seed` column), never waived.

Bounds, per case, for `out` and for `gate`, switch on and off: with e_direct = max|baseline - ref| of the same block through the three
calls on the exact direct kernel (ops.attach_split(w, False), no Winograd planes) and scale = max(1, max|ref|),
    err <= FACTOR * e_direct + SLACK * scale    and    err <= 4e-5 * scale
(two layers at the 2e-5 per-layer ceiling of test_gpu_conv_f64.py::test_winograd_envelope).  test_gpu_conv_f64.py rule (d) holds one
layer to tall <= 8x direct and square split <= 3x tall split; FACTOR may not exceed their product, 24.  The baseline runs the SE
tail of se_tail.h as both paths do, so the relative bound cannot see an error there (reading hid[] in reverse in se_gate gives
err = e_direct = 0.85 .. 2.8); the ceiling does, and it is asserted on the baseline too.  Every case prints err, e_direct, their
ratio and its tags under -s.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
# Bounds, with what the first MI355X run of this module measured over all cases (switch on == switch off bit for bit, so one figure):
#   out:  err / e_direct 0.36 .. 3.05 (worst: w1, then c64-fit 1.86, h7-w3 1.79; C >= 256 0.36 .. 0.62); err / scale 1.9e-7 .. 6.6e-7
#   gate: err / e_direct 0.78 .. 1.73; err 7.1e-8 .. 3.2e-7
# FACTOR is twice the worst ratio (the ceiling for it is 24, the product of the per-layer rules); with it no case needs the slack.
FACTOR, SLACK = 6.0, 1e-7
CEILING = 4e-5

# name, N (None: the device's CU count + 3), H, W, Cin, C, stride, view of x, tags with the switch on, also with gate=None, seed
CASES = [
    ("h3-w7", 2, 3, 7, 64, 64, 1, "dense", ["chain", "se"], True, 2),            # H < 4: one partial tile row; W % 4 == 3
    ("h5-w6", 2, 5, 6, 128, 128, 1, "dense", ["chain", "se"], False, 1),         # H % 4 == 1, W % 4 == 2
    ("h6-w9-tail", 2, 6, 9, 128, 128, 1, "dense", ["chain", "se"], False, 0),    # H % 4 == 2: the tail column on a partial tile row
    ("h7-w3", 3, 7, 3, 64, 64, 1, "dense", ["chain", "se"], False, 2),           # H % 4 == 3, W < 4: one partial tile per tile row
    ("w1", 2, 4, 1, 64, 64, 1, "dense", ["chain", "se"], False, 0),              # W % 4 == 1 below the tail form's W >= 5: padded tile
    ("h1-w33-c1024", 2, 1, 33, 1024, 1024, 1, "dense", ["chain", "se"], False, 0),   # H == 1 with a tail column; 160 000 B
    ("c1024-fit", 2, 3, 11, 1024, 1024, 1, "dense", ["chain", "se"], False, 0),  # C = 1024 (PG = 4): 33 pixels, 160 000 B
    ("c512-fit", 2, 3, 23, 512, 512, 1, "dense", ["chain", "se"], False, 0),     # 69 pixels: 161 920 B of 163 840 B
    ("c512-over", 2, 5, 14, 512, 512, 1, "dense", [], True, 0),                  # 70 pixels: 163 968 B, the three calls
    ("c256-fit", 1, 3, 47, 256, 256, 1, "dense", ["chain", "se"], False, 0),     # 141 pixels: 162 880 B
    ("c128-fit", 1, 15, 19, 128, 128, 1, "dense", ["chain", "se"], False, 0),    # 285 pixels: 163 360 B
    ("c64-fit", 1, 3, 191, 64, 64, 1, "dense", ["chain", "se"], False, 1),       # 573 pixels: 163 600 B; 36 pixel rounds per virtual thread
    ("n-over-cus", None, 4, 5, 64, 64, 1, "dense", ["chain", "se"], False, 1),   # more workgroups than CUs
    ("cin128-c256", 2, 5, 7, 128, 256, 1, "dense", ["se"], True, 0),             # conv1 cannot chain; partial tiles
    ("stride2", 2, 10, 13, 128, 256, 2, "dense", ["se"], False, 0),              # strided conv1 onto 5 x 7
    ("x-channel-slice", 2, 4, 13, 128, 128, 1, "chan", ["chain", "se"], False, 0),   # x = buf[..., 32:32 + C], identity separate
    ("x-row-gap", 2, 5, 6, 64, 64, 1, "rowgap", ["chain", "se"], False, 0),      # x = buf[:, :, :W] of a [N, H, W + 3, C] buffer
]
SEED = 20261020


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


def _square_everywhere(ops, monkeypatch):
    """As test_gpu_se_block_fused.py: every 3x3 weight of at least 64 channels gets the square form's planes, and conv2d takes them on
    every map."""
    monkeypatch.setattr(ops, "WINOGRAD_MIN_CIN", 64)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE_MIN_CIN", 64)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 1)
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    monkeypatch.setattr(ops, "WINOGRAD_TALL", 1)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    monkeypatch.setattr(ops, "_tall_pays", lambda H_: True)
    monkeypatch.setattr(ops, "_square_pays", lambda W_: True)


def _fused_tags(tags):
    return [t[2] for t in tags if len(t) > 2]


def _lds_bytes(H, W, C):
    return 4 * (H * W * C + 4096 + 2 * C + C // 16)


def _inputs(case, N):
    """Seeded CPU f32 tensors of one block: the raw weights first (they do not depend on N), then the buffer x is a view of, x and
    the identity."""
    name, _, H, W, Cin, C, stride, view = case[:8]
    g = torch.Generator().manual_seed(SEED + 1000 * case[10] + sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g)
    conv1 = (rn(C, 3, 3, Cin) * (2.0 / (Cin * 9)) ** 0.5, rn(C) * 0.1)
    conv2 = (rn(C, 3, 3, C) * (2.0 / (C * 9)) ** 0.5, rn(C) * 1.0)    # a spread of biases: the channel means differ by more than the noise
    se = (rn(C // 16, C) * (1.0 / C) ** 0.5, rn(C, C // 16) * (1.2 / (C // 16)) ** 0.5)
    if view == "chan":
        buf = rn(N, H, W, Cin + 64)
        x = buf[..., 32:32 + Cin]
    elif view == "rowgap":
        buf = rn(N, H, W + 3, Cin)
        x = buf[:, :, :W]
    else:
        buf = x = rn(N, H, W, Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    idt = rn(N, Ho, Wo, C)
    return buf, x, idt, conv1, conv2, se


def _view_of(buf, case):
    """The view of `_inputs` on a copy of its buffer."""
    W, Cin, view = case[3], case[4], case[7]
    return buf[..., 32:32 + Cin] if view == "chan" else buf[:, :, :W] if view == "rowgap" else buf


def _block_ref64(x, idt, conv1, conv2, se, stride):
    """The block in float64 on the CPU from the raw weights: (out, gate, hid), NHWC / [N, C] / [N, C / 16]."""
    d = lambda t: t.detach().cpu().double()
    (w1, b1), (w2, b2), (s1, s2) = conv1, conv2, se
    a = F.relu(F.conv2d(d(x).permute(0, 3, 1, 2), d(w1).permute(0, 3, 1, 2), d(b1), stride=stride, padding=1))
    y = F.conv2d(a, d(w2).permute(0, 3, 1, 2), d(b2), padding=1)
    hid = F.relu(y.mean(dim=(2, 3)) @ d(s1).t())
    gate = torch.sigmoid(hid @ d(s2).t())
    out = F.relu(y * gate[:, :, None, None] + d(idt).permute(0, 3, 1, 2))
    return out.permute(0, 2, 3, 1).contiguous(), gate, hid


def _conditions(out, gate, hid):
    """The figures the inputs must meet, and whether they do."""
    active = (hid > 0).double().mean().item()
    gstd = gate.std(dim=1).min().item()
    gmin, gmax = gate.min().item(), gate.max().item()
    pos = (out > 0).double().mean().item()
    figures = dict(active=active, gate_std=gstd, gate_min=gmin, gate_max=gmax, positive=pos, clipped=1 - pos)
    ok = 0.25 <= active <= 0.75 and gstd >= 0.1 and gmin >= 0.01 and gmax <= 0.99 and pos >= 0.25 and 1 - pos >= 0.1
    return figures, ok


def _run(ops, fused, x, conv1, conv2, idt, se, stride, with_gate=True, profile=False):
    """(out, gates, wino_out tags, conv_gemm names) of ops.se_block with the switch set.  The gates go to rows 1 .. N of an
    [N + 2, C] buffer whose first and last rows must keep their sentinel."""
    N, C = x.shape[0], conv2[0].shape[0]
    gbuf = torch.full((N + 2, C), SENTINEL, device="cuda")
    gate = gbuf[1:N + 1] if with_gate else None
    old, ops.SE_BLOCK_FUSED = ops.SE_BLOCK_FUSED, int(fused)
    if profile:
        ops.PROFILE = []
    try:
        out = ops.se_block(x, conv1, conv2, idt, se, stride=(stride, stride), gate=gate)
    finally:
        recs, ops.PROFILE = ops.PROFILE, None
        ops.SE_BLOCK_FUSED = old
    torch.cuda.synchronize()
    assert torch.all(gbuf[0] == SENTINEL) and torch.all(gbuf[N + 1] == SENTINEL), "gates written outside rows 1 .. N"
    if with_gate:
        assert not torch.any(gate == SENTINEL)
    else:
        assert torch.all(gbuf == SENTINEL)
    if not profile:
        return out, gate, None, None
    return out, gate, _fused_tags([r[4] for r in recs if r[2] == "wino_out"]), [r[4][3] for r in recs if r[2] == "conv_gemm"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_se_block_against_f64(ops, case, monkeypatch):
    _square_everywhere(ops, monkeypatch)
    name, N, H, W, Cin, C, stride, view, want_tags, gate_none = case[:10]
    if N is None:
        N = torch.cuda.get_device_properties(0).multi_processor_count + 3
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert (_lds_bytes(Ho, Wo, C) <= 160 * 1024) == bool(want_tags), name
    buf, x, idt, conv1, conv2, se = _inputs(case, N)
    ref, ref_gate, hid = _block_ref64(x, idt, conv1, conv2, se, stride)
    figures, ok = _conditions(ref, ref_gate, hid)
    assert ok, (name, figures)

    dev = lambda t: t.cuda().contiguous()
    xd, idtd, sed = _view_of(dev(buf), case), dev(idt), (dev(se[0]), dev(se[1]))
    assert xd.shape == x.shape and xd.stride() == x.stride()
    wino = [(ops.attach_winograd(dev(w), True), dev(b)) for w, b in (conv1, conv2)]
    exact = [(ops.attach_split(dev(w), False), dev(b)) for w, b in (conv1, conv2)]
    assert all(getattr(w, "_msocr_wino44ct_split", None) is not None for w, _ in wino)
    assert not any(hasattr(w, a) for w, _ in exact for a in ("_msocr_wino", "_msocr_wino42_fused", "_msocr_split"))

    def errs(out, gate):
        return (out.cpu().double() - ref).abs().max().item(), (gate.cpu().double() - ref_gate).abs().max().item()

    base, base_gate, base_tags, base_gemms = _run(ops, False, xd, *exact, idtd, sed, stride, profile=True)
    assert base_tags == [] and base_gemms == ["direct", "direct"], (base_tags, base_gemms)
    e_direct = errs(base, base_gate)
    scale = (max(1.0, ref.abs().max().item()), 1.0)
    # the baseline shares se_tail.h with both paths: an error there is in e_direct too, and only the ceiling sees it
    assert e_direct[0] <= CEILING * scale[0] and e_direct[1] <= CEILING * scale[1], (name, "baseline", e_direct, scale)

    conv1_gemm = "winograd44_split" if stride == 1 else "direct_split"
    off, off_gate, off_tags, off_gemms = _run(ops, False, xd, *wino, idtd, sed, stride, profile=True)
    on, on_gate, on_tags, on_gemms = _run(ops, True, xd, *wino, idtd, sed, stride, profile=True)
    assert off_tags == [] and on_tags == want_tags, (name, off_tags, on_tags)
    assert off_gemms == on_gemms == [conv1_gemm, "winograd44_split"], (name, off_gemms, on_gemms)
    for sw, (out, gate) in (("off", (off, off_gate)), ("on", (on, on_gate))):
        e = errs(out, gate)
        for what, err, e_d, sc in zip(("out", "gate"), e, e_direct, scale):
            print(f"{name} N={N} {Ho}x{Wo}x{C} lds {_lds_bytes(Ho, Wo, C)} tags {on_tags} switch {sw} {what}: err {err:.3e} = "
                  f"{err / sc:.2e} of scale, e_direct {e_d:.3e}, ratio {err / max(e_d, 1e-300):.2f}")
            assert err <= FACTOR * e_d + SLACK * sc, (name, sw, what, err, e_d, sc)
            assert err <= CEILING * sc, (name, sw, what, err, sc)
    assert torch.equal(on, off) and torch.equal(on_gate, off_gate), name
    plain, plain_gate, _, _ = _run(ops, True, xd, *wino, idtd, sed, stride)
    assert torch.equal(plain, on) and torch.equal(plain_gate, on_gate), name
    if gate_none:
        for fused in (True, False):
            nog, _, _, _ = _run(ops, fused, xd, *wino, idtd, sed, stride, with_gate=False)
            assert torch.equal(nog, on), (name, fused)


def _trba_maps(h, w):
    """Canvas h x w -> the map of layer3 / layer4 (TrbaNet.cnn: conv0b's 2x2 pool, then the strides of LAYER_SPEC on 3x3 / pad 1)."""
    from manuscript_ocr_amd.recognizers._trba.net import LAYER_SPEC
    hh, ww = h // 2, w // 2
    for lname, _, stride in LAYER_SPEC:
        hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
        if lname == "layer3":
            h3, w3 = hh, ww
    assert (hh, ww) == (h3, w3)   # layer4 keeps layer3's map
    return h3, w3, (h3 - 2) // 2   # and the height behind conv_out's two 2x2 convolutions, the first with stride 2 along H


def test_trba_cnn_features_bit_identical_on_an_odd_map(ops):
    """TrbaNet.cnn with the library's own dispatch on the smallest canvas whose layer3 / layer4 map has a partial tile and still takes
    the square form: 26 x 18 -> 13 x 9 -> 7 x 5 -> 4 x 3 (W % 4 == 3, one partial tile; a map of fewer than 4 rows leaves nothing behind
    conv_out).  The kernels run on every block of the two layers and the features do not change."""
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers._trba.net import LAYER_SPEC, TrbaNet
    h, w = 26, 18
    H3, W3, Hf = _trba_maps(h, w)
    assert (H3, W3, Hf) == (4, 3, 1) and (H3 % 4 != 0 or W3 % 4 in (2, 3))
    assert ops._tall_pays(H3) and ops._square_pays(W3) and _lds_bytes(H3, W3, 512) <= 160 * 1024
    for a, b in ((a, b) for a in range(1, h + 1) for b in range(1, w + 1) if (a, b) != (h, w)):
        A3, B3, Af = _trba_maps(a, b)   # no canvas inside this one has such a map on which the library's dispatch takes the square form
        assert not (Af >= 1 and ops._tall_pays(A3) and ops._square_pays(B3) and (A3 % 4 != 0 or B3 % 4 in (2, 3))), (a, b)
    # the tags LAYER_SPEC gives: the square planes are on the Cin = 512 layers, so layer3 / layer4; a layer's first block chains only
    # where it neither strides nor changes the channel count
    want, cin = [], 128
    for (lname, blocks, stride), planes in zip(LAYER_SPEC, (256, 256, 512, 512)):
        for i in range(blocks):
            if planes >= ops.WINOGRAD_SQUARE_MIN_CIN:
                want += ["chain", "se"] if (i > 0 or stride == 1) and cin == planes else ["se"]
            cin = planes
    assert want == ["se"] + ["chain", "se"] * 7
    net = TrbaNet(synth.trba_state_dict(194, 256, seed=20260128), 194, 256, torch.float32)
    cd = torch.from_numpy(synth.synth_crops(37, 3, h, w)).cuda()
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
        assert tags == (want if fused else []), tags
    assert feats[0].shape == (3, 1, W3, 512) and torch.isfinite(feats[0]).all() and (feats[0] > 0).any()
    assert torch.equal(feats[0], feats[1])
