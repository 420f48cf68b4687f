"""precision="fp32" (the default) of both networks held to float64 layer by layer, at the smallest shapes that cross every switch of the
f32 dispatch.  tests/f32_replay.py holds the recorder, the recogniser's f32 graph and the replay; the bf16 mode's twin is
tests/test_gpu_bf16_networks.py.

In this mode ops.conv2d and ops.se_block route every layer by its map and channel counts: F(2x2,3x3), the tall or the square Winograd
form (with or without the tail column), the fused Cin = 64 kernel with or without its pool, split or exact operands, the per-crop SE
kernels or the three calls.  tests/test_gpu_f64.py holds the networks to float64 end to end at shapes where EAST is all tall and the
recogniser all square + tail column; a wiring error at any other routing (a wrong bias or flag on one stage, the wrong slice of cat1..3
or yx, a residual leading dimension, a layer falling to another form) passed.  Here every `ops.*` call of the real network is recorded
(with ops.PROFILE on, which names the kernel family of every launch), and

(1) the recorded calls must be exactly the graph written down from net.py and the reference architecture, in order; every input a call
    read must be, bit for bit, the recorded output of the call the graph names; weights, biases and SE weights by identity;
(2) every call's output is held to a float64 reference computed from the DEVICE's recorded inputs (teacher-forced: errors do not
    accumulate), with the bounds of the modules that own the kernels, imported: normalize_u8 and maxpool2d bit for bit; direct
    convolutions (stems, 1x1, strided 3x3, out0 / out1, the encoder's GEMMs) per element gamma_K A (rules (a) / (b) of
    test_gpu_conv_f64.py); Winograd layers max err <= 2e-5 scale and <= F e_direct + 1e-6 scale, e_direct the same call through the
    exact direct kernel on the device and F rule (d)'s factors multiplied up to the form taken (f32_replay.WINO_FACTOR); se_block calls
    FACTOR / SLACK / CEILING of test_gpu_se_block_f64.py against the three calls on the exact direct kernel; upsample2x_into and east_head
    the f32 bounds of test_gpu_stream_f64.py; se_residual, its gates and mean_over_h those of test_gpu_seq_f64.py part (f) (the gates lie
    in (0, 1), so SE_F32_RTOL of max(1, max|ref|) is 5e-7 for them); the recurrences part (e)'s reference and 2e-5;
(3) the form every layer took and the shape every SE block took must be what ROUTING states for the case, and ROUTING is held to
    ops._tall_pays / _square_pays / _coltail without a GPU (`derive_*` mirror ops._wino_form and ops.se_block), so a case can neither
    pass vacuously nor drift when a default changes; over the cases every form and every block shape occurs;
(4) the network is run twice per case, recorded (ops.PROFILE on: the staged entry points) and plain: the final outputs are torch.equal
    (asserted last, so that a layer that fails is named first);
(5) the f64 references must not be degenerate (constants of the bf16 module): the same three conditions are asserted without a GPU on
    the oracle networks in float64 at every case's shape;
(6) end to end (score, geometry, features, batch_H against the oracle in f64, beside the oracle's own f32) is printed, not asserted:
    the recogniser already sits at 1.79 .. 1.91 of the allowed 2.0 at its one tested shape (ops.py, above WINOGRAD_SQUARE).

Which heights take F(2x2): ops._tall_pays(H) is 24 ceil(H / 4) < 16 ceil(H / 2), false exactly for H in {1, 2, 5, 6} (H = 3, 9, 10, 13 and
14 do pay: 24 < 32, 72 < 80, 96 < 112), so of the pages here 160 rows put layer4 / dec1.b (5 rows) and 96 rows layer3 / dec2.b (6 rows)
on F(2x2); 224 x 64 is all tall (7, 14, 28, 56 rows) and stays as the W / 32 = 2 case.

First MI355X run: DESIGN.md section 5.1 has every figure."""
import copy

import numpy as np
import pytest
import torch

import f32_replay as fr
import test_gpu_bf16_networks as tb
import test_gpu_se_block_f64 as sb
from manuscript_ocr_amd import synth
from test_gpu_f64 import _report

gpu = pytest.mark.gpu
POSITIVE_MIN, SCORE_STD_MIN, GATE_STD_MIN = tb.POSITIVE_MIN, tb.SCORE_STD_MIN, tb.GATE_STD_MIN
EAST_SEED, TRBA_SEED, PAGE_SEED, CROP_SEED = 20260128, 5, 31, 14

# name, H, W, pages, mode ("default", "square": net.EAST_WINO_SQUARE on, "exact": EastNet(sd, split=False))
EAST_CASES = [("128x96x2", 128, 96, 2, "default"), ("160x128", 160, 128, 1, "default"), ("96x160", 96, 160, 1, "default"),
              ("224x64", 224, 64, 1, "default"), ("128x160-square", 128, 160, 1, "square"), ("128x96x2-exact", 128, 96, 2, "exact")]
# canvas (h, w), three crops each
TRBA_CASES = [("32x100", 32, 100), ("32x128", 32, 128), ("32x36", 32, 36), ("32x44", 32, 44), ("48x100", 48, 100)]
CROPS = 3

# The form every group of Winograd layers must take.  EAST: layerK = the 3x3 / 1 convolutions of the trunk's layer K (map H / 4 .. H / 32),
# decK.b the decoder's (H / 32 .. H / 4); layer1 and dec4.b have Cin = 64 (the fused kernel; dec4.b's 32 output channels keep it exact).
_ALL_TALL = {"layer1": "fused_split", "layer2": "tall_split", "layer3": "tall_split", "layer4": "tall_split",
             "dec1.b": "tall_split", "dec2.b": "tall_split", "dec3.b": "tall_split", "dec4.b": "fused"}
EAST_ROUTING = {
    "128x96x2": _ALL_TALL,                                                               # maps of 4 / 8 / 16 / 32 rows; W / 32 = 3
    "160x128": dict(_ALL_TALL, **{"layer4": "f2x2", "dec1.b": "f2x2"}),                 # 5 rows at 512 channels
    "96x160": dict(_ALL_TALL, **{"layer3": "f2x2", "dec2.b": "f2x2"}),                  # 6 rows at 256 channels; 3 and 12 rows are tall
    "224x64": _ALL_TALL,                                                                 # 7 / 14 / 28 / 56 rows; W / 32 = 2
    "128x160-square": dict(_ALL_TALL, **{"layer4": "square+tail", "dec1.b": "square+tail"}),   # 4 x 5 at Cin = 512
    "128x96x2-exact": {"layer1": "fused", "layer2": "tall", "layer3": "tall", "layer4": "tall",
                       "dec1.b": "tall", "dec2.b": "tall", "dec3.b": "tall", "dec4.b": "fused"},
}
# TRBA: conv0b (Cin = 64 -> 128 with the pool), c256 = the blocks of layer1 / layer2, layer3.0 (strided, widening conv1: direct), c512 = the
# other blocks of layer3 / layer4.  (form of the block's 3x3 / 1 convolutions, leaf shape of the block)
TRBA_ROUTING = {
    "32x100": {"conv0b": ("fused_split", "pool2"), "c256": ("tall_split", "three"), "layer3.0": ("square+tail", "se"), "c512": ("square+tail", "chain")},
    "32x128": {"conv0b": ("fused_split", "pool2"), "c256": ("tall_split", "three"), "layer3.0": ("square", "se"), "c512": ("square", "chain")},
    "32x36": {"conv0b": ("fused_split", "pool2"), "c256": ("tall_split", "three"), "layer3.0": ("square+tail", "se"), "c512": ("square+tail", "chain")},
    "32x44": {"conv0b": ("fused_split", "pool2"), "c256": ("tall_split", "three"), "layer3.0": ("tall_split", "three"), "c512": ("tall_split", "three")},
    "48x100": {"conv0b": ("fused_split", "pool2"), "c256": ("tall_split", "three"), "layer3.0": ("f2x2", "three"), "c512": ("f2x2", "three")},
}
ALL_FORMS = {"f2x2", "tall_split", "tall", "square", "square+tail", "fused_split", "fused"}
ALL_SHAPES = {"three", "se", "chain"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ================================================================================================ the tables against the host predicates
def derive_form(ops, Cin, Cout, H, W, split, square):
    """The form ops.conv2d gives a 3x3 / 1 / 1 convolution on H x W maps (the fused test of conv2d, then ops._wino_form): split = the
    network carries split planes, square = its 3x3 weights were given the square form's planes where Cin allows."""
    if Cin == 64:
        assert ops.WINOGRAD_FUSED64 and ops.WINOGRAD_TALL and ops._tall_pays(H), "a Cin = 64 layer off the fused kernel runs direct"
        return "fused_split" if split and (Cout % 64 == 0 or Cout >= 128) else "fused"
    assert Cin >= ops.WINOGRAD_MIN_CIN and Cin % 32 == 0 and Cout % 64 == 0
    if not (ops.WINOGRAD_TALL and ops._tall_pays(H)):
        return "f2x2"
    if not (split and ops.SPLIT_BF16X3):
        return "tall"
    if square and ops.WINOGRAD_SQUARE and Cin >= ops.WINOGRAD_SQUARE_MIN_CIN and ops._square_pays(W):
        return "square+tail" if ops._coltail(W) else "square"
    return "tall_split"


def derive_east(ops, H, W, mode):
    split, square = mode != "exact", mode == "square"
    r = {}
    for group, div, Cin, Cout in (("layer1", 4, 64, 64), ("layer2", 8, 128, 128), ("layer3", 16, 256, 256), ("layer4", 32, 512, 512),
                                  ("dec1.b", 32, 512, 512), ("dec2.b", 16, 256, 256), ("dec3.b", 8, 128, 128), ("dec4.b", 4, 64, 32)):
        r[group] = derive_form(ops, Cin, Cout, H // div, W // div, split, square)
    return r


def trba_maps(h, w):
    """Canvas -> (the map of layer1 / layer2, the map of layer3 / layer4): conv0b's pool, then 3x3 / pad 1 with stride 2."""
    h1, w1 = (h // 2 - 1) // 2 + 1, (w // 2 - 1) // 2 + 1
    return (h1, w1), ((h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1)


def derive_trba(ops, h, w):
    assert h % 2 == 0 and w % 2 == 0 and ops._tall_pays(h)   # conv2d(pool2=True) stays one call
    (h1, w1), (h3, w3) = trba_maps(h, w)

    def block(C, H, W, chains):
        form = derive_form(ops, C, C, H, W, True, True)
        fits = ops.SE_BLOCK_FUSED and form in ("square", "square+tail") and sb._lds_bytes(H, W, C) <= 160 * 1024
        return form, ("chain" if chains else "se") if fits else "three"

    return {"conv0b": (derive_form(ops, 64, 128, h, w, True, True), "pool2"), "c256": block(256, h1, w1, True),
            "layer3.0": block(512, h3, w3, False), "c512": block(512, h3, w3, True)}


def test_case_tables_follow_the_host_predicates():
    """ROUTING is what ops._tall_pays / _square_pays / _coltail give at the cases' maps, and over the cases every Winograd form, both
    se_block leaf shapes and the three-call shape occur (in the manner of test_envelope_reaches_all_16_instances)."""
    from manuscript_ocr_amd import ops
    assert [H for H in range(1, 17) if not ops._tall_pays(H)] == [1, 2, 5, 6]
    for name, H, W, pages, mode in EAST_CASES:
        assert EAST_ROUTING[name] == derive_east(ops, H, W, mode), (name, derive_east(ops, H, W, mode))
    for name, h, w in TRBA_CASES:
        assert TRBA_ROUTING[name] == derive_trba(ops, h, w), (name, derive_trba(ops, h, w))
    assert trba_maps(32, 100) == ((8, 25), (4, 13)) and trba_maps(32, 36)[1] == (4, 5) and trba_maps(48, 100) == ((12, 25), (6, 13))
    assert trba_maps(32, 128)[1] == (4, 16) and trba_maps(32, 44)[1] == (4, 6)
    assert not ops._square_pays(6) and not ops._tall_pays(6) and ops._coltail(5) and not ops._coltail(16)
    assert all((H // 32) * (W // 32) and H // 4 <= 56 and W // 4 <= 40 for _, H, W, _, _ in EAST_CASES)
    forms = {f for r in EAST_ROUTING.values() for f in r.values()} | {f for r in TRBA_ROUTING.values() for f, _ in r.values()}
    shapes = {s for r in TRBA_ROUTING.values() for k, (_, s) in r.items() if k != "conv0b"}
    assert forms == ALL_FORMS, sorted(forms ^ ALL_FORMS)
    assert shapes == ALL_SHAPES, sorted(shapes ^ ALL_SHAPES)


# ================================================================================================ inputs, networks (cached)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _east_sd():
    return _cached(("east-sd", EAST_SEED), lambda: synth.east_state_dict(seed=EAST_SEED))


def _trba_sd():
    return _cached(("trba-sd", TRBA_SEED), lambda: synth.trba_state_dict(194, 256, TRBA_SEED))


def _east_pages(H, W, pages):
    return np.stack([synth.synth_page(PAGE_SEED + k, H, W)[0] for k in range(pages)])


def _east_x(pg):
    from oracle import imgproc
    return torch.from_numpy(np.concatenate([imgproc.east_preprocess(p, p.shape[1], p.shape[0]) for p in pg]))


def _trba_crops(h, w):
    return synth.synth_crops(CROP_SEED, CROPS, h, w)


def _oracle_east():
    def make():
        from oracle import east_model as oem
        net32 = oem.EASTNet()
        net32.load_state_dict(_east_sd())
        net32.eval()
        return net32, copy.deepcopy(net32).double()
    return _cached(("east-oracle", EAST_SEED), make)


def _oracle_trba():
    def make():
        from oracle import trba_model as otm
        net32 = otm.TRBANet(194, 256)
        net32.load_state_dict(_trba_sd(), strict=True)
        net32.eval()
        return net32, copy.deepcopy(net32).double()
    return _cached(("trba-oracle", TRBA_SEED), make)


def _east_net(mode, monkeypatch):
    def make():
        from manuscript_ocr_amd.detectors._east import net as east_net
        if mode == "square":
            monkeypatch.setattr(east_net, "EAST_WINO_SQUARE", True)
        n = east_net.EastNet(_east_sd(), torch.float32, split=False if mode == "exact" else None)
        for k in ("layer4.1.conv2", "layer4.2.conv2", "dec1.b"):
            assert (getattr(n.P[k][0], "_msocr_wino44ct_split", None) is not None) == (mode == "square"), (mode, k)
        return n
    return _cached(("east-net", EAST_SEED, mode), make)


def _trba_net():
    def make():
        from manuscript_ocr_amd.recognizers._trba.net import TrbaNet
        n = TrbaNet(_trba_sd(), 194, 256, torch.float32)
        assert n.cpad == 4 and n.cin_pad == 16
        return n
    return _cached(("trba-net", TRBA_SEED), make)


# ================================================================================================ the oracle networks are usable inputs
def _hook_stats(net, relu_modules, gate_modules, positive_of=()):
    """Forward hooks: the positive share of every ReLU output (and of relu(output) of `positive_of`), the standard deviation of every gate."""
    pos, gates, handles = [], [], []
    for m in relu_modules:
        handles.append(m.register_forward_hook(lambda mod, i, o: pos.append(float((o > 0).double().mean()))))
    for m in positive_of:
        handles.append(m.register_forward_hook(lambda mod, i, o: pos.append(float((o > 0).double().mean()))))
    for m in gate_modules:
        handles.append(m.register_forward_hook(lambda mod, i, o: gates.append(float(o.std()))))
    return pos, gates, handles


_EAST_SHAPES = [c for c in EAST_CASES if c[4] != "exact"]   # the exact case has the first case's shape and pages


@pytest.mark.parametrize("name,H,W,pages,mode", _EAST_SHAPES, ids=[c[0] for c in _EAST_SHAPES])
def test_oracle_east_in_f64_is_not_degenerate_at_the_case_shape(name, H, W, pages, mode):
    _, net64 = _oracle_east()
    pos, _, handles = _hook_stats(net64, [m for m in net64.modules() if isinstance(m, torch.nn.ReLU)], [])
    try:
        with torch.no_grad():
            r = net64(_east_x(_east_pages(H, W, pages)).double())
    finally:
        for h in handles:
            h.remove()
    std = float(r["score"].std())
    print(f"[f32-oracle] EAST {name}: {len(pos)} ReLU outputs, smallest positive share {min(pos):.2f}, score std {std:.3f}")
    assert len(pos) == 57 and min(pos) >= POSITIVE_MIN, (name, "degenerate case: reseed it", min(pos))
    assert std > SCORE_STD_MIN, (name, "degenerate score map: reseed the case", std)


@pytest.mark.parametrize("name,h,w", TRBA_CASES, ids=[c[0] for c in TRBA_CASES])
def test_oracle_trba_in_f64_is_not_degenerate_at_the_case_shape(name, h, w):
    from oracle import trba_model as otm
    _, net64 = _oracle_trba()
    cnn = net64.cnn
    blocks = [m for m in cnn.modules() if isinstance(m, otm.SEBasicBlock)]
    relus = [m for m in list(cnn.conv0) + list(cnn.conv_out) if isinstance(m, torch.nn.ReLU)] + blocks   # a block's output is behind its ReLU
    pos, gates, handles = _hook_stats(net64, relus, [b.se.fc for b in blocks], positive_of=[b.bn1 for b in blocks])
    try:
        with torch.no_grad():
            hb = net64.encode(tb._x_trba(_trba_crops(h, w)).double())
    finally:
        for hd in handles:
            hd.remove()
    print(f"[f32-oracle] TRBA {name}: {len(pos)} ReLU outputs, smallest positive share {min(pos):.2f}, gate std {min(gates):.3f} .. {max(gates):.3f}, "
          f"batch_H {tuple(hb.shape)}")
    assert len(pos) == 26 and min(pos) >= POSITIVE_MIN, (name, "degenerate case: reseed it", min(pos))
    assert len(gates) == 11 and min(gates) >= GATE_STD_MIN, (name, "degenerate case: SE gates that hardly vary, reseed it", min(gates))


# ================================================================================================ layer-by-layer replay
def _record(monkeypatch, ops, table, run):
    """run() twice: recorded with ops.PROFILE on (the staged entry points), then plain.  -> (recorder, recorded result, plain result)."""
    rec = fr.Recorder(monkeypatch, ops, table)
    monkeypatch.setattr(ops, "PROFILE", [])
    a = run()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert ops.PROFILE is None
    b = run()
    torch.cuda.synchronize()
    return rec, a, b


def _want_direct(ops, w, split):
    return "direct_split" if split and ops.SPLIT_BF16X3 and ops._split_eligible(w) else "direct"


def _summary(what, graph, ratios):
    by = {}
    for n in graph:
        kind = {"conv": "conv", "gemm": "gemm", "stem": "stem"}.get(n.op, n.op)
        for k, v in ratios.items():
            if k == n.name or k.startswith(n.name + ":"):
                by.setdefault(kind + k[len(n.name):], []).append(v)
    print(f"[f32-replay] {what}: worst error / bound " + ", ".join(f"{k} {max(v):.3f}" for k, v in by.items()))


def _east_group(name):
    """The ROUTING group of a node of east_graph: the decoder's 3x3s and the trunk's 3x3 / 1s (a layer's first block strides, but layer1's)."""
    parts = name.split(".")
    if parts[0].startswith("dec"):
        return name if parts[1] == "b" else None
    if parts[-1] == "conv2" and (parts[0] == "layer1" or parts[1] != "0"):
        return parts[0]
    return None


@gpu
@pytest.mark.parametrize("name,H,W,pages,mode", EAST_CASES, ids=[c[0] for c in EAST_CASES])
def test_east_f32_layer_by_layer_replay(monkeypatch, name, H, W, pages, mode):
    _need_gpu()
    from manuscript_ocr_amd import ops
    net = _east_net(mode, monkeypatch)
    pg = _east_pages(H, W, pages)
    dev_pages = torch.from_numpy(pg).cuda()
    rec, (score, geo), (score_p, geo_p) = _record(monkeypatch, ops, net.P, lambda: net.forward(dev_pages))
    assert all(r.depth == 0 for r in rec.records), "EAST's forward nests no recorded call"
    graph = fr.east_graph()
    fails, ratios, stats, forms, _ = fr.replay(graph, rec.leaves(), net.P, ops, head=(net.w9, net.b9), tag=f"f32-replay EAST {name}")
    head = rec.leaves()[-1]
    assert torch.equal(head.output[0], score.cpu()) and torch.equal(head.output[1], geo.cpu())
    # routing: every Winograd group in the form the table states, every other convolution on the direct kernel its weight is eligible for
    routing, wrong = EAST_ROUTING[name], []
    for n in graph:
        if n.op not in ("conv", "stem"):
            continue
        group = _east_group(n.name)
        want = routing[group] if group else _want_direct(ops, net.P[n.name][0], mode != "exact")
        if forms.get(n.name) != want:
            wrong.append(f"{n.name}: ran as {forms.get(n.name)}, the table has {want}")
    _summary(f"EAST {name}", graph, ratios)
    # end to end, printed: the figures of test_gpu_f64._report
    net32, net64 = _oracle_east()
    x = _east_x(pg)
    with torch.no_grad():
        r32, r64 = net32(x), net64(x.double())
    _report(f"[f32-e2e] EAST {name} score", score.cpu().numpy(), r32["score"][:, 0].numpy(), r64["score"][:, 0].numpy())
    _report(f"[f32-e2e] EAST {name} geometry", geo.cpu().numpy(), r32["geometry"].permute(0, 2, 3, 1).numpy(), r64["geometry"].permute(0, 2, 3, 1).numpy())
    print(f"[f32-replay] EAST {name}: worst error / bound over {len(ratios)} checks {max(ratios.values()):.3f}; smallest positive share "
          f"{min(stats.positive.values()):.2f}, score std {stats.score_std:.3f}")
    assert not wrong, f"EAST {name}: {len(wrong)} layers off the routing table; the first in network order: " + "\n  ".join(wrong[:6])
    assert stats.score_std > SCORE_STD_MIN, (name, "degenerate score map — reseed the case", stats.score_std)
    tb._assert_replay(f"EAST {name}", fails, stats, relu_outputs=57, se_blocks=0)
    assert torch.equal(score, score_p) and torch.equal(geo, geo_p), (name, "recorded (staged) and plain runs differ")


def _trba_block_group(p):
    return "layer3.0" if p == "layer3.0" else "c256" if p.startswith(("layer1", "layer2")) else "c512"


@gpu
@pytest.mark.parametrize("name,h,w", TRBA_CASES, ids=[c[0] for c in TRBA_CASES])
def test_trba_f32_layer_by_layer_replay(monkeypatch, name, h, w):
    _need_gpu()
    from manuscript_ocr_amd import ops
    net = _trba_net()
    canv = _trba_crops(h, w)
    cd = torch.from_numpy(canv).cuda()
    table = {**net.P, **fr.encoder_table(net)}
    rec, (bh, proj), (bh_p, proj_p) = _record(monkeypatch, ops, table, lambda: net.encode(cd))
    routing = TRBA_ROUTING[name]
    blocks = [f"{l}.{i}" for l, _, n, _ in fr.TRBA_LAYERS for i in range(n)]
    graph = fr.trba_graph({p: routing[_trba_block_group(p)][1] for p in blocks}, conv0b_fused=routing["conv0b"][1] == "pool2")
    leaves = rec.leaves()
    fails, ratios, stats, forms, shapes = fr.replay(graph, leaves, table, ops, rnn=net.rnn, tag=f"f32-replay TRBA {name}")
    assert torch.equal(leaves[-1].output.reshape(bh.shape[0], bh.shape[1], -1), proj.cpu()) and torch.equal(leaves[-2].output.reshape(bh.shape), bh.cpu())
    _, (h3, w3) = trba_maps(h, w)
    mean = next(r for r in leaves if r.label == "mean_over_h")
    assert tuple(bh.shape) == (CROPS, w3, 256) and mean.inputs["x"].shape[1] == (h3 - 2) // 2, (tuple(bh.shape), tuple(mean.inputs["x"].shape))
    wrong = []
    for n in graph:
        if n.op in ("stem", "gemm") or n.name in ("out0", "out1") or n.name.endswith(".down"):
            want = _want_direct(ops, table[n.name][0], True)
        elif n.name == "conv0b":
            want = routing["conv0b"][0]
        elif n.op == "conv":   # conv1 / conv2 of a block: conv1 of a strided block is a direct convolution
            p = n.name.rsplit(".", 1)[0]
            strided = n.name.endswith(".conv1") and tuple(n.stride) != (1, 1)
            want = _want_direct(ops, table[n.name][0], True) if strided else routing[_trba_block_group(p)][0]
        else:
            continue
        if forms.get(n.name) != want:
            wrong.append(f"{n.name}: ran as {forms.get(n.name)}, the table has {want}")
    for p in blocks:
        form, shape = routing[_trba_block_group(p)]
        if shapes.get(p) != shape:
            wrong.append(f"{p}: the block ran as {shapes.get(p)}, the table has {shape}")
        if shape != "three":
            got = [forms[k] for k in (p + ".conv1", p + ".conv2") if k in forms and not (shape == "se" and k.endswith("conv1"))]
            if got != [form] * (2 if shape == "chain" else 1):
                wrong.append(f"{p}: se_block's GEMMs ran as {got}, the table has {form}")
    _summary(f"TRBA {name}", graph, ratios)
    # end to end, printed
    net32, net64 = _oracle_trba()
    x = tb._x_trba(canv)
    with torch.no_grad():
        f32_, f64_ = net32.cnn(x).permute(0, 2, 3, 1).numpy(), net64.cnn(x.double()).permute(0, 2, 3, 1).numpy()
        h32, h64 = net32.encode(x).numpy(), net64.encode(x.double()).numpy()
    f_dev = next(r for r in leaves if r.label == "conv2d:out1").output.numpy()
    _report(f"[f32-e2e] TRBA {name} features", f_dev, f32_, f64_)
    _report(f"[f32-e2e] TRBA {name} batch_H", bh.cpu().numpy(), h32, h64)
    print(f"[f32-replay] TRBA {name}: worst error / bound over {len(ratios)} checks {max(ratios.values()):.3f}; smallest positive share "
          f"{min(stats.positive.values()):.2f}, gate std {min(stats.gate_std.values()):.3f} .. {max(stats.gate_std.values()):.3f}")
    assert not wrong, f"TRBA {name}: {len(wrong)} layers off the routing table; the first in network order: " + "\n  ".join(wrong[:6])
    tb._assert_replay(f"TRBA {name}", fails, stats, relu_outputs=26, se_blocks=11)
    assert torch.equal(bh, bh_p) and torch.equal(proj, proj_p), (name, "recorded (staged) and plain runs differ")
