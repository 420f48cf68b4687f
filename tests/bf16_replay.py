"""Test-side tools of tests/test_gpu_bf16_networks.py: a recorder of the ops.* calls a network makes, the two networks written down as
graphs from their reference definitions (torchvision Bottleneck, the feature-merging decoder, the SE basic block; oracle/east_model.py and
oracle/trba_model.py), the float64 reference of every graph node computed from the DEVICE's recorded outputs of the nodes that feed it,
a float64 BatchNorm fold of the raw state dicts, and a bf16-storage emulation of the oracle networks on the CPU.  Nothing here runs
a kernel; nothing of the package changes for it."""
import inspect
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import test_gpu_conv_f64 as cf
import test_gpu_seq_f64 as sq
import test_gpu_stream_f64 as st

BN_EPS = 1e-5
U32 = 2.0 ** -24
RECORDED_OPS = ("normalize_u8", "conv2d", "maxpool2d", "upsample2x_into", "east_head", "se_block", "se_residual", "mean_over_h")
_OUTPUT_ARGS = {"conv2d": ("out",), "maxpool2d": ("out",), "upsample2x_into": ("out",), "east_head": ("score", "geo"),
                "se_residual": ("out", "gate")}
_BY_IDENTITY = {"conv2d": ("w", "bias"), "east_head": ("w9", "b9"), "se_residual": ("w1", "w2")}  # kept as objects, not cloned


# ================================================================================================ recorder
def _values(t):
    """The values of a tensor or view as the kernel saw them, on the CPU (a copy, never a view of device memory that changes later)."""
    return t.detach().clone().cpu()


class Recorder:
    """monkeypatch.setattr on the ops.* functions of RECORDED_OPS: every wrapper calls the original, synchronises and stores a record
    (op, label, keyword arguments, input values, output values, the output's storage pointer / shape / strides, nesting depth).
    net.py calls them as ops.<name>, and ops.se_block / conv2d(pool2=True) resolve conv2d, maxpool2d and se_residual through the module's
    globals, so the inner calls are caught too; `leaves()` are the calls that launched a kernel themselves."""

    def __init__(self, monkeypatch, ops, P):
        self.records, self.depth = [], 0
        self.weights = {id(v[0]): k for k, v in P.items()}
        assert len(self.weights) == len(P)
        for name in RECORDED_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, orig):
        sig = inspect.signature(orig)

        def wrapper(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            args = ba.arguments
            if name == "se_residual" and args["gate"] is None:  # the gates are scratch otherwise: have them written where we can read them
                x = args["x"]
                args["gate"] = torch.empty((x.shape[0], x.shape[3]), dtype=torch.float32, device=x.device)
            rec = SimpleNamespace(op=name, label=name, depth=self.depth, leaf=True, inputs={}, objects={}, kwargs={}, extra={})
            for k, v in args.items():
                if isinstance(v, torch.Tensor):
                    if k in _BY_IDENTITY.get(name, ()):
                        rec.objects[k] = v
                    elif k not in _OUTPUT_ARGS.get(name, ()):
                        rec.inputs[k] = _values(v)
                elif not (isinstance(v, tuple) and any(isinstance(e, (tuple, torch.Tensor)) for e in v)):
                    rec.kwargs[k] = v
            if name == "conv2d":
                key = self.weights.get(id(args["w"]))
                assert key is not None, f"conv2d call {len(self.records)} with a weight {tuple(args['w'].shape)} that is in no table of the network"
                rec.label = f"conv2d:{key}"
                rec.key = key
            self.records.append(rec)
            n = len(self.records)
            self.depth += 1
            try:
                out = orig(*ba.args, **ba.kwargs)
            finally:
                self.depth -= 1
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            rec.leaf = len(self.records) == n
            res = out
            if name == "upsample2x_into":
                res = out[..., : args["x"].shape[3]]
            if name == "se_residual":
                rec.extra["gate"] = _values(args["gate"])
            outs = res if isinstance(res, tuple) else (res,)
            rec.output = tuple(_values(t) for t in outs) if isinstance(res, tuple) else _values(res)
            rec.ptr, rec.shape, rec.strides = outs[0].data_ptr(), tuple(outs[0].shape), tuple(outs[0].stride())
            return out

        return wrapper

    def leaves(self):
        return [r for r in self.records if r.leaf]


# ================================================================================================ the networks as graphs
def _node(name, op, src=(), **kw):
    label = f"conv2d:{name}" if op in ("conv", "stem") else {"normalize": "normalize_u8", "maxpool": "maxpool2d", "upsample": "upsample2x_into",
                                                            "head": "east_head", "se": "se_residual", "mean_h": "mean_over_h"}[op]
    return SimpleNamespace(name=name, op=op, src=tuple(src), label=label, **kw)


def _conv(name, src, stride=(1, 1), pad=(0, 0), relu=False, res=None):
    return _node(name, "conv", src, stride=stride, pad=pad, relu=relu, res=res)


def east_graph():
    """ResNet-50 trunk (torchvision Bottleneck v1.5: 1x1, 3x3 with the block's stride, 1x1, out = relu(bn3(conv3(o2)) + identity),
    identity = downsample(x) in the first block of a layer), the feature-merging decoder (cat([upsample(h), f]) -> 1x1 -> 3x3, both with
    ReLU) and the output head, in the order of the reference forward.  Two things are the device's and stated by the issue: the first
    block of layer1 is ONE launch relu(W3 o2 + Wd x + b3 + bd) over the sources [o2, x] (`conv3d`), and a block's identity is an
    operand of the launch that adds it, so a `down` comes before the conv3 that consumes it."""
    g = [_node("image", "normalize", mode=0, pad=(3, 3), extra=(3, 3), cpad=4),
         _node("stem", "stem", ["image"], k=(7, 7), stride=(2, 2), pad=(3, 3), relu=True, cin_pad=32),
         _node("pool", "maxpool", ["stem"], k=3, s=2, p=1)]
    x, taps = "pool", {}
    for lname, blocks, stride in (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2), ("layer4", 3, 2)):
        for i in range(blocks):
            p, s = f"{lname}.{i}", (stride if i == 0 else 1)
            g.append(_conv(p + ".conv1", [x], relu=True))
            g.append(_conv(p + ".conv2", [p + ".conv1"], stride=(s, s), pad=(1, 1), relu=True))
            if i == 0 and lname == "layer1":
                g.append(_conv(p + ".conv3d", [p + ".conv2", x], relu=True))
            elif i == 0:
                g.append(_conv(p + ".down", [x], stride=(s, s)))
                g.append(_conv(p + ".conv3", [p + ".conv2"], relu=True, res=p + ".down"))
            else:
                g.append(_conv(p + ".conv3", [p + ".conv2"], relu=True, res=x))
            x = g[-1].name
        taps[lname] = x
    h = None
    for k, f in ((1, "layer4"), (2, "layer3"), (3, "layer2"), (4, "layer1")):
        src = [taps[f]]
        if h is not None:
            g.append(_node(f"up{k}", "upsample", [h]))
            src = [f"up{k}", taps[f]]          # torch.cat([upsample(h), f], dim=1)
        g.append(_conv(f"dec{k}.a", src, relu=True))
        g.append(_conv(f"dec{k}.b", [f"dec{k}.a"], pad=(1, 1), relu=True))
        h = f"dec{k}.b"
    g.append(_node("head", "head", [h]))
    return g


def trba_graph():
    """SE-ResNet31 (conv0: two 3x3 + ReLU and a 2x2 max-pool; four layers of SE basic blocks, relu(y * sigmoid(W2 relu(W1 mean_hw(y))) +
    identity) with y = conv2(relu(conv1 x)) and a 1x1 downsample where the stride or the width changes; conv_out: two 2x2 + ReLU) and the
    mean over H.  As in east_graph, a block's `down` comes before the launch that adds it."""
    g = [_node("image", "normalize", mode=1, pad=(1, 1), extra=(1, 3), cpad=8),
         _node("stem", "stem", ["image"], k=(3, 3), stride=(1, 1), pad=(1, 1), relu=True, cin_pad=32),
         _conv("conv0b", ["stem"], pad=(1, 1), relu=True),
         _node("pool", "maxpool", ["conv0b"], k=2, s=2, p=0)]
    x, inplanes = "pool", 128
    for lname, planes, blocks, stride in (("layer1", 256, 1, 2), ("layer2", 256, 2, 1), ("layer3", 512, 5, 2), ("layer4", 512, 3, 1)):
        for i in range(blocks):
            p, s = f"{lname}.{i}", (stride if i == 0 else 1)
            idt = x
            if i == 0 and (stride != 1 or inplanes != planes):
                g.append(_conv(p + ".down", [x], stride=(s, s)))
                idt = p + ".down"
            g.append(_conv(p + ".conv1", [x], stride=(s, s), pad=(1, 1), relu=True))
            g.append(_conv(p + ".conv2", [p + ".conv1"], pad=(1, 1)))
            g.append(_node(p + ".se", "se", [p + ".conv2", idt]))
            x, inplanes = p + ".se", planes
    g.append(_conv("out0", [x], stride=(2, 1), pad=(0, 1), relu=True))
    g.append(_conv("out1", ["out0"], relu=True))
    g.append(_node("mean", "mean_h", ["out1"]))
    return g


# ================================================================================================ references of one node
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv_ref(srcs, w, b, res, stride, pad, relu):
    """f64 convolution of the channel concatenation of `srcs` (NHWC f64) with w [Cout,KH,KW,Cin] f64, every source convolved with its
    own channel range of w, + bias + residual, ReLU; and A = conv(|x|, |w|) + |b| + |res|.  NHWC."""
    ref = A = None
    c0 = 0
    for s in srcs:
        c = s.shape[3]
        wk = _nchw(w[..., c0:c0 + c]).contiguous()
        r = F.conv2d(_nchw(s), wk, stride=stride, padding=pad)
        a = F.conv2d(_nchw(s.abs()), wk.abs(), stride=stride, padding=pad)
        ref, A = (r, a) if ref is None else (ref + r, A + a)
        c0 += c
    assert c0 == w.shape[3], (c0, tuple(w.shape))
    ref, A = ref.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)
    if b is not None:
        ref, A = ref + b, A + b.abs()
    if res is not None:
        ref, A = ref + res, A + res.abs()
    return (ref.clamp_min(0) if relu else ref), A


def conv_bound(ref, A, K):
    """Bound (c) of tests/test_gpu_conv_f64.py for conv_igemm_kernel<__bf16>, per element."""
    return cf.BF16_U * ref.abs() * (1 + cf.BF16_EPS) + 2 * cf._gamma(K) * A


def unpack_stem(w, k, cpad):
    """The device's packed stem weight [Cout][KH][1][cin_pad] (element kw * cpad + c) -> (taps [Cout,KH,KW,3], the padded elements)."""
    Cout, KH, one, cin_pad = w.shape
    assert (KH, one) == (k[0], 1) and cin_pad % cpad == 0
    t = w.reshape(Cout, KH, cin_pad // cpad, cpad)
    pad = torch.ones(t.shape, dtype=torch.bool)
    pad[:, :, : k[1], :3] = False
    return t[:, :, : k[1], :3], t[pad]


def window_view(canvas, cin_pad):
    """The overlapping-window view of a [N,Hp,Wp,cpad] canvas as the stem kernel reads it, by its definition: element kw * cpad + c of
    window (n, h, w) is canvas[n, h, w + kw, c].  Built with unfold, not with as_strided."""
    cpad = canvas.shape[3]
    return canvas.unfold(2, cin_pad // cpad, 1).permute(0, 1, 2, 4, 3).reshape(canvas.shape[0], canvas.shape[1], -1, cin_pad)


def upsample_ref(x):
    """(ref, A) of test_gpu_stream_f64._up_ref_pixels on every output pixel of x (NHWC f64), as NHWC."""
    N, H, W, C = x.shape
    n, yo, xo = torch.meshgrid(torch.arange(N), torch.arange(2 * H), torch.arange(2 * W), indexing="ij")
    ref, A = st._up_ref_pixels(x, n.reshape(-1), yo.reshape(-1), xo.reshape(-1))
    return ref.reshape(N, 2 * H, 2 * W, C), A.reshape(N, 2 * H, 2 * W, C)


def se_gate_ref(y, w1, w2):
    return torch.sigmoid(torch.relu(y.double().mean((1, 2)) @ w1.double().t()) @ w2.double().t())


# ================================================================================================ float64 fold of the raw state dict
def fold(sd, conv, bn, bias=None, dtype=torch.float64):
    """w * gamma / sqrt(var + 1e-5), beta - mean * s (+ conv_bias * s), by the formula of the reference module, in `dtype`; also the
    magnitude |beta| + |mean * s| + |conv_bias * s| that the f32 bias tolerance is relative to."""
    g = lambda k: sd[k].to(dtype)
    s = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + BN_EPS)
    w = g(conv + ".weight") * s.view(-1, 1, 1, 1)
    b = g(bn + ".bias") - g(bn + ".running_mean") * s
    mag = g(bn + ".bias").abs() + (g(bn + ".running_mean") * s).abs()
    if bias is not None:
        b = b + g(bias) * s
        mag = mag + (g(bias) * s).abs()
    return w, b, mag


def east_fold_table():
    """P key -> (conv key, bn key, conv bias key or None) of the reference's state dict, for every entry of EastNet.P but the two
    special ones (stem: packed; layer1.0.conv3d: [W3 | Wd])."""
    t, bb = {"stem": ("conv1", "bn1", None)}, "backbone.extractor."
    for lname, blocks in (("layer1", 3), ("layer2", 4), ("layer3", 6), ("layer4", 3)):
        for i in range(blocks):
            for j in (1, 2, 3):
                t[f"{lname}.{i}.conv{j}"] = (f"{lname}.{i}.conv{j}", f"{lname}.{i}.bn{j}", None)
            if i == 0:
                t[f"{lname}.{i}.down"] = (f"{lname}.{i}.downsample.0", f"{lname}.{i}.downsample.1", None)
    t = {k: (bb + c, bb + b, None) for k, (c, b, _) in t.items()}
    for k in (1, 2, 3, 4):
        for s, m in (("a", "conv1x1"), ("b", "conv3x3")):
            t[f"dec{k}.{s}"] = (f"decoder.block{k}.{m}.0", f"decoder.block{k}.{m}.1", f"decoder.block{k}.{m}.0.bias")
    return t


def trba_fold_table(sd):
    t = {"stem": ("cnn.conv0.0", "cnn.conv0.1", None), "conv0b": ("cnn.conv0.3", "cnn.conv0.4", None),
         "out0": ("cnn.conv_out.0", "cnn.conv_out.1", None), "out1": ("cnn.conv_out.3", "cnn.conv_out.4", None)}
    for lname, blocks in (("layer1", 1), ("layer2", 2), ("layer3", 5), ("layer4", 3)):
        for i in range(blocks):
            p = f"cnn.{lname}.{i}."
            for j in (1, 2):
                t[f"{lname}.{i}.conv{j}"] = (p + f"conv{j}", p + f"bn{j}", None)
            if p + "downsample.0.weight" in sd:
                t[f"{lname}.{i}.down"] = (p + "downsample.0", p + "downsample.1", None)
    return t


def folded_layers(sd, table, stem_k, fused=(), dtype=torch.float64):
    """P key -> (weight as the reference network defines the layer: [Cout][KH][KW][Cin] in `dtype`, bias, bias magnitude).  fused:
    (key, key of W3, key of Wd) entries that are [W3 | Wd] along Cin with bias b3 + bd."""
    out = {}
    for k, (c, b, cb) in table.items():
        w, bias, mag = fold(sd, c, b, cb, dtype)
        assert k != "stem" or tuple(w.shape[2:]) == tuple(stem_k)
        out[k] = (w.permute(0, 2, 3, 1).contiguous(), bias, mag)
    for k, k3, kd in fused:
        (w3, b3, m3), (wd, bd, md) = out[k3], out[kd]
        out[k] = (torch.cat([w3, wd], dim=3), b3 + bd, m3 + md + (b3.abs() + bd.abs()) / 4)  # one more rounded addition: u (|b3| + |bd|)
    return out


def bf16_bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bf16_ulp_distance(a, b):
    """Distance in units of the last place between two bf16 tensors (sign-magnitude: across zero the magnitudes add)."""
    ba, bb = bf16_bits(a), bf16_bits(b)
    ma, mb = ba & 0x7FFF, bb & 0x7FFF
    return torch.where(((ba ^ bb) & 0x8000) != 0, ma + mb, (ma - mb).abs())


def flip_share(sd, table, stem_k, fused=()):
    """Largest share, over the layers, of the weight elements on which bf16(f32 fold) != bf16(f64 fold), on the CPU: what a correct
    device fold (f32, then one rounding) may differ by from the f64 fold."""
    f32 = folded_layers(sd, table, stem_k, fused, torch.float32)
    f64 = folded_layers(sd, table, stem_k, fused, torch.float64)
    worst, total, diff = 0.0, 0, 0
    for k in f64:
        a, b = f32[k][0].to(torch.bfloat16), f64[k][0].to(torch.bfloat16)
        n = int((bf16_bits(a) != bf16_bits(b)).sum())
        worst, total, diff = max(worst, n / a.numel()), total + a.numel(), diff + n
    return worst, diff / total


# ================================================================================================ bf16-storage emulation of the oracle
def _q(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _emul_tools(sd, acc, rounding):
    q = _q if rounding else (lambda x: x)

    def conv_bn(x, conv, bn, stride=1, pad=0, bias=None):
        """A BatchNorm-folded convolution: f64 fold, weight rounded to bf16, accumulated in `acc`, the output rounded to bf16."""
        w, b, _ = fold(sd, conv, bn, bias)
        return q(F.conv2d(x.to(acc), q(w).to(acc), b.to(acc), stride=stride, padding=pad).double())

    return q, conv_bn


def emul_east(sd, x, acc=torch.float64, rounding=True):
    """oracle/east_model.py's forward on x [N,3,H,W] f64 with bf16 storage: conv weights rounded to bf16 after an f64 fold, the output of
    every BatchNorm-folded convolution, ReLU, max-pool and upsample rounded to bf16, sums in `acc`.  rounding=False, acc=f64: the
    oracle network in f64 itself.  -> (score [N,H/4,W/4], geometry [N,H/4,W/4,8]) f64."""
    q, conv_bn = _emul_tools(sd, acc, rounding)
    relu = lambda t: q(torch.relu(t))
    bb = "backbone.extractor."
    x = relu(conv_bn(x, bb + "conv1", bb + "bn1", 2, 3))
    x = q(F.max_pool2d(x, 3, 2, 1))
    feats = []
    for lname, blocks, stride in (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2), ("layer4", 3, 2)):
        for i in range(blocks):
            p = f"{bb}{lname}.{i}."
            o = relu(conv_bn(x, p + "conv1", p + "bn1"))
            o = relu(conv_bn(o, p + "conv2", p + "bn2", stride if i == 0 else 1, 1))
            o = conv_bn(o, p + "conv3", p + "bn3")
            idt = conv_bn(x, p + "downsample.0", p + "downsample.1", stride) if i == 0 else x
            x = relu((o.to(acc) + idt.to(acc)).double())
        feats.append(x)
    h = None
    for k, f in zip((1, 2, 3, 4), reversed(feats)):
        p = f"decoder.block{k}."
        if h is not None:
            up = q(F.interpolate(h.to(acc), scale_factor=2, mode="bilinear", align_corners=False).double())
            f = torch.cat([up, f], dim=1)
        h = relu(conv_bn(f, p + "conv1x1.0", p + "conv1x1.1", bias=p + "conv1x1.0.bias"))
        h = relu(conv_bn(h, p + "conv3x3.0", p + "conv3x3.1", pad=1, bias=p + "conv3x3.0.bias"))
    head = lambda k: F.conv2d(h.to(acc), sd[f"output_head.{k}.weight"].to(acc), sd[f"output_head.{k}.bias"].to(acc)).double()
    return torch.sigmoid(head("score_map"))[:, 0], head("geo_map").permute(0, 2, 3, 1)


def emul_trba_cnn(sd, x, acc=torch.float64, rounding=True):
    """oracle/trba_model.py's SEResNet31 on x [B,3,h,w] f64 with bf16 storage, as emul_east -> features [B,Hf,T,512] f64 (NHWC)."""
    q, conv_bn = _emul_tools(sd, acc, rounding)
    relu = lambda t: q(torch.relu(t))
    x = relu(conv_bn(x, "cnn.conv0.0", "cnn.conv0.1", 1, 1))
    x = relu(conv_bn(x, "cnn.conv0.3", "cnn.conv0.4", 1, 1))
    x = q(F.max_pool2d(x, 2, 2))
    for lname, blocks, stride in (("layer1", 1, 2), ("layer2", 2, 1), ("layer3", 5, 2), ("layer4", 3, 1)):
        for i in range(blocks):
            p, s = f"cnn.{lname}.{i}.", (stride if i == 0 else 1)
            o = relu(conv_bn(x, p + "conv1", p + "bn1", s, 1))
            o = conv_bn(o, p + "conv2", p + "bn2", 1, 1).to(acc)
            gate = torch.sigmoid(torch.relu(o.mean((2, 3)) @ sd[p + "se.fc.0.weight"].to(acc).t()) @ sd[p + "se.fc.2.weight"].to(acc).t())
            idt = conv_bn(x, p + "downsample.0", p + "downsample.1", s) if p + "downsample.0.weight" in sd else x
            x = relu((o * gate[:, :, None, None] + idt.to(acc)).double())
    x = relu(conv_bn(x, "cnn.conv_out.0", "cnn.conv_out.1", (2, 1), (0, 1)))
    x = relu(conv_bn(x, "cnn.conv_out.3", "cnn.conv_out.4"))
    return x.permute(0, 2, 3, 1)


def rel_distance(a, ref):
    """max|a - ref| relative to max(1, max|ref|)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


# ================================================================================================ the replay
def replay(graph, leaves, P, head=None, dtype=torch.bfloat16, report=print):
    """Every node of `graph` against its float64 reference, computed from the recorded DEVICE outputs of the nodes that feed it and the
    device's own weight and bias of that layer (P; head = (w9, b9)).  The recorded leaf calls must be exactly the graph's labels, in
    order.  Returns (failures in network order as strings, per-node worst error / bound, the f64 references' statistics: positive share
    after every ReLU, score standard deviation, gate standard deviation per SE block)."""
    want, got = [n.label for n in graph], [r.label for r in leaves]
    assert got == want, "the recorded calls are not the expected graph:\n" + "\n".join(
        f"  {i}: recorded {g!r}, expected {w!r}" for i, (g, w) in enumerate(zip(got + ["-"] * len(want), want + ["-"] * len(got))) if g != w)
    out, fails, ratios = {}, [], {}
    stats = SimpleNamespace(positive={}, score_std=None, gate_std={})
    cpu = lambda t: t.detach().cpu()

    def fail(node, msg):
        fails.append(f"{node.name} ({node.label}): {msg}")

    def same_input(node, rec, arg, parts):
        """The recorded input `arg` must be, bit for bit, the channel concatenation of the recorded outputs `parts`."""
        x, c0 = rec.inputs[arg], 0
        for name in parts:
            o = out[name]
            c = o.shape[-1]
            if x.shape[:-1] != o.shape[:-1] or not torch.equal(x[..., c0:c0 + c], o):
                fail(node, f"input `{arg}` channels {c0}:{c0 + c} are not the recorded output of {name}")
            c0 += c
        if c0 != x.shape[-1]:
            fail(node, f"input `{arg}` has {x.shape[-1]} channels, its sources {parts} have {c0}")

    def bounded(node, dev, ref, lim, what=""):
        if tuple(dev.shape) != tuple(ref.shape):
            fail(node, f"output shape {tuple(dev.shape)}, reference {tuple(ref.shape)}")
            return
        e = (dev.double() - ref).abs()
        worst = float((e / lim.clamp_min(1e-300)).max())
        worst = float("inf") if worst != worst else worst
        ratios[node.name + what] = worst
        if not bool(torch.all(e <= lim)):
            fail(node, f"{what or 'output'} off its bound by a factor {worst:.3g} (max error {float(e.max()):.3e})")

    for node, rec in zip(graph, leaves):
        o = rec.output
        if node.op == "normalize":
            img = rec.inputs["imgs_u8"]
            N, H, W, _ = img.shape
            pt, pl = node.pad
            exp = torch.zeros((N, H + pt + node.extra[0], W + pl + node.extra[1], node.cpad), dtype=torch.float32)
            exp[:, pt:pt + H, pl:pl + W, :3] = torch.from_numpy(st._norm_ref(img.numpy(), node.mode))
            exp = exp.to(dtype)
            if tuple(o.shape) != tuple(exp.shape) or not torch.equal(bf16_bits(o) if dtype == torch.bfloat16 else o, bf16_bits(exp) if dtype == torch.bfloat16 else exp):
                fail(node, f"canvas {tuple(o.shape)} differs from the normalised image in a zero canvas {tuple(exp.shape)}")
            ratios[node.name] = 0.0
            out[node.name] = o
            out["image:pixels"] = o[:, pt:pt + H, pl:pl + W, :3]
        elif node.op == "stem":
            w, b = P[node.name]
            canvas = out[node.src[0]]
            win = window_view(canvas, node.cin_pad)
            if tuple(rec.inputs["x"].shape) != tuple(win.shape) or not torch.equal(rec.inputs["x"], win):
                fail(node, "the kernel's input is not the overlapping-window view of the recorded canvas")
            if rec.objects.get("bias") is not b:
                fail(node, "called with another bias than the layer's")
            taps, _ = unpack_stem(cpu(w), node.k, canvas.shape[3])
            ref, A = conv_ref([out["image:pixels"].double()], taps.double(), cpu(b).double(), None, node.stride, node.pad, node.relu)
            bounded(node, o, ref, conv_bound(ref, A, w.shape[1] * w.shape[2] * w.shape[3]))
            stats.positive[node.name] = float((ref > 0).double().mean())
            out[node.name] = o
        elif node.op == "conv":
            w, b = P[node.name]
            same_input(node, rec, "x", node.src)
            if rec.objects.get("bias") is not b:
                fail(node, "called with another bias than the layer's")
            called = (tuple(rec.kwargs["stride"]), tuple(rec.kwargs["pad"]), bool(rec.kwargs["relu"]))
            if called != (tuple(node.stride), tuple(node.pad), node.relu):
                fail(node, f"called with (stride, pad, relu) = {called}, the graph has {(tuple(node.stride), tuple(node.pad), node.relu)}")
            if (node.res is None) != ("residual" not in rec.inputs):
                fail(node, "residual given where the graph has none, or missing")
            elif node.res is not None and not (rec.inputs["residual"].shape == out[node.res].shape and torch.equal(rec.inputs["residual"], out[node.res])):
                fail(node, f"the residual is not the recorded output of {node.res}")
            res = out[node.res].double() if node.res is not None else None
            ref, A = conv_ref([out[s].double() for s in node.src], cpu(w).double(), cpu(b).double(), res, node.stride, node.pad, node.relu)
            bounded(node, o, ref, conv_bound(ref, A, w.shape[1] * w.shape[2] * w.shape[3]))
            if node.relu:
                stats.positive[node.name] = float((ref > 0).double().mean())
            out[node.name] = o
        elif node.op == "maxpool":
            same_input(node, rec, "x", node.src)
            exp = st._pool_ref(out[node.src[0]].float(), node.k, node.s, node.p).to(dtype)
            if tuple(o.shape) != tuple(exp.shape) or not torch.equal(o, exp):
                fail(node, "differs from F.max_pool2d of the recorded input")
            ratios[node.name] = 0.0
            out[node.name] = o
        elif node.op == "upsample":
            same_input(node, rec, "x", node.src)
            ref, A = upsample_ref(out[node.src[0]].double())
            bounded(node, o, ref, st.BF16_U * ref.abs() * (1 + st.BF16_EPS) + 2 * st._gamma(st.UP_GAMMA) * A)
            out[node.name] = o
        elif node.op == "head":
            w9, b9 = head
            same_input(node, rec, "h1", node.src)
            if rec.objects["w9"] is not w9 or rec.objects["b9"] is not b9:
                fail(node, "called with other head weights than the network's")
            h1 = out[node.src[0]].double()
            lo, A = st._head_ref(h1.reshape(-1, 32), cpu(w9), cpu(b9))
            G = st._gamma(st.HEAD_GAMMA) * A
            score, geo = o
            s = torch.sigmoid(lo[:, 0])
            lim = s * (1 - s) * (1 + G[:, 0]) * G[:, 0] + s * ((1 - s) * st.EXPF_REL + 2 * st.U) + 2.0 ** -126
            bounded(node, score.reshape(-1), s, lim, ":score")
            bounded(node, geo.reshape(-1, 8), lo[:, 1:], G[:, 1:], ":geometry")
            stats.score_std = float(s.std())
            out[node.name] = o
        elif node.op == "se":
            w1, w2 = P[node.name]
            same_input(node, rec, "x", node.src[:1])
            same_input(node, rec, "identity", node.src[1:])
            if rec.objects["w1"] is not w1 or rec.objects["w2"] is not w2:
                fail(node, "called with another block's SE weights")
            y, idt = out[node.src[0]], out[node.src[1]]
            gate = se_gate_ref(y, cpu(w1), cpu(w2))
            ref = torch.from_numpy(sq._se_ref(y.float(), idt.float(), cpu(w1), cpu(w2)))
            bounded(node, o, ref, sq.SE_BF16_U * ref.abs() + sq.SE_BF16_ABS)
            bounded(node, rec.extra["gate"], gate, torch.full_like(gate, sq.SE_BF16_ABS), ":gate")
            stats.gate_std[node.name] = float(gate.std())
            stats.positive[node.name] = float((ref > 0).double().mean())
            out[node.name] = o
        elif node.op == "mean_h":
            same_input(node, rec, "x", node.src)
            ref = out[node.src[0]].double().mean(1)
            bounded(node, o, ref, torch.full_like(ref, sq.MEAN_H_RTOL * max(1.0, float(ref.abs().max()))))
            out[node.name] = o
        else:
            raise ValueError(node.op)
    for node in graph:
        keys = [k for k in ratios if k == node.name or k.startswith(node.name + ":")]
        report(f"[bf16-replay] {node.name:18s} {node.label:28s} " + "  ".join(f"err/bound{k[len(node.name):]} {ratios[k]:.3f}" for k in keys))
    return fails, ratios, stats
