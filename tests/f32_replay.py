"""Test-side tools of tests/test_gpu_f32_networks.py: the default f32 mode of both networks, replayed layer by layer against float64.
What does not depend on the dtype comes from tests/bf16_replay.py (the recorder, conv_ref, window_view, unpack_stem, upsample_ref,
se_gate_ref, east_graph); here are what the f32 mode adds: a recorder that also stores, per call, the kernel family ops.PROFILE names
(and that takes ops.se_block and ops.bilstm_recurrent as calls of their own), the recogniser's f32 graph (conv0b with its pool in one
call, an SE block as one call where a per-crop kernel runs, the encoder behind the CNN), and the replay with the f32 bounds.  Every bound
is imported from the module that owns it; nothing of the package changes for this module."""
import inspect
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import bf16_replay as br
import test_gpu_conv_f64 as cf
import test_gpu_se_block_f64 as sb
import test_gpu_seq_f64 as sq
import test_gpu_stream_f64 as st

RECORDED_OPS = br.RECORDED_OPS + ("bilstm_recurrent",)
_OUTPUT_ARGS = dict(br._OUTPUT_ARGS)
_BY_IDENTITY = dict(br._BY_IDENTITY, bilstm_recurrent=("whh_t", "whh_planes"))
_GATED = ("se_residual", "se_block")   # calls with a `gate` argument that is scratch unless given
_TUPLES = {"se_block": ("conv1", "conv2", "se")}   # tuples of weights, kept as objects

# conv_gemm tag of ops.PROFILE -> the name of the form in the case tables ("winograd44_split" is "square" or "square+tail" by its rows)
FORM_OF_TAG = {"direct": "direct", "direct_split": "direct_split", "winograd": "f2x2", "winograd42": "tall", "winograd42_split": "tall_split",
               "winograd42_fused": "fused", "winograd42_fused_split": "fused_split"}
# rule (d) of tests/test_gpu_conv_f64.py multiplied from the direct exact kernel to the form taken
_TALL = cf.WINO_DIRECT_FACTOR["42"]
WINO_FACTOR = {"f2x2": cf.WINO_DIRECT_FACTOR["2x2"], "tall": _TALL, "fused": cf.WINO_DIRECT_FACTOR["f64"], "fused_split": cf.WINO_DIRECT_FACTOR["f64s"],
               "tall_split": cf.SPLIT_EXACT_FACTOR * _TALL, "square": cf.SQUARE_TALL_FACTOR * cf.SPLIT_EXACT_FACTOR * _TALL,
               "square+tail": cf.SQUARE_TALL_FACTOR * cf.SPLIT_EXACT_FACTOR * _TALL}
WINO_SLACK, WINO_CEILING = cf.SPLIT_SLACK, cf.WINO_CEILING


# ================================================================================================ recorder
class Recorder(br.Recorder):
    """bf16_replay.Recorder with ops.PROFILE on: every record also holds `gemms`, the (form name, point rows) of the conv_gemm launches the
    call made ITSELF (not those of recorded calls inside it), and `fused`, the "chain" / "se" tags of its per-crop kernels.  An
    ops.se_block call that ran a per-crop kernel is a leaf, placed behind the conv1 call it may have made; its three weight tuples are
    kept as objects and its gates are read out, as se_residual's are."""

    def __init__(self, monkeypatch, ops, P):
        self.records, self.depth, self.ops, self._inner = [], 0, ops, [[]]
        self.weights = {id(v[0]): k for k, v in P.items()}
        assert len(self.weights) == len(P)
        for name in RECORDED_OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    @staticmethod
    def _form(entry):
        M, N, K, tag = entry[4]
        if tag != "winograd44_split":
            return FORM_OF_TAG[tag], None
        rows = int(round(entry[3][1] / (2.0 * (K // 9) * N)))
        return ("square", "square+tail"), rows   # told apart by the rows, in the replay, where the map is known

    def _wrap(self, name, orig):
        sig = inspect.signature(orig)
        ops = self.ops

        def wrapper(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            args = ba.arguments
            if name in _GATED and args["gate"] is None:  # the gates are scratch otherwise: have them written where we can read them
                x = args["x"]
                C = args["w2"].shape[0] if name == "se_residual" else args["conv2"][0].shape[0]
                args["gate"] = torch.empty((x.shape[0], C), dtype=torch.float32, device=x.device)
            rec = SimpleNamespace(op=name, label=name, depth=self.depth, leaf=True, inputs={}, objects={}, kwargs={}, extra={})
            for k, v in args.items():
                if isinstance(v, torch.Tensor):
                    if k in _BY_IDENTITY.get(name, ()):
                        rec.objects[k] = v
                    elif k == "gate" and name in _GATED:
                        pass
                    elif k not in _OUTPUT_ARGS.get(name, ()):
                        rec.inputs[k] = br._values(v)
                elif k in _TUPLES.get(name, ()):
                    rec.objects[k] = v
                elif not (isinstance(v, tuple) and any(isinstance(e, (tuple, torch.Tensor)) for e in v)):
                    rec.kwargs[k] = v
            if name == "conv2d":
                key = self.weights.get(id(args["w"]))
                assert key is not None, f"conv2d call {len(self.records)} with a weight {tuple(args['w'].shape)} that is in no table of the network"
                rec.label = f"conv2d:{key}"
                rec.key = key
            self.records.append(rec)
            n = len(self.records)
            assert ops.PROFILE is not None, "the f32 recorder runs with ops.PROFILE on"
            p0 = len(ops.PROFILE)
            self._inner.append([])
            self.depth += 1
            try:
                out = orig(*ba.args, **ba.kwargs)
            finally:
                self.depth -= 1
                inner = self._inner.pop()
            torch.cuda.synchronize()
            p1 = len(ops.PROFILE)
            self._inner[-1].append((p0, p1))
            own = [ops.PROFILE[i] for i in range(p0, p1) if not any(lo <= i < hi for lo, hi in inner)]
            rec.gemms = [self._form(e) for e in own if e[2] == "conv_gemm"]
            rec.fused = [e[4][2] for e in own if e[2] == "wino_out" and len(e[4]) > 2]
            rec.leaf = len(self.records) == n
            if name == "se_block" and rec.fused:   # a per-crop kernel ran: the block is a call of its own, behind its conv1 if that was one
                assert [r.label.split(".")[-1] for r in self.records[n:]] in ([], ["conv1"]), [r.label for r in self.records[n:]]
                rec.leaf = True
                self.records.remove(rec)
                self.records.append(rec)
            res = out
            if name == "upsample2x_into":
                res = out[..., : args["x"].shape[3]]
            if name in _GATED:
                rec.extra["gate"] = br._values(args["gate"])
            outs = res if isinstance(res, tuple) else (res,)
            rec.output = tuple(br._values(t) for t in outs) if isinstance(res, tuple) else br._values(res)
            rec.ptr, rec.shape, rec.strides = outs[0].data_ptr(), tuple(outs[0].shape), tuple(outs[0].stride())
            return out

        return wrapper


# ================================================================================================ the networks as graphs
east_graph = br.east_graph   # the same calls as in bf16: stem canvas with cpad 4 and cin_pad 32, written down in bf16_replay


def _node(name, op, label, src=(), **kw):
    return SimpleNamespace(name=name, op=op, src=tuple(src), label=label, **kw)


TRBA_LAYERS = (("layer1", 256, 1, 2), ("layer2", 256, 2, 1), ("layer3", 512, 5, 2), ("layer4", 512, 3, 1))


def encoder_table(net):
    """The GEMM weights of TrbaNet.encode behind the CNN, keyed as the graph names them: (weight, bias)."""
    t = {}
    for l in (0, 1):
        r = net.rnn[l]
        t[f"rnn{l}.proj"] = (r["w_ih"], r["b"])
        t[f"rnn{l}.lin"] = (r["lin_w"], r["lin_b"])
    t["i2h"] = (net.att["i2h_w"], None)
    return t


def trba_graph(block_shapes, conv0b_fused=True):
    """TrbaNet.encode in f32, from recognizers/_trba/net.py and the reference architecture (oracle/trba_model.py: SEResNet31, the mean over
    H, two BidirectionalLSTM, the attention cell's i2h): the stem over a canvas with cpad 4 and cin_pad 16; conv0b with its 2x2 / 2 max-pool
    in one call where the fused Cin = 64 kernel applies; per SE block, by block_shapes[block] (the case table's leaf shape):
      "three"  [down,] conv1, conv2, se_residual                       (as in bf16)
      "se"     [down,] conv1, se_block (conv2 -> SE tail per crop)     (a strided or widening conv1 cannot chain)
      "chain"  se_block (conv1 -> conv2 -> SE tail per crop)
    a block's `down` comes before the call that adds it; then conv_out, the mean over H, and per BiLSTM layer the input projection
    (K = 512 / 256), the recurrence and the linear (K = 512), and the i2h projection (K = 256)."""
    g = [_node("image", "normalize", "normalize_u8", mode=1, pad=(1, 1), extra=(1, 3), cpad=4),
         _node("stem", "stem", "conv2d:stem", ["image"], k=(3, 3), stride=(1, 1), pad=(1, 1), relu=True, cin_pad=16)]
    if conv0b_fused:
        g.append(_node("conv0b", "conv", "conv2d:conv0b", ["stem"], stride=(1, 1), pad=(1, 1), relu=True, res=None, pool2=True))
        x = "conv0b"
    else:
        g.append(_node("conv0b", "conv", "conv2d:conv0b", ["stem"], stride=(1, 1), pad=(1, 1), relu=True, res=None))
        g.append(_node("pool", "maxpool", "maxpool2d", ["conv0b"], k=2, s=2, p=0))
        x = "pool"
    inplanes = 128
    for lname, planes, blocks, stride in TRBA_LAYERS:
        for i in range(blocks):
            p, s = f"{lname}.{i}", (stride if i == 0 else 1)
            shape, idt = block_shapes[p], x
            if i == 0 and (stride != 1 or inplanes != planes):
                g.append(_node(p + ".down", "conv", f"conv2d:{p}.down", [x], stride=(s, s), pad=(0, 0), relu=False, res=None))
                idt = p + ".down"
            if shape in ("three", "se"):
                g.append(_node(p + ".conv1", "conv", f"conv2d:{p}.conv1", [x], stride=(s, s), pad=(1, 1), relu=True, res=None))
            if shape == "three":
                g.append(_node(p + ".conv2", "conv", f"conv2d:{p}.conv2", [p + ".conv1"], stride=(1, 1), pad=(1, 1), relu=False, res=None))
                g.append(_node(p + ".se", "se", "se_residual", [p + ".conv2", idt]))
            else:
                assert shape in ("se", "chain") and not (shape == "chain" and idt != x), (p, shape)
                g.append(_node(p + ".se", "seblock", "se_block", [x, idt], block=p, stride=(s, s), shape=shape))
            x, inplanes = p + ".se", planes
    g.append(_node("out0", "conv", "conv2d:out0", [x], stride=(2, 1), pad=(0, 1), relu=True, res=None))
    g.append(_node("out1", "conv", "conv2d:out1", ["out0"], stride=(1, 1), pad=(0, 0), relu=True, res=None))
    g.append(_node("mean", "mean_h", "mean_over_h", ["out1"]))
    seq = "mean"
    for l in (0, 1):
        g.append(_node(f"rnn{l}.proj", "gemm", f"conv2d:rnn{l}.proj", [seq]))
        g.append(_node(f"rnn{l}.rec", "bilstm", "bilstm_recurrent", [f"rnn{l}.proj"], layer=l))
        g.append(_node(f"rnn{l}.lin", "gemm", f"conv2d:rnn{l}.lin", [f"rnn{l}.rec"]))
        seq = f"rnn{l}.lin"
    g.append(_node("i2h", "gemm", "conv2d:i2h", [seq]))
    return g


# ================================================================================================ references of one node
def bilstm_ref(xproj, whh_t, B, T, H):
    """The reference of tests/test_gpu_seq_f64.py part (e) (_bilstm_problem): a bidirectional nn.LSTM in float64 whose input weights select
    the direction's half of xproj [B*T, 2*4H] exactly (identity blocks, zero bias), with the recurrent weights taken back from the device's
    gate-interleaved whh_t [2][H(k)][H(j)][4]."""
    lstm = torch.nn.LSTM(8 * H, H, bidirectional=True, batch_first=True).double()
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, 4 * H, dtype=torch.float64)
    whh = [whh_t[d].double().permute(2, 1, 0).reshape(4 * H, H) for d in (0, 1)]   # [k][j][gate] -> [gate * H + j][k]
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        lstm.weight_hh_l0.copy_(whh[0])
        lstm.weight_hh_l0_reverse.copy_(whh[1])
        for n in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(lstm, n).zero_()
        ref, _ = lstm(xproj.double().reshape(B, T, 8 * H))
    return ref


def pool2_ref(t):
    return F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


def block_ref(x, idt, conv1, conv2, se, stride):
    """The SE basic block in float64 from the device's weights ([Cout][3][3][Cin], bias; SE w1, w2): (out, gate, relu(conv1)) NHWC."""
    a, _ = br.conv_ref([x], conv1[0], conv1[1], None, stride, (1, 1), True)
    y, _ = br.conv_ref([a], conv2[0], conv2[1], None, (1, 1), (1, 1), False)
    gate = torch.sigmoid(torch.relu(y.mean((1, 2)) @ se[0].t()) @ se[1].t())
    return torch.relu(y * gate[:, None, None, :] + idt), gate, a


# ================================================================================================ the replay
def replay(graph, leaves, P, ops, head=None, rnn=None, tag="f32-replay", report=print):
    """Every node of `graph` against its float64 reference, computed from the recorded DEVICE outputs of the nodes that feed it and the
    device's own weight and bias of that layer (P, with the encoder's GEMM weights beside it; head = (w9, b9); rnn = TrbaNet.rnn).  The
    recorded leaf calls must be exactly the graph's labels, in order; every input must be, bit for bit, the recorded output of the node
    the graph names.  The Winograd layers and the SE blocks are run once more ON THE DEVICE through the exact direct kernel
    (ops.attach_split(w.clone(), False), no Winograd planes) from the recorded inputs: that error is the yardstick of their bounds.
    Returns (failures in network order as strings, per-node worst error / bound, the f64 references' statistics, node name -> the form
    its convolution took, SE block name -> its leaf shape)."""
    want, got = [n.label for n in graph], [r.label for r in leaves]
    assert got == want, "the recorded calls are not the expected graph:\n" + "\n".join(
        f"  {i}: recorded {g!r}, expected {w!r}" for i, (g, w) in enumerate(zip(got + ["-"] * len(want), want + ["-"] * len(got))) if g != w)
    out, fails, ratios, forms, shapes = {}, [], {}, {}, {}
    stats = SimpleNamespace(positive={}, score_std=None, gate_std={})
    cpu = lambda t: t.detach().cpu()
    dev = lambda t: t.contiguous().cuda()
    from manuscript_ocr_amd import _native as nat

    def fail(node, msg):
        fails.append(f"{node.name} ({node.label}): {msg}")

    def same(node, x, arg, parts):
        """The recorded input must be, bit for bit, the channel concatenation of `parts`: (node name, its recorded output) pairs."""
        c0 = 0
        for name, o in parts:
            c = o.shape[-1]
            if x.shape[:-1] != o.shape[:-1] or not torch.equal(x[..., c0:c0 + c], o):
                fail(node, f"input `{arg}` channels {c0}:{c0 + c} are not the recorded output of {name}")
            c0 += c
        if c0 != x.shape[-1]:
            fail(node, f"input `{arg}` has {x.shape[-1]} channels, its sources {[n for n, _ in parts]} have {c0}")

    def same_input(node, rec, arg, names):
        same(node, rec.inputs[arg], arg, [(n, out[n]) for n in names])

    def bounded(node, d, ref, lim, what=""):
        if tuple(d.shape) != tuple(ref.shape):
            fail(node, f"output shape {tuple(d.shape)}, reference {tuple(ref.shape)}")
            return
        e = (d.double() - ref).abs()
        worst = float((e / lim.clamp_min(1e-300)).max())
        worst = float("inf") if worst != worst else worst
        ratios[node.name + what] = worst
        if not bool(torch.all(e <= lim)):
            fail(node, f"{what or 'output'} off its bound by a factor {worst:.3g} (max error {float(e.max()):.3e})")

    def max_bounded(node, d, ref, e_direct, factor, slack, ceiling, what, how):
        """max|dev - ref| <= factor * e_direct + slack * scale and <= ceiling * scale, scale = max(1, max|ref|)."""
        if tuple(d.shape) != tuple(ref.shape):
            fail(node, f"output shape {tuple(d.shape)}, reference {tuple(ref.shape)}")
            return
        scale = max(1.0, float(ref.abs().max()))
        err = float((d.double() - ref).abs().max())
        err = float("inf") if err != err else err
        lim = min(factor * e_direct + slack * scale, ceiling * scale)
        ratios[node.name + what] = err / lim
        if not err <= lim:
            fail(node, f"{what or 'output'} {how}: error {err:.3e} against {factor:g} x {e_direct:.3e} (exact direct kernel) + {slack:g} x {scale:.3g}, "
                       f"ceiling {ceiling:g} x {scale:.3g}: off by a factor {err / lim:.3g}")

    def gemm_form(rec, i, N, H, W):
        form, rows = rec.gemms[i]
        if rows is None:
            return form
        for f, fid in (("square", nat.WINO_4X4), ("square+tail", nat.WINO_4X4_COLTAIL)):
            if rows == ops._wino_rows(fid, N, H, W)[0] and (f == "square+tail") == ops._coltail(W):
                return f
        return f"winograd44_split with {rows} point rows"

    def check_conv_call(node, rec, b):
        if rec.objects.get("bias") is not b:
            fail(node, "called with another bias than the layer's")
        called = (tuple(rec.kwargs["stride"]), tuple(rec.kwargs["pad"]), bool(rec.kwargs["relu"]), bool(rec.kwargs.get("pool2", False)))
        graph_has = (tuple(node.stride), tuple(node.pad), node.relu, bool(getattr(node, "pool2", False)))
        if called != graph_has:
            fail(node, f"called with (stride, pad, relu, pool2) = {called}, the graph has {graph_has}")

    for node, rec in zip(graph, leaves):
        o = rec.output
        if node.op == "normalize":
            img = rec.inputs["imgs_u8"]
            N, H, W, _ = img.shape
            pt, pl = node.pad
            exp = torch.zeros((N, H + pt + node.extra[0], W + pl + node.extra[1], node.cpad), dtype=torch.float32)
            exp[:, pt:pt + H, pl:pl + W, :3] = torch.from_numpy(st._norm_ref(img.numpy(), node.mode))
            if o.dtype != torch.float32 or tuple(o.shape) != tuple(exp.shape) or not torch.equal(o.view(torch.int32), exp.view(torch.int32)):
                fail(node, f"canvas {tuple(o.shape)} differs from the normalised image in a zero canvas {tuple(exp.shape)}")
            ratios[node.name] = 0.0
            out[node.name] = o
            out["image:pixels"] = o[:, pt:pt + H, pl:pl + W, :3]
        elif node.op == "stem":
            w, b = P[node.name]
            canvas = out[node.src[0]]
            win = br.window_view(canvas, node.cin_pad)
            if tuple(rec.inputs["x"].shape) != tuple(win.shape) or not torch.equal(rec.inputs["x"], win):
                fail(node, "the kernel's input is not the overlapping-window view of the recorded canvas")
            check_conv_call(SimpleNamespace(name=node.name, label=node.label, stride=node.stride, pad=(0, 0), relu=node.relu), rec, b)
            taps, padded = br.unpack_stem(cpu(w), node.k, canvas.shape[3])
            if bool((padded != 0).any()):
                fail(node, "a padded element of the packed stem weight is not zero")
            ref, A = br.conv_ref([out["image:pixels"].double()], taps.double(), cpu(b).double(), None, node.stride, node.pad, node.relu)
            K = w.shape[1] * w.shape[2] * w.shape[3]   # the packed K, as the kernel sums it
            forms[node.name] = gemm_form(rec, 0, 0, 0, 0) if len(rec.gemms) == 1 else str(rec.gemms)
            if forms[node.name] not in ("direct", "direct_split"):
                fail(node, f"ran as {forms[node.name]}, not on a direct kernel")
            bounded(node, o, ref, (cf.SPLIT_GAMMA if forms[node.name] == "direct_split" else 1.0) * cf._gamma(K) * A)
            stats.positive[node.name] = float((ref > 0).double().mean())
            out[node.name] = o
        elif node.op in ("conv", "gemm"):
            w, b = P[node.name]
            if node.op == "gemm":   # TrbaNet._gemm: a 1x1 convolution over the rows of [M, K], viewed as [1, M, 1, K]
                src = out[node.src[0]]
                srcs = [src.reshape(1, -1, 1, src.shape[-1])]
                same(node, rec.inputs["x"], "x", [(node.src[0], srcs[0])])
                node = SimpleNamespace(**vars(node), stride=(1, 1), pad=(0, 0), relu=False, res=None)
            else:
                same_input(node, rec, "x", node.src)
                srcs = [out[s] for s in node.src]
            check_conv_call(node, rec, b)
            if (node.res is None) != ("residual" not in rec.inputs):
                fail(node, "residual given where the graph has none, or missing")
            elif node.res is not None and not (rec.inputs["residual"].shape == out[node.res].shape and torch.equal(rec.inputs["residual"], out[node.res])):
                fail(node, f"the residual is not the recorded output of {node.res}")
            res = out[node.res] if node.res is not None else None
            pool2 = bool(getattr(node, "pool2", False))
            bias64 = cpu(b).double() if b is not None else None
            ref, A = br.conv_ref([s.double() for s in srcs], cpu(w).double(), bias64, res.double() if res is not None else None,
                                 node.stride, node.pad, node.relu)
            if node.relu:
                stats.positive[node.name] = float((ref > 0).double().mean())
            if pool2:
                ref = pool2_ref(ref)   # the 2x2 / 2 max-pool of the f64 convolution
            N, H, W, _ = rec.inputs["x"].shape
            forms[node.name] = form = gemm_form(rec, 0, N, H, W) if len(rec.gemms) == 1 else str(rec.gemms)
            K = w.shape[1] * w.shape[2] * w.shape[3]
            if form in ("direct", "direct_split"):
                if pool2:
                    fail(node, "conv2d(pool2=True) as one call, but on a direct kernel")
                bounded(node, o, ref, (cf.SPLIT_GAMMA if form == "direct_split" else 1.0) * cf._gamma(K) * A)
            elif form in WINO_FACTOR:
                direct = ops.conv2d(dev(rec.inputs["x"]), ops.attach_split(w.clone(), False), b, node.stride, node.pad, node.relu,
                                    dev(res) if res is not None else None, pool2=pool2)
                e_direct = float((cpu(direct).double() - ref).abs().max())
                max_bounded(node, o, ref, e_direct, WINO_FACTOR[form], WINO_SLACK, WINO_CEILING, "", f"as {form}")
            else:
                fail(node, f"ran as {form}: no kernel family this replay knows")
            out[node.name] = o
        elif node.op == "maxpool":
            same_input(node, rec, "x", node.src)
            exp = st._pool_ref(out[node.src[0]], node.k, node.s, node.p)
            if tuple(o.shape) != tuple(exp.shape) or not torch.equal(o, exp):
                fail(node, "differs from F.max_pool2d of the recorded input")
            ratios[node.name] = 0.0
            out[node.name] = o
        elif node.op == "upsample":
            same_input(node, rec, "x", node.src)
            ref, A = br.upsample_ref(out[node.src[0]].double())
            bounded(node, o, ref, st._gamma(st.UP_GAMMA) * A)
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
            gate = br.se_gate_ref(y, cpu(w1), cpu(w2))
            ref = torch.from_numpy(sq._se_ref(y, idt, cpu(w1), cpu(w2)))
            # part (f) of tests/test_gpu_seq_f64.py holds the f32 kernel to SE_F32_RTOL of max(1, max|ref|); the gates lie in (0, 1)
            bounded(node, o, ref, torch.full_like(ref, sq.SE_F32_RTOL * max(1.0, float(ref.abs().max()))))
            bounded(node, rec.extra["gate"], gate, torch.full_like(gate, sq.SE_F32_RTOL * max(1.0, float(gate.abs().max()))), ":gate")
            stats.gate_std[node.name] = float(gate.std())
            stats.positive[node.name] = float((ref > 0).double().mean())
            shapes[node.name[:-3]] = "three"
            out[node.name] = o
        elif node.op == "seblock":
            p = node.block
            conv1, conv2, se = P[p + ".conv1"], P[p + ".conv2"], P[p + ".se"]
            same_input(node, rec, "x", node.src[:1])
            same_input(node, rec, "identity", node.src[1:])
            for k, mine in (("conv1", conv1), ("conv2", conv2), ("se", se)):
                if not (rec.objects[k][0] is mine[0] and rec.objects[k][1] is mine[1]):
                    fail(node, f"called with another `{k}` than the block's")
            if tuple(rec.kwargs["stride"]) != tuple(node.stride):
                fail(node, f"called with stride {tuple(rec.kwargs['stride'])}, the graph has {tuple(node.stride)}")
            x, idt = out[node.src[0]], out[node.src[1]]
            c64 = lambda t: tuple(cpu(e).double() for e in t)
            ref, gate, a = block_ref(x.double(), idt.double(), c64(conv1), c64(conv2), c64(se), node.stride)
            N, Ho, Wo, _ = ref.shape
            shapes[p] = {("chain", "se"): "chain", ("se",): "se"}.get(tuple(rec.fused), str(rec.fused))
            want_gemms = 2 if shapes[p] == "chain" else 1
            gf = [gemm_form(rec, i, N, Ho, Wo) for i in range(len(rec.gemms))]
            if shapes[p] != node.shape or len(gf) != want_gemms:
                fail(node, f"ran as {shapes[p]} with GEMMs {gf}, the graph has {node.shape}")
            forms[p + ".conv2"] = gf[-1] if gf else "none"
            if shapes[p] == "chain" and gf:
                forms[p + ".conv1"] = gf[0]
            # the block through the three calls on the exact direct kernel, from the recorded x and identity
            exact = [(ops.attach_split(w.clone(), False), b) for w, b in (conv1, conv2)]
            gbuf = torch.empty((N, ref.shape[3]), dtype=torch.float32, device="cuda")
            y1 = ops.conv2d(dev(x), *exact[0], stride=node.stride, pad=(1, 1), relu=True)
            base = ops.se_residual(ops.conv2d(y1, *exact[1], pad=(1, 1)), dev(idt), *se, gate=gbuf)
            e_out, e_gate = float((cpu(base).double() - ref).abs().max()), float((cpu(gbuf).double() - gate).abs().max())
            max_bounded(node, o, ref, e_out, sb.FACTOR, sb.SLACK, sb.CEILING, "", f"as {shapes[p]}")
            max_bounded(node, rec.extra["gate"], gate, e_gate, sb.FACTOR, sb.SLACK, sb.CEILING, ":gate", f"as {shapes[p]}")
            stats.gate_std[node.name] = float(gate.std())
            stats.positive[p + ".conv1"] = float((a > 0).double().mean())
            stats.positive[node.name] = float((ref > 0).double().mean())
            out[node.name] = o
        elif node.op == "mean_h":
            same_input(node, rec, "x", node.src)
            ref = out[node.src[0]].double().mean(1)
            bounded(node, o, ref, torch.full_like(ref, sq.MEAN_H_RTOL * max(1.0, float(ref.abs().max()))))
            out[node.name] = o
        elif node.op == "bilstm":
            r = rnn[node.layer]
            B, T, H = rec.kwargs["B"], rec.kwargs["T"], rec.kwargs["H"]
            xp = out[node.src[0]]
            same(node, rec.inputs["xproj"].reshape(xp.shape), "xproj", [(node.src[0], xp)])
            if rec.objects["whh_t"] is not r["whh_t"] or rec.objects.get("whh_planes") is not r["whh_p"]:
                fail(node, "called with another layer's recurrent weights")
            ref = bilstm_ref(rec.inputs["xproj"], cpu(r["whh_t"]), B, T, H)
            bounded(node, o, ref, torch.full_like(ref, sq.BILSTM_ATOL))
            out[node.name] = o
        else:
            raise ValueError(node.op)
    for node in graph:
        keys = [k for k in ratios if k == node.name or k.startswith(node.name + ":")]
        how = forms.get(node.name, "")
        if node.op == "seblock":
            how = f"{shapes[node.block]}: " + ", ".join(forms[k] for k in (node.block + ".conv1", node.block + ".conv2") if k in forms)
        report(f"[{tag}] {node.name:18s} {node.label:28s} {how:30s} " + "  ".join(f"err/bound{k[len(node.name):]} {ratios[k]:.3f}" for k in keys))
    return fails, ratios, stats, forms, shapes
