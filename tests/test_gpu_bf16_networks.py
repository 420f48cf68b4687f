"""precision="bf16" of both networks held to float64: the weight preparation, every layer of the real networks (teacher-forced), the
maps / features / batch_H end to end, and the public interface in this mode.  tests/bf16_replay.py holds the recorder, the graphs and
the references.

(1) Weight preparation.  Every entry of EastNet(sd, bf16).P and TrbaNet(sd, 194, 256, bf16).P against a float64 BatchNorm fold of the
    raw state dict, arranged as the reference network defines the layer ([Cout][KH][KW][Cin]; layer1.0.conv3d = [W3 | Wd] with bias
    b3 + bd; the stems unpacked from pack_stem_weight's layout, every padded element exactly zero).  The device weight lies within one
    bf16 ulp of bf16(fold64) everywhere and equals it on all but a share of the elements: at most 4x the largest share that an f32 fold
    followed by bf16 differs from an f64 fold followed by bf16 on the CPU, floor 1e-4 (FLIP_FLOOR); the share is computed when the
    test runs.  Measured, largest per-layer share / share over the network: EAST seed 20260128 6.1e-5 / 5.9e-6, seed 7 6.1e-5 / 7.3e-6;
    TRBA seed 5 3.1e-5 / 7.0e-6, seed 11 1.1e-5 / 5.6e-6 (about 2^-17 of the elements; the largest per-layer share is one element
    of a 16 384-element layer), so the allowed share is 2.4e-4; the device's weights differ on 6.1e-5 / 3.1e-5 / 1.1e-5 of a layer at
    most, the shares of the CPU's f32 fold.  Biases stay f32 (measured worst error / bound 0.81):
    within 4 * 2^-24 * (|beta| + |mean s| + |conv_bias s|) of the f64 value.  w9 / b9 and the SE weights equal the state dict's f32
    values.  The same check runs on networks built on the CPU (no kernel is involved) in the suite without a GPU.
(2) Layer-by-layer replay.  A recorder (monkeypatch on ops.*) stores every call's inputs and output; every layer's reference is computed
    in float64 from the DEVICE's recorded outputs of the layers that feed it and the device's own weight and bias, following the graph
    written down from the reference architecture (bf16_replay.east_graph / trba_graph); the recorded leaf calls must be exactly that
    graph, in order.  Bounds are the project's own, imported: convolutions and stems bound (c) of test_gpu_conv_f64.py on every output
    element (the stems against the TRUE 7x7 / 2 / 3 and 3x3 / 1 / 1 convolution of the recorded image with the unpacked taps, the
    kernel's input against the window view of the canvas built by its definition); normalize_u8 bit for bit; maxpool2d torch.equal;
    upsample2x_into and east_head the bounds of test_gpu_stream_f64.py; se_residual (with its gates) and mean_over_h the bf16 bounds
    of test_gpu_seq_f64.py part (f); every input a layer read must equal, bit for bit, the recorded output of the layer the graph
    names (so the right slice of cat1 / cat2 / cat3 and both halves of yx are held to the layers told to write there).  The f64
    references must not be degenerate: positive share >= 0.25 after every ReLU, score standard deviation > 0.01, gate standard
    deviation >= 0.03 in every SE block.
(3) End to end.  The device's maps, features and batch_H against the oracle network in float64; the yardstick is a bf16-storage
    emulation of the oracle on the CPU (bf16_replay.emul_east / emul_trba_cnn: weights rounded to bf16 after an f64 fold, the output of
    every folded convolution, ReLU, max-pool and upsample rounded to bf16), accumulating in f64 and in f32, e_emul the larger of the two
    distances from f64: e_dev <= test_gpu_f64.F64_FACTOR * e_emul, and e_dev within the percentages of the two older bf16 tests.
(4) EAST / TRBA / Pipeline constructed with precision="bf16": eager == hipGraph replay, alone == in a batch, the texts the oracle's f32
    Attention decodes from the device's batch_H, the decode's route without split weights.

First MI355X run (every figure is printed under -s).  Replay, error / bound over the five cases: normalize_u8, maxpool2d, mean_over_h
(H = 1) 0 (bit for bit); stems 0.946 .. 0.988; convolutions 0.352 .. 0.991; upsample2x_into 0.995; se_residual 0.988 .. 0.995, its gates
0.006 .. 0.010; east_head score 0.026 .. 0.033, geometry 0.098 .. 0.118 (round to nearest reaches the bf16 bounds; a truncating store
would read 2).  Smallest positive share after a ReLU 0.38 (EAST) / 0.43 (TRBA), score standard deviation 0.054 .. 0.068, gate
standard deviation 0.037 .. 0.139.  End to end, e_dev / e_emul (e_dev, emulation with f64 sums, with f32 sums, relative to
max(1, max|ref|)): EAST 64x96 seed 20260128 score 0.84 (4.5e-3, 5.3e-3, 5.0e-3), geometry 1.19 (7.1e-3, 5.6e-3, 6.0e-3); seed 7 score
1.31 (9.6e-3, 7.3e-3, 7.0e-3), geometry 1.03 (1.45e-2, 1.39e-2, 1.41e-2); 96x64 score 0.93 (5.9e-3, 6.3e-3, 4.9e-3), geometry 1.21
(8.0e-3, 6.6e-3, 5.8e-3); TRBA seed 5 features 1.05 (1.10e-2, 1.05e-2, 9.9e-3), batch_H 0.71 (6.9e-2, 9.7e-2, 8.0e-2); seed 11 features
1.04 (9.1e-3, 8.7e-3, 7.5e-3), batch_H 1.17 (1.47e-1, 1.03e-1, 1.26e-1).  The factor stays 2.0.  batch_H of seed 11 sits at 14.7 % of
max(1, max|ref|), just inside the older test's 15 %: the x6 recurrent weights of the synthetic state dict amplify the CNN's 0.9 %, and
the two legitimate emulations are 10 % and 13 % away themselves.

The 26 ReLU outputs of the recogniser's graph are the stem, conv0b, conv1 and the block output of the 11 SE blocks, out0 and out1."""
import copy
import os

import numpy as np
import pytest
import torch

import bf16_replay as br
from manuscript_ocr_amd import synth
from test_gpu_f64 import F64_FACTOR

gpu = pytest.mark.gpu

FLIP_FACTOR, FLIP_FLOOR = 4.0, 1e-4
POSITIVE_MIN, SCORE_STD_MIN, GATE_STD_MIN = 0.25, 0.01, 0.03
# the older bf16 tests' bounds (tests/test_gpu_east.py::test_east_forward_bf16_close, tests/test_gpu_trba.py::test_trba_bf16_cnn_close):
# they must hold here too and never bind
OLD_SCORE_ABS, OLD_GEO_REL, OLD_FEATURES_REL, OLD_BATCH_H_REL = 0.05, 0.05, 0.03, 0.15
EAST_CASES = [("64x96-seed20260128", 64, 96, 2, 20260128), ("64x96-seed7", 64, 96, 2, 7), ("96x64-seed20260128", 96, 64, 1, 20260128)]
TRBA_SEEDS = [5, 11]
CHARSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "manuscript_ocr_amd", "recognizers", "_trba",
                       "configs", "charset.txt")
CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_SD = {}


def _east_sd(seed):
    if ("east", seed) not in _SD:
        _SD["east", seed] = synth.east_state_dict(seed=seed)
    return _SD["east", seed]


def _trba_sd(seed):
    if ("trba", seed) not in _SD:
        _SD["trba", seed] = synth.trba_state_dict(194, 256, seed)
    return _SD["trba", seed]


def _east_pages(H, W, pages):
    return np.stack([synth.synth_page(31 + k, H, W)[0] for k in range(pages)])


def _trba_crops():
    return synth.synth_crops(14, 3, 32, 100)


def _x_trba(canv):
    return torch.from_numpy(((canv.astype(np.float32) - 127.5) * np.float32(1 / 127.5)).transpose(0, 3, 1, 2).copy())


# ================================================================================================ the CPU side of the yardsticks
def test_emulation_without_rounding_is_the_oracle_in_f64():
    """The emulation's own wiring: with the rounding off and f64 sums it is the oracle network in float64 (BatchNorm folded)."""
    from oracle import east_model as oem
    from oracle import imgproc
    from oracle import trba_model as otm
    sd = _east_sd(7)
    net = oem.EASTNet()
    net.load_state_dict(sd)
    net = net.eval().double()
    x = torch.from_numpy(imgproc.east_preprocess(_east_pages(64, 96, 1)[0], 96, 64)).double()
    with torch.no_grad():
        r = net(x)
    s, g = br.emul_east(sd, x, torch.float64, rounding=False)
    assert br.rel_distance(s, r["score"][:, 0]) <= 1e-12 and br.rel_distance(g, r["geometry"].permute(0, 2, 3, 1)) <= 1e-12
    tsd = _trba_sd(5)
    tnet = otm.TRBANet(194, 256)
    tnet.load_state_dict(tsd, strict=True)
    tnet = tnet.eval().double()
    xt = _x_trba(_trba_crops()[:1]).double()
    with torch.no_grad():
        f = tnet.cnn(xt).permute(0, 2, 3, 1)
    assert br.rel_distance(br.emul_trba_cnn(tsd, xt, torch.float64, rounding=False), f) <= 1e-12


_FLIPS = {}


def _flip_bound():
    """4x the largest share, over the synthetic state dicts and their layers, on which bf16(f32 fold) != bf16(f64 fold) on the CPU."""
    if not _FLIPS:
        for seed in (20260128, 7):
            _FLIPS["east", seed] = br.flip_share(_east_sd(seed), br.east_fold_table(), (7, 7), EAST_FUSED)
        for seed in TRBA_SEEDS:
            _FLIPS["trba", seed] = br.flip_share(_trba_sd(seed), br.trba_fold_table(_trba_sd(seed)), (3, 3))
        for k, (worst, overall) in _FLIPS.items():
            print(f"[bf16-weights] CPU f32 fold against f64 fold, {k}: largest per-layer share of differing bf16 elements {worst:.2e}, over the network {overall:.2e}")
    return max(FLIP_FACTOR * max(w for w, _ in _FLIPS.values()), FLIP_FLOOR)


EAST_FUSED = (("layer1.0.conv3d", "layer1.0.conv3", "layer1.0.down"),)


def _check_weights(P, sd, table, stem_k, cpad, fused, what):
    ref = br.folded_layers(sd, table, stem_k, fused)
    bound = _flip_bound()
    conv_keys = [k for k in P if not k.endswith(".se")]
    assert sorted(conv_keys) == sorted(ref), ("entries of P without a float64 fold, or folds without an entry", set(conv_keys) ^ set(ref))
    worst_share = worst_bias = 0.0
    for k in conv_keys:
        w, b = P[k][0].detach().cpu(), P[k][1].detach().cpu()
        w64, b64, mag = ref[k]
        assert w.dtype == torch.bfloat16 and b.dtype == torch.float32, (what, k, w.dtype, b.dtype)
        if k == "stem":
            w, padded = br.unpack_stem(w, stem_k, cpad)
            assert bool((br.bf16_bits(padded) == 0).all()), (what, k, "a padded element of the packed stem weight is not zero")
        assert tuple(w.shape) == tuple(w64.shape), (what, k, tuple(w.shape), tuple(w64.shape))
        d = br.bf16_ulp_distance(w, w64.to(torch.bfloat16))
        share = float((d != 0).double().mean())
        worst_share = max(worst_share, share)
        assert int(d.max()) <= 1, (what, k, f"a weight is {int(d.max())} bf16 ulp from bf16(fold64)")
        assert share <= bound, (what, k, f"{share:.2e} of the weights differ from bf16(fold64), allowed {bound:.2e}")
        eb = (b.double() - b64).abs()
        lim = 4 * br.U32 * mag
        worst_bias = max(worst_bias, float((eb / lim.clamp_min(1e-300)).max()))
        assert bool((eb <= lim).all()), (what, k, "bias", float((eb / lim.clamp_min(1e-300)).max()))
    print(f"[bf16-weights] {what}: {len(conv_keys)} layers, largest share of elements off bf16(fold64) {worst_share:.2e} (allowed {bound:.2e}), "
          f"worst bias error / bound {worst_bias:.3f}")


def _east_weights(device, seed):
    from manuscript_ocr_amd.detectors._east.net import EastNet
    sd = _east_sd(seed)
    net = EastNet(sd, torch.bfloat16, device=device)
    _check_weights(net.P, sd, br.east_fold_table(), (7, 7), 4, EAST_FUSED, f"EAST seed {seed} on {device}")
    w9 = torch.cat([sd["output_head.score_map.weight"].view(1, 32), sd["output_head.geo_map.weight"].view(8, 32)])
    b9 = torch.cat([sd["output_head.score_map.bias"].view(1), sd["output_head.geo_map.bias"].view(8)])
    assert net.w9.dtype == net.b9.dtype == torch.float32 and torch.equal(net.w9.cpu(), w9) and torch.equal(net.b9.cpu(), b9)


def _trba_weights(device, seed):
    from manuscript_ocr_amd.recognizers._trba.net import TrbaNet
    sd = _trba_sd(seed)
    net = TrbaNet(sd, 194, 256, torch.bfloat16, device=device)
    assert net.cpad == 8 and net.cin_pad == 32
    _check_weights(net.P, sd, br.trba_fold_table(sd), (3, 3), 8, (), f"TRBA seed {seed} on {device}")
    se = [k for k in net.P if k.endswith(".se")]
    assert len(se) == 11
    for k in se:
        for got, key in zip(net.P[k], ("se.fc.0.weight", "se.fc.2.weight")):
            assert got.dtype == torch.float32 and torch.equal(got.cpu(), sd[f"cnn.{k[:-3]}.{key}"]), k


@pytest.mark.parametrize("seed", [20260128, 7])
def test_east_weight_preparation_against_a_float64_fold_cpu(seed):
    _east_weights("cpu", seed)


@pytest.mark.parametrize("seed", TRBA_SEEDS)
def test_trba_weight_preparation_against_a_float64_fold_cpu(seed):
    _trba_weights("cpu", seed)


@gpu
@pytest.mark.parametrize("seed", [20260128, 7])
def test_east_weight_preparation_against_a_float64_fold(seed):
    _need_gpu()
    _east_weights("cuda", seed)


@gpu
@pytest.mark.parametrize("seed", TRBA_SEEDS)
def test_trba_weight_preparation_against_a_float64_fold(seed):
    _need_gpu()
    _trba_weights("cuda", seed)


# ================================================================================================ layer-by-layer replay
def _assert_replay(what, fails, stats, relu_outputs, se_blocks):
    assert len(stats.positive) == relu_outputs, (what, len(stats.positive))
    low = {k: v for k, v in stats.positive.items() if v < POSITIVE_MIN}
    assert not low, (what, "degenerate case: ReLU outputs with a positive share below 0.25 — reseed it", low)
    assert len(stats.gate_std) == se_blocks
    flat = {k: v for k, v in stats.gate_std.items() if v < GATE_STD_MIN}
    assert not flat, (what, "degenerate case: SE gates that hardly vary — reseed it", flat)
    assert not fails, f"{what}: {len(fails)} layers fail; the first in network order: {fails[0]}" + "".join("\n  " + f for f in fails[1:6])


@gpu
@pytest.mark.parametrize("name,H,W,pages,seed", EAST_CASES, ids=[c[0] for c in EAST_CASES])
def test_east_layer_by_layer_replay(monkeypatch, name, H, W, pages, seed):
    _need_gpu()
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd.detectors._east.net import EastNet
    net = EastNet(_east_sd(seed), torch.bfloat16)
    rec = br.Recorder(monkeypatch, ops, net.P)
    score, geo = net.forward(torch.from_numpy(_east_pages(H, W, pages)).cuda())
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert all(r.depth == 0 for r in rec.records), "EAST's forward nests no recorded call"
    graph = br.east_graph()
    fails, ratios, stats = br.replay(graph, rec.leaves(), net.P, head=(net.w9, net.b9))
    head = rec.leaves()[-1]
    assert torch.equal(head.output[0], score.cpu()) and torch.equal(head.output[1], geo.cpu())
    assert tuple(rec.leaves()[graph.index(next(n for n in graph if n.name == "layer4.2.conv3"))].shape[1:3]) == (H // 32, W // 32)
    print(f"[bf16-replay] EAST {name}: worst error / bound over {len(ratios)} checks {max(ratios.values()):.3f}; smallest positive share "
          f"{min(stats.positive.values()):.2f}, score std {stats.score_std:.3f}")
    assert stats.score_std > SCORE_STD_MIN, (name, "degenerate score map — reseed the case", stats.score_std)
    _assert_replay(f"EAST {name}", fails, stats, relu_outputs=57, se_blocks=0)


@gpu
@pytest.mark.parametrize("seed", TRBA_SEEDS)
def test_trba_layer_by_layer_replay(monkeypatch, seed):
    _need_gpu()
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd.recognizers._trba.net import TrbaNet
    net = TrbaNet(_trba_sd(seed), 194, 256, torch.bfloat16)
    rec = br.Recorder(monkeypatch, ops, net.P)
    f = net.cnn(torch.from_numpy(_trba_crops()).cuda())
    seq = ops.mean_over_h(f)
    torch.cuda.synchronize()
    monkeypatch.undo()
    nested = [r.label for r in rec.records if not r.leaf]
    assert nested == ["conv2d:conv0b"] + ["se_block"] * 11, ("conv2d(pool2=True) and the SE blocks are the calls that nest others", nested)
    assert [r.depth for r in rec.records if r.leaf].count(1) == 2 + 3 * 11
    graph = br.trba_graph()
    fails, ratios, stats = br.replay(graph, rec.leaves(), net.P)
    assert torch.equal(rec.leaves()[-1].output, seq.cpu()) and tuple(seq.shape) == (3, 13, 512)
    print(f"[bf16-replay] TRBA seed {seed}: worst error / bound over {len(ratios)} checks {max(ratios.values()):.3f}; smallest positive share "
          f"{min(stats.positive.values()):.2f}, gate std {min(stats.gate_std.values()):.3f} .. {max(stats.gate_std.values()):.3f}")
    _assert_replay(f"TRBA seed {seed}", fails, stats, relu_outputs=26, se_blocks=11)


# ================================================================================================ end to end against float64
def _arbitrate(what, dev, emul64, emul32, ref64):
    e_dev, e64, e32 = br.rel_distance(dev, ref64), br.rel_distance(emul64, ref64), br.rel_distance(emul32, ref64)
    e_emul = max(e64, e32)
    print(f"[bf16-e2e] {what}: device {e_dev:.3e}, emulation f64 sums {e64:.3e}, f32 sums {e32:.3e} (of max(1, max|ref|) = "
          f"{max(1.0, float(np.abs(np.asarray(ref64)).max())):.3g}), ratio {e_dev / e_emul:.2f}")
    return e_dev, e_emul


@gpu
@pytest.mark.parametrize("name,H,W,pages,seed", EAST_CASES, ids=[c[0] for c in EAST_CASES])
def test_east_end_to_end_against_f64_with_the_bf16_emulation_as_yardstick(name, H, W, pages, seed):
    _need_gpu()
    from manuscript_ocr_amd.detectors._east.net import EastNet
    from oracle import east_model as oem
    from oracle import imgproc
    sd = _east_sd(seed)
    pg = _east_pages(H, W, pages)
    x = torch.from_numpy(np.concatenate([imgproc.east_preprocess(p, W, H) for p in pg])).double()
    net64 = oem.EASTNet()
    net64.load_state_dict(sd)
    net64 = net64.eval().double()
    with torch.no_grad():
        r64 = net64(x)
    s64, g64 = r64["score"][:, 0].numpy(), r64["geometry"].permute(0, 2, 3, 1).numpy()
    (sa, ga), (sb, gb) = br.emul_east(sd, x, torch.float64), br.emul_east(sd, x, torch.float32)
    score, geo = EastNet(sd, torch.bfloat16).forward(torch.from_numpy(pg).cuda())
    es_d, es_e = _arbitrate(f"EAST {name} score", score.cpu().numpy(), sa.numpy(), sb.numpy(), s64)
    eg_d, eg_e = _arbitrate(f"EAST {name} geometry", geo.cpu().numpy(), ga.numpy(), gb.numpy(), g64)
    assert es_d <= F64_FACTOR * es_e, (es_d, es_e)
    assert eg_d <= F64_FACTOR * eg_e, (eg_d, eg_e)
    assert es_d < OLD_SCORE_ABS and eg_d < OLD_GEO_REL, (es_d, eg_d)


@gpu
@pytest.mark.parametrize("seed", TRBA_SEEDS)
def test_trba_end_to_end_against_f64_with_the_bf16_emulation_as_yardstick(seed):
    _need_gpu()
    from manuscript_ocr_amd.recognizers._trba.net import TrbaNet
    from oracle import trba_model as otm
    sd = _trba_sd(seed)
    net32 = otm.TRBANet(194, 256)
    net32.load_state_dict(sd, strict=True)
    net32.eval()
    net64 = copy.deepcopy(net32).double()
    canv = _trba_crops()
    x = _x_trba(canv).double()
    with torch.no_grad():
        f64_ = net64.cnn(x).permute(0, 2, 3, 1)
        h64 = net64.encode(x)
        fa, fb = br.emul_trba_cnn(sd, x, torch.float64), br.emul_trba_cnn(sd, x, torch.float32)
        ha, hb = net64.enc_rnn(fa.mean(1)), net32.enc_rnn(fb.float().mean(1))
    net = TrbaNet(sd, 194, 256, torch.bfloat16)
    cd = torch.from_numpy(canv).cuda()
    f_dev = net.cnn(cd).float().cpu().numpy()
    h_dev = net.encode(cd)[0].cpu().numpy()
    ef_d, ef_e = _arbitrate(f"TRBA seed {seed} features", f_dev, fa.numpy(), fb.numpy(), f64_.numpy())
    eh_d, eh_e = _arbitrate(f"TRBA seed {seed} batch_H", h_dev, ha.numpy(), hb.numpy(), h64.numpy())
    assert ef_d <= F64_FACTOR * ef_e, (ef_d, ef_e)
    assert eh_d <= F64_FACTOR * eh_e, (eh_d, eh_e)
    assert float(np.abs(f_dev - f64_.numpy()).max()) < OLD_FEATURES_REL * float(np.abs(f64_.numpy()).max())
    assert eh_d < OLD_BATCH_H_REL, eh_d


# ================================================================================================ the public interface in bf16
def _polys(res):
    return [w.polygon for w in res["page"].blocks[0].words]


@gpu
def test_east_bf16_public_interface():
    """EAST(precision="bf16"): eager == hipGraph replay over four rounds of fresh pages, a page alone == the page in a batch of three,
    the maps == EastNet(sd, bf16).forward on the same bytes, all bit for bit."""
    _need_gpu()
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._east.net import EastNet
    sd = _east_sd(20260128)
    H, W = 128, 160
    page = lambda s: synth.synth_page(s, H, W)[0]
    eager = EAST(state_dict=sd, target_size=(W, H), device="cuda", score_thresh=0.5, precision="bf16")
    graph = EAST(state_dict=sd, target_size=(W, H), device="cuda", score_thresh=0.5, precision="bf16", use_graphs=True)
    assert eager.model.dtype == graph.model.dtype == torch.bfloat16
    for rnd in range(4):  # 1st call warm-up (eager), 2nd captures + replays, later ones replay
        pages = [page(10 * rnd + k) for k in range(2)]
        a, b = eager.predict_batch(pages, return_maps=True), graph.predict_batch(pages, return_maps=True)
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["score_map"], rb["score_map"]) and np.array_equal(ra["geo_map"], rb["geo_map"])
            assert _polys(ra) == _polys(rb)
    pool = next(iter(graph._graphs.buckets.values()))
    assert pool.warm and len(pool.inst) == 2 and not any(i.busy for i in pool.inst)
    three = [page(50), page(51), page(52)]
    batch = eager.predict_batch(three, return_maps=True)
    alone = eager.predict_batch([three[1]], return_maps=True)[0]
    assert np.array_equal(alone["score_map"], batch[1]["score_map"]) and np.array_equal(alone["geo_map"], batch[1]["geo_map"])
    assert _polys(alone) == _polys(batch[1])
    assert alone["score_map"].std() > SCORE_STD_MIN
    score, geo = EastNet(sd, torch.bfloat16).forward(torch.from_numpy(np.stack(three)).cuda())
    for n, r in enumerate(batch):
        assert np.array_equal(r["score_map"], score[n].cpu().numpy())
        assert np.array_equal(r["geo_map"], geo[n].permute(2, 0, 1).contiguous().cpu().numpy())


@pytest.fixture(scope="module")
def trba_bf16():
    _need_gpu()
    from manuscript_ocr_amd.recognizers import TRBA
    from oracle import trba_model as otm
    sd = synth.trba_state_dict_confident(194, 256, seed=3)
    rec = TRBA(state_dict=sd, config=CFG, device="cuda", precision="bf16")
    ref = otm.TRBANet(194, 256)
    ref.load_state_dict(sd, strict=True)
    return rec, ref.eval(), otm


@gpu
@pytest.mark.parametrize("mode", ["greedy", "beam"])
def test_trba_bf16_predict_reads_what_the_oracle_decodes_from_the_device_encoder(trba_bf16, mode):
    """TRBA(precision="bf16").predict on 5 crops: the texts the oracle's f32 Attention decodes from the DEVICE's batch_H (planted
    decoder: the decisions carry margins); without split weights greedy runs on the general kernel and beam on the matrix-core
    kernel's exact-f32 form; one crop alone == the same crop in the batch, ids and logits bit for bit."""
    rec, ref, otm = trba_bf16
    model = rec.model
    assert model.dtype == torch.bfloat16 and model._asw is None and model.dec._asw is None
    crops = list(synth.synth_crops(27, 5, 32, 100))
    canv = torch.from_numpy(rec._canvases(crops)).cuda()
    batch_H, _ = model.encode(canv)
    T = batch_H.shape[1]
    assert model.dec._matrix_core(T) is False, "greedy without split weights: the general kernel"
    assert model.dec._matrix_core(T, 8) is True, "beam 8: the matrix-core kernel, exact-f32 form"
    itos, _ = otm.load_charset(CHARSET)
    with torch.no_grad():
        if mode == "greedy":
            lg, ids = ref.attn.greedy(batch_H.cpu(), max_len=25)
        else:
            lg, ids = ref.attn.beam(batch_H.cpu(), max_len=25, beam_size=8, alpha=0.9, temperature=1.7)
    exp = otm.texts_and_confidences(lg, ids, itos, 0, 2, None)
    got = rec.predict(crops, mode=mode)
    assert [r["text"] for r in got] == [e["text"] for e in exp]
    assert len({e["text"] for e in exp}) >= 3 and all(e["text"] for e in exp), "degenerate fixture: the texts do not vary"
    np.testing.assert_allclose([r["confidence"] for r in got], [e["confidence"] for e in exp], atol=1e-4)
    ids_b, trun_b, conf_b, lg_b = rec.recognize_canvases(canv, mode=mode, return_logits=True)
    ids_a, trun_a, conf_a, lg_a = rec.recognize_canvases(canv[2:3].contiguous(), mode=mode, return_logits=True)
    t = int(min(trun_a[0], trun_b[2]))
    assert t >= 2 and np.array_equal(np.asarray(ids_a)[0, :t], np.asarray(ids_b)[2, :t])
    assert np.array_equal(np.asarray(lg_a)[0, :t], np.asarray(lg_b)[2, :t])


def _bf16_pipe(use_graphs=False):
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA
    rec = TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda", precision="bf16", use_graphs=use_graphs)
    return Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(320, 224), device="cuda", precision="bf16"), rec)


def _key(p):
    return [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words]


@gpu
def test_pipeline_bf16_eager_graphs_and_sub_batches(monkeypatch):
    """Pipeline over EAST(precision="bf16") and TRBA(precision="bf16") on one synthetic page (injected maps, as test_gpu_nbest.py's
    fixtures): the same words, polygons and texts eagerly, on a replayed graph and with sub-batches; its boxes are EAST.predict_batch's."""
    _need_gpu()
    H, W = 224, 320
    pg, rects = synth.synth_page(41, H, W)
    score, geo = synth.synth_maps(rects, (H, W), (H // 4, W // 4), 41)
    mo = (torch.from_numpy(score[None]).cuda(), torch.from_numpy(geo[None]).cuda())
    pipe = _bf16_pipe()
    assert pipe.detector.model.dtype == pipe.recognizer.model.dtype == torch.bfloat16
    base = pipe.predict_batch([pg], _maps_override=mo)
    words = base[0].blocks[0].words
    assert len(words) >= 3 and len({w.text for w in words if w.text}) >= 2, "degenerate page"
    det = pipe.detector.predict_batch([pg], _maps_override=mo)[0]
    assert sorted(_polys(det)) == sorted(w.polygon for w in words)
    assert [_key(p) for p in pipe.predict_batch([pg], sub_batches=2, _maps_override=mo)] == [_key(p) for p in base]
    gpipe = _bf16_pipe(use_graphs=True)
    grec = gpipe.recognizer
    gpipe.stream_sets = 1  # one set of launch streams: consecutive calls land in the same graph bucket
    pages_dev = torch.from_numpy(pg[None]).cuda()  # graphs are keyed by the page tensor
    seen, finish = [], grec.recognize_finish

    def spy(handle, *a, **kw):
        seen.append(handle.graph_inst is not None)
        return finish(handle, *a, **kw)

    monkeypatch.setattr(grec, "recognize_finish", spy)
    first = gpipe.predict_batch([pg], pages_dev=pages_dev, _maps_override=mo)
    replayed = gpipe.predict_batch([pg], pages_dev=pages_dev, _maps_override=mo)
    assert seen == [False, True], seen
    assert [_key(p) for p in first] == [_key(p) for p in base] and [_key(p) for p in replayed] == [_key(p) for p in base]
