"""The recogniser's sequence kernels against float64, without the CNN: the attention decoders (csrc/attn_beam_mfma.hip,
csrc/attn_general.hip, behind the entry points of csrc/trba_kernels.hip), the BiLSTM recurrences (bilstm_kernel<H>, csrc/bilstm_mfma.hip),
se_residual, mean_over_h and seq_confidence, over the envelope DESIGN.md states (hidden 64..512, charsets <= 512 tokens, <= 64
frames and steps, beam <= 16 with beam x hidden <= 4096).

Decoder inputs are seeded encoder-like tensors (batch_H ~ N(0, 1.4^2), the spread of a real encoder output), proj_H = f32(i2h(batch_H))
evaluated in f64, and the decoder of synth.trba_state_dict (random weights: every decision an arg-max over near-Gaussian logits, the
most rounding-sensitive decoder we build).  The reference is the oracle's own Attention (oracle/trba_model.py) evaluated in float64 on
the GPU; its torch-CPU f32 evaluation measures what f32 arithmetic itself costs (the convention of test_gpu_f64.py).

(a) Teacher-forced replay: the oracle's AttentionCell + generator are run along the DEVICE's token path (greedy: SOS then the device's
    ids, every step; beam: the finalized best path, t < t_run, divided by the temperature).  A hypothesis's state is a function of its
    token prefix, so this also checks the beam-state reorder by back-pointer, finished-beam handling and beam_finalize's path walk.
    e_dev = max |device - f64| <= E_F32_FACTOR * e_f32 + 1e-7 * scale and e_dev <= E_REL_MAX * scale (blank column left out; it must
    equal the f32 value of -1e4, or -1e4 / tau in beam mode, exactly).
(b) Decisions.  Greedy: every device id is an arg-max of the f64 replay up to 2 e_dev, never the blank.  Beam: the oracle's f64 beam
    search on each row alone; on every row whose smallest top-k boundary gap and final best-vs-second score gap both exceed
    20 e_dev / tau, ids and finish step equal the oracle's; at least 75 % of the rows must be such rows.
(c) Batch-composition invariance: a row's outputs do not depend on which rows share its launch (bit-for-bit).
(d) Shapes outside the envelope return MSOCR_E_ARG from the C ABI (device buffers sized for the rejected shape).
(e) BiLSTM, (f) se_residual / mean_over_h / seq_confidence against f64."""
import numpy as np
import pytest
import torch

from attn_call import attn_decode
from manuscript_ocr_amd import synth

pytestmark = pytest.mark.gpu

SOS, EOS, PAD = 1, 2, 0
SEED = 20261015
B_DEF, T_DEF, STEPS_G, STEPS_B, ALPHA, TAU = 37, 13, 26, 25, 0.9, 1.7
BH_STD = 1.4  # standard deviation of the encoder output of synth.trba_state_dict weights on synthetic crops
# Recurrent / attention gain of the random decoder.  At synth's default x6 the decoder is chaotic: along one token path the torch-CPU
# f32 replay is 1.1e-4 of max|logit| away from f64 after 26 steps and 6.7e-2 after 64, so no f32 implementation could meet
# E_REL_MAX; at x4 it is 8.6e-7 / 3.0e-6 (measured on the H 256 / V 194 fixture) and the bound measures the kernels, not the fixture.
RNN_SCALE = 4.0

# Bounds of (a) and (b), set from the first MI355X run (every case prints its values with -s):
#   e_dev <= E_F32_FACTOR * e_f32: measured e_dev / e_f32 0.16 .. 0.95 over the 37-row cases; 1.92 (a VALU kernel since retired) and
#     2.09 (matrix cores) at B = 1, T = 48, where the maximum is over one row and both errors are a few ulp of max|logit| (6.0e-6
#     against 2.9e-6 at 13.95, whose ulp is 9.5e-7).
#   e_dev <= E_REL_MAX * max|logit|: measured 4.0e-7 .. 2.1e-6 (greedy, general kernel, H 320); the issue's ceiling was 1e-4.
#   decisive rows: measured 89 % .. 100 % per case at DECISIVE_FACTOR = 20.
E_F32_FACTOR = 4.0
E_REL_MAX = 1e-5
DECISIVE_FACTOR = 20.0
DECISIVE_MIN_FRACTION = 0.75
E_ARG = -1


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ fixtures shared by the cases
_SD, _DEC, _ORC = {}, {}, {}


def _sd(V, H, conf=False):
    """conf: the planted decoder of synth.trba_state_dict_confident (decisive rows where the random one has none)."""
    if (V, H, conf) not in _SD:
        _SD[(V, H, conf)] = (synth.trba_state_dict_confident(V, H, seed=SEED) if conf else
                             synth.trba_state_dict(V, H, seed=SEED, rnn_scale=RNN_SCALE))
    return _SD[(V, H, conf)]


def _decoder(V, H, conf=False, exact=False):
    """exact: without the split form of the per-step matrices (precision "fp32-exact"): the matrix-core beam kernel on exact-f32 MFMA."""
    from manuscript_ocr_amd.recognizers._trba.net import AttnDecoder
    if (V, H, conf, exact) not in _DEC:
        _DEC[(V, H, conf, exact)] = AttnDecoder(_sd(V, H, conf), V, H, step_split=False if exact else None)
    return _DEC[(V, H, conf, exact)]


def _kernel(monkeypatch, V, H, kernel, conf=False):
    """The decoder for a case's kernel choice: "auto" (what the routing picks for the shape), "exact" (the same without the split
    weights) or "valu" (the general kernel, csrc/attn_general.hip — the VALU decoder — even where the matrix-core kernels would take
    the shape: net.HOIST_CTX = False)."""
    from manuscript_ocr_amd.recognizers._trba import net
    monkeypatch.setattr(net, "HOIST_CTX", kernel != "valu")
    return _decoder(V, H, conf, exact=kernel == "exact")


def _oracle(V, H, blank, where, conf=False):
    """The oracle's Attention loaded with the `attn.*` weights: "f64" on the GPU, "f32" on the CPU."""
    from oracle import trba_model as otm
    if (V, H, where, conf) not in _ORC:
        att = otm.Attention(H, H, V, SOS, EOS, PAD, None)
        att.load_state_dict({k[5:]: v for k, v in _sd(V, H, conf).items() if k.startswith("attn.")}, strict=True)
        att.eval()
        _ORC[(V, H, where, conf)] = att.double().cuda() if where == "f64" else att
    att = _ORC[(V, H, where, conf)]
    att.blank_id = blank
    return att


def _inputs(B, T, H, V, conf=False):
    """batch_H (f32, seeded) and proj_H = f32(i2h(batch_H)) with i2h evaluated in f64."""
    g = torch.Generator().manual_seed(B * 1000003 + T * 1009 + H * 7 + V)
    bH = torch.randn(B, T, H, generator=g) * BH_STD
    w = _sd(V, H, conf)["attn.attention_cell.i2h.weight"].double()
    pH = (bH.double() @ w.t()).float()
    return bH.cuda(), pH.cuda()


def _replay(att, bH, tok_in):
    """Teacher-forced decode: the oracle's AttentionCell + generator (+ blank mask) along the given input tokens
    tok_in [B, S] (SOS, then the tokens the device emitted).  Returns logits [B, S, V] in att's dtype, on att's device."""
    B, S = tok_in.shape
    fd = bH.dtype
    hid = (torch.zeros(B, att.hidden_size, dtype=fd, device=bH.device), torch.zeros(B, att.hidden_size, dtype=fd, device=bH.device))
    tok_in = tok_in.to(bH.device)
    out = []
    with torch.no_grad():
        for s in range(S):
            hid = att.attention_cell(hid, bH, att._onehot(tok_in[:, s], fd))
            out.append(att._mask(att.generator(hid[0])))
    return torch.stack(out, 1)


def _replay_f32(att, bH, tok_in):
    """The f32 replay on the CPU in two evaluation orders: all rows in one batch, and row by row.  Two f32 evaluations of the same
    decode land at different distances from f64 (their rounding is amplified by different rows): on the random decoder the per-row
    one was 5.6x as far as the batched one in one case (H 256, beam 12).  The f32 yardstick is the farther of the two."""
    bH = bH.cpu()
    return [_replay(att, bH, tok_in), torch.cat([_replay(att, bH[b:b + 1], tok_in[b:b + 1]) for b in range(bH.shape[0])])]


def _errors(dev, r64, r32s, valid, blank):
    """max |dev - r64|, max over the f32 replays of max |r32 - r64|, and max |r64|, over the valid (row, step) entries and the
    non-blank columns."""
    cols = np.ones(dev.shape[-1], dtype=bool)
    if blank is not None:
        cols[blank] = False
    d = dev[valid][:, cols].astype(np.float64)
    f64 = r64[valid][:, cols]
    e_f32 = max(float(np.abs(r32[valid][:, cols].astype(np.float64) - f64).max()) for r32 in r32s)
    return float(np.abs(d - f64).max()), e_f32, float(np.abs(f64).max())


def _check_arith(what, e_dev, e_f32, scale):
    ratio = e_dev / max(e_f32, 1e-30)
    print(f"[seq-f64] {what}: e_dev {e_dev:.3e} = {e_dev / scale:.2e} of max|logit| {scale:.2f}, e_f32 {e_f32:.3e}, "
          f"e_dev / e_f32 {ratio:.2f}")
    assert e_dev <= E_F32_FACTOR * e_f32 + 1e-7 * scale, (what, e_dev, e_f32, ratio)
    assert e_dev <= E_REL_MAX * scale, (what, e_dev, scale)


# ------------------------------------------------------------------------------------------------ (a) + (b) greedy
GREEDY_CASES = [
    # (id, H, V, B, T, steps, kernel): see _kernel
    ("mfma-H256-V194", 256, 194, B_DEF, T_DEF, STEPS_G, "auto"),
    ("valu-H256-V194", 256, 194, B_DEF, T_DEF, STEPS_G, "valu"),
    ("mfma-V256-T48-B1", 256, 256, 1, 48, STEPS_G, "auto"),
    ("valu-V256-T48-B1", 256, 256, 1, 48, STEPS_G, "valu"),
    ("mfma-V256-T48-B70", 256, 256, 70, 48, STEPS_G, "auto"),
    ("valu-V256-T48-B70", 256, 256, 70, 48, STEPS_G, "valu"),
] + [(f"general-H{h}", h, 194, B_DEF, T_DEF, STEPS_G, "auto") for h in (64, 128, 192, 320, 384, 448, 512)] + [
    ("general-V257", 256, 257, B_DEF, T_DEF, STEPS_G, "auto"),
    ("general-T49", 256, 194, B_DEF, 49, STEPS_G, "auto"),
    ("general-H128-V512-T64-S64", 128, 512, B_DEF, 64, 64, "auto"),
]


def _greedy_case(monkeypatch, what, H, V, B, T, steps, kernel, blank):
    dec = _kernel(monkeypatch, V, H, kernel)
    bH, pH = _inputs(B, T, H, V)
    lg, ids = dec.greedy(bH, pH, steps - 1, SOS, EOS, blank)
    torch.cuda.synchronize()
    lg, ids = lg.cpu().numpy(), ids.cpu().numpy().astype(np.int64)
    assert lg.shape == (B, steps, V) and ids.shape == (B, steps)
    assert ((ids >= 0) & (ids < V)).all()
    tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), ids[:, :-1]], 1))
    r64 = _replay(_oracle(V, H, blank, "f64"), bH.double(), tok_in).cpu().numpy()
    r32 = [r.numpy() for r in _replay_f32(_oracle(V, H, blank, "f32"), bH, tok_in)]
    valid = np.ones((B, steps), dtype=bool)
    e_dev, e_f32, scale = _errors(lg, r64, r32, valid, blank)
    _check_arith(f"greedy {what}", e_dev, e_f32, scale)
    if blank is not None:
        assert (lg[..., blank] == np.float32(-1e4)).all()
        assert not (ids == blank).any()
        r64 = r64.copy()
        r64[..., blank] = -np.inf
    # (b) every decision is an arg-max of the f64 logits up to 2 e_dev (by induction over steps: the device's decode is the f64
    #     free-running decode wherever the margins exceed that)
    chosen = np.take_along_axis(r64, ids[..., None], -1)[..., 0]
    gap = r64.max(-1) - chosen
    print(f"[seq-f64] greedy {what}: largest f64 shortfall of a chosen token {gap.max():.3e} (allowed {2 * e_dev:.3e})")
    assert (gap <= 2 * e_dev).all(), (what, np.argwhere(gap > 2 * e_dev)[:8].tolist())


@pytest.mark.parametrize("what,H,V,B,T,steps,kernel", GREEDY_CASES, ids=[c[0] for c in GREEDY_CASES])
def test_greedy_decode_against_f64_replay(cuda, monkeypatch, what, H, V, B, T, steps, kernel):
    _greedy_case(monkeypatch, what, H, V, B, T, steps, kernel, None)


# ------------------------------------------------------------------------------------------------ (a) + (b) beam
BEAM_CASES = [
    # (id, H, V, K, T, steps, kernel): see _kernel
    ("mfma-split-hoisted", 256, 194, 8, T_DEF, STEPS_B, "auto"),
    ("mfma-exact-hoisted", 256, 194, 8, T_DEF, STEPS_B, "exact"),
    ("valu", 256, 194, 8, T_DEF, STEPS_B, "valu"),
    # T 48: phase (b) loops over more (crop, t) groups than one pass holds; V 256: every generator column and top-k slot is in use
    ("mfma-V256-T48", 256, 256, 8, 48, STEPS_B, "auto"),
    ("mfma-exact-V256-T48", 256, 256, 8, 48, STEPS_B, "exact"),
] + [(f"mfma-K{k}", 256, 194, k, T_DEF, STEPS_B, "auto") for k in (1, 2, 3, 5)] + [
    (f"general-K{k}", 256, 194, k, T_DEF, STEPS_B, "auto") for k in (9, 12, 16)] + [
    ("general-H64-K16", 64, 194, 16, T_DEF, STEPS_B, "auto"),
    ("general-H320-K12", 320, 194, 12, T_DEF, STEPS_B, "auto"),
    ("general-H448-K9", 448, 194, 9, T_DEF, STEPS_B, "auto"),
    ("general-H512-K8", 512, 194, 8, T_DEF, STEPS_B, "auto"),
    ("general-V512-K16-T64-S64-planted", 256, 512, 16, 64, 64, "auto"),  # random decoder: 0/37 decisive rows (16 of 8192 candidates)
]


def _beam_case(monkeypatch, what, H, V, K, T, steps, kernel, blank, alpha=ALPHA, tau=TAU):
    B, conf = B_DEF, what.endswith("planted")
    dec = _kernel(monkeypatch, V, H, kernel, conf)
    bH, pH = _inputs(B, T, H, V, conf)
    ws, fin, _ = dec.beam(bH, pH, steps, K, alpha, tau, SOS, EOS, blank)
    lg, ids = dec.beam_finalize(ws, B, steps, K, fin)  # every row its own chunk: t_run = its finish step
    torch.cuda.synchronize()
    trun, lg, ids = fin.cpu().numpy(), lg.cpu().numpy(), ids.cpu().numpy().astype(np.int64)
    assert ((trun >= 1) & (trun <= steps)).all()
    valid = np.arange(steps)[None, :] < trun[:, None]
    assert (ids[~valid] == -1).all(), "finalize writes -1 beyond t_run"
    assert ((ids[valid] >= 0) & (ids[valid] < V)).all()
    tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), np.where(ids[:, :-1] >= 0, ids[:, :-1], EOS)], 1))
    t_div = max(tau, 1e-6)
    r64 = _replay(_oracle(V, H, blank, "f64", conf), bH.double(), tok_in)
    r32 = _replay_f32(_oracle(V, H, blank, "f32", conf), bH, tok_in)
    if tau != 1.0:
        r64, r32 = r64 / t_div, [r / t_div for r in r32]
    r64, r32 = r64.cpu().numpy(), [r.numpy() for r in r32]
    e_dev, e_f32, scale = _errors(lg, r64, r32, valid, blank)
    _check_arith(f"beam {what}", e_dev, e_f32, scale)
    if blank is not None:
        bl = np.float32(-1e4) / np.float32(t_div) if tau != 1.0 else np.float32(-1e4)
        assert (lg[valid][:, blank] == bl).all()
        assert not (ids == blank).any()
    # (b) the oracle's f64 beam search, one row per call (its loop stops when that row's beams are all finished, as the device's
    #     fin_step does), with the margins of every decision it takes
    att = _oracle(V, H, blank, "f64", conf)
    delta = DECISIVE_FACTOR * e_dev / t_div
    decisive, bad = 0, []
    with torch.no_grad():
        for b in range(B):
            d = {}
            _, oid = att.beam(bH[b:b + 1].double(), steps, K, alpha, tau, diag=d)
            oid = oid[0].cpu().numpy()
            sc = np.sort(d["beam_scores"][0])[::-1]
            score_gap = sc[0] - sc[1] if K > 1 else np.inf
            bgap = np.nanmin(np.where(np.isnan(d["boundary_gap"][0]), -np.inf, d["boundary_gap"][0]))
            if min(bgap, score_gap) > delta:
                decisive += 1
                if not (len(oid) == trun[b] and np.array_equal(ids[b, :trun[b]], oid)):
                    bad.append((b, int(trun[b]), len(oid)))
    frac = decisive / B
    print(f"[seq-f64] beam {what}: decisive rows {decisive}/{B} ({frac:.0%}) at delta {delta:.2e}; t_run {trun.min()}..{trun.max()}")
    assert not bad, (what, bad)
    assert frac >= DECISIVE_MIN_FRACTION, f"degenerate fixture: {decisive}/{B} decisive rows ({what})"


@pytest.mark.parametrize("what,H,V,K,T,steps,kernel", BEAM_CASES, ids=[c[0] for c in BEAM_CASES])
def test_beam_decode_against_f64_replay_and_oracle(cuda, monkeypatch, what, H, V, K, T, steps, kernel):
    _beam_case(monkeypatch, what, H, V, K, T, steps, kernel, None)


@pytest.mark.parametrize("mode,what", [("greedy", "mfma"), ("greedy", "valu"), ("greedy", "general-H128"), ("beam", "mfma-K8"),
                                       ("beam", "valu-K8"), ("beam", "general-K12")])
def test_blank_id_is_masked(cuda, monkeypatch, mode, what):
    """blank_id = 3 (the reference sets one whenever the charset has <BLANK>): its logit is exactly -1e4 (/ tau), it is never emitted,
    and every other column still meets the f64 bounds.  Both kernel families mask it (attn_general.hip, attn_beam_mfma.hip)."""
    H = 128 if "H128" in what else 256
    kernel = "valu" if what.startswith("valu") else "auto"
    if mode == "greedy":
        _greedy_case(monkeypatch, f"{what} blank 3", H, 194, B_DEF, T_DEF, STEPS_G, kernel, 3)
    else:
        _beam_case(monkeypatch, f"{what} blank 3", 256, 194, 12 if "K12" in what else 8, T_DEF, STEPS_B, kernel, 3)


@pytest.mark.parametrize("K", [8, 12])
def test_beam_without_length_penalty_or_temperature(cuda, monkeypatch, K):
    """alpha = 0 (no length penalty: lp_dev = NULL) and temperature = 1 (no division) on the matrix-core (K 8) and general (K 12) kernels."""
    _beam_case(monkeypatch, f"K{K} alpha 0 tau 1", 256, 194, K, T_DEF, STEPS_B, "auto", None, alpha=0.0, tau=1.0)


# ------------------------------------------------------------------------------------------------ (c) batch composition
COMPOSITION_CASES = [
    ("greedy-mfma", "greedy", 256, 194, 8, "auto"),
    ("greedy-valu", "greedy", 256, 194, 8, "valu"),
    ("greedy-general", "greedy", 128, 194, 8, "auto"),
    ("beam-mfma", "beam", 256, 194, 8, "auto"),
    ("beam-valu", "beam", 256, 194, 8, "valu"),
    ("beam-general", "beam", 256, 194, 12, "auto"),
]


@pytest.mark.parametrize("what,mode,H,V,K,kernel", COMPOSITION_CASES, ids=[c[0] for c in COMPOSITION_CASES])
def test_decode_does_not_depend_on_batch_composition(cuda, monkeypatch, what, mode, H, V, K, kernel):
    """70 rows decoded as one batch, each row alone, and in a permuted order: every row's ids, logits (and finish step) bit-identical.
    The context gates are computed once for the 70 rows and every run gets its rows' slice (the GEMM producing them may pick another
    kernel for another row count; only the decode kernels are held to bit-equality).  Catches cross-row interference in the 32-row
    greedy and 4-row beam matrix-core workgroups."""
    B, T = 70, T_DEF
    dec = _kernel(monkeypatch, V, H, kernel)
    bH, pH = _inputs(B, T, H, V)
    cg = dec.ctx_gates(bH).view(B, -1) if H == 256 else None  # the general kernels take none

    def run(rows):
        idx = torch.as_tensor(rows, device=bH.device)
        b, p = bH[idx].contiguous(), pH[idx].contiguous()
        c = cg[idx].contiguous().view(len(rows) * T, -1) if cg is not None else None
        if mode == "greedy":
            lg, ids = dec.greedy(b, p, STEPS_G - 1, SOS, EOS, None, ctx_gates=c)
            return lg.cpu(), ids.cpu(), None
        ws, fin, _ = dec.beam(b, p, STEPS_B, K, ALPHA, TAU, SOS, EOS, None, ctx_gates=c)
        lg, ids = dec.beam_finalize(ws, len(rows), STEPS_B, K, fin)
        lg, fin = lg.cpu(), fin.cpu()
        lg[torch.arange(STEPS_B)[None, :] >= fin[:, None].long()] = 0.0  # finalize leaves the logits beyond t_run unwritten
        return lg, ids.cpu(), fin

    full = run(list(range(B)))
    perm = np.random.default_rng(5).permutation(B).tolist()
    permuted = run(perm)
    for j, b in enumerate(perm):
        for x, y in zip(full, permuted):
            if x is not None:
                assert torch.equal(x[b], y[j]), (what, "permuted", b)
    for b in range(B):
        alone = run([b])
        for x, y in zip(full, alone):
            if x is not None:
                assert torch.equal(x[b], y[0]), (what, "alone", b)


def test_se_residual_does_not_depend_on_batch_composition(cuda):
    """msocr_se_residual promises results independent of the batch composition (trba_kernels.hip: one workgroup size for every N)."""
    from manuscript_ocr_amd import ops
    for dt in (torch.float32, torch.bfloat16):
        x, idt, w1, w2 = _se_inputs(19, 4, 13, 512, 3)
        x, idt = x.to(dt).cuda(), idt.to(dt).cuda()
        w1, w2 = w1.float().cuda(), w2.float().cuda()
        full = ops.se_residual(x, idt, w1, w2)
        perm = torch.from_numpy(np.random.default_rng(2).permutation(19)).cuda()
        permuted = ops.se_residual(x[perm].contiguous(), idt[perm].contiguous(), w1, w2)
        assert torch.equal(full[perm], permuted), dt
        for n in range(19):
            assert torch.equal(full[n:n + 1], ops.se_residual(x[n:n + 1].contiguous(), idt[n:n + 1].contiguous(), w1, w2)), (dt, n)


# ------------------------------------------------------------------------------------------------ (d) envelope rejections
def _attn_buffers(B, T, H, V, steps, K):
    """Device buffers sized for the (rejected) shape: a kernel launched by a broken check runs on valid memory."""
    from manuscript_ocr_amd import _native as nat
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    bufs = {"bH": z(B, T, H), "pH": z(B, T, H), "ctx": z(B * T, 4 * H), "logits": z(B, steps, V),
            "ids": torch.zeros((B, steps), dtype=torch.int32, device="cuda"), "fin": torch.zeros((B,), dtype=torch.int32, device="cuda"),
            "ws": torch.zeros((max(nat.lib().msocr_attn_beam_workspace_bytes(B, steps, K, V), 16),), dtype=torch.uint8, device="cuda"),
            "lp": z(steps) + 1.0, "trun": torch.ones((B,), dtype=torch.int32, device="cuda")}
    w = {"h2h_wt": z(H, H), "h2h_b": z(H), "score_w": z(H), "wih_ctx_t": z(H, H, 4), "wih_tok": z(V, H, 4), "whh_t": z(H, H, 4),
         "b_gates": z(H, 4), "gen_wt": z(H, V), "gen_b": z(V)}
    aw = nat.AttnWeights()
    for k, t in w.items():
        setattr(aw, k, t.data_ptr())
    sp = {k: torch.zeros((nat.lib().msocr_attn_pack_split_elems(n),), dtype=torch.int16, device="cuda")
          for k, n in (("h2h_p", H), ("whh_p", 4 * H), ("gen_p", V))}
    asw = nat.AttnSplitWeights()
    for k, t in sp.items():
        setattr(asw, k, t.data_ptr())
    bufs["_keep"] = (w, sp)
    return bufs, aw, asw


def _greedy_rc(B, T, H, V, steps, sos=SOS, hoisted=False):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, 1)
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "logits_out": b["logits"], "ids_out": b["ids"]}
    if hoisted:
        bufs.update(ctx_gates=b["ctx"], ws=asw)
    rc = attn_decode(nat.ATTN_GREEDY, bufs, B=B, T=T, H=H, V=V, steps=steps, sos_id=sos, eos_id=EOS, blank_id=-1, stream=ops._stream())
    torch.cuda.synchronize()
    return rc


def _beam_rc(B, T, H, V, steps, K, sos=SOS, ctx=False):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, K)
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "lp": b["lp"], "fin_step_out": b["fin"], "workspace": b["ws"]}
    if ctx:
        bufs["ctx_gates"] = b["ctx"]
    rc = attn_decode(nat.ATTN_BEAM, bufs, B=B, T=T, H=H, V=V, steps=steps, beam=K, temperature=1.7, sos_id=sos, eos_id=EOS, blank_id=-1,
                     stream=ops._stream())
    torch.cuda.synchronize()
    return rc


def test_c_abi_rejects_shapes_outside_the_envelope(cuda):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    B = 2
    for H in (96, 576):
        assert _greedy_rc(B, T_DEF, H, 194, STEPS_G) == E_ARG, H
        assert _beam_rc(B, T_DEF, H, 194, STEPS_B, 8) == E_ARG, H
    assert _greedy_rc(B, T_DEF, 256, 513, STEPS_G) == E_ARG
    assert _beam_rc(B, T_DEF, 256, 513, STEPS_B, 8) == E_ARG
    assert _greedy_rc(B, 65, 256, 194, STEPS_G) == E_ARG
    assert _beam_rc(B, 65, 256, 194, STEPS_B, 8) == E_ARG
    assert _greedy_rc(B, T_DEF, 256, 194, 65) == E_ARG
    assert _beam_rc(B, T_DEF, 256, 194, 65, 8) == E_ARG
    assert _beam_rc(B, T_DEF, 256, 194, STEPS_B, 17) == E_ARG
    assert _beam_rc(B, T_DEF, 320, 194, STEPS_B, 13) == E_ARG   # 13 x 320 > 4096
    assert _beam_rc(B, T_DEF, 512, 194, STEPS_B, 9) == E_ARG    # 9 x 512 > 4096
    assert _greedy_rc(B, T_DEF, 256, 194, STEPS_G, sos=194) == E_ARG
    assert _beam_rc(B, T_DEF, 256, 194, STEPS_B, 8, sos=194) == E_ARG
    assert _greedy_rc(B, T_DEF, 128, 194, STEPS_G, hoisted=True) == E_ARG   # the matrix-core greedy kernel takes H 256 only
    assert _greedy_rc(B, T_DEF, 256, 257, STEPS_G, hoisted=True) == E_ARG
    assert _beam_rc(B, T_DEF, 256, 194, STEPS_B, 12, ctx=True) == E_ARG    # context gates on a general shape
    assert _beam_rc(B, T_DEF, 128, 194, STEPS_B, 8, ctx=True) == E_ARG
    b, _, _ = _attn_buffers(B, T_DEF, 256, 194, 65, 8)
    assert nat.lib().msocr_attn_beam_finalize(b["ws"].data_ptr(), B, 194, 65, 8, b["trun"].data_ptr(), b["logits"].data_ptr(),
                                              b["ids"].data_ptr(), None, 0, None, ops._stream()) == E_ARG
    # the shapes at the envelope's edge are accepted (same buffers, so a rejection above is the check, not the buffers)
    assert _greedy_rc(B, 64, 128, 512, 64) == 0
    assert _beam_rc(B, T_DEF, 512, 194, STEPS_B, 8) == 0
    # BiLSTM
    for H in (96, 576):
        xp = torch.zeros((B * T_DEF, 8 * H), device="cuda")
        whh = torch.zeros((2, H, H, 4), device="cuda")
        out = torch.zeros((B, T_DEF, 2 * H), device="cuda")
        assert nat.lib().msocr_bilstm_recurrent(xp.data_ptr(), whh.data_ptr(), B, T_DEF, H, out.data_ptr(), ops._stream()) == E_ARG
    for H in (128, 512):  # buffers also large enough for the H 256 kernel a broken check would launch
        xp = torch.zeros((B * T_DEF, 8 * max(H, 256)), device="cuda")
        planes = torch.zeros((2, nat.lib().msocr_attn_pack_split_elems(4 * max(H, 256))), dtype=torch.int16, device="cuda")
        out = torch.zeros((B, T_DEF, 2 * max(H, 256)), device="cuda")
        assert nat.lib().msocr_bilstm_recurrent_split(xp.data_ptr(), planes.data_ptr(), B, T_DEF, H, out.data_ptr(), ops._stream()) == E_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (e) BiLSTM
def _bilstm_problem(B, T, H, seed):
    """Random W_hh (PyTorch's init range x 3) and an f32 xproj [B][T][2][4H]; the f64 reference is a bidirectional nn.LSTM whose input
    weights select the direction's half of xproj exactly (identity blocks, zero bias)."""
    g = torch.Generator().manual_seed(seed)
    k = 3.0 / H ** 0.5
    whh = [(torch.rand(4 * H, H, generator=g) * 2 - 1) * k for _ in range(2)]
    xproj = torch.randn(B, T, 2, 4 * H, generator=g) * 2.0
    lstm = torch.nn.LSTM(8 * H, H, bidirectional=True, batch_first=True).double()
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, 4 * H, dtype=torch.float64)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        lstm.weight_hh_l0.copy_(whh[0].double())
        lstm.weight_hh_l0_reverse.copy_(whh[1].double())
        for n in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(lstm, n).zero_()
        ref, _ = lstm(xproj.double().reshape(B, T, 8 * H))
    il = lambda w: w.t().reshape(H, 4, H).permute(0, 2, 1).contiguous()  # [k][j][gate]
    whh_t = torch.stack([il(whh[0]), il(whh[1])])
    return xproj.reshape(B * T, 8 * H).contiguous(), whh_t, ref.numpy()


BILSTM_ATOL = 2e-5  # the bound of test_gpu_trba.py; measured 7.1e-8 .. 1.1e-6 (VALU, every H) and 1.8e-7 .. 1.1e-6 (split, H 256)


@pytest.mark.parametrize("H", [64, 128, 192, 256, 320, 384, 448, 512])
def test_bilstm_every_hidden_size_against_f64(cuda, H):
    """msocr_bilstm_recurrent for every template instance it dispatches, B in {1, 6} (6 leaves the second 4-row block ragged),
    T in {1, 13}; the existing 2e-5 absolute bound."""
    from manuscript_ocr_amd import ops
    for B in (1, 6):
        for T in (1, 13):
            xp, whh_t, ref = _bilstm_problem(B, T, H, H + 10 * B + T)
            got = ops.bilstm_recurrent(xp.cuda(), whh_t.cuda(), B, T, H).cpu().numpy()
            err = float(np.abs(got - ref).max())
            print(f"[seq-f64] bilstm H {H} B {B} T {T}: max err {err:.2e}")
            assert err < BILSTM_ATOL, (H, B, T, err)


@pytest.mark.parametrize("B", [1, 33, 70])
def test_bilstm_split_against_f64(cuda, B):
    """msocr_bilstm_recurrent_split (H 256, 32 crops per workgroup): one, one-and-a-bit and two-and-a-bit row blocks, T in {1, 13, 64}."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    H = 256
    for T in (1, 13, 64):
        xp, whh_t, ref = _bilstm_problem(B, T, H, 7 * B + T)
        n = nat.lib().msocr_attn_pack_split_elems(4 * H)
        packed = torch.empty((2, n), dtype=torch.int16)
        for d in (0, 1):
            assert nat.lib().msocr_attn_pack_split_host(whh_t[d].contiguous().data_ptr(), 4 * H, 1, packed[d].data_ptr()) == 0
        planes, xp_d = packed.cuda(), xp.cuda()
        out = torch.empty((B, T, 2 * H), dtype=torch.float32, device="cuda")
        nat.check(nat.lib().msocr_bilstm_recurrent_split(xp_d.data_ptr(), planes.data_ptr(), B, T, H, out.data_ptr(), ops._stream()),
                  "bilstm_recurrent_split")
        err = float(np.abs(out.cpu().numpy() - ref).max())
        print(f"[seq-f64] bilstm split B {B} T {T}: max err {err:.2e}")
        assert err < BILSTM_ATOL, (B, T, err)


# ------------------------------------------------------------------------------------------------ (f) se_residual, mean_over_h, seq_confidence
def _se_inputs(N, Hh, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x, idt = torch.randn(N, Hh, W, C, generator=g), torch.randn(N, Hh, W, C, generator=g)
    w1 = (torch.rand(C // 16, C, generator=g) * 2 - 1) / C ** 0.5 * 3
    w2 = (torch.rand(C, C // 16, generator=g) * 2 - 1) / (C // 16) ** 0.5 * 3
    return x, idt, w1, w2


def _se_ref(x, idt, w1, w2):
    x, idt, w1, w2 = x.double(), idt.double(), w1.double(), w2.double()
    gate = torch.sigmoid(torch.relu(x.mean((1, 2)) @ w1.t()) @ w2.t())
    return torch.relu(x * gate[:, None, None, :] + idt).numpy()


# f32: measured 3.2e-7 .. 4.3e-7 absolute at max|ref| 4.8 .. 5.8 (the issue's ceiling was 1e-5 of max(1, max|ref|)).  bf16: the output's
# own rounding (up to 2^-8 relative) plus 1e-5; measured within 1e-5 of the rounding term (the f32 arithmetic before it is exact enough).
SE_F32_RTOL = 5e-7
SE_BF16_U, SE_BF16_ABS = 2.0 ** -8, 1e-5  # bf16 se_residual: |dev - ref| <= 2^-8 |ref| + 1e-5 per element
MEAN_H_RTOL = 1e-6                       # mean_over_h, f32 and bf16 input: 1e-6 of max(1, max|ref|)


@pytest.mark.parametrize("N,Hh,W,C", [(37, 8, 25, 256), (37, 4, 13, 512), (3, 16, 64, 256), (2, 5, 7, 1024)])
def test_se_residual_against_f64(cuda, N, Hh, W, C):
    from manuscript_ocr_amd import ops
    x, idt, w1, w2 = _se_inputs(N, Hh, W, C, C + N)
    ref = _se_ref(x, idt, w1, w2)
    got = ops.se_residual(x.cuda(), idt.cuda(), w1.cuda(), w2.cuda()).cpu().numpy()
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"[seq-f64] se_residual f32 {(N, Hh, W, C)}: max err {err:.2e} (scale {scale:.2f})")
    assert err <= SE_F32_RTOL * max(1.0, scale), err
    xb, ib = x.bfloat16(), idt.bfloat16()
    refb = _se_ref(xb.float(), ib.float(), w1, w2)
    gotb = ops.se_residual(xb.cuda(), ib.cuda(), w1.cuda(), w2.cuda()).float().cpu().numpy()
    excess = np.abs(gotb - refb) - (SE_BF16_U * np.abs(refb) + SE_BF16_ABS)
    print(f"[seq-f64] se_residual bf16 {(N, Hh, W, C)}: max err {np.abs(gotb - refb).max():.2e}, worst excess over the bound {excess.max():.2e}")
    assert (excess <= 0).all(), float(excess.max())


@pytest.mark.parametrize("Hh", [1, 4, 8])
def test_mean_over_h_against_f64(cuda, Hh):
    """Bound 1e-6 of max(1, max|ref|); measured 0 (H 1), up to 6.3e-7 absolute (f32, H 8)."""
    from manuscript_ocr_amd import ops
    g = torch.Generator().manual_seed(Hh)
    x = torch.randn(3, Hh, 25, 512, generator=g) * 4
    for xd in (x, x.bfloat16()):
        ref = xd.double().mean(1).numpy()
        got = ops.mean_over_h(xd.cuda()).cpu().numpy()
        err = float(np.abs(got - ref).max())
        print(f"[seq-f64] mean_over_h H {Hh} {xd.dtype}: max err {err:.2e} (scale {float(np.abs(ref).max()):.2f})")
        assert err <= MEAN_H_RTOL * max(1.0, float(np.abs(ref).max())), (xd.dtype, err)


@pytest.mark.parametrize("V", [194, 512])
def test_seq_confidence_against_f64(cuda, V):
    """mean over t < t_run of exp(log_softmax(logits)[id]); t_run 0 gives 0.  Bound 1e-6 absolute; measured 1.2e-7 (V 194), 9.5e-8 (V 512)."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    B, steps = 40, 26
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, steps, V, generator=g) * 6
    ids = torch.randint(0, V, (B, steps), generator=g, dtype=torch.int32)
    ids[::3] = logits[::3].argmax(-1).int()  # rows of confident picks beside the random ones
    trun = torch.randint(2, steps, (B,), generator=g, dtype=torch.int32)
    trun[0], trun[1], trun[2], trun[3] = 0, 1, steps, steps
    conf = torch.empty(B, dtype=torch.float32, device="cuda")
    lg_d, ids_d, trun_d = logits.cuda(), ids.cuda(), trun.cuda()  # held: the kernel runs after this line returns
    nat.check(nat.lib().msocr_seq_confidence(lg_d.data_ptr(), ids_d.data_ptr(), trun_d.data_ptr(), B, V, steps, conf.data_ptr(),
                                             ops._stream()), "seq_confidence")
    lp = torch.log_softmax(logits.double(), -1)
    p = lp.gather(-1, ids.long()[..., None])[..., 0].exp()
    ref = np.array([p[b, :int(trun[b])].mean().item() if trun[b] > 0 else 0.0 for b in range(B)])
    err = float(np.abs(conf.cpu().numpy() - ref).max())
    print(f"[seq-f64] seq_confidence V {V}: max err {err:.2e}")
    assert float(conf[0]) == 0.0
    assert err <= 1e-6, err
