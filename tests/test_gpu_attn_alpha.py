"""The attention-weight output of the decode kernels (msocr_attn_decode with alpha_out, csrc/trba_kernels.hip: attn_beam_mfma_alpha.hip,
attn_general.hip, attn_beam_finalize_kernel) and msocr_seq_char_details, against float64.

Fixtures are those of test_gpu_seq_f64.py (copied, not imported): the decoder of synth.trba_state_dict(V, H, seed, rnn_scale=4.0),
batch_H ~ N(0, 1.4^2), proj_H = f32(i2h(batch_H)) with i2h in f64, SOS / EOS / PAD = 1 / 2 / 0, length penalty 0.9, temperature 1.7.
The reference is the oracle's AttentionCell replayed along the DEVICE's token path (greedy: SOS, then the device's ids; beam: the
finalized path for t < t_run): before every cell step softmax_t(score(tanh(i2h(bH) + h2h(h)))) is formed from the cell's own
submodules, in f64 on the GPU and in torch-CPU f32 in two evaluation orders (all rows at once, row by row); the farther f32 one is
the yardstick.

(1) parity: e_dev = max |alpha_dev - alpha_f64| <= E_F32_FACTOR * e_f32 + 1e-7 and e_dev <= E_REL_MAX (a probability's scale is 1);
    the factor and the cap are test_gpu_seq_f64.py's own.  On the CPU e_f32 of these fixtures is 3.4e-7 .. 6.1e-7 (cases a, b, d), so
    the first bound is about 1.5e-6 .. 2.5e-6 and the cap does not decide.
(2) every stored row sums to 1 within 64 * 2^-24.
(3) no stray writes: the alpha buffers sit inside larger sentinel-filled tensors whose guards must be intact; beam rows t >= t_run
    are exactly zero after finalize; the beam cases run with two chunks and the chunked early exit, and hold rows with t_run < steps.
(4) off means off: logits, ids and fin_step with the output on are bit-identical to the plain entry points.
(5) msocr_seq_char_details against numpy f64 of the device's own inputs.
(6) a descriptor with alpha_out is refused where the plain one is, and for a misaligned alpha workspace.

Measured on MI355X (pytest -s prints them): e_dev, e_f32, e_dev / e_f32 per case
  a-mfma-greedy              4.2e-7  1.24e-6  0.34        d-general-greedy           1.9e-7  3.9e-7  0.49
  b-mfma-beam-split          2.6e-7  5.2e-7   0.49        e-general-beam-K12         2.9e-7  3.4e-7  0.86
  b-mfma-beam-exact          2.7e-7  5.2e-7   0.53        f-general-beam-mfma-shape  3.1e-7  6.5e-7  0.48
  c-mfma-beam-K5             7.5e-7  1.49e-6  0.51
so the first bound (1.4e-6 .. 6.0e-6 here) decides everywhere and the cap of 1e-5 nowhere; row sums within 3.2e-7 of 1 (bound
3.8e-6); seq_char_details: prob within 2.6e-7, centre within 4.7e-7 (T 13) / 1.9e-6 (T 64, half an ulp of a centre near 32).
"""
import numpy as np
import pytest
import torch

from attn_call import attn_decode
from manuscript_ocr_amd import synth

pytestmark = pytest.mark.gpu

SOS, EOS, PAD = 1, 2, 0
SEED = 20261015
ALPHA, TAU = 0.9, 1.7
BH_STD = 1.4
RNN_SCALE = 4.0
E_F32_FACTOR = 4.0
E_REL_MAX = 1e-5
E_ARG = -1
SENT = -7.0     # no attention weight is negative
GUARD = 256     # floats on either side of a guarded buffer (a multiple of 4: the buffer stays 16-byte aligned)
ROW_SUM_TOL = 64 * 2.0 ** -24

CASES = {
    # id: (mode, kernel, B, T, H, V, steps, beam); kernel as test_gpu_seq_f64._kernel: "auto" (what the routing picks), "exact" (no
    # split weights: exact-f32 MFMA) or "valu" (the general kernel at a matrix-core shape: net.HOIST_CTX = False)
    "a-mfma-greedy": ("greedy", "auto", 37, 13, 256, 194, 26, 0),        # 32 crops per workgroup: one full, one partial
    "b-mfma-beam-split": ("beam", "auto", 5, 48, 256, 194, 25, 8),       # 4 crops x 8 slots per workgroup: one full, one partial
    "b-mfma-beam-exact": ("beam", "exact", 5, 48, 256, 194, 25, 8),
    "c-mfma-beam-K5": ("beam", "auto", 37, 13, 256, 194, 25, 5),         # unused slots
    "d-general-greedy": ("greedy", "auto", 3, 64, 128, 400, 41, 0),
    "e-general-beam-K12": ("beam", "auto", 3, 13, 128, 400, 25, 12),
    "f-general-beam-mfma-shape": ("beam", "valu", 5, 13, 256, 194, 25, 8),
}
MATRIX_CORE = {"a-mfma-greedy", "b-mfma-beam-split", "b-mfma-beam-exact", "c-mfma-beam-K5"}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ fixtures (test_gpu_seq_f64.py's)
_SD, _DEC, _ORC, _RUN = {}, {}, {}, {}


def _sd(V, H):
    if (V, H) not in _SD:
        _SD[(V, H)] = synth.trba_state_dict(V, H, seed=SEED, rnn_scale=RNN_SCALE)
    return _SD[(V, H)]


def _decoder(V, H, exact=False):
    from manuscript_ocr_amd.recognizers._trba.net import AttnDecoder
    if (V, H, exact) not in _DEC:
        _DEC[(V, H, exact)] = AttnDecoder(_sd(V, H), V, H, step_split=False if exact else None)
    return _DEC[(V, H, exact)]


def _oracle(V, H, where):
    """The oracle's Attention loaded with the `attn.*` weights: "f64" on the GPU, "f32" on the CPU."""
    from oracle import trba_model as otm
    if (V, H, where) not in _ORC:
        att = otm.Attention(H, H, V, SOS, EOS, PAD, None)
        att.load_state_dict({k[5:]: v for k, v in _sd(V, H).items() if k.startswith("attn.")}, strict=True)
        att.eval()
        _ORC[(V, H, where)] = att.double().cuda() if where == "f64" else att
    return _ORC[(V, H, where)]


def _inputs(B, T, H, V):
    g = torch.Generator().manual_seed(B * 1000003 + T * 1009 + H * 7 + V)
    bH = torch.randn(B, T, H, generator=g) * BH_STD
    w = _sd(V, H)["attn.attention_cell.i2h.weight"].double()
    pH = (bH.double() @ w.t()).float()
    return bH.cuda(), pH.cuda()


def _replay_alpha(att, bH, tok_in):
    """Teacher-forced decode along tok_in [B, S]: the attention weights the oracle's AttentionCell forms before every cell step, from
    its own submodules (model.py:36-40) -> [B, S, T] in att's dtype."""
    B, S = tok_in.shape
    fd, cell = bH.dtype, att.attention_cell
    hid = (torch.zeros(B, att.hidden_size, dtype=fd, device=bH.device), torch.zeros(B, att.hidden_size, dtype=fd, device=bH.device))
    tok_in = tok_in.to(bH.device)
    out = []
    with torch.no_grad():
        for s in range(S):
            e = cell.score(torch.tanh(cell.i2h(bH) + cell.h2h(hid[0]).unsqueeze(1)))
            out.append(torch.softmax(e, dim=1)[..., 0])
            hid = cell(hid, bH, att._onehot(tok_in[:, s], fd))
    return torch.stack(out, 1)


def _replay_alpha_f32(att, bH, tok_in):
    """The f32 replay on the CPU in the two evaluation orders of test_gpu_seq_f64._replay_f32: all rows in one batch, and row by row."""
    bH = bH.cpu()
    return [_replay_alpha(att, bH, tok_in), torch.cat([_replay_alpha(att, bH[b:b + 1], tok_in[b:b + 1]) for b in range(bH.shape[0])])]


def _guarded(*shape):
    """A sentinel-filled flat tensor with a view of `shape` in its middle, GUARD floats on either side."""
    n = int(np.prod(shape))
    big = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    return big, big[GUARD:GUARD + n].view(*shape)


def _guards_intact(big):
    h = big.cpu().numpy()
    return bool((h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all())


def _run(name):
    """One case, computed once and shared (never modified): the device's outputs with the alpha output on and off, the replays."""
    if name in _RUN:
        return _RUN[name]
    from manuscript_ocr_amd.recognizers._trba import net
    mode, kernel, B, T, H, V, steps, K = CASES[name]
    hoist0 = net.HOIST_CTX
    net.HOIST_CTX = kernel != "valu"
    try:
        dec = _decoder(V, H, exact=kernel == "exact")
        assert (dec._matrix_core(T, K if mode == "beam" else None)) == (name in MATRIX_CORE), "the case must run on the kernel it names"
        bH, pH = _inputs(B, T, H, V)
        r = {"B": B, "T": T, "steps": steps, "K": K, "mode": mode}
        if mode == "greedy":
            big, view = _guarded(B, steps, T)
            lg, ids, al = dec.greedy(bH, pH, steps - 1, SOS, EOS, None, want_alpha=True, alpha_out=view)
            lg0, ids0 = dec.greedy(bH, pH, steps - 1, SOS, EOS, None)
            torch.cuda.synchronize()
            assert al.data_ptr() == view.data_ptr()
            r.update(bigs=[big], alpha=al.cpu().numpy(), on=(lg.cpu(), ids.cpu()), off=(lg0.cpu(), ids0.cpu()))
            ids_h = ids.cpu().numpy().astype(np.int64)
            r["valid"] = np.ones((B, steps), dtype=bool)
            r["trun"] = np.full(B, steps)
            tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), ids_h[:, :-1]], 1))
        else:
            # two chunks, chosen from a plain run's finish steps: the rows that finish before `steps`, and the others (a chunk stops
            # at its slowest row, so the first chunk's t_run is < steps); then the decode with the chunked early exit and the output on
            _, fin_plain, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None)
            early = fin_plain.cpu().numpy() < steps
            if early.all() or not early.any():
                early = np.arange(B) < B // 2
            cid = np.where(early, 0, 1).astype(np.int32)
            csz = np.array([int(early.sum()), int((~early).sum())], dtype=np.int32)

            def chunks():
                return (torch.from_numpy(cid).cuda(), torch.from_numpy(csz).cuda(), torch.zeros(4, dtype=torch.int32, device="cuda"))

            big_ws, view_ws = _guarded(B, steps, K, T)
            big_out, view_out = _guarded(B, steps, T)
            ws, fin, _, aws = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, chunks(), want_alpha=True, alpha_ws=view_ws)
            torch.cuda.synchronize()
            fin_h = fin.cpu().numpy()
            trun = np.where(early, fin_h[early].max(), fin_h[~early].max()).astype(np.int32)
            trun_d = torch.from_numpy(trun).cuda()
            lg, ids, al = dec.beam_finalize(ws, B, steps, K, trun_d, alpha_ws=aws, alpha_out=view_out)
            ws0, fin0, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, chunks())
            lg0, ids0 = dec.beam_finalize(ws0, B, steps, K, trun_d)
            torch.cuda.synchronize()
            valid = np.arange(steps)[None, :] < trun[:, None]
            vt = torch.from_numpy(valid)
            lg, lg0 = lg.cpu(), lg0.cpu()
            lg[~vt], lg0[~vt] = 0.0, 0.0  # finalize leaves the logits beyond t_run unwritten
            r.update(bigs=[big_ws, big_out], alpha=al.cpu().numpy(), alpha_ws=aws.cpu().numpy(), on=(lg, ids.cpu(), fin.cpu()),
                     off=(lg0, ids0.cpu(), fin0.cpu()), valid=valid, trun=trun)
            ids_h = ids.cpu().numpy().astype(np.int64)
            assert (ids_h[~valid] == -1).all() and ((ids_h[valid] >= 0) & (ids_h[valid] < V)).all()
            tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), np.where(ids_h[:, :-1] >= 0, ids_h[:, :-1], EOS)], 1))
        r["a64"] = _replay_alpha(_oracle(V, H, "f64"), bH.double(), tok_in).cpu().numpy()
        r["a32"] = [a.numpy() for a in _replay_alpha_f32(_oracle(V, H, "f32"), bH, tok_in)]
    finally:
        net.HOIST_CTX = hoist0
    _RUN[name] = r
    return r


# ------------------------------------------------------------------------------------------------ (1) parity
@pytest.mark.parametrize("name", list(CASES))
def test_alpha_against_f64_replay(cuda, name):
    r = _run(name)
    v = r["valid"]
    a64 = r["a64"][v]
    e_dev = float(np.abs(r["alpha"][v].astype(np.float64) - a64).max())
    e_f32 = max(float(np.abs(a[v].astype(np.float64) - a64).max()) for a in r["a32"])
    print(f"[attn-alpha] {name}: e_dev {e_dev:.3e}, e_f32 {e_f32:.3e}, e_dev / e_f32 {e_dev / max(e_f32, 1e-30):.2f}; "
          f"t_run {r['trun'].min()}..{r['trun'].max()}")
    assert r["alpha"].shape == (r["B"], r["steps"], r["T"])
    assert e_dev <= E_F32_FACTOR * e_f32 + 1e-7, (name, e_dev, e_f32)
    assert e_dev <= E_REL_MAX, (name, e_dev)


# ------------------------------------------------------------------------------------------------ (2) rows sum to 1
@pytest.mark.parametrize("name", list(CASES))
def test_alpha_rows_sum_to_one(cuda, name):
    r = _run(name)
    a = r["alpha"][r["valid"]].astype(np.float64)
    assert ((a >= 0) & (a <= 1)).all()
    err = float(np.abs(a.sum(-1) - 1.0).max())
    print(f"[attn-alpha] {name}: max |row sum - 1| {err:.2e} (bound {ROW_SUM_TOL:.2e})")
    assert err <= ROW_SUM_TOL, (name, err)
    if r["mode"] == "beam":  # every slot the kernel stored, not only the best path's
        ws = r["alpha_ws"].astype(np.float64)
        stored = (ws != SENT).all(-1)
        assert ((ws != SENT).any(-1) == stored).all(), "a row of the trace is stored whole or not at all"
        assert stored[r["valid"]].all(), "every slot of every step t < t_run is stored"
        assert float(np.abs(ws[stored].sum(-1) - 1.0).max()) <= ROW_SUM_TOL


# ------------------------------------------------------------------------------------------------ (3) no stray writes
@pytest.mark.parametrize("name", list(CASES))
def test_alpha_no_stray_writes(cuda, name):
    r = _run(name)
    for big in r["bigs"]:
        assert _guards_intact(big), name
    if r["mode"] == "beam":
        assert (r["trun"] < r["steps"]).any(), "the case must hold rows with t_run < steps"
        assert (r["alpha"][~r["valid"]] == 0.0).all(), "finalize writes zeros for t >= t_run"
        assert (r["alpha"] != SENT).all()
    else:
        assert (r["alpha"] != SENT).all(), "greedy: every step written"


# ------------------------------------------------------------------------------------------------ (4) off means off
@pytest.mark.parametrize("name", list(CASES))
def test_alpha_output_changes_no_other_output(cuda, name):
    r = _run(name)
    for x, y in zip(r["on"], r["off"]):
        assert x.dtype == y.dtype and torch.equal(x, y), name


# ------------------------------------------------------------------------------------------------ (5) seq_char_details
@pytest.mark.parametrize("V,T", [(194, 13), (512, 64)])
def test_seq_char_details_against_f64(cuda, V, T):
    """Inputs as test_seq_confidence_against_f64 (B 40, 26 steps, t_run including 0, 1 and steps) plus seeded softmax rows as the
    weights.  prob within 1e-6 (that test's bound); centre within T * 2^-23 (the f32 rounding of a sum <= T is T * 2^-24, the kernel
    sums in f64); peak equal wherever the two largest weights differ by more than 1e-6, and the smaller index on planted exact ties;
    0, 0, -1 beyond t_run; the mean of prob[: t_run] is msocr_seq_confidence's value within 64 * 2^-24."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    B, steps = 40, 26
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, steps, V, generator=g) * 6
    ids = torch.randint(0, V, (B, steps), generator=g, dtype=torch.int32)
    ids[::3] = logits[::3].argmax(-1).int()
    trun = torch.randint(2, steps, (B,), generator=g, dtype=torch.int32)
    trun[0], trun[1], trun[2], trun[3] = 0, 1, steps, steps
    alpha = torch.softmax(torch.randn(B, steps, T, generator=g) * 3, -1)
    alpha[2, :, :] = 0.0        # exact ties: the smaller index wins
    alpha[2, :, 5], alpha[2, :, 9] = 0.5, 0.5
    alpha[3, :, :] = 1.0 / T if T == 64 else 0.0
    if T != 64:
        alpha[3, :, T - 1], alpha[3, :, 0] = 0.5, 0.5
    dev = lambda t: t.cuda()
    lg_d, ids_d, al_d, tr_d = dev(logits), dev(ids), dev(alpha), dev(trun)
    prob = torch.full((B, steps), SENT, device="cuda")
    centre = torch.full((B, steps), SENT, device="cuda")
    peak = torch.full((B, steps), -9, dtype=torch.int32, device="cuda")
    conf = torch.empty(B, dtype=torch.float32, device="cuda")
    nat.check(nat.lib().msocr_seq_char_details(lg_d.data_ptr(), ids_d.data_ptr(), al_d.data_ptr(), tr_d.data_ptr(), B, V, steps, T,
                                               prob.data_ptr(), centre.data_ptr(), peak.data_ptr(), ops._stream()), "seq_char_details")
    nat.check(nat.lib().msocr_seq_confidence(lg_d.data_ptr(), ids_d.data_ptr(), tr_d.data_ptr(), B, V, steps, conf.data_ptr(),
                                             ops._stream()), "seq_confidence")
    torch.cuda.synchronize()
    prob, centre, peak, conf = prob.cpu().numpy(), centre.cpu().numpy(), peak.cpu().numpy(), conf.cpu().numpy()
    tr = trun.numpy()
    valid = np.arange(steps)[None, :] < tr[:, None]
    assert (prob[~valid] == 0).all() and (centre[~valid] == 0).all() and (peak[~valid] == -1).all()
    p64 = torch.log_softmax(logits.double(), -1).gather(-1, ids.long()[..., None])[..., 0].exp().numpy()
    a64 = alpha.double().numpy()
    c64 = (a64 * (np.arange(T) + 0.5)).sum(-1)
    e_p = float(np.abs(prob - p64)[valid].max())
    e_c = float(np.abs(centre - c64)[valid].max())
    print(f"[attn-alpha] seq_char_details V {V} T {T}: prob err {e_p:.2e} (1e-6), centre err {e_c:.2e} ({T * 2.0 ** -23:.2e})")
    assert e_p <= 1e-6 and e_c <= T * 2.0 ** -23
    top2 = np.sort(a64, -1)[..., -2:]
    clear = valid & (top2[..., 1] - top2[..., 0] > 1e-6)
    assert clear.sum() > 0.8 * valid.sum()
    assert (peak[clear] == a64.argmax(-1)[clear]).all()
    assert ((peak[valid] >= 0) & (peak[valid] < T)).all()
    assert (peak[2][valid[2]] == 5).all() and (peak[3][valid[3]] == 0).all()  # ties
    for b in range(B):
        mean = float(prob[b, :tr[b]].astype(np.float64).mean()) if tr[b] > 0 else 0.0
        assert abs(mean - float(conf[b])) <= 64 * 2.0 ** -24, (b, mean, float(conf[b]))


# ------------------------------------------------------------------------------------------------ (6) ABI rejections
def _attn_buffers(B, T, H, V, steps, K):
    """Device buffers sized for the (rejected) shape, the alpha buffers sentinel-filled: a kernel launched by a broken check runs on
    valid memory and leaves a trace."""
    from manuscript_ocr_amd import _native as nat
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    bufs = {"bH": z(B, T, H), "pH": z(B, T, H), "ctx": z(B * T, 4 * H), "logits": z(B, steps, V),
            "ids": torch.zeros((B, steps), dtype=torch.int32, device="cuda"), "fin": torch.zeros((B,), dtype=torch.int32, device="cuda"),
            "ws": torch.zeros((max(nat.lib().msocr_attn_beam_workspace_bytes(B, steps, K, V), 16),), dtype=torch.uint8, device="cuda"),
            "lp": z(steps) + 1.0, "trun": torch.ones((B,), dtype=torch.int32, device="cuda"),
            "alpha_ws": torch.full((B * steps * K * T + 4,), SENT, device="cuda"), "alpha": torch.full((B * steps * T + 4,), SENT, device="cuda")}
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


def _untouched(b):
    torch.cuda.synchronize()
    return bool((b["alpha_ws"] == SENT).all()) and bool((b["alpha"] == SENT).all())


def _greedy_rc(B, T, H, V, steps, sos=SOS, hoisted=False):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, 1)
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "logits_out": b["logits"], "ids_out": b["ids"], "alpha_out": b["alpha"]}
    if hoisted:
        bufs.update(ctx_gates=b["ctx"], ws=asw)
    rc = attn_decode(nat.ATTN_GREEDY, bufs, B=B, T=T, H=H, V=V, steps=steps, sos_id=sos, eos_id=EOS, blank_id=-1, stream=ops._stream())
    assert rc == 0 or _untouched(b)
    return rc


def _beam_rc(B, T, H, V, steps, K, sos=SOS, ctx=False, alpha_ws="ok"):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, K)
    ap = {"ok": b["alpha_ws"].data_ptr(), "misaligned": b["alpha_ws"].data_ptr() + 4}[alpha_ws]
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "lp": b["lp"], "fin_step_out": b["fin"], "workspace": b["ws"], "alpha_out": ap}
    if ctx:
        bufs["ctx_gates"] = b["ctx"]
    rc = attn_decode(nat.ATTN_BEAM, bufs, B=B, T=T, H=H, V=V, steps=steps, beam=K, temperature=1.7, sos_id=sos, eos_id=EOS, blank_id=-1,
                     stream=ops._stream())
    assert rc == 0 or _untouched(b)
    return rc


def test_alpha_entry_points_reject_what_the_plain_ones_reject(cuda):
    """The shapes of test_c_abi_rejects_shapes_outside_the_envelope through descriptors with alpha_out, plus a misaligned alpha
    workspace and the finalize step's alpha arguments; buffers sized for the rejected shape, the alpha buffers' sentinels untouched after every rejection."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    B, T_DEF, STEPS_G, STEPS_B = 2, 13, 26, 25
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
    # the alpha workspace itself: 16-byte aligned (accepted shapes otherwise).  A NULL one is the plain decode now, not an error:
    # "the weight entry without its workspace" cannot be written as a descriptor.
    for ctx in (False, True):
        assert _beam_rc(B, T_DEF, 256, 194, STEPS_B, 8, ctx=ctx, alpha_ws="misaligned") == E_ARG
    L = nat.lib()
    b, _, _ = _attn_buffers(B, T_DEF, 256, 194, 65, 8)
    fz = lambda steps, ap, T, out: L.msocr_attn_beam_finalize(b["ws"].data_ptr(), B, 194, steps, 8, b["trun"].data_ptr(),
                                                              b["logits"].data_ptr(), b["ids"].data_ptr(), ap, T, out, ops._stream())
    ws_p, out_p = b["alpha_ws"].data_ptr(), b["alpha"].data_ptr()
    assert fz(65, ws_p, T_DEF, out_p) == E_ARG
    assert fz(STEPS_B, None, T_DEF, out_p) == E_ARG
    assert fz(STEPS_B, ws_p + 4, T_DEF, out_p) == E_ARG
    assert fz(STEPS_B, ws_p, T_DEF, None) == E_ARG
    assert fz(STEPS_B, ws_p, 0, out_p) == E_ARG
    assert fz(STEPS_B, ws_p, 65, out_p) == E_ARG
    assert _untouched(b)
    cd = lambda lg, al, T, pr: L.msocr_seq_char_details(lg, b["ids"].data_ptr(), al, b["trun"].data_ptr(), B, 194, STEPS_B, T, pr,
                                                        out_p, b["ids"].data_ptr(), ops._stream())
    assert cd(b["logits"].data_ptr(), ws_p, 65, out_p) == E_ARG
    assert cd(b["logits"].data_ptr(), ws_p, 0, out_p) == E_ARG
    assert cd(None, ws_p, T_DEF, out_p) == E_ARG
    assert cd(b["logits"].data_ptr(), None, T_DEF, out_p) == E_ARG
    assert cd(b["logits"].data_ptr(), ws_p, T_DEF, None) == E_ARG
    assert _untouched(b)
    assert L.msocr_attn_beam_alpha_bytes(B, STEPS_B, 8, T_DEF) == B * STEPS_B * 8 * T_DEF * 4
    # the shapes at the envelope's edge are accepted (same buffers, so a rejection above is the check, not the buffers)
    assert _greedy_rc(B, 64, 128, 512, 64) == 0
    assert _beam_rc(B, T_DEF, 512, 194, STEPS_B, 8) == 0
    assert _beam_rc(B, 48, 256, 256, STEPS_B, 8, ctx=True) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (7) the one finalize entry
def test_finalize_with_and_without_the_alpha_arguments(cuda):
    """msocr_attn_beam_finalize on a hand-filled workspace (the random fill of test_nbest_cpu.py; B 5, steps 4, beam 3, V 7, T 6,
    t_run 1 .. steps): with NULL, 0, NULL nothing writes to an attention-weight buffer; with the arguments set the logits and ids
    are those of the NULL call bit for bit, and the gathered weights are a numpy walk of the back-pointers, zeros for t >= t_run."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    from test_nbest_cpu import _pack, _workspace
    L = nat.lib()
    B, steps, K, V, T = 5, 4, 3, 7, 6
    logits, back, tokv, best_at = _workspace(B, V, steps, K, seed=11)
    ws = torch.from_numpy(_pack(logits, back, tokv, best_at)).cuda()
    assert ws.numel() == L.msocr_attn_beam_workspace_bytes(B, steps, K, V)
    aws_h = np.random.default_rng(12).random((B, steps, K, T), dtype=np.float32)
    aws = torch.from_numpy(aws_h).cuda()
    assert aws.numel() * 4 == L.msocr_attn_beam_alpha_bytes(B, steps, K, T)
    trun_h = np.array([4, 1, 3, 2, 4], dtype=np.int32)
    trun = torch.from_numpy(trun_h).cuda()
    big, al = _guarded(B, steps, T)

    def run(alpha_ws, T_, alpha_out):
        lg = torch.full((B, steps, V), SENT, dtype=torch.float32, device="cuda")
        ids = torch.full((B, steps), -7, dtype=torch.int32, device="cuda")
        assert L.msocr_attn_beam_finalize(ws.data_ptr(), B, V, steps, K, trun.data_ptr(), lg.data_ptr(), ids.data_ptr(), alpha_ws, T_,
                                          alpha_out, ops._stream()) == 0
        torch.cuda.synchronize()
        return lg.cpu().numpy(), ids.cpu().numpy()

    lg0, ids0 = run(None, 0, None)
    assert bool((big == SENT).all())  # off: the buffer the next call writes is still untouched
    lg1, ids1 = run(aws.data_ptr(), T, al.data_ptr())
    assert np.array_equal(lg0.view(np.int32), lg1.view(np.int32)) and np.array_equal(ids0, ids1)
    exp_lg = np.full((B, steps, V), SENT, dtype=np.float32)  # rows t >= t_run are not written
    exp_ids = np.full((B, steps), -1, dtype=np.int32)
    exp_al = np.zeros((B, steps, T), dtype=np.float32)
    for b in range(B):
        cur = int(best_at[b, trun_h[b] - 1])
        for t in range(trun_h[b] - 1, -1, -1):
            exp_ids[b, t] = tokv[b, t, cur]
            cur = int(back[b, t, cur])  # the slot whose logits and weights produced the token
            exp_lg[b, t], exp_al[b, t] = logits[b, t, cur], aws_h[b, t, cur]
    assert np.array_equal(ids1, exp_ids) and np.array_equal(lg1.view(np.int32), exp_lg.view(np.int32))
    got = al.cpu().numpy()
    assert np.array_equal(got.view(np.int32), exp_al.view(np.int32)) and (got[np.arange(steps)[None, :] >= trun_h[:, None]] == 0).all()
    assert _guards_intact(big)
