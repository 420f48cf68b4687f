"""The beam decode fused with a character n-gram language model, on the device: msocr_attn_decode with lm
(csrc/attn_general_lm.hip on the general route, csrc/attn_lm_mfma.hip on the matrix cores) on the decoder fixtures of test_gpu_seq_f64.py (its
inputs, decoders, oracle and bounds) and the kernel cases of test_gpu_lexicon.py, then the switch through TRBA and Pipeline on
test_gpu_nbest.py's pipeline fixture.

(1) lm_weight 0 is the plain decode with the attention-weight output, bit for bit: workspace, fin_step, weight trace.
(2) The fused beam search written here on the oracle's Attention in float64, one row at a time (lambda 1 and 0.3, temperature 1 and
    1.7): ids and finish step equal on the rows it decides by more than DECISIVE_FACTOR * e_dev / tau; logits within E_REL_MAX.  The
    float64 fused search must read another text than the float64 plain search on at least half of the rows (asserted): otherwise a
    decode without the addend could pass.
(3) ctx_out is CharLM.walk of every slot's back-traced token path, exactly, for orders 1, 2 and 3.
(4) The slots are in fused-score order, recomputed in float64 from the stored logits and the table.
(5) TRBA.predict(lm=..., n_best=3): logp is TRBA.score's of the returned text, lm_logp is CharLM.logp of it.
(6) Batch composition, bit for bit; the two kernel families against each other on decisive rows.
(7) A table that favours one path makes it win.  (8) MSOCR_E_ARG from the C ABI.  (9) Pipeline.lm with the other switches; refusals.

Tables: log_softmax(2 * randn) per context, seeded, with three special columns at -30: <PAD>, <SOS> and the charset's last token (the
fixture charsets have no <BLANK>; the last token stands where the shipped charset has it).  Order 3 where V <= 256, order 2 above.
The condition of (2) was checked on the CPU before this file was written, with E_REL_MAX * max|logit| standing in for e_dev: see the
figures in DESIGN.md section 4.16."""
import numpy as np
import pytest
import torch

from attn_call import attn_decode
from test_gpu_lexicon import KERNEL_CASES
from test_gpu_nbest import _pages_and_maps, _pipe
from test_gpu_seq_f64 import (B_DEF, DECISIVE_FACTOR, DECISIVE_MIN_FRACTION, E_REL_MAX, EOS, PAD, SOS, T_DEF, TAU, _attn_buffers, _inputs,
                              _kernel, _oracle, _replay)

pytestmark = pytest.mark.gpu

E_ARG = -1
STEPS = 9
ALPHA = 0.9
FLOOR = -30.0
FUSIONS = [(1.0, 1.0), (1.0, 1.7), (0.3, 1.0), (0.3, 1.7)]  # (lambda, temperature)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ tables and launches
_LM = {}


def _order_for(V):
    return 3 if V <= 256 else 2


def _lm(V, order=None, seed=5):
    from manuscript_ocr_amd.recognizers import CharLM
    order = _order_for(V) if order is None else order
    if (V, order, seed) not in _LM:
        g = torch.Generator().manual_seed(seed * 100003 + V * 7 + order)
        t = torch.log_softmax(2.0 * torch.randn(V ** (order - 1), V, generator=g, dtype=torch.float64), -1)
        t[:, [PAD, SOS, V - 1]] = FLOOR
        _LM[(V, order, seed)] = CharLM(t.numpy(), V, order, SOS, EOS)
    return _LM[(V, order, seed)]


def _split(buf, B, steps, K, V):
    n = B * steps * K
    lg = buf[:n * V * 4].view(np.float32).reshape(B, steps, K, V)
    back = buf[n * V * 4:n * V * 4 + n * 4].view(np.int32).reshape(B, steps, K)
    tokv = buf[n * V * 4 + n * 4:n * V * 4 + 2 * n * 4].view(np.int32).reshape(B, steps, K)
    best = buf[n * V * 4 + 2 * n * 4:n * V * 4 + 2 * n * 4 + B * steps * 4].view(np.int32).reshape(B, steps)
    return lg, back, tokv, best


def _chunk_ids(fin):
    """Two reference chunks from a run's finish steps, as test_gpu_nbest.py forms them: chunk 0 holds the rows that finish first."""
    return (fin > np.median(fin)).astype(np.int32)


def _chunk_args(cid):
    csz = np.bincount(cid).astype(np.int32)
    return (torch.from_numpy(cid).cuda(), torch.from_numpy(csz).cuda(), torch.zeros(2 * len(csz), dtype=torch.int32, device="cuda"))


def _host(dec, res, cid, B, steps, K):
    """A decode's results as host arrays; t_run = the chunk's largest finish step (what the product passes on), or the row's own."""
    ws, fin, _lp, aws = res[:4]
    torch.cuda.synchronize()
    fin_h = fin.cpu().numpy()
    trun = np.array([fin_h[cid == c].max() for c in range(cid.max() + 1)], dtype=np.int32)[cid] if cid is not None else fin_h.copy()
    lg, back, tokv, best = _split(ws.cpu().numpy(), B, steps, K, dec.V)
    out = dict(ws=ws, aws=aws.cpu().numpy(), lg=lg, back=back, tokv=tokv, best=best, fin=fin_h, trun=trun)
    if len(res) == 5:
        out["ctx"] = res[4].cpu().numpy()
    return out


def _decode(dec, bH, pH, steps, K, alpha, tau, lm, lam, early, ctx_gates=None):
    """One fused decode -> host arrays (early: in two chunks formed from the finish steps of a run of the same decode without chunks)."""
    B = bH.shape[0]
    cid = None
    if early:
        cid = _chunk_ids(dec.beam(bH, pH, steps, K, alpha, tau, SOS, EOS, None, None, ctx_gates=ctx_gates, lm=lm, lm_weight=lam)[1].cpu().numpy())
    res = dec.beam(bH, pH, steps, K, alpha, tau, SOS, EOS, None, None if cid is None else _chunk_args(cid), ctx_gates=ctx_gates, lm=lm,
                   lm_weight=lam)
    assert len(res) == 5 and res[4].shape == (B, steps, K) and res[4].dtype == torch.int32
    return _host(dec, res, cid, B, steps, K)


def _finalize(dec, r, K, steps):
    B = len(r["trun"])
    lg, ids = dec.beam_finalize(r["ws"], B, steps, K, torch.from_numpy(r["trun"]).cuda())
    return lg.cpu().numpy(), ids.cpu().numpy()


def _case(monkeypatch, what, H, V, K, kernel):
    dec = _kernel(monkeypatch, V, H, kernel)
    assert dec._matrix_core(T_DEF, K) == what.startswith("mfma"), "the case must run on the kernel it names"
    return dec, _inputs(B_DEF, T_DEF, H, V)


# ------------------------------------------------------------------------------------------------ (1) weight 0
@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("what,H,V,K,steps,kernel", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_weight_zero_is_the_plain_decode_bit_for_bit(cuda, monkeypatch, what, H, V, K, steps, kernel, early):
    B = B_DEF
    dec, (bH, pH) = _case(monkeypatch, what, H, V, K, kernel)
    lm = _lm(V)
    cid = None
    if early:
        cid = _chunk_ids(dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, None, want_alpha=True)[1].cpu().numpy())
    chunks = (lambda: None) if cid is None else (lambda: _chunk_args(cid))  # a zeroed chunk state for every launch
    plain = _host(dec, dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, chunks(), want_alpha=True), cid, B, steps, K)
    fused = _host(dec, dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, chunks(), lm=lm, lm_weight=0.0), cid, B, steps, K)
    assert np.array_equal(plain["fin"], fused["fin"])
    # steps behind a chunk's run length are the ones the early exit may skip: whether a workgroup computed them depends on when it
    # saw the other workgroups' flags, in either decode
    w = np.arange(steps)[None, :] < plain["trun"][:, None]
    if not early:  # every launch ran every step
        w = np.ones_like(w)
    for name in ("lg", "aws", "back", "tokv", "best"):
        a, b = plain[name][w], fused[name][w]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, name, int((a.view(np.int32) != b.view(np.int32)).sum()))
    print(f"[charlm] weight 0 {what} {'chunk exit' if early else 'all steps'}: finish steps {fused['fin'].min()}..{fused['fin'].max()}, "
          f"{int(w.sum())}/{w.size} (row, step) pairs compared")


# ------------------------------------------------------------------------------------------------ (2) float64 fused search
def _search64(att, bH_row, table, ctx0, lam, steps, K, alpha, tau):
    """The fused beam search in the oracle's arithmetic (Attention.beam, oracle/trba_model.py:166-224) on one row in att's dtype, with
    the two additions of DESIGN.md section 4.16: a table row per hypothesis, and lam * table[ctx] added to a live hypothesis'
    log-softmax where the candidates are formed (finished ones: EOS alone at 0).  table: [n_ctx, V] in att's dtype on its device.
    Ties: larger value, then smaller flat index.  lam = 0 is the plain search.  -> (ids of the best hypothesis up to the finish step,
    finish step, smallest top-K boundary gap, final best-minus-second score)."""
    dev, fd, V, H = bH_row.device, bH_row.dtype, att.num_classes, att.hidden_size
    n_ctx = table.shape[0]
    toks = [[SOS] for _ in range(K)]
    score = torch.full((K,), float("-inf"), dtype=fd, device=dev)
    score[0] = 0.0
    bh, bc = torch.zeros(K, H, dtype=fd, device=dev), torch.zeros(K, H, dtype=fd, device=dev)
    ctx, done = [ctx0] * K, [False] * K
    rep = bH_row.expand(K, -1, -1)
    only_eos = torch.full((V,), float("-inf"), dtype=fd, device=dev)
    only_eos[EOS] = 0.0
    bgap, fin = np.inf, steps
    for t in range(steps):
        last = torch.tensor([tk[-1] for tk in toks], device=dev)
        h1, c1 = att.attention_cell((bh, bc), rep, att._onehot(last, fd))
        logits = att._mask(att.generator(h1))
        if tau != 1.0:
            logits = logits / max(tau, 1e-6)
        logp = torch.log_softmax(logits, -1) + lam * table[torch.tensor(ctx, device=dev)]
        logp = torch.where(torch.tensor(done, device=dev)[:, None], only_eos[None, :], logp)
        total = score[:, None] + logp
        lp = ((5.0 + (t + 1)) ** alpha) / (6.0 ** alpha) if alpha > 0 else 1.0
        cand = (total / lp if alpha > 0 else total).reshape(-1)
        order = torch.sort(cand, descending=True, stable=True)  # stable: equal values keep the smaller flat index first
        top, idx = order.values[:K], order.indices[:K]
        if bool(torch.isfinite(order.values[K])):
            bgap = min(bgap, float(order.values[K - 1] - order.values[K]))
        src, nxt = (idx // V).tolist(), (idx % V).tolist()
        ended = [done[src[k]] or nxt[k] == EOS for k in range(K)]
        ctx = [ctx[src[k]] if ended[k] else (ctx[src[k]] * V + nxt[k]) % n_ctx for k in range(K)]
        si = torch.tensor(src, device=dev)
        bh, bc = h1[si], c1[si]
        toks = [toks[src[k]] + [nxt[k]] for k in range(K)]
        score = top * lp if alpha > 0 else top
        done = ended
        if all(done):
            fin = t + 1
            break
    sc = score.tolist()
    best = int(np.argmax(sc))
    rest = sorted((x for i, x in enumerate(sc) if i != best and np.isfinite(x)), reverse=True)
    sgap = sc[best] - rest[0] if rest else np.inf
    return toks[best][1:], fin, bgap, sgap


_REF = {}


def _reference_search(H, V, K, steps, lam, tau, att=None, bH=None):
    """The float64 search of every row, computed once per (shape, lambda, temperature); lam 0 = the plain search."""
    lm = _lm(V)
    key = (H, V, K, steps, lam, tau)
    if key not in _REF:
        att = att if att is not None else _oracle(V, H, None, "f64")
        bH = bH if bH is not None else _inputs(B_DEF, T_DEF, H, V)[0]
        dev = next(att.parameters()).device
        table = torch.from_numpy(lm.table).to(dev).double()
        with torch.no_grad():
            _REF[key] = [_search64(att, bH[b:b + 1].to(dev).double(), table, lm.ctx0, lam, steps, K, ALPHA, tau) for b in range(bH.shape[0])]
    return _REF[key]


def _text(ids):
    """A reading as the product would show it: the tokens before the first EOS."""
    ids = list(ids)
    return tuple(ids[:ids.index(EOS)] if EOS in ids else ids)


SEARCH_CASES = [c for c in KERNEL_CASES if c[4] == STEPS]


@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("what,H,V,K,steps,kernel", SEARCH_CASES, ids=[c[0] for c in SEARCH_CASES])
def test_fused_search_against_f64_fused_beam_search(cuda, monkeypatch, what, H, V, K, steps, kernel, early):
    B = B_DEF
    dec, (bH, pH) = _case(monkeypatch, what, H, V, K, kernel)
    lm = _lm(V)
    for lam, tau in FUSIONS:
        r = _decode(dec, bH, pH, steps, K, ALPHA, tau, lm, lam, early)
        lg, ids = _finalize(dec, r, K, steps)
        fin = r["fin"]
        # e_dev along the finalized path, as test_gpu_seq_f64._beam_case measures it: the trace holds the model's logits
        tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), np.where(ids[:, :-1] >= 0, ids[:, :-1], EOS)], 1).astype(np.int64))
        r64 = (_replay(_oracle(V, H, None, "f64"), bH.double(), tok_in) / tau).cpu().numpy()
        valid = np.arange(steps)[None, :] < fin[:, None]
        e_dev, scale = float(np.abs(lg[valid].astype(np.float64) - r64[valid]).max()), float(np.abs(r64[valid]).max()) * tau
        delta = DECISIVE_FACTOR * e_dev / tau
        ref, ref_plain = _reference_search(H, V, K, steps, lam, tau), _reference_search(H, V, K, steps, 0.0, tau)
        differ = sum(_text(f[0]) != _text(p[0]) for f, p in zip(ref, ref_plain))
        decisive, bad = 0, []
        for b, (oid, ofin, bgap, sgap) in enumerate(ref):
            if min(bgap, sgap) > delta:
                decisive += 1
                if not (ofin == fin[b] and np.array_equal(ids[b, :ofin], oid)):
                    bad.append((b, int(fin[b]), ofin))
        print(f"[charlm] search {what} {'chunk exit' if early else 'all steps'} lambda {lam} tau {tau}: e_dev {e_dev:.2e} ({e_dev / scale:.1e} "
              f"of max|logit| {scale:.2f}), decisive rows {decisive}/{B} at {delta:.2e}, f64 fused reading != f64 plain reading on {differ}/{B}")
        assert e_dev <= E_REL_MAX * scale, (what, lam, tau, e_dev, scale)
        assert 2 * differ >= B, f"the fixture does not tell a fused search from a plain one: {differ}/{B} rows differ ({what}, {lam}, {tau})"
        assert not bad, (what, lam, tau, bad)
        assert decisive / B >= DECISIVE_MIN_FRACTION, f"degenerate fixture: {decisive}/{B} decisive rows ({what}, {lam}, {tau})"


# ------------------------------------------------------------------------------------------------ (3) state trace
def _paths(r, K, steps):
    """paths[b][s][k]: the tokens of the hypothesis in slot k after step s (back-traced), for the written steps."""
    out = []
    for b in range(len(r["fin"])):
        prev, rows = [[] for _ in range(K)], []
        for s in range(int(r["trun"][b])):
            cur = []
            for k in range(K):
                src, tok = int(r["back"][b, s, k]), int(r["tokv"][b, s, k])
                assert 0 <= src < K, (b, s, k, src)
                cur.append(prev[src] + [tok])
            rows.append(cur)
            prev = cur
        out.append(rows)
    return out


TRACE_CASES = [(c, None) for c in KERNEL_CASES] + [(KERNEL_CASES[0], 1), (KERNEL_CASES[0], 2), (KERNEL_CASES[4], 1), (KERNEL_CASES[4], 2)]


@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("case,order", TRACE_CASES, ids=[f"{c[0]}-order{o or _order_for(c[2])}" for c, o in TRACE_CASES])
def test_ctx_out_is_the_host_walk_of_every_slot(cuda, monkeypatch, case, order, early):
    what, H, V, K, steps, kernel = case
    dec, (bH, pH) = _case(monkeypatch, what, H, V, K, kernel)
    lm = _lm(V, order)
    r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lm, 0.7, early)
    fin, trun = r["fin"], r["trun"]
    assert ((fin >= 1) & (fin <= steps)).all() and (trun >= fin).all()
    n, n_moving = 0, 0
    for b, rows in enumerate(_paths(r, K, steps)):
        for s, cur in enumerate(rows):
            want = [lm.walk(p)[-1] for p in cur]
            got = r["ctx"][b, s].tolist()
            assert got == want, (what, b, s, got, want)
            n += K
            n_moving += sum(EOS not in p for p in cur)
    written = r["ctx"][np.broadcast_to(np.arange(steps)[None, :, None] < trun[:, None, None], r["ctx"].shape)]
    assert ((written >= 0) & (written < lm.n_ctx)).all() and n_moving > 0
    if lm.order == 1:
        assert (written == 0).all()
    print(f"[charlm] trace {what} order {lm.order} {'chunk exit' if early else 'all steps'}: {n} (row, step, slot) contexts equal the host "
          f"walk, {n_moving} of them of unfinished hypotheses")


# ------------------------------------------------------------------------------------------------ (4) slot order
# The 9-step cases.  The slack the section states, 1e-4 + steps * 2^-23 * lambda * max|table|, is absolute; the device's f32 score of a
# hypothesis takes three roundings of at most 2^-24 |score| per step (the addition, the division by the length penalty and the
# multiplication back) and the log-sum-exp's few ulp of |logit| <= 14: over 9 steps of at most about 8 nats each that is at most
# 9 * (1.8e-7 * 72 + 1e-6) = 1.3e-4 before the last division by the length penalty (2.1 at step 9), so 6e-5: inside the slack.  At 25
# steps the same count gives 2.2e-4, so the stated slack is not a bound there and the long cases are left to (1) and (3).
ORDER_LAMBDA = 0.7


@pytest.mark.parametrize("what,H,V,K,steps,kernel", SEARCH_CASES, ids=[c[0] for c in SEARCH_CASES])
def test_slots_are_in_fused_score_order(cuda, monkeypatch, what, H, V, K, steps, kernel):
    dec, (bH, pH) = _case(monkeypatch, what, H, V, K, kernel)
    lm = _lm(V)
    lam = ORDER_LAMBDA
    r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lm, lam, False)
    tab = lm.table.astype(np.float64)
    slack = 1e-4 + steps * 2.0 ** -23 * lam * float(np.abs(tab).max())
    worst = 0.0
    for b in range(len(r["fin"])):
        last = int(r["fin"][b]) - 1
        lp = ((5.0 + (last + 1)) ** ALPHA) / (6.0 ** ALPHA)
        scores = []
        for k in range(K):
            slots, cur = [], k  # the slots the hypothesis sat in before each step: its logits are there
            for t in range(last, -1, -1):
                cur = int(r["back"][b, t, cur])
                slots.append(cur)
            slots = slots[::-1]
            path = _paths_of(r, b, last, k)
            model, lmsum, ctx, done = 0.0, 0.0, lm.ctx0, False
            for t, tok in enumerate(path):
                if not done:
                    x = r["lg"][b, t, slots[t]].astype(np.float64)
                    m = x.max()
                    model += x[tok] - m - np.log(np.exp(x - m).sum())
                    lmsum += tab[ctx, tok]
                    done = tok == EOS
                    if not done:
                        ctx = (ctx * lm.num_classes + tok) % lm.n_ctx
                else:
                    assert tok == EOS
            scores.append((model + lam * lmsum) / lp)
        d = np.diff(np.array(scores))  # > 0 where a later slot scores higher
        worst = max(worst, float(d.max()))
        assert (d <= slack).all(), (what, b, scores)
        assert r["best"][b, last] == 0
    print(f"[charlm] slot order {what}: largest violation {max(worst, 0.0):.2e} (slack {slack:.2e})")


def _paths_of(r, b, at, slot):
    out, cur = [], slot
    for t in range(at, -1, -1):
        out.append(int(r["tokv"][b, t, cur]))
        cur = int(r["back"][b, t, cur])
    return out[::-1]


# ------------------------------------------------------------------------------------------------ (6) independence and agreement
@pytest.mark.parametrize("kernel", ["auto", "valu"])
def test_fused_decode_does_not_depend_on_batch_composition(cuda, monkeypatch, kernel):
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    dec = _kernel(monkeypatch, V, H, kernel)
    lm = _lm(V)
    bH, pH = _inputs(B, T, H, V)
    cg = dec.ctx_gates(bH).view(B, -1)

    def run(rows):
        idx = torch.as_tensor(rows, device=bH.device)
        c = cg[idx].contiguous().view(len(rows) * T, -1)
        r = _decode(dec, bH[idx].contiguous(), pH[idx].contiguous(), steps, K, ALPHA, TAU, lm, 0.7, False, ctx_gates=c)
        lg, ids = _finalize(dec, r, K, steps)
        return r["lg"].view(np.int32), r["back"], r["tokv"], r["ctx"], r["aws"].view(np.int32), lg.view(np.int32), ids, r["fin"]

    full = run(list(range(B)))
    perm = np.random.default_rng(5).permutation(B).tolist()
    permuted = run(perm)
    for j, b in enumerate(perm):
        assert all(np.array_equal(x[b], y[j]) for x, y in zip(full, permuted)), ("permuted", b)
    for b in (0, 1, 2, 3, 17, 35, 36):  # a full workgroup of the matrix-core kernel, a row in the middle, the partial last workgroup
        alone = run([b])
        assert all(np.array_equal(x[b], y[0]) for x, y in zip(full, alone)), ("alone", b)


def test_matrix_core_and_general_kernels_agree_on_decisive_rows(cuda, monkeypatch):
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    lm = _lm(V)
    lam, tau = FUSIONS[1]
    bH, pH = _inputs(B, T, H, V)
    out = {}
    for kernel in ("auto", "valu"):
        dec = _kernel(monkeypatch, V, H, kernel)
        assert dec._matrix_core(T, K) == (kernel == "auto")
        r = _decode(dec, bH, pH, steps, K, ALPHA, tau, lm, lam, False)
        out[kernel] = (r, _finalize(dec, r, K, steps)[1])
    delta = DECISIVE_FACTOR * E_REL_MAX * 13.95 / tau  # the largest threshold test (2) can apply at the fixture's logit scale
    rows = [b for b, (_o, _f, bgap, sgap) in enumerate(_reference_search(H, V, K, steps, lam, tau)) if min(bgap, sgap) > delta]
    assert len(rows) >= DECISIVE_MIN_FRACTION * B
    (ra, ia), (rv, iv) = out["auto"], out["valu"]
    for b in rows:
        f = ra["fin"][b]
        assert f == rv["fin"][b] and np.array_equal(ia[b], iv[b]) and np.array_equal(ra["ctx"][b, :f], rv["ctx"][b, :f]), b


# ------------------------------------------------------------------------------------------------ (7) extreme table
@pytest.mark.parametrize("kernel", ["auto", "valu"])
def test_a_table_that_admits_one_path_makes_it_win(cuda, monkeypatch, kernel):
    from manuscript_ocr_amd.recognizers import CharLM
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    dec = _kernel(monkeypatch, V, H, kernel)
    bH, pH = _inputs(B, T, H, V)
    path = [40, 9, 133, 9, EOS]
    table = np.full((V * V, V), FLOOR, dtype=np.float32)
    lm0 = CharLM(table, V, 3, SOS, EOS)
    for ctx, tok in zip([lm0.ctx0] + lm0.walk(path)[:-1], path):
        table[ctx, tok] = 0.0
    lm = CharLM(table, V, 3, SOS, EOS)
    # lambda from the fixture's logit range: a token's log-softmax lies in [-(range + log V), 0], so the path's model score over its
    # n steps is at least -n (range + log V), and any hypothesis that leaves the path carries at least one addend of lambda * -30
    # (its model score is at most 0).  Twice the break-even weight; the range is the plain decode's, over every slot and step.
    lg = _host(dec, dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, None, want_alpha=True), None, B, steps, K)["lg"]
    rng = float(lg.max() - lg.min())
    lam = 2.0 * len(path) * (rng + np.log(V)) / -FLOOR
    r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lm, lam, False)
    _, ids = _finalize(dec, r, K, steps)
    assert (ids[:, :len(path)] == np.array(path)).all(), ids[:, :len(path)].tolist()
    assert (r["tokv"][:, :len(path), 0] == np.array(path)).all() and (r["best"][:, :len(path)] == 0).all()
    print(f"[charlm] one path {kernel}: logit range {rng:.2f}, lambda {lam:.2f}")


# ------------------------------------------------------------------------------------------------ (8) C ABI
def _lm_rc(B, T, H, V, steps, K, hoisted, order=2, null=None, sos=SOS, weight=0.5, lm_V=None, n_ctx=None, table_elems=None):
    """Device buffers sized for the (rejected) shape, the table for the shape the struct claims: a kernel launched by a broken check
    runs on valid memory."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, K)
    aws = torch.zeros((B, steps, K, T), dtype=torch.float32, device="cuda")
    ctx = torch.zeros((B, steps, K), dtype=torch.int32, device="cuda")
    st = nat.CharLMTable()
    st.order, st.V = order, V if lm_V is None else lm_V
    st.n_ctx = (st.V ** max(order - 1, 0)) if n_ctx is None else n_ctx
    elems = max(int(st.n_ctx), 1) * max(V, st.V) if table_elems is None else table_elems
    table = (torch.zeros if elems <= 1 << 24 else torch.empty)((elems,), dtype=torch.float32, device="cuda")
    st.table = None if null == "table" else table.data_ptr()
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "lp": b["lp"], "fin_step_out": b["fin"], "workspace": b["ws"],
            "alpha_out": None if null == "alpha_ws" else aws, "lm": None if null == "lm" else st, "ctx_out": None if null == "ctx_out" else ctx}
    if hoisted:
        bufs["ctx_gates"] = b["ctx"]
    rc = attn_decode(nat.ATTN_BEAM, bufs, B=B, T=T, H=H, V=V, steps=steps, beam=K, temperature=1.7, sos_id=sos, eos_id=EOS, blank_id=-1,
                     lm_weight=float(weight), stream=ops._stream())
    torch.cuda.synchronize()
    return rc


def test_c_abi_rejects_bad_arguments_and_shapes_outside_the_envelope(cuda):
    B, T, steps = 2, T_DEF, STEPS
    for hoisted in (False, True):
        ok = dict(B=B, T=T, H=256, V=194, steps=steps, K=8, hoisted=hoisted)
        for order in (1, 2, 3):
            assert _lm_rc(**ok, order=order) == 0  # same buffers: a rejection below is the check, not the buffers
        assert _lm_rc(**ok, weight=0.0) == 0
        for null in ("lm", "table", "ctx_out", "alpha_ws"):
            assert _lm_rc(**ok, null=null) == E_ARG, (hoisted, null)
        for order in (0, 4, -1):
            assert _lm_rc(**ok, order=order, n_ctx=1) == E_ARG, (hoisted, order)
        assert _lm_rc(**ok, lm_V=193) == E_ARG and _lm_rc(**ok, lm_V=195) == E_ARG
        assert _lm_rc(**ok, order=2, n_ctx=193) == E_ARG and _lm_rc(**ok, order=3, n_ctx=194) == E_ARG
        assert _lm_rc(**ok, order=1, n_ctx=194) == E_ARG and _lm_rc(**ok, order=2, n_ctx=0) == E_ARG
        for weight in (-0.5, float("nan"), float("inf"), -float("inf")):
            assert _lm_rc(**ok, weight=weight) == E_ARG, (hoisted, weight)
        assert _lm_rc(**ok, sos=-1) == E_ARG and _lm_rc(**ok, sos=194) == E_ARG
        assert _lm_rc(**{**ok, "steps": 65}) == E_ARG
        assert _lm_rc(**{**ok, "T": 65}) == E_ARG
        assert _lm_rc(**{**ok, "V": 513}) == E_ARG
        assert _lm_rc(**{**ok, "K": 17}) == E_ARG
        assert _lm_rc(**{**ok, "H": 96}) == E_ARG
    gen = dict(B=B, T=T, steps=steps, hoisted=False)
    assert _lm_rc(**gen, H=320, V=194, K=13) == E_ARG  # 13 x 320 > 4096
    assert _lm_rc(**gen, H=512, V=194, K=9) == E_ARG
    assert _lm_rc(**gen, H=512, V=194, K=8) == 0 and _lm_rc(**gen, H=64, V=512, K=16) == 0
    # the size cap: 407^3 > 2^26 >= 406^3 (the table is allocated at the size the struct claims, 270 MB, and never read)
    assert _lm_rc(**gen, H=64, V=407, K=8, order=3) == E_ARG
    assert _lm_rc(**gen, H=64, V=406, K=8, order=3) == 0
    hst = dict(B=B, steps=steps, hoisted=True)
    assert _lm_rc(**hst, T=T, H=128, V=194, K=8) == E_ARG   # the matrix-core kernel takes H 256 only
    assert _lm_rc(**hst, T=T, H=256, V=257, K=8) == E_ARG
    assert _lm_rc(**hst, T=49, H=256, V=194, K=8) == E_ARG
    assert _lm_rc(**hst, T=T, H=256, V=194, K=9) == E_ARG


# ------------------------------------------------------------------------------------------------ (5), (9) through the product
def _product_lm(rec):
    """Trained by from_texts on seeded words over the recogniser's charset, order 3: the shipped size of the table (29 MB)."""
    from manuscript_ocr_amd.recognizers import CharLM
    rng = np.random.default_rng(16)
    symbols = [s for s in rec.itos if len(s) == 1 and not s.isspace()]
    words = ["".join(symbols[int(i)] for i in rng.integers(0, 40, size=int(rng.integers(1, 11)))) for _ in range(300)]
    return CharLM.from_texts(words, rec.stoi, order=3)


def _named(pages):
    return [[w for blk in p.blocks for w in blk.words if w.text is not None] for p in pages]


@pytest.fixture(scope="module")
def lmpipe(cuda):
    """The pipeline of test_gpu_nbest.py, its pages, the pages read without a language model (the attribute never set) and with one."""
    pipe = _pipe()
    pages, mo = _pages_and_maps()
    assert pipe.lm is None and pipe.lm_weight == 0.5
    off = pipe.predict_batch(pages, _maps_override=mo)
    lm = _product_lm(pipe.recognizer)
    assert lm.table.shape == (194 * 194, 194) and lm.eos_id == pipe.recognizer.eos_id
    pipe.lm, pipe.lm_weight = lm, 0.8
    on = pipe.predict_batch(pages, _maps_override=mo)
    pipe.lm, pipe.lm_weight = None, 0.5
    return pipe, pages, mo, off, lm, on


def _lm_logp_of(rec, lm, text):
    ids = [rec.stoi[c] for c in text]
    return lm.logp(ids + [rec.eos_id] if len(ids) < rec.max_length else ids)


def _base(pages):
    return [[(w.text, w.recognition_confidence, w.lm_logp) for w in p] for p in _named(pages)]


def test_predict_with_a_language_model_decomposes(lmpipe):
    """TRBA.predict on the words' host crops: logp is TRBA.score's of the text it read (the model's own number, to the tolerance
    test_gpu_lexicon.py uses for the same comparison), lm_logp is CharLM.logp of it."""
    from test_forced_cpu import STEP_ATOL
    pipe, pages, _mo, _off, lm, on = lmpipe
    rec, tau = pipe.recognizer, 1.3
    n = 0
    for page, arr in zip(on, pages):
        words = [w for w in page.blocks[0].words if w.text is not None]
        crops = [pipe._extract_word_image(arr, np.array(w.polygon, dtype=np.int32)) for w in words][:6]
        res = rec.predict(crops, temperature=tau, n_best=3, return_chars=True, lm=lm, lm_weight=0.8)
        assert all(set(r) == {"text", "confidence", "lm_logp", "alternatives", "chars"} for r in res)
        plain = rec.predict(crops, temperature=tau, lm=lm, lm_weight=0.8)
        assert all(set(r) == {"text", "confidence", "lm_logp"} for r in plain)
        scored_all = rec.score(crops, [[a["text"] for a in r["alternatives"]] for r in res], temperature=tau)
        for r, p, scored in zip(res, plain, scored_all):
            assert (r["text"], r["confidence"], r["lm_logp"]) == (p["text"], p["confidence"], p["lm_logp"])
            assert len(r["chars"]) == len(r["text"]) and 1 <= len(r["alternatives"]) <= 3
            assert r["alternatives"][0]["text"] == r["text"] and r["alternatives"][0]["lm_logp"] == r["lm_logp"]
            for a, s in zip(r["alternatives"], scored):
                assert set(a) == {"text", "confidence", "logp", "lm_logp"}
                # msocr_seq_logp's stated bound: STEP_ATOL per counted step (the symbols and the EOS)
                assert abs(a["logp"] - s["logp"]) <= (len(a["text"]) + 1) * STEP_ATOL, (a["logp"], s["logp"])
                want = _lm_logp_of(rec, lm, a["text"])
                assert isinstance(a["lm_logp"], float) and abs(a["lm_logp"] - want) <= 1e-6 * max(1.0, abs(want)), (a["lm_logp"], want)
                n += 1
    assert n > 0
    # the generic route with this package's recogniser asks predict for the same
    from manuscript_ocr_amd.detectors._types import LmWord
    try:
        pipe.lm, pipe.native_fast_path = lm, False
        page = pipe.predict(pages[0])
    finally:
        pipe.lm, pipe.native_fast_path = None, True
    named = [w for w in page.blocks[0].words if w.text is not None]
    assert named and all(type(w) is LmWord and abs(w.lm_logp - _lm_logp_of(rec, lm, w.text)) <= 1e-6 * max(1.0, abs(w.lm_logp)) for w in named)


def test_pipeline_lm_with_the_other_switches(lmpipe):
    from manuscript_ocr_amd.detectors._types import LmAlternative, LmWord
    pipe, pages, mo, off, lm, on = lmpipe
    rec = pipe.recognizer
    n_words = 0
    drop = {"blocks": {"__all__": {"words": {"__all__": {"text", "recognition_confidence"}}}}}
    for p_on, p_off in zip(on, off):
        assert p_on.model_dump(exclude=drop) == p_off.model_dump(exclude=drop)
        for w, w0 in zip(p_on.blocks[0].words, p_off.blocks[0].words):
            assert (w.text is None) == (w0.text is None)
            if w.text is None:
                continue
            assert type(w) is LmWord and w.alternatives == [] and w.chars == []
            assert abs(w.lm_logp - _lm_logp_of(rec, lm, w.text)) <= 1e-6 * max(1.0, abs(w.lm_logp))
            n_words += 1
    assert n_words == sum(w.text is not None for p in off for w in p.blocks[0].words) > 0
    print(f"[charlm] pipeline: the language model changes {sum(w.text != w0.text for p, p0 in zip(_named(on), _named(off)) for w, w0 in zip(p, p0))} "
          f"of {n_words} readings at weight 0.8")
    base = _base(on)
    try:
        pipe.lm, pipe.lm_weight = lm, 0.0  # weight 0: the decode is the plain one, bit for bit
        zero = pipe.predict_batch(pages, _maps_override=mo)
        assert [[(w.text, w.recognition_confidence) for w in p] for p in _named(zero)] == \
            [[(w.text, w.recognition_confidence) for w in p] for p in _named(off)]
        pipe.lm, pipe.lm_weight, pipe.n_best = lm, 0.8, 3
        alt = pipe.predict_batch(pages, _maps_override=mo)
        assert _base(alt) == base
        n_second = 0
        for p in _named(alt):
            for w in p:
                assert 1 <= len(w.alternatives) <= 3 and all(type(a) is LmAlternative for a in w.alternatives)
                assert w.alternatives[0].text == w.text and w.alternatives[0].lm_logp == w.lm_logp
                assert all(abs(a.lm_logp - _lm_logp_of(rec, lm, a.text)) <= 1e-6 * max(1.0, abs(a.lm_logp)) for a in w.alternatives)
                assert len({a.text for a in w.alternatives}) == len(w.alternatives)
                assert all(np.isfinite([a.logp for a in w.alternatives]))
                n_second += len(w.alternatives) > 1
        assert n_second > 0
        for switch in ("char_details", "group_lines", "rectify_crops"):
            setattr(pipe, switch, True)
            got = pipe.predict_batch(pages, _maps_override=mo)
            setattr(pipe, switch, False)
            for p in _named(got):
                for w in p:
                    assert type(w) is LmWord and w.alternatives[0].text == w.text
                    assert len(w.chars) == (len(w.text) if switch == "char_details" else 0)
                    assert switch != "char_details" or "".join(c.char for c in w.chars) == w.text
            if switch != "rectify_crops":  # rectified crops are other pixels
                assert _base(got) == base
        pipe.n_best, pipe.device_order = 0, False
        assert _base(pipe.predict_batch(pages, _maps_override=mo)) == base
    finally:
        pipe.lm, pipe.lm_weight, pipe.n_best, pipe.device_order = None, 0.5, 0, True


def test_no_language_model_changes_nothing_and_refusals(lmpipe):
    from manuscript_ocr_amd.recognizers import CharLM, Lexicon
    pipe, pages, mo, off, lm, _on = lmpipe
    rec = pipe.recognizer
    # lm = None after one was used: what the pipeline gave before the attribute was ever set
    assert pipe.lm is None
    again = pipe.predict_batch(pages, _maps_override=mo)
    key = lambda ps: [[(type(w).__name__, w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words] for p in ps]
    assert key(again) == key(off) and [p.model_dump() for p in again] == [p.model_dump() for p in off]
    crop = np.full((32, 100, 3), 255, dtype=np.uint8)
    assert rec.predict([crop], lm=None) == rec.predict([crop])
    lex = Lexicon(["ab"], rec.stoi, rec.max_length)
    V = len(rec.itos)
    with pytest.raises(ValueError, match="greedy"):
        rec.predict([crop], mode="greedy", lm=lm)
    with pytest.raises(ValueError, match="lexicon"):
        rec.predict([crop], lm=lm, lexicon=lex)
    with pytest.raises(ValueError, match="charset"):
        rec.predict([crop], lm=CharLM(np.zeros((1, V + 1)), V + 1, 1, rec.sos_id))
    with pytest.raises(ValueError, match="sos_id"):
        rec.predict([crop], lm=CharLM(np.zeros((1, V)), V, 1, rec.sos_id + 1))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            rec.predict([crop], lm=lm, lm_weight=bad)
    with pytest.raises(ValueError, match="lexicon"):
        rec.model.dec.beam(torch.zeros((1, 13, 256), device="cuda"), torch.zeros((1, 13, 256), device="cuda"), rec.max_length, 8, 0.9, 1.7,
                           rec.sos_id, rec.eos_id, None, lm=lm, lm_weight=0.5, lexicon=lex)
    try:
        pipe.lm, pipe.lexicon = lm, lex
        with pytest.raises(ValueError, match="lexicon"):
            pipe.predict_batch(pages, _maps_override=mo)
        pipe.lexicon, pipe.lm_weight = None, -1.0
        with pytest.raises(ValueError, match="lm_weight"):
            pipe.predict_batch(pages, _maps_override=mo)
        pipe.lm_weight, rec.use_graphs = 0.5, True  # a graph recogniser: refused at submit, before anything is captured
        with pytest.raises(ValueError, match="graph"):
            pipe.predict_batch(pages, _maps_override=mo)
        with pytest.raises(ValueError, match="graph"):
            rec.recognize_start_graph(torch.zeros((1, 224, 320, 3), dtype=torch.uint8, device="cuda"),
                                      torch.zeros((1, 8), dtype=torch.int32, device="cuda"), [(0, 1)], lm=lm)
    finally:
        pipe.lm, pipe.lm_weight, pipe.lexicon, rec.use_graphs = None, 0.5, None, False
