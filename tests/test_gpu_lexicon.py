"""The lexicon-constrained beam decode on the device: msocr_attn_decode with lexicon (csrc/attn_general_lexicon.hip
on the general route, csrc/attn_lexicon_mfma.hip on the matrix cores) on the decoder fixtures of test_gpu_seq_f64.py (its inputs, decoders, oracle
and bounds), then the switch through TRBA and Pipeline on test_gpu_nbest.py's pipeline fixture.

(1) Structural invariants, no tolerance, every row: node_out is the host trie walk of every slot's back-traced token path (-1 exactly
    where the walk leaves the trie or the slot was filled from a -inf candidate), the finalized ids are a lexicon word followed by EOS,
    slots are in descending score order, fin_step is the first step at which every slot is done or dead.
(2) A lexicon of 6 words under 8 slots: the search is exhaustive, so the device's ranking of its finite ranks must be the float64
    ranking of the six words' joint log-probabilities (teacher-forced replay), on every row whose adjacent score gaps exceed
    DECISIVE_FACTOR * e_dev / tau; logp of every finite rank within test_gpu_nbest.py's bound of the float64 sum.
(3) 200 words: the same constrained beam search written here on the oracle's Attention in float64, one row at a time; ids and finish
    step equal on the rows it decides by more than DECISIVE_FACTOR * e_dev / tau (test_gpu_seq_f64.py (b)).
(4) Identities, bit for bit: a one-word lexicon against the forced decode of that word; batch composition; the two kernel families
    against each other on decisive rows.
(5) MSOCR_E_ARG from the C ABI.  (6) TRBA.predict / Pipeline.lexicon.
The fixtures of (2) and (3) were checked on the CPU beforehand: with E_REL_MAX * max|logit| standing in for e_dev the float64 search
alone leaves 37/37 rows decisive in (2) and at least 34/37 in every case of (3)."""
import numpy as np
import pytest
import torch

from attn_call import attn_decode
from test_gpu_nbest import _pages_and_maps, _pipe
from test_gpu_seq_f64 import (B_DEF, DECISIVE_FACTOR, DECISIVE_MIN_FRACTION, E_REL_MAX, EOS, SOS, T_DEF, TAU, _attn_buffers, _inputs,
                              _kernel, _oracle, _replay)

pytestmark = pytest.mark.gpu

E_ARG = -1
STEPS = 9
ALPHA = 0.9


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ lexicons and launches
def _itos(V):
    return ["<PAD>", "<SOS>", "<EOS>"] + [chr(0x400 + i) for i in range(V - 3)]


_LEX = {}


def _lexicon(V, steps, n_words=200, seed=7, extra=()):
    """Seeded random words over the charset of V tokens, lengths 1 .. steps - 1 (one of them of length steps - 1); the first two
    symbols come from 12 tokens, so prefixes are shared and the root has more children than the beam has slots."""
    from manuscript_ocr_amd.recognizers import Lexicon
    key = (V, steps, n_words, seed, tuple(extra))
    if key not in _LEX:
        rng = np.random.default_rng(seed + 1000 * V + steps)
        itos = _itos(V)
        head, body = rng.choice(np.arange(3, V), 12, replace=False), rng.choice(np.arange(3, V), min(40, V - 3), replace=False)
        words = []
        for i in range(n_words):
            L = steps - 1 if i == 0 else int(rng.integers(1, steps))
            words.append("".join(itos[int(rng.choice(head if k < 2 else body))] for k in range(L)))
        _LEX[key] = Lexicon(list(extra) + words, itos, steps)
    return _LEX[key]


def _chunks(fin_plain):
    """Two reference chunks from a plain run's finish steps, as test_gpu_nbest.py forms them: chunk 0 holds the rows that finish first,
    so the matrix-core kernel can leave it before the last step (one chunk when all rows finish together)."""
    cid = (fin_plain > np.median(fin_plain)).astype(np.int32)
    csz = np.bincount(cid).astype(np.int32)
    return cid, (torch.from_numpy(cid).cuda(), torch.from_numpy(csz).cuda(), torch.zeros(2 * len(csz), dtype=torch.int32, device="cuda"))


def _decode(dec, bH, pH, steps, K, alpha, tau, lex, early, ctx_gates=None):
    """One constrained decode -> host arrays: the four parts of the workspace, fin, nodes, and t_run (early: the chunk's largest finish
    step, what the product would pass on; else the row's own), plus the device workspace for finalize / n-best."""
    B, V = bH.shape[0], dec.V
    cid, chunks = None, None
    if early:
        cid, chunks = _chunks(dec.beam(bH, pH, steps, K, alpha, tau, SOS, EOS, None, None, ctx_gates=ctx_gates, lexicon=lex)[1].cpu().numpy())
    ws, fin, _lp, aws, nodes = dec.beam(bH, pH, steps, K, alpha, tau, SOS, EOS, None, chunks, ctx_gates=ctx_gates, lexicon=lex)
    torch.cuda.synchronize()
    fin_h = fin.cpu().numpy()
    trun = np.array([fin_h[cid == c].max() for c in range(cid.max() + 1)], dtype=np.int32)[cid] if early else fin_h.copy()
    buf = ws.cpu().numpy()
    n = B * steps * K
    lg = buf[:n * V * 4].view(np.float32).reshape(B, steps, K, V)
    back = buf[n * V * 4:n * V * 4 + n * 4].view(np.int32).reshape(B, steps, K)
    tokv = buf[n * V * 4 + n * 4:n * V * 4 + 2 * n * 4].view(np.int32).reshape(B, steps, K)
    best = buf[n * V * 4 + 2 * n * 4:n * V * 4 + 2 * n * 4 + B * steps * 4].view(np.int32).reshape(B, steps)
    return dict(ws=ws, aws=aws, lg=lg, back=back, tokv=tokv, best=best, fin=fin_h, trun=trun, nodes=nodes.cpu().numpy())


def _finalize(dec, r, K, steps):
    B = len(r["trun"])
    lg, ids = dec.beam_finalize(r["ws"], B, steps, K, torch.from_numpy(r["trun"]).cuda())
    return lg.cpu().numpy(), ids.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (1) structural invariants
KERNEL_CASES = [
    # (id, H, V, K, steps, kernel): see test_gpu_seq_f64._kernel
    ("mfma-K8", 256, 194, 8, STEPS, "auto"),
    ("mfma-K3", 256, 194, 3, STEPS, "auto"),
    ("mfma-exact-K8", 256, 194, 8, STEPS, "exact"),
    ("mfma-exact-K3", 256, 194, 3, STEPS, "exact"),
    ("general-H256-K8", 256, 194, 8, STEPS, "valu"),
    ("general-H64-V512-K16", 64, 512, 16, STEPS, "auto"),
    ("general-H512-V257-K8", 512, 257, 8, STEPS, "auto"),
    ("mfma-K8-steps25", 256, 194, 8, 25, "auto"),
    ("general-H128-K8-steps64", 128, 194, 8, 64, "auto"),
]


def _expected_states(lex, r, K, steps):
    """The host's walk, forward over the steps: for every (row, step, slot) the node the back-traced token path leads to, whether the
    hypothesis is done, and whether its score is finite (slot 0 starts at 0, the others at -inf; a candidate is finite iff its parent
    is and the token is allowed there)."""
    B = len(r["fin"])
    node = np.full((B, steps, K), -2, dtype=np.int64)
    done = np.zeros((B, steps, K), dtype=bool)
    finite = np.zeros((B, steps, K), dtype=bool)
    term = lex.terminal
    for b in range(B):
        pn, pd, pf = [0] * K, [False] * K, [k == 0 for k in range(K)]
        for s in range(int(r["trun"][b])):
            cn, cd, cf = [], [], []
            for k in range(K):
                src, tok = int(r["back"][b, s, k]), int(r["tokv"][b, s, k])
                assert 0 <= src < K and 0 <= tok < lex.num_classes, (b, s, k, src, tok)
                if pn[src] < 0:
                    ok, nn = False, -1
                elif pd[src]:
                    ok, nn = tok == EOS, pn[src]
                elif tok == EOS:
                    ok, nn = bool(term[pn[src]]), pn[src]
                else:
                    nn = lex.walk(pn[src], tok)
                    ok = nn >= 0
                f = pf[src] and ok
                n2 = nn if f else -1
                cn.append(n2), cf.append(f), cd.append(pd[src] or tok == EOS or n2 < 0)
            node[b, s], done[b, s], finite[b, s] = cn, cd, cf
            pn, pd, pf = cn, cd, cf
    return node, done, finite


def _scores64(r, K, steps, tau, alpha, finite):
    """Every slot's score after every step, recomputed in float64 from the workspace's own logits (already divided by tau): the
    parent's score plus log_softmax(logits of the parent slot)[token], 0 for the EOS a finished hypothesis is extended by."""
    B = len(r["fin"])
    sc = np.full((B, steps, K), -np.inf)
    for b in range(B):
        prev, pdone = np.where(np.arange(K) == 0, 0.0, -np.inf), np.zeros(K, dtype=bool)
        for s in range(int(r["trun"][b])):
            x = r["lg"][b, s].astype(np.float64)
            m = x.max(-1, keepdims=True)
            lsm = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))
            src, tok = r["back"][b, s], r["tokv"][b, s]
            step = np.where(pdone[src], 0.0, lsm[src, tok])
            cur = np.where(finite[b, s], prev[src] + step, -np.inf)
            sc[b, s] = cur
            pdone = pdone[src] | (tok == EOS)
            prev = cur
    return sc


@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("what,H,V,K,steps,kernel", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_structural_invariants(cuda, monkeypatch, what, H, V, K, steps, kernel, early):
    B, T = B_DEF, T_DEF
    dec = _kernel(monkeypatch, V, H, kernel)
    assert dec._matrix_core(T, K) == what.startswith("mfma"), "the case must run on the kernel it names"
    lex = _lexicon(V, steps)
    assert max(len(w) for w in lex.words) == steps - 1
    bH, pH = _inputs(B, T, H, V)
    r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lex, early)
    trun, fin = r["trun"], r["fin"]
    assert ((fin >= 1) & (fin <= steps)).all() and (trun >= fin).all()
    node, done, finite = _expected_states(lex, r, K, steps)
    written = np.arange(steps)[None, :, None] < trun[:, None, None]
    w3 = np.broadcast_to(written, node.shape)
    assert np.array_equal(r["nodes"][w3], node[w3]), np.argwhere((r["nodes"] != node) & w3)[:8].tolist()
    assert ((r["nodes"][w3] >= -1) & (r["nodes"][w3] < lex.n_nodes)).all()
    # fin_step: the first step at which every slot is done or dead
    alld = done.all(-1) & written[:, :, 0]
    fin_exp = np.where(alld.any(1), alld.argmax(1) + 1, steps)
    assert np.array_equal(fin, fin_exp), np.flatnonzero(fin != fin_exp)[:8].tolist()
    # slot order: the finite slots first, in non-increasing score order.  The device ranks by f32 scores; the float64 recomputation
    # from the same logits differs from them by the rounding of up to `steps` f32 additions and log-sum-exps of numbers of size
    # max|score|: 4 * steps * 2^-24 * max|score| bounds that generously.
    sc = _scores64(r, K, steps, TAU, ALPHA, finite)
    assert not (finite[:, :, 1:] & ~finite[:, :, :-1])[np.broadcast_to(written, finite[:, :, 1:].shape)].any(), "a dead slot before a live one"
    fs = np.where(finite, sc, 0.0)
    tol = 4 * steps * 2.0 ** -24 * float(np.abs(fs).max())
    both = finite[:, :, 1:] & finite[:, :, :-1] & written
    assert (sc[:, :, :-1][both] >= sc[:, :, 1:][both] - tol).all(), (what, tol)
    assert (r["best"][written[:, :, 0]] == 0).all(), "the best slot is the first"
    # the finalized ids: a lexicon word, EOS, then EOS up to t_run and -1 behind
    _, ids = _finalize(dec, r, K, steps)
    n_long = 0
    for b in range(B):
        k = lex.find(ids[b])
        assert k >= 0, (b, ids[b].tolist())
        L = len(lex.words[k])
        n_long += L == steps - 1
        assert (ids[b, L:trun[b]] == EOS).all() and (ids[b, trun[b]:] == -1).all() and L + 1 <= fin[b], (b, ids[b].tolist())
        assert node[b, fin[b] - 1, 0] >= 0 and lex.word_of_node[node[b, fin[b] - 1, 0]] == k
    print(f"[lexicon] {what} {'chunk exit' if early else 'all steps'}: finish steps {fin.min()}..{fin.max()}, t_run {trun.min()}..{trun.max()}, "
          f"dead slots at the last step {int((node[np.arange(B), trun - 1] < 0).sum())}/{B * K}, rows reading the longest word {n_long}")


# ------------------------------------------------------------------------------------------------ float64 references
def _oracle_dev(att):
    return next(att.parameters()).device


def _search64(att, bH_row, lex, steps, K, alpha, tau):
    """The constrained beam search in the oracle's arithmetic (Attention.beam, oracle/trba_model.py:166-224) on one row in att's dtype,
    with the two additions of DESIGN.md section 4.15: a trie node per hypothesis, and the mask where the candidates are formed (no renormalisation: the
    log-softmax is over the full row).  Ties: larger value, then smaller flat index.  -> (ids of the best hypothesis up to the finish
    step, finish step, smallest top-K boundary gap over finite candidates, final best-minus-second score)."""
    dev, fd, V, H = bH_row.device, bH_row.dtype, att.num_classes, att.hidden_size
    toks = [[SOS] for _ in range(K)]
    score = torch.full((K,), float("-inf"), dtype=fd, device=dev)
    score[0] = 0.0
    bh, bc = torch.zeros(K, H, dtype=fd, device=dev), torch.zeros(K, H, dtype=fd, device=dev)
    node, done = [0] * K, [False] * K
    rep = bH_row.expand(K, -1, -1)
    bgap, fin = np.inf, steps
    for t in range(steps):
        last = torch.tensor([tk[-1] for tk in toks], device=dev)
        h1, c1 = att.attention_cell((bh, bc), rep, att._onehot(last, fd))
        logits = att._mask(att.generator(h1))
        if tau != 1.0:
            logits = logits / max(tau, 1e-6)
        logp = torch.log_softmax(logits, -1)
        mask = torch.zeros(K, V, dtype=torch.bool)
        for k in range(K):
            if node[k] < 0:
                continue
            if done[k]:
                mask[k, EOS] = True
                continue
            lo, hi = lex.edge_begin[node[k]], lex.edge_begin[node[k] + 1]
            mask[k, lex.edge_tok[lo:hi]] = True
            if lex.terminal[node[k]]:
                mask[k, EOS] = True
        mask = mask.to(dev)
        dn = torch.tensor(done, device=dev)
        logp = torch.where(dn[:, None], torch.zeros_like(logp), logp)
        logp = torch.where(mask, logp, torch.full_like(logp, float("-inf")))
        total = score[:, None] + logp
        lp = ((5.0 + (t + 1)) ** alpha) / (6.0 ** alpha) if alpha > 0 else 1.0
        cand = (total / lp if alpha > 0 else total).reshape(-1)
        order = torch.sort(cand, descending=True, stable=True)  # stable: equal values keep the smaller flat index first
        top, idx = order.values[:K], order.indices[:K]
        if bool(torch.isfinite(order.values[K])):
            bgap = min(bgap, float(order.values[K - 1] - order.values[K]))
        src, nxt = (idx // V).tolist(), (idx % V).tolist()
        topl = top.tolist()
        n2, d2 = [], []
        for k in range(K):
            ended = done[src[k]] or nxt[k] == EOS
            nn = node[src[k]] if ended else lex.walk(node[src[k]], nxt[k])
            if not np.isfinite(topl[k]):
                nn = -1
            n2.append(nn), d2.append(ended or nn < 0)
        si = torch.tensor(src, device=dev)
        bh, bc = h1[si], c1[si]
        toks = [toks[src[k]] + [nxt[k]] for k in range(K)]
        score = top * lp if alpha > 0 else top
        node, done = n2, d2
        if all(done):
            fin = t + 1
            break
    sc = score.tolist()
    best = int(np.argmax(sc))
    rest = sorted((x for i, x in enumerate(sc) if i != best and np.isfinite(x)), reverse=True)
    sgap = sc[best] - rest[0] if rest else np.inf
    return toks[best][1:], fin, bgap, sgap


_REF = {}


def _reference_search(H, V, K, T, steps, lex, att=None, bH=None):
    key = (H, V, K, T, steps, id(lex))
    if key not in _REF:
        att = att if att is not None else _oracle(V, H, None, "f64")
        bH = bH if bH is not None else _inputs(B_DEF, T, H, V)[0]
        with torch.no_grad():
            _REF[key] = [_search64(att, bH[b:b + 1].to(_oracle_dev(att)).double(), lex, steps, K, ALPHA, TAU) for b in range(bH.shape[0])]
    return _REF[key]


def _path_logits(r, b, slot, at, n):
    """The workspace logits along the hypothesis that sits in `slot` after step `at`, its first n steps: [n, V]."""
    out, cur = [], slot
    for t in range(at, -1, -1):
        cur = int(r["back"][b, t, cur])
        out.append(r["lg"][b, t, cur])
    return np.stack(out[::-1])[:n]


# ------------------------------------------------------------------------------------------------ (2) exhaustive lexicon
SIX_SEED = 3


def _six_words(V, steps):
    """Six words under eight slots, one a prefix of another: the beam holds every live prefix, so the search is exhaustive."""
    rng = np.random.default_rng(SIX_SEED)
    itos = _itos(V)
    ws = ["".join(itos[int(t)] for t in rng.integers(3, V, size=L)) for L in (1, 3, 4, 6, steps - 1)]
    return ws + [ws[2][:2]]


def _word_scores64(att, bH, lex, steps, tau, alpha):
    """float64 joint log-probability of every lexicon word and its EOS on every row, by teacher-forced replay: (score [B, W] = the sum
    over the word's len + 1 steps of log_softmax(logits / tau), divided by the reference's length penalty at the row's last step, the
    raw sums [B, W], the replayed logits / tau per word, max |logit| before the temperature)."""
    B = bH.shape[0]
    W = len(lex.words)
    sums, logits, scale = np.zeros((B, W)), [], 0.0
    itos = _itos(lex.num_classes)
    enc = [[itos.index(c) for c in w] for w in lex.words]
    for j, ids in enumerate(enc):
        tok_in = torch.tensor([[SOS] + ids + [EOS] * (steps - 1 - len(ids))] * B)
        lg = _replay(att, bH, tok_in)
        scale = max(scale, float(lg[:, :len(ids) + 1].abs().max()))
        lg = lg / max(tau, 1e-6) if tau != 1.0 else lg
        lsm = torch.log_softmax(lg, -1).cpu().numpy()
        tgt = ids + [EOS]
        sums[:, j] = sum(lsm[:, t, tgt[t]] for t in range(len(tgt)))
        logits.append(lg.cpu().numpy())
    t_last = max(len(e) for e in enc) + 1  # every row's search ends when its longest word has its EOS
    lp = ((5.0 + t_last) ** alpha) / (6.0 ** alpha) if alpha > 0 else 1.0
    return sums / lp, sums, logits, scale, enc


@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("alpha", [0.0, 0.9])
@pytest.mark.parametrize("kernel", ["auto", "exact", "valu"])
def test_exhaustive_lexicon_against_f64(cuda, monkeypatch, kernel, alpha, early):
    from manuscript_ocr_amd.recognizers import Lexicon
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    dec = _kernel(monkeypatch, V, H, kernel)
    lex = Lexicon(_six_words(V, steps), _itos(V), steps)
    assert len(lex) == 6
    bH, pH = _inputs(B, T, H, V)
    r = _decode(dec, bH, pH, steps, K, alpha, TAU, lex, early)
    assert (r["fin"] == steps).all()  # the longest word has steps - 1 symbols: every search runs to the last step
    trun_d = torch.from_numpy(r["trun"]).cuda()
    ids, _prob, _conf, logp = (t.cpu().numpy() for t in dec.beam_nbest(r["ws"], B, steps, K, trun_d, K, EOS))
    score, sums, ref_logits, scale, _enc = _word_scores64(_oracle(V, H, None, "f64"), bH.double(), lex, steps, TAU, alpha)
    last = r["nodes"][:, steps - 1]
    live = last >= 0
    assert (live.sum(1) == 6).all() and live[:, :6].all(), "six finite ranks, in front"
    rank_word = np.array([[lex.find(ids[b, k]) for k in range(6)] for b in range(B)])
    assert (np.sort(rank_word, 1) == np.arange(6)).all(), "every word is in the beam exactly once"
    assert np.array_equal(rank_word, lex.word_of_node[last[:, :6]])
    # e_dev: the device's logits along every rank's path against the replay of that word
    e_dev = 0.0
    for b in range(B):
        for k in range(6):
            n = len(lex.words[rank_word[b, k]]) + 1
            e_dev = max(e_dev, float(np.abs(_path_logits(r, b, k, steps - 1, n).astype(np.float64) - ref_logits[rank_word[b, k]][b, :n]).max()))
    assert e_dev <= E_REL_MAX * scale, (e_dev, scale)
    delta = DECISIVE_FACTOR * e_dev / TAU
    order = np.argsort(-score, 1, kind="stable")
    gaps = -np.diff(np.take_along_axis(score, order, 1), axis=1)
    decisive = (gaps > delta).all(1)
    bad = [b for b in np.flatnonzero(decisive) if not np.array_equal(rank_word[b], order[b])]
    tol = 2 * steps * E_REL_MAX * scale
    err = np.abs(logp[:, :6].astype(np.float64) - np.take_along_axis(sums, rank_word, 1))
    print(f"[lexicon] exhaustive {kernel} alpha {alpha} {'chunk exit' if early else 'all steps'}: e_dev {e_dev:.2e} ({e_dev / scale:.1e} of "
          f"max|logit| {scale:.2f}), decisive rows {int(decisive.sum())}/{B} at {delta:.2e}, largest |logp - f64| {err.max():.2e} (allowed {tol:.2e})")
    assert not bad, bad
    assert decisive.mean() >= DECISIVE_MIN_FRACTION
    assert np.isfinite(logp[:, :6]).all() and (err <= tol).all(), float(err.max())


# ------------------------------------------------------------------------------------------------ (3) pruned search
SEARCH_CASES = [c for c in KERNEL_CASES if c[4] == STEPS]


@pytest.mark.parametrize("early", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("what,H,V,K,steps,kernel", SEARCH_CASES, ids=[c[0] for c in SEARCH_CASES])
def test_pruned_search_against_f64_constrained_beam_search(cuda, monkeypatch, what, H, V, K, steps, kernel, early):
    B, T = B_DEF, T_DEF
    dec = _kernel(monkeypatch, V, H, kernel)
    lex = _lexicon(V, steps)
    bH, pH = _inputs(B, T, H, V)
    r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lex, early)
    lg, ids = _finalize(dec, r, K, steps)
    fin = r["fin"]
    # e_dev along the finalized path, as test_gpu_seq_f64._beam_case measures it
    tok_in = torch.from_numpy(np.concatenate([np.full((B, 1), SOS), np.where(ids[:, :-1] >= 0, ids[:, :-1], EOS)], 1).astype(np.int64))
    r64 = (_replay(_oracle(V, H, None, "f64"), bH.double(), tok_in) / TAU).cpu().numpy()
    valid = np.arange(steps)[None, :] < fin[:, None]
    e_dev, scale = float(np.abs(lg[valid].astype(np.float64) - r64[valid]).max()), float(np.abs(r64[valid]).max()) * TAU
    assert e_dev <= E_REL_MAX * scale, (e_dev, scale)
    delta = DECISIVE_FACTOR * e_dev / TAU
    ref = _reference_search(H, V, K, T, steps, lex)
    decisive, bad = 0, []
    for b, (oid, ofin, bgap, sgap) in enumerate(ref):
        if min(bgap, sgap) > delta:
            decisive += 1
            if not (ofin == fin[b] and np.array_equal(ids[b, :ofin], oid)):
                bad.append((b, int(fin[b]), ofin))
    print(f"[lexicon] search {what} {'chunk exit' if early else 'all steps'}: e_dev {e_dev:.2e} ({e_dev / scale:.1e} of max|logit| {scale:.2f}), "
          f"decisive rows {decisive}/{B} at {delta:.2e}")
    assert not bad, (what, bad)
    assert decisive / B >= DECISIVE_MIN_FRACTION, f"degenerate fixture: {decisive}/{B} decisive rows ({what})"


# ------------------------------------------------------------------------------------------------ (4) identities
def test_single_word_lexicon_equals_the_forced_decode(cuda, monkeypatch):
    """{w}: the only path is w.  General kernel, temperature 1, no length penalty: slot 0's logits are the forced decode's for w bit for
    bit, and the rank-0 logp is msocr_seq_logp of that forced pass."""
    from manuscript_ocr_amd.recognizers import Lexicon
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    dec = _kernel(monkeypatch, V, H, "valu")
    itos = _itos(V)
    for w_ids in ([17], [40, 9, 133, 9, 77], list(range(50, 50 + steps - 1))):
        lex = Lexicon(["".join(itos[t] for t in w_ids)], itos, steps)
        bH, pH = _inputs(B, T, H, V)
        r = _decode(dec, bH, pH, steps, K, 0.0, 1.0, lex, False)
        n = len(w_ids) + 1
        assert (r["fin"] == n).all()
        _, ids = _finalize(dec, r, K, steps)
        assert (ids[:, :n] == np.array(w_ids + [EOS])).all()
        assert (r["nodes"][:, :n, 1:] == -1).all() and (r["nodes"][:, :n, 0] >= 0).all()
        tok_in = torch.tensor([[SOS] + w_ids + [0] * (steps - n)] * B, dtype=torch.int32).cuda()
        flg, _al = dec.forced(bH, pH, tok_in, SOS, None)
        assert (r["back"][:, :n, 0] == 0).all()
        assert np.array_equal(r["lg"][:, :n, 0].view(np.int32), flg.cpu().numpy()[:, :n].view(np.int32)), w_ids
        trun_d = torch.full((B,), n, dtype=torch.int32, device="cuda")
        tgt = torch.tensor([w_ids + [EOS] + [0] * (steps - n)] * B, dtype=torch.int32).cuda()
        _lps, lp = dec.seq_logp(flg, tgt, trun_d, 1.0)
        _i, _p, _c, logp = dec.beam_nbest(r["ws"], B, steps, K, trun_d, 1, EOS)
        assert np.array_equal(logp.cpu().numpy()[:, 0].view(np.int32), lp.cpu().numpy().view(np.int32)), w_ids


@pytest.mark.parametrize("kernel", ["auto", "valu"])
def test_constrained_decode_does_not_depend_on_batch_composition(cuda, monkeypatch, kernel):
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    dec = _kernel(monkeypatch, V, H, kernel)
    lex = _lexicon(V, steps)
    bH, pH = _inputs(B, T, H, V)
    cg = dec.ctx_gates(bH).view(B, -1)

    def run(rows):
        idx = torch.as_tensor(rows, device=bH.device)
        c = cg[idx].contiguous().view(len(rows) * T, -1)
        r = _decode(dec, bH[idx].contiguous(), pH[idx].contiguous(), steps, K, ALPHA, TAU, lex, False, ctx_gates=c)
        lg, ids = _finalize(dec, r, K, steps)
        w = np.arange(steps)[None, :] < r["fin"][:, None]
        return np.where(w[..., None], lg, 0).view(np.int32), ids, r["fin"], np.where(w[..., None], r["nodes"], -9)

    full = run(list(range(B)))
    perm = np.random.default_rng(5).permutation(B).tolist()
    permuted = run(perm)
    for j, b in enumerate(perm):
        assert all(np.array_equal(x[b], y[j]) for x, y in zip(full, permuted)), ("permuted", b)
    for b in range(B):
        alone = run([b])
        assert all(np.array_equal(x[b], y[0]) for x, y in zip(full, alone)), ("alone", b)


def test_matrix_core_and_general_kernels_agree_on_decisive_rows(cuda, monkeypatch):
    H, V, K, B, T, steps = 256, 194, 8, B_DEF, T_DEF, STEPS
    lex = _lexicon(V, steps)
    bH, pH = _inputs(B, T, H, V)
    out = {}
    for kernel in ("auto", "valu"):
        dec = _kernel(monkeypatch, V, H, kernel)
        assert dec._matrix_core(T, K) == (kernel == "auto")
        r = _decode(dec, bH, pH, steps, K, ALPHA, TAU, lex, False)
        out[kernel] = (r, _finalize(dec, r, K, steps)[1])
    delta = DECISIVE_FACTOR * E_REL_MAX * 13.95 / TAU  # the largest threshold test (3) can apply at its logit scale
    rows = [b for b, (_o, _f, bgap, sgap) in enumerate(_reference_search(H, V, K, T, steps, lex)) if min(bgap, sgap) > delta]
    assert len(rows) >= DECISIVE_MIN_FRACTION * B
    (ra, ia), (rv, iv) = out["auto"], out["valu"]
    for b in rows:
        f = ra["fin"][b]
        assert f == rv["fin"][b] and np.array_equal(ia[b], iv[b]) and np.array_equal(ra["nodes"][b, :f], rv["nodes"][b, :f]), b


# ------------------------------------------------------------------------------------------------ (5) C ABI
def _lexicon_rc(lex, B, T, H, V, steps, K, hoisted, null=None, n_nodes=None, n_edges=None):
    """Device buffers sized for the (rejected) shape: a kernel launched by a broken check runs on valid memory."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    b, aw, asw = _attn_buffers(B, T, H, V, steps, K)
    aws = torch.zeros((B, steps, K, T), dtype=torch.float32, device="cuda")
    nodes = torch.zeros((B, steps, K), dtype=torch.int32, device="cuda")
    src = lex.to("cuda")[4]
    la = nat.LexiconArrays()
    for f in ("edge_begin", "edge_tok", "edge_child", "terminal"):
        setattr(la, f, None if null == f else getattr(src, f))
    la.n_nodes = lex.n_nodes if n_nodes is None else n_nodes
    la.n_edges = lex.n_edges if n_edges is None else n_edges
    bufs = {"batch_H": b["bH"], "proj_H": b["pH"], "w": aw, "lp": b["lp"], "fin_step_out": b["fin"], "workspace": b["ws"],
            "alpha_out": None if null == "alpha_ws" else aws, "lexicon": None if null == "lex" else la,
            "node_out": None if null == "node_out" else nodes}
    if hoisted:
        bufs["ctx_gates"] = b["ctx"]
    rc = attn_decode(nat.ATTN_BEAM, bufs, B=B, T=T, H=H, V=V, steps=steps, beam=K, temperature=1.7, sos_id=SOS, eos_id=EOS, blank_id=-1,
                     stream=ops._stream())
    torch.cuda.synchronize()
    return rc


def test_c_abi_rejects_null_members_and_shapes_outside_the_envelope(cuda):
    B, T, steps = 2, T_DEF, STEPS
    lex = _lexicon(194, steps)
    for hoisted in (False, True):
        ok = dict(lex=lex, B=B, T=T, H=256, V=194, steps=steps, K=8, hoisted=hoisted)
        assert _lexicon_rc(**ok) == 0  # same buffers: a rejection below is the check, not the buffers
        for null in ("edge_begin", "edge_tok", "edge_child", "terminal", "lex", "node_out", "alpha_ws"):
            assert _lexicon_rc(**ok, null=null) == E_ARG, (hoisted, null)
        assert _lexicon_rc(**ok, n_nodes=0) == E_ARG and _lexicon_rc(**ok, n_edges=-1) == E_ARG
        assert _lexicon_rc(**{**ok, "steps": 65}) == E_ARG
        assert _lexicon_rc(**{**ok, "T": 65}) == E_ARG
        assert _lexicon_rc(**{**ok, "V": 513}) == E_ARG
        assert _lexicon_rc(**{**ok, "K": 17}) == E_ARG
        assert _lexicon_rc(**{**ok, "H": 96}) == E_ARG
    gen = dict(lex=lex, B=B, T=T, steps=steps, hoisted=False)
    assert _lexicon_rc(**gen, H=320, V=194, K=13) == E_ARG  # 13 x 320 > 4096
    assert _lexicon_rc(**gen, H=512, V=194, K=9) == E_ARG
    assert _lexicon_rc(**gen, H=512, V=194, K=8) == 0 and _lexicon_rc(**gen, H=64, V=512, K=16) == 0
    hst = dict(lex=lex, B=B, steps=steps, hoisted=True)
    assert _lexicon_rc(**hst, T=T, H=128, V=194, K=8) == E_ARG   # the matrix-core kernel takes H 256 only
    assert _lexicon_rc(**hst, T=T, H=256, V=257, K=8) == E_ARG
    assert _lexicon_rc(**hst, T=49, H=256, V=194, K=8) == E_ARG
    assert _lexicon_rc(**hst, T=T, H=256, V=194, K=9) == E_ARG


# ------------------------------------------------------------------------------------------------ (6) through the product
def _lexicon40(rec):
    from manuscript_ocr_amd.recognizers import Lexicon
    rng = np.random.default_rng(40)
    symbols = [s for s in rec.itos if len(s) == 1 and not s.isspace()]
    words = ["".join(symbols[int(i)] for i in rng.integers(0, len(symbols), size=int(rng.integers(1, 11)))) for _ in range(40)]
    return Lexicon(words, rec.stoi, rec.max_length)


def _named(pages):
    return [[w for blk in p.blocks for w in blk.words if w.text is not None] for p in pages]


@pytest.fixture(scope="module")
def lexpipe(cuda):
    """The pipeline of test_gpu_nbest.py, its pages, the pages read without a lexicon (the attribute never set) and with one."""
    pipe = _pipe()
    pages, mo = _pages_and_maps()
    assert pipe.lexicon is None
    off = pipe.predict_batch(pages, _maps_override=mo)
    lex = _lexicon40(pipe.recognizer)
    assert len(lex) == 40
    pipe.lexicon = lex
    on = pipe.predict_batch(pages, _maps_override=mo)
    pipe.lexicon = None
    return pipe, pages, mo, off, lex, on


def _base(pages):
    return [[(w.text, w.recognition_confidence, w.lexicon_index) for w in p] for p in _named(pages)]


def test_pipeline_lexicon_with_the_other_switches(lexpipe):
    from manuscript_ocr_amd.detectors._types import LexAlternative, LexWord
    pipe, pages, mo, off, lex, on = lexpipe
    n_words = 0
    drop = {"blocks": {"__all__": {"words": {"__all__": {"text", "recognition_confidence"}}}}}
    for p_on, p_off in zip(on, off):
        assert p_on.model_dump(exclude=drop) == p_off.model_dump(exclude=drop)
        for w, w0 in zip(p_on.blocks[0].words, p_off.blocks[0].words):
            assert (w.text is None) == (w0.text is None)
            if w.text is None:
                continue
            assert type(w) is LexWord and w.text in lex.words and lex.words[w.lexicon_index] == w.text
            assert w.alternatives == [] and w.chars == []
            n_words += 1
    assert n_words == sum(w.text is not None for p in off for w in p.blocks[0].words) > 0
    assert len({w.text for p in _named(on) for w in p}) > 1, "the lexicon's words are told apart"
    base = _base(on)
    try:
        pipe.lexicon, pipe.n_best = lex, 3
        alt = pipe.predict_batch(pages, _maps_override=mo)
        assert _base(alt) == base
        n_second = 0
        for p in _named(alt):
            for w in p:
                assert 1 <= len(w.alternatives) <= 3 and all(type(a) is LexAlternative for a in w.alternatives)
                assert w.alternatives[0].text == w.text and w.alternatives[0].lexicon_index == w.lexicon_index
                assert all(lex.words[a.lexicon_index] == a.text for a in w.alternatives)
                assert len({a.text for a in w.alternatives}) == len(w.alternatives)
                lps = [a.logp for a in w.alternatives]
                assert all(x >= y for x, y in zip(lps, lps[1:])) and all(np.isfinite(lps)), lps
                n_second += len(w.alternatives) > 1
        assert n_second > 0
        for switch in ("char_details", "group_lines", "rectify_crops"):
            setattr(pipe, switch, True)
            got = pipe.predict_batch(pages, _maps_override=mo)
            setattr(pipe, switch, False)
            for p in _named(got):
                for w in p:
                    assert type(w) is LexWord and lex.words[w.lexicon_index] == w.text and w.alternatives[0].text == w.text
                    assert len(w.chars) == (len(w.text) if switch == "char_details" else 0)
                    assert switch != "char_details" or "".join(c.char for c in w.chars) == w.text
            if switch != "rectify_crops":  # rectified crops are other pixels
                assert _base(got) == base
        pipe.n_best, pipe.device_order = 0, False
        assert _base(pipe.predict_batch(pages, _maps_override=mo)) == base
    finally:
        pipe.lexicon, pipe.n_best, pipe.device_order = None, 0, True


def test_predict_with_a_lexicon_and_score_of_its_reading(lexpipe):
    """TRBA.predict on the words' host crops, and TRBA.score of the text it read, at the temperature passed to both."""
    from manuscript_ocr_amd.detectors._types import LexWord
    from test_forced_cpu import STEP_ATOL
    pipe, pages, _mo, _off, lex, on = lexpipe
    rec, tau = pipe.recognizer, 1.3
    for page, arr in zip(on, pages):
        words = [w for w in page.blocks[0].words if w.text is not None]
        crops = [pipe._extract_word_image(arr, np.array(w.polygon, dtype=np.int32)) for w in words]
        res = rec.predict(crops, temperature=tau, n_best=3, return_chars=True, lexicon=lex)
        assert all(set(r) == {"text", "confidence", "lexicon_index", "alternatives", "chars"} for r in res)
        plain = rec.predict(crops, temperature=tau, lexicon=lex)
        assert all(set(r) == {"text", "confidence", "lexicon_index"} for r in plain)
        scored = rec.score(crops, [r["text"] for r in res], temperature=tau)
        for r, p, s in zip(res, plain, scored):
            assert (r["text"], r["confidence"], r["lexicon_index"]) == (p["text"], p["confidence"], p["lexicon_index"])
            assert lex.words[r["lexicon_index"]] == r["text"] and len(r["chars"]) == len(r["text"])
            assert r["alternatives"][0]["text"] == r["text"] and r["alternatives"][0]["lexicon_index"] == r["lexicon_index"]
            # msocr_seq_logp's stated bound: STEP_ATOL per counted step (the symbols and the EOS)
            assert abs(r["alternatives"][0]["logp"] - s["logp"]) <= (len(r["text"]) + 1) * STEP_ATOL, (r["alternatives"][0]["logp"], s["logp"])
    # the generic route with this package's recogniser asks predict for the same
    try:
        pipe.lexicon, pipe.native_fast_path = lex, False
        page = pipe.predict(pages[0])
    finally:
        pipe.lexicon, pipe.native_fast_path = None, True
    named = [w for w in page.blocks[0].words if w.text is not None]
    assert named and all(type(w) is LexWord and lex.words[w.lexicon_index] == w.text for w in named)


def test_no_lexicon_changes_nothing_and_refusals(lexpipe):
    from manuscript_ocr_amd.recognizers import Lexicon
    pipe, pages, mo, off, lex, _on = lexpipe
    rec = pipe.recognizer
    # lexicon = None after a lexicon was used: what the pipeline gave before the attribute was ever set
    assert pipe.lexicon is None
    again = pipe.predict_batch(pages, _maps_override=mo)
    key = lambda ps: [[(type(w).__name__, w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words] for p in ps]
    assert key(again) == key(off) and [p.model_dump() for p in again] == [p.model_dump() for p in off]
    crop = np.full((32, 100, 3), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="greedy|beam"):
        rec.predict([crop], mode="greedy", lexicon=lex)
    with pytest.raises(ValueError, match="max_len"):
        rec.predict([crop], lexicon=Lexicon(lex.words, rec.stoi, rec.max_length - 1))
    with pytest.raises(ValueError, match="charset"):
        rec.predict([crop], lexicon=Lexicon(["ab"], rec.itos + ["\u2603"], rec.max_length))
    try:
        pipe.lexicon = Lexicon(lex.words, rec.stoi, rec.max_length - 1)
        with pytest.raises(ValueError, match="max_len"):
            pipe.predict_batch(pages, _maps_override=mo)
        pipe.lexicon, rec.use_graphs = lex, True  # a graph recogniser: refused at submit, before anything is captured
        with pytest.raises(ValueError, match="graph"):
            pipe.predict_batch(pages, _maps_override=mo)
        with pytest.raises(ValueError, match="graph"):
            rec.recognize_start_graph(torch.zeros((1, 224, 320, 3), dtype=torch.uint8, device="cuda"),
                                      torch.zeros((1, 8), dtype=torch.int32, device="cuda"), [(0, 1)], lexicon=lex)
    finally:
        pipe.lexicon, rec.use_graphs = None, False
