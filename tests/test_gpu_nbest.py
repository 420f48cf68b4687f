"""N-best readings on the device: msocr_attn_beam_nbest against its host twin on the device's own workspaces, rank 0 against
today's finalize + confidence, every rank against the oracle's float64 beam search, the switch through TRBA and Pipeline, and the
argument checks.  Decoder-only cases run on the fixtures of test_gpu_seq_f64.py (its inputs, decoders, oracle and constants).

(a) kernel == host twin: ids exact, floats within 1e-6 relative (two f32 expf / logf roundings on values <= 1).
(b) rank 0 == beam_finalize's ids and, bit for bit, msocr_seq_confidence of the finalized logits.
(c) on rows the float64 search decides by more than G at every top-k boundary and between every pair of consecutive final scores:
    every rank's ids equal the oracle's final hypotheses, EOS from the row's finish step to t_run, |logp - beam_scores| <= 2 * steps *
    E_REL_MAX * max|logit|; at least DECISIVE_MIN_FRACTION of the rows are such rows.
(d) Pipeline.n_best / TRBA.predict(n_best=...): alternatives[0] is the word, non-increasing logp, distinct texts, nothing else moves;
    also on a replayed graph and together with char_details.
(e) MSOCR_E_ARG outside the envelope, ValueError from TRBA.predict."""
import numpy as np
import pytest
import torch

from test_gpu_seq_f64 import (ALPHA, B_DEF, DECISIVE_FACTOR, DECISIVE_MIN_FRACTION, E_REL_MAX, EOS, SOS, STEPS_B, T_DEF, TAU, _inputs,
                              _kernel, _oracle)

pytestmark = pytest.mark.gpu

RTOL = 1e-6
# Threshold of (c): DECISIVE_FACTOR * E_REL_MAX * max|logit| / TAU, the largest threshold test_gpu_seq_f64.py can apply, at that
# file's measured logit scale of 13.95 (1.64e-3), rounded up.  It is a constant: the oracle alone, in float64 on the CPU, leaves 31 of
# 37 (V 194, K 8), 34 of 37 (K 3) and 13 of 16 (V 400, K 12) rows decisive at 2e-3.  The planted decoder's own logits are larger
# (30.4 over the tokens it can emit, 55.6 with the -50 biases of PAD and SOS); the formula evaluated on them gives 3.6e-3 / 6.5e-3,
# at which the float64 search alone leaves 27 / 21 of 37 rows and the fixture, not the kernel, would miss the fraction.  The smaller
# threshold is the stricter one for the code under test: more rows have to match in every rank.
G = 2e-3
assert DECISIVE_FACTOR * E_REL_MAX * 13.95 / TAU <= G
E_ARG = -1
CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ (a) + (b) kernel, twin, rank 0
KERNEL_CASES = [
    # (id, V, H, K, B, T, matrix cores)
    ("mfma-V194-H256-K8-B37", 194, 256, 8, 37, 13, True),   # 4 crops per decode workgroup: the last one partial
    ("general-V400-H128-K12-B16", 400, 128, 12, 16, 20, False),
    ("general-V512-H64-K16-B5", 512, 64, 16, 5, T_DEF, False),
    ("mfma-K1-B1", 194, 256, 1, 1, T_DEF, True),
]


def _twin(ws, B, V, steps, K, n, trun):
    from manuscript_ocr_amd import _native as nat
    buf = ws.cpu().numpy()
    trun = np.ascontiguousarray(trun, dtype=np.int32)
    ids = np.full((B, n, steps), -7, dtype=np.int32)
    prob = np.full((B, n, steps), np.nan, dtype=np.float32)
    conf, logp = np.full((B, n), np.nan, dtype=np.float32), np.full((B, n), np.nan, dtype=np.float32)
    nat.check(nat.lib().msocr_attn_beam_nbest_host(buf.ctypes.data, B, V, steps, K, n, EOS, trun.ctypes.data, ids.ctypes.data,
                                                   prob.ctypes.data, conf.ctypes.data, logp.ctypes.data), "attn_beam_nbest_host")
    return ids, prob, conf, logp


def _rel(a, r):
    a, r = a.astype(np.float64), r.astype(np.float64)
    return float((np.abs(a - r) / np.maximum(np.abs(r), 1e-300))[np.abs(a - r) > 0].max(initial=0.0))


@pytest.mark.parametrize("early_exit", [True, False], ids=["chunk-exit", "all-steps"])
@pytest.mark.parametrize("what,V,H,K,B,T,mfma", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_equals_host_twin_and_rank0_is_todays_result(cuda, monkeypatch, what, V, H, K, B, T, mfma, early_exit):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    steps = STEPS_B
    dec = _kernel(monkeypatch, V, H, "auto", conf=True)  # the planted decoder: its rows finish, so a chunk can stop early
    assert dec._matrix_core(T, K) == mfma, "the case must run on the kernel it names"
    bH, pH = _inputs(B, T, H, V, conf=True)
    if early_exit:
        # two chunks from a plain run's finish steps, as the reference's batch_size slices would form them: a chunk stops at its
        # slowest row, the matrix-core kernel leaves the later steps of the workspace unwritten
        _, fin_plain, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None)
        fp = fin_plain.cpu().numpy()
        cid = (fp > np.median(fp)).astype(np.int32)  # chunk 0: the rows that finish first; one chunk when all finish together
        csz = np.bincount(cid).astype(np.int32)
        chunks = (torch.from_numpy(cid).cuda(), torch.from_numpy(csz).cuda(), torch.zeros(2 * len(csz), dtype=torch.int32, device="cuda"))
        ws, fin, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None, chunks)
        fh = fin.cpu().numpy()
        trun = np.array([fh[cid == c].max() for c in range(len(csz))], dtype=np.int32)[cid]
        if B > 1:
            assert trun.min() < steps, "the planted decoder finishes before the last step"
    else:
        ws, fin, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None)
        trun = np.full(B, steps, dtype=np.int32)
    trun_d = torch.from_numpy(trun).cuda()
    twin = _twin(ws, B, V, steps, K, K, trun)
    lg, ids_fin = dec.beam_finalize(ws, B, steps, K, trun_d)
    conf_fin = torch.empty((B,), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().msocr_seq_confidence(lg.data_ptr(), ids_fin.data_ptr(), trun_d.data_ptr(), B, V, steps, conf_fin.data_ptr(),
                                             ops._stream()), "seq_confidence")
    worst = 0.0
    for n in sorted({1, min(3, K), K}):
        ids, prob, conf, logp = (t.cpu().numpy() for t in dec.beam_nbest(ws, B, steps, K, trun_d, n, EOS))
        assert ids.shape == prob.shape == (B, n, steps) and conf.shape == logp.shape == (B, n)
        # (a)
        assert np.array_equal(ids, twin[0][:, :n]), (what, n)
        for name, a, r in (("prob", prob, twin[1][:, :n]), ("conf", conf, twin[2][:, :n]), ("logp", logp, twin[3][:, :n])):
            assert np.isfinite(a).all(), (what, n, name)
            worst = max(worst, _rel(a, r))
            assert (np.abs(a.astype(np.float64) - r) <= RTOL * np.abs(r.astype(np.float64))).all(), (what, n, name, _rel(a, r))
        beyond = np.broadcast_to(np.arange(steps)[None, None, :] >= trun[:, None, None], ids.shape)
        assert (ids[beyond] == -1).all() and (prob[beyond] == 0).all()
        assert ((ids[~beyond] >= 0) & (ids[~beyond] < V)).all() and (logp <= 0).all() and ((conf >= 0) & (conf <= 1)).all()
        # (b)
        assert np.array_equal(ids[:, 0], ids_fin.cpu().numpy()), (what, n)
        assert np.array_equal(conf[:, 0].view(np.int32), conf_fin.cpu().numpy().view(np.int32)), (what, n)
    print(f"[nbest] {what} {'chunk exit' if early_exit else 'all steps'}: t_run {trun.min()}..{trun.max()}, largest relative distance "
          f"kernel - twin {worst:.2e}")


# ------------------------------------------------------------------------------------------------ (c) the oracle's final hypotheses
ORACLE_CASES = [("V194-H256-K8", 194, 256, 8, B_DEF, T_DEF), ("V194-H256-K3", 194, 256, 3, B_DEF, T_DEF),
                ("V400-H128-K12", 400, 128, 12, 16, 20)]


@pytest.mark.parametrize("what,V,H,K,B,T", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_every_rank_against_the_oracles_f64_beam_search(cuda, monkeypatch, what, V, H, K, B, T):
    steps = STEPS_B
    dec = _kernel(monkeypatch, V, H, "auto", conf=True)
    bH, pH = _inputs(B, T, H, V, conf=True)
    ws, fin, _ = dec.beam(bH, pH, steps, K, ALPHA, TAU, SOS, EOS, None)
    fin_h = fin.cpu().numpy()
    trun = np.full(B, fin_h.max(), dtype=np.int32)  # one chunk: every row runs to the slowest row's finish step
    ids, _prob, _conf, logp = (t.cpu().numpy() for t in dec.beam_nbest(ws, B, steps, K, torch.from_numpy(trun).cuda(), K, EOS))
    att = _oracle(V, H, None, "f64", conf=True)
    rows = []
    with torch.no_grad():
        for b in range(B):
            d = {}
            trace, _ = att.beam(bH[b:b + 1].double(), steps, K, ALPHA, TAU, diag=d)
            rows.append((d["beam_scores"][0], d["beam_tokens"][0], d["boundary_gap"][0], float(trace.abs().max()) * max(TAU, 1e-6)))
    scale = max(r[3] for r in rows)  # the largest |logit| of the oracle's best paths, before the temperature
    g = G
    tol = 2 * steps * E_REL_MAX * scale
    decisive, bad, worst = 0, [], 0.0
    for b, (sc, toks, bgap, _) in enumerate(rows):
        sgap = sc[:-1] - sc[1:] if K > 1 else np.array([np.inf])
        gaps = np.concatenate([np.where(np.isnan(bgap), -np.inf, bgap), np.where(np.isnan(sgap), -np.inf, sgap)])
        if not gaps.min() > g:
            continue
        decisive += 1
        f = toks.shape[1]
        err = np.abs(logp[b].astype(np.float64) - sc)
        worst = max(worst, float(err.max()))
        if not (f == fin_h[b] and np.array_equal(ids[b, :, :f], toks) and (ids[b, :, f:trun[b]] == EOS).all() and (err <= tol).all()):
            bad.append((b, f, int(fin_h[b]), float(err.max())))
    print(f"[nbest] oracle {what}: decisive rows {decisive}/{B} at g {g:.2e} (max|logit| {scale:.2f}); t_run {trun[0]}, finish steps "
          f"{fin_h.min()}..{fin_h.max()}; largest |logp - beam_scores| {worst:.2e} (allowed {tol:.2e})")
    assert not bad, (what, bad)
    assert decisive / B >= DECISIVE_MIN_FRACTION, f"degenerate fixture: {decisive}/{B} decisive rows ({what})"


# ------------------------------------------------------------------------------------------------ (d) through the product
def _pages_and_maps():
    from manuscript_ocr_amd import synth
    H, W = 224, 320
    pages, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, H, W)
        pages.append(pg)
        maps.append(synth.synth_maps(rects, (H, W), (H // 4, W // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pages, mo


def _pipe(use_graphs=False):
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA
    rec = TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda", use_graphs=use_graphs)
    return Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(320, 224), device="cuda"), rec)


@pytest.fixture(scope="module")
def plain_pipe(cuda):
    return _pipe()


def _key(p):
    return [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words]


def _check_altwords(on, off, n, with_chars=False):
    from manuscript_ocr_amd.detectors._types import AltWord, Word
    n_words = n_alts = 0
    for p_on, p_off in zip(on, off):
        assert _key(p_on) == _key(p_off)
        assert p_on.model_dump() == p_off.model_dump()
        for w in p_on.blocks[0].words:
            if w.text is None:
                assert type(w) is Word  # too small to recognise: left as it was
                continue
            assert type(w) is AltWord and 1 <= len(w.alternatives) <= n
            assert w.alternatives[0].text == w.text and w.alternatives[0].confidence == w.recognition_confidence
            lps = [a.logp for a in w.alternatives]
            assert all(x >= y for x, y in zip(lps, lps[1:])) and all(lp <= 0 for lp in lps), lps
            assert len({a.text for a in w.alternatives}) == len(w.alternatives)
            assert ("".join(c.char for c in w.chars) == w.text) if with_chars else (w.chars == [])
            n_words += 1
            n_alts += len(w.alternatives)
    assert n_words == sum(w.text is not None for p in off for w in p.blocks[0].words) > 0
    assert n_alts > n_words, "no word has a second reading"
    return [[[(a.text, a.confidence, a.logp) for a in w.alternatives] for w in p.blocks[0].words if w.text is not None] for p in on]


def test_pipeline_n_best_and_predict(plain_pipe):
    from manuscript_ocr_amd.detectors._types import CharWord
    pipe = plain_pipe
    rec = pipe.recognizer
    pages, mo = _pages_and_maps()
    assert pipe.n_best == 0
    off = pipe.predict_batch(pages, _maps_override=mo)
    assert not any(isinstance(w, CharWord) for p in off for w in p.blocks[0].words)
    pipe.n_best = 3
    alts = None
    for device_order in (True, False):  # crops ordered and described on the device, and the host path
        pipe.device_order = device_order
        got = _check_altwords(pipe.predict_batch(pages, _maps_override=mo), off, 3)
        assert alts is None or got == alts
        alts = got
    pipe.device_order = True
    for switch in ("char_details", "group_lines", "rectify_crops"):
        setattr(pipe, switch, True)
        on = pipe.predict_batch(pages, _maps_override=mo)
        pipe.n_best = 0
        base = pipe.predict_batch(pages, _maps_override=mo)
        pipe.n_best = 3
        setattr(pipe, switch, False)
        if switch == "group_lines":  # one block per line: the words in page order are the same words
            flat = lambda ps: [[w for blk in p.blocks for w in blk.words] for p in ps]
            assert [[type(w).__name__ for w in p] for p in flat(on)] == [["AltWord" if w.text is not None else "Word" for w in p] for p in flat(base)]
            assert [[(w.polygon, w.text, w.recognition_confidence) for w in p] for p in flat(on)] == \
                   [[(w.polygon, w.text, w.recognition_confidence) for w in p] for p in flat(base)]
            assert [p.model_dump() for p in on] == [p.model_dump() for p in base]
        else:
            got = _check_altwords(on, base, 3, with_chars=switch == "char_details")
            assert switch == "rectify_crops" or got == alts  # rectified crops are other pixels
    # TRBA.predict on the words' host crops, page by page (a page is one call of the reference): the same readings
    for page, arr, want in zip(off, pages, alts):
        words = [w for w in page.blocks[0].words if w.text is not None]
        crops = [pipe._extract_word_image(arr, np.array(w.polygon, dtype=np.int32)) for w in words]
        res = rec.predict(crops, n_best=3)
        plain = rec.predict(crops)
        assert all(set(r) == {"text", "confidence", "alternatives"} for r in res) and all(set(r) == {"text", "confidence"} for r in plain)
        both = rec.predict(crops, return_chars=True, n_best=3)
        for w, r, p, bth, wa in zip(words, res, plain, both, want):
            assert (r["text"], r["confidence"]) == (p["text"], p["confidence"]) and r["text"] == w.text
            assert r["alternatives"][0]["text"] == r["text"] and r["alternatives"][0]["confidence"] == r["confidence"]
            assert bth["alternatives"] == r["alternatives"] and "".join(c["char"] for c in bth["chars"]) == r["text"]
            assert [a["text"] for a in r["alternatives"]] == [a[0] for a in wa]
            # the batch path's canvases come from the device crop kernel and another GEMM row count: test_gpu_pipeline.py holds the
            # two routes' confidences to 1e-6; a log-probability is a sum of up to `max_len` such terms
            np.testing.assert_allclose([a["confidence"] for a in r["alternatives"]], [a[1] for a in wa], atol=1e-6)
            np.testing.assert_allclose([a["logp"] for a in r["alternatives"]], [a[2] for a in wa], atol=25e-6)
    # the generic route with this package's recogniser asks predict for them
    pipe.native_fast_path = False
    page = pipe.predict(pages[0])
    pipe.native_fast_path = True
    named = [w for w in page.blocks[0].words if w.text is not None]
    assert named and all(type(w).__name__ == "AltWord" and w.alternatives[0].text == w.text for w in named)
    pipe.n_best = 9
    with pytest.raises(ValueError):
        pipe.predict_batch(pages, _maps_override=mo)
    pipe.n_best = 0
    again = pipe.predict_batch(pages, _maps_override=mo)
    assert [_key(p) for p in again] == [_key(p) for p in off]
    assert not any(isinstance(w, CharWord) for p in again for w in p.blocks[0].words)


def test_pipeline_n_best_on_a_replayed_graph(cuda, monkeypatch):
    """use_graphs=True: the second call of a bucket replays the captured graph, and the alternatives are read from the workspace that
    replay filled; with char_details also on the graph route declines and the eager path returns the same readings."""
    pipe = _pipe(use_graphs=True)
    grec = pipe.recognizer
    pipe.stream_sets = 1  # one set of launch streams: consecutive calls land in the same graph bucket
    pages, mo = _pages_and_maps()
    pages_dev = torch.from_numpy(np.stack(pages)).cuda()  # graphs are keyed by the page tensor
    seen, finish = [], grec.recognize_finish

    def spy(handle, *a, **kw):
        seen.append((handle.graph_inst is not None, kw.get("n_best", 0)))
        return finish(handle, *a, **kw)

    monkeypatch.setattr(grec, "recognize_finish", spy)
    off = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    pipe.n_best = 3
    replayed = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen == [(False, 0), (True, 3)], seen
    alts = _check_altwords(replayed, off, 3)
    pipe.char_details = True
    eager = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen[2] == (False, 3), seen
    assert _check_altwords(eager, off, 3, with_chars=True) == alts


# ------------------------------------------------------------------------------------------------ (e) envelope and arguments
def test_c_abi_and_predict_reject_what_is_outside_the_envelope(plain_pipe):
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops

    def rc(B, V, steps, K, n):
        """Device buffers sized for the (rejected) shape: a kernel launched by a broken check runs on valid memory."""
        ws = torch.zeros((nat.lib().msocr_attn_beam_workspace_bytes(B, steps, K, V),), dtype=torch.uint8, device="cuda")
        trun = torch.ones((B,), dtype=torch.int32, device="cuda")
        ids = torch.zeros((B, max(n, 1), steps), dtype=torch.int32, device="cuda")
        prob = torch.zeros((B, max(n, 1), steps), dtype=torch.float32, device="cuda")
        conf, logp = torch.zeros((B, max(n, 1)), device="cuda"), torch.zeros((B, max(n, 1)), device="cuda")
        r = nat.lib().msocr_attn_beam_nbest(ws.data_ptr(), B, V, steps, K, n, EOS, trun.data_ptr(), ids.data_ptr(), prob.data_ptr(),
                                            conf.data_ptr(), logp.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        return r

    assert rc(2, 194, 25, 8, 8) == 0 and rc(2, 512, 64, 16, 16) == 0
    assert rc(2, 194, 25, 8, 9) == E_ARG     # n_best > beam
    assert rc(2, 194, 25, 8, 0) == E_ARG
    assert rc(2, 194, 65, 8, 8) == E_ARG     # steps
    assert rc(2, 513, 25, 8, 8) == E_ARG     # V
    assert rc(2, 194, 25, 17, 8) == E_ARG    # beam
    rec = plain_pipe.recognizer
    crop = np.full((32, 100, 3), 255, dtype=np.uint8)
    for kw in (dict(mode="greedy", n_best=1), dict(n_best=-1), dict(n_best=9), dict(beam_size=4, n_best=5)):
        with pytest.raises(ValueError):
            rec.predict([crop], **kw)
    assert len(rec.predict([crop], beam_size=4, n_best=4)[0]["alternatives"]) >= 1
