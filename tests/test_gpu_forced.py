"""Forced (teacher-forced) decode on the device: msocr_attn_decode in forced mode and msocr_seq_logp behind
AttnDecoder.forced / seq_logp, TRBA.score and Pipeline.score_page.  Fixtures, replays and bounds are those of test_gpu_seq_f64.py
(decoder of synth.trba_state_dict at rnn_scale 4, batch_H ~ N(0, 1.4^2)); nothing here depends on a discrete decision of the code
under test: the decoder is told which tokens to follow.

1. fed greedy's own ids, the forced decode IS the greedy decode: logits and attention weights bit for bit, on both kernels;
2. fed a beam search's finalized ids, it gives the logits the search read them from (general kernel, temperature 1), bit for bit;
3. along arbitrary token strings it meets the f64 replay as the greedy decode does (E_F32_FACTOR, E_REL_MAX);
4. a row does not depend on which rows share its launch;
5. msocr_seq_logp equals its host twin and f64 within the host test's bound;
6. TRBA.score and 7. Pipeline.score_page: the public calls, consistent with predict and with each other."""
import copy

import numpy as np
import pytest
import torch

from test_forced_cpu import STEP_ATOL, _logp_host, _logp_problem
from test_gpu_seq_f64 import (ALPHA, B_DEF, EOS, PAD, SOS, STEPS_B, STEPS_G, T_DEF, _check_arith, _errors, _inputs, _kernel, _oracle, _replay,
                              _replay_f32, cuda)  # noqa: F401  (cuda: the module's GPU fixture)

pytestmark = pytest.mark.gpu


def _strings(B, steps, V, seed, blank=None):
    """Seeded random token strings of lengths 0 .. steps - 1 (row 0 empty, row 1 full) over the ordinary tokens, packed as
    transforms.pack_targets packs: tok_in = SOS, ids, PAD...; target = ids, EOS, PAD...; trun = length + 1."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, steps, B)
    L[0] = 0
    if B > 1:
        L[1] = steps - 1
    pool = np.array([v for v in range(3, V) if v != blank])
    tok_in, target = np.full((B, steps), PAD, dtype=np.int32), np.full((B, steps), PAD, dtype=np.int32)
    tok_in[:, 0] = SOS
    for b in range(B):
        ids = rng.choice(pool, L[b])
        tok_in[b, 1:1 + L[b]] = ids
        target[b, :L[b]] = ids
        target[b, L[b]] = EOS
    return tok_in, target, (L + 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. identity with greedy
GREEDY_IDENTITY = [
    # (id, H, V, B, T, steps, kernel)
    ("mfma-B37", 256, 194, B_DEF, T_DEF, STEPS_G, "auto"),  # two workgroups, the second partial
    ("mfma-V256-T48-B1", 256, 256, 1, 48, STEPS_G, "auto"),
    ("general-H128-B5", 128, 194, 5, T_DEF, STEPS_G, "auto"),
    ("general-H256", 256, 194, 5, T_DEF, STEPS_G, "valu"),
]


@pytest.mark.parametrize("what,H,V,B,T,steps,kernel", GREEDY_IDENTITY, ids=[c[0] for c in GREEDY_IDENTITY])
def test_forced_along_greedy_ids_is_the_greedy_decode(cuda, monkeypatch, what, H, V, B, T, steps, kernel):
    dec = _kernel(monkeypatch, V, H, kernel)
    assert dec._matrix_core(T) == what.startswith("mfma")
    bH, pH = _inputs(B, T, H, V)
    lg, ids, al = dec.greedy(bH, pH, steps - 1, SOS, EOS, None, want_alpha=True)
    tok_in = torch.cat([torch.full((B, 1), SOS, dtype=torch.int32, device=ids.device), ids[:, :-1]], 1).contiguous()
    flg, fal = dec.forced(bH, pH, tok_in, SOS, None)
    torch.cuda.synchronize()
    assert flg.shape == (B, steps, V) and fal.shape == (B, steps, T)
    assert torch.equal(flg, lg), (what, float((flg - lg).abs().max()))
    assert torch.equal(fal, al), (what, float((fal - al).abs().max()))


# ------------------------------------------------------------------------------------------------ 2. identity with beam
def test_forced_along_beam_ids_gives_the_finalized_logits(cuda, monkeypatch):
    H, V, K, B, T, steps = 256, 194, 8, 9, T_DEF, STEPS_B
    dec = _kernel(monkeypatch, V, H, "valu")
    bH, pH = _inputs(B, T, H, V)
    ws, fin, _ = dec.beam(bH, pH, steps, K, ALPHA, 1.0, SOS, EOS, None)
    lg, ids = dec.beam_finalize(ws, B, steps, K, fin)
    torch.cuda.synchronize()
    trun, ids_h = fin.cpu().numpy(), ids.cpu().numpy()
    tok_in = np.concatenate([np.full((B, 1), SOS), np.where(ids_h[:, :-1] >= 0, ids_h[:, :-1], PAD)], 1).astype(np.int32)
    flg, _ = dec.forced(bH, pH, torch.from_numpy(tok_in).cuda(), SOS, None)
    valid = np.arange(steps)[None, :] < trun[:, None]
    assert valid.sum() > B  # paths of more than one step
    assert np.array_equal(flg.cpu().numpy()[valid], lg.cpu().numpy()[valid])


# ------------------------------------------------------------------------------------------------ 3. arbitrary tokens against f64
F64_CASES = [
    # (id, H, V, B, T, steps, kernel)
    ("mfma-H256-V194", 256, 194, B_DEF, T_DEF, STEPS_G, "auto"),
    ("general-H64", 64, 194, B_DEF, T_DEF, STEPS_G, "auto"),
    ("general-H512-V512-T64-S64-B3", 512, 512, 3, 64, 64, "auto"),
    ("general-V257", 256, 257, B_DEF, T_DEF, STEPS_G, "auto"),
    ("general-T49", 256, 194, B_DEF, 49, STEPS_G, "auto"),
]


@pytest.mark.parametrize("what,H,V,B,T,steps,kernel", F64_CASES, ids=[c[0] for c in F64_CASES])
def test_forced_along_arbitrary_tokens_against_f64_replay(cuda, monkeypatch, what, H, V, B, T, steps, kernel):
    blank = 3
    dec = _kernel(monkeypatch, V, H, kernel)
    assert dec._matrix_core(T) == what.startswith("mfma")
    bH, pH = _inputs(B, T, H, V)
    tok_in, _target, trun = _strings(B, steps, V, seed=H + V + T, blank=blank)
    lg, al = dec.forced(bH, pH, torch.from_numpy(tok_in).cuda(), SOS, blank)
    torch.cuda.synchronize()
    lg, al = lg.cpu().numpy(), al.cpu().numpy()
    tok = torch.from_numpy(tok_in.astype(np.int64))
    r64 = _replay(_oracle(V, H, blank, "f64"), bH.double(), tok).cpu().numpy()
    r32 = [r.numpy() for r in _replay_f32(_oracle(V, H, blank, "f32"), bH, tok)]
    valid = np.arange(steps)[None, :] < trun[:, None]
    e_dev, e_f32, scale = _errors(lg, r64, r32, valid, blank)
    _check_arith(f"forced {what}", e_dev, e_f32, scale)
    assert (lg[..., blank] == np.float32(-1e4)).all()
    s = al.astype(np.float64).sum(-1)
    print(f"[forced] {what}: alpha row sums within {np.abs(s - 1).max():.2e} of 1")
    assert (al >= 0).all() and np.abs(s - 1).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ 4. batch composition
@pytest.mark.parametrize("what,H,kernel", [("mfma", 256, "auto"), ("general", 128, "auto")])
def test_forced_row_does_not_depend_on_batch_composition(cuda, monkeypatch, what, H, kernel):
    """Rows 5 and 35 of 37 (the first matrix-core workgroup's full block of 32 and the second's partial one), each alone and among
    the 36 others: logits, weights and log-probabilities bit-equal.  The context gates are computed once for the 37 rows (the GEMM
    may pick another kernel for another row count; the decode kernel is what is held to this)."""
    V, B, T, steps = 194, B_DEF, T_DEF, STEPS_G
    dec = _kernel(monkeypatch, V, H, kernel)
    assert dec._matrix_core(T) == (what == "mfma")
    bH, pH = _inputs(B, T, H, V)
    tok_in, target, trun = _strings(B, steps, V, seed=77)
    tok_d, tgt_d, trun_d = (torch.from_numpy(a).cuda() for a in (tok_in, target, trun))
    cg = dec.ctx_gates(bH).view(B, -1) if what == "mfma" else None

    def run(rows):
        idx = torch.as_tensor(rows, device=bH.device)
        c = cg[idx].contiguous().view(len(rows) * T, -1) if cg is not None else None
        lg, al = dec.forced(bH[idx].contiguous(), pH[idx].contiguous(), tok_d[idx].contiguous(), SOS, None, ctx_gates=c)
        lps, lp = dec.seq_logp(lg, tgt_d[idx].contiguous(), trun_d[idx].contiguous())
        return [x.cpu() for x in (lg, al, lps, lp)]

    full = run(list(range(B)))
    for b in (5, 35):
        for x, y in zip(full, run([b])):
            assert torch.equal(x[b], y[0]), (what, b)
    assert torch.isfinite(full[3]).all() and (full[3] < 0).all()


# ------------------------------------------------------------------------------------------------ 5. msocr_seq_logp
@pytest.mark.parametrize("temperature", [1.0, 1.7])
@pytest.mark.parametrize("V", [40, 194, 512])
def test_seq_logp_device_against_host_twin_and_f64(cuda, V, temperature):
    from manuscript_ocr_amd import _native as nat, ops
    logits, ids, trun, ref = _logp_problem(V, temperature=temperature)
    B, steps = logits.shape[:2]
    h_lps, h_lp = _logp_host(logits, ids, trun, temperature)
    lg_d, ids_d, trun_d = (torch.from_numpy(a).cuda() for a in (logits, ids, trun))
    d_lps, d_lp = torch.full((B, steps), 7.0, device=cuda), torch.full((B,), 7.0, device=cuda)
    nat.check(nat.lib().msocr_seq_logp(lg_d.data_ptr(), ids_d.data_ptr(), trun_d.data_ptr(), B, V, steps, temperature, d_lps.data_ptr(),
                                       d_lp.data_ptr(), ops._stream()), "seq_logp")
    torch.cuda.synchronize()
    d_lps, d_lp = d_lps.cpu().numpy(), d_lp.cpu().numpy()
    e_host, e_f64 = np.abs(d_lps - h_lps).max(), np.abs(d_lps.astype(np.float64) - ref).max()
    print(f"[forced] seq_logp V {V} tau {temperature}: device - host {e_host:.2e}, device - f64 {e_f64:.2e}")
    assert e_host <= STEP_ATOL and e_f64 <= STEP_ATOL
    assert np.abs(d_lp.astype(np.float64) - ref.sum(1)).max() <= steps * STEP_ATOL
    assert (d_lps[np.arange(steps)[None, :] >= trun[:, None]] == 0).all() and d_lp[trun == 0] == 0
    for b in range(len(trun)):  # the f64 sum in step order of the f32 step values, rounded once
        s = 0.0
        for t in range(trun[b]):
            s += float(d_lps[b, t])
        assert d_lp[b] == np.float32(s)


# ------------------------------------------------------------------------------------------------ 6. TRBA.score
CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def rec(cuda):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


@pytest.fixture(scope="module")
def crops():
    """6 crops of 32 x 100, one cut to 32 x 60 (padding on the canvas) and one to 20 x 100."""
    from manuscript_ocr_amd import synth
    c = [np.ascontiguousarray(x) for x in synth.synth_crops(1, 6, 32, 100)]
    c[1], c[2] = np.ascontiguousarray(c[1][:, :60]), np.ascontiguousarray(c[2][:20])
    return c


def test_score_of_the_greedy_reading_is_predicts_own(rec, crops):
    """batch_size = 1: every row is its own reference chunk, so predict's run length is the row's own length + 1, the forced row's."""
    own = rec.predict(crops, batch_size=1, mode="greedy", return_chars=True)
    texts = [r["text"] for r in own]
    assert all(1 <= len(t) <= rec.max_length for t in texts), texts  # the planted decoder writes words and ends them
    got = rec.score(crops, texts)
    assert len(got) == 6
    for r, g in zip(own, got):
        assert set(g) == {"text", "logp", "confidence", "chars"}
        assert g["text"] == r["text"] and g["confidence"] == r["confidence"]
        assert g["chars"] == r["chars"]
        assert "".join(c["char"] for c in g["chars"]) == g["text"]
        assert np.isfinite(g["logp"]) and g["logp"] < 0
        # logp sums the log of what confidence averages, the same per-token probabilities: geometric <= arithmetic mean
        assert np.exp(g["logp"] / (len(g["text"]) + 1)) <= g["confidence"] + 1e-6


def test_score_candidates(rec, crops):
    own = [r["text"] for r in rec.predict(crops, batch_size=1, mode="greedy")]
    single = rec.score(crops, own)
    alt = lambda t: ("b" if t[:1] != "b" else "c") + t[1:]  # another first letter
    lists = [[alt(t), t, t[:-1]] for t in own]
    multi = rec.score(crops, lists)
    assert [type(m) for m in multi] == [list] * 6 and type(single[0]) is dict
    for s, m, cand in zip(single, multi, lists):
        assert [e["text"] for e in m] == cand  # the given order
        assert m[1] == s  # the shared candidate: the same numbers, whatever rows surround it
        assert m[0]["logp"] < m[1]["logp"] and all("".join(c["char"] for c in e["chars"]) == e["text"] for e in m)
    # one image, a list of candidates; and mixed entries
    one = rec.score(crops[0], lists[0])
    assert [e["text"] for e in one[0]] == lists[0]
    mixed = rec.score(crops[:2], [own[0], lists[1]])
    assert type(mixed[0]) is dict and type(mixed[1]) is list and mixed[0]["text"] == own[0]
    # temperature enters logp only
    hot = rec.score(crops, own, temperature=1.7)
    assert all(h["confidence"] == s["confidence"] and h["logp"] != s["logp"] for h, s in zip(hot, single))
    # strict: nothing is silently narrowed
    with pytest.raises(ValueError, match="image 1"):
        rec.score(crops[:2], ["ab", "a一"])
    with pytest.raises(ValueError, match="max_len"):
        rec.score(crops[:1], ["a" * 26])
    lenient = rec.score(crops[:1], ["a一" + "b" * 30], strict=False)
    assert lenient[0]["text"] == "a" + "b" * 24
    with pytest.raises(ValueError):
        rec.score(crops[:2], ["ab"])


# ------------------------------------------------------------------------------------------------ 7. Pipeline.score_page
@pytest.mark.parametrize("rectify", [False, True])
def test_score_page(cuda, rec, rectify):
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import CharWord, Word
    H, W = 224, 320
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda"), rec)
    pipe.rectify_crops = rectify
    img, rects = synth.synth_page(41, H, W)
    score, geo = synth.synth_maps(rects, (H, W), (H // 4, W // 4), 41)
    page = pipe.predict_batch([img], _maps_override=(torch.from_numpy(score)[None].cuda(), torch.from_numpy(geo)[None].cuda()))[0]
    words = page.blocks[0].words
    before = page.model_dump()
    scored, logps = pipe.score_page(img, page)
    assert page.model_dump() == before, "the caller's page is not touched"
    out = scored.blocks[0].words
    assert len(out) == len(words) == len(logps)
    assert [(w.polygon, w.text) for w in out] == [(w.polygon, w.text) for w in words], "word order and texts are the caller's"
    rows = [k for k, w in enumerate(words) if w.text is not None]
    assert len(rows) >= 3
    for k, (w, o) in enumerate(zip(words, out)):
        if w.text is None:
            assert type(o) is Word and logps[k] is None and o == w
            continue
        assert isinstance(o, CharWord) and "".join(c.char for c in o.chars) == o.text
        assert logps[k] is not None and logps[k] < 0
        xs = [pt[0] for pt in np.array(w.polygon, dtype=np.int32).tolist()]
        assert all(max(0, min(xs)) - 1 <= c.x <= min(W, max(xs)) + 1 for c in o.chars)
    if not rectify:  # a direct TRBA.score of the same windows (the host's ResizeAndPadA is the device crop's, byte for byte)
        wins = []
        for k in rows:
            p = np.array(words[k].polygon, dtype=np.int32)
            (x0, y0), (x1, y1) = p.min(0), p.max(0)
            wins.append(np.ascontiguousarray(img[max(0, y0):min(H, y1), max(0, x0):min(W, x1)]))
        direct = rec.score(wins, [words[k].text for k in rows])
        for k, d in zip(rows, direct):
            assert out[k].recognition_confidence == min(max(d["confidence"], 0.0), 1.0) and logps[k] == d["logp"]
            assert [c.confidence for c in out[k].chars] == [c["confidence"] for c in d["chars"]]
    # one word's text changed: that word fits worse, the others do not move
    k = next(k for k in rows if len(words[k].text) >= 2)
    other = copy.deepcopy(page)
    t = other.blocks[0].words[k].text
    other.blocks[0].words[k].text = ("b" if t[0] != "b" else "c") + t[1:]
    scored2, logps2 = pipe.score_page(img, other)
    assert logps2[k] < logps[k]
    assert [l for j, l in enumerate(logps2) if j != k] == [l for j, l in enumerate(logps) if j != k]
    assert [w for j, w in enumerate(scored2.blocks[0].words) if j != k] == [w for j, w in enumerate(out) if j != k]
