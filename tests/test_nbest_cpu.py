"""Host side of the n-best readings (no GPU): the host twin msocr_attn_beam_nbest_host against a numpy walk of hand-made beam
workspaces evaluated in float64, TRBA.alternatives, the Alternative / AltWord result objects, the switches' signatures and the C
ABI's declarations."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAD, SOS, EOS = 0, 1, 2
E_ARG = -1
RTOL = 1e-6  # the twin's f32 results against float64
NEW_SYMBOLS = {"msocr_attn_beam_nbest", "msocr_attn_beam_nbest_host"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from manuscript_ocr_amd import _native
    return _native.lib()


# ------------------------------------------------------------------------------------------------ hand-made workspaces
def _workspace(B, V, steps, K, seed):
    """A beam workspace with random contents in the layout logits [B][steps][K][V] f32 | back [B][steps][K] i32 | tokv [B][steps][K]
    i32 | best_at [B][steps] i32 (+ the 256 spare bytes of msocr_attn_beam_workspace_bytes).  Not the trace of a search: tokens may
    follow an EOS, which is what shows where the log-probability sum stops."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, steps, K, V)) * 2.0).astype(np.float32)
    back = rng.integers(0, K, (B, steps, K), dtype=np.int32)
    tokv = rng.integers(0, V, (B, steps, K), dtype=np.int32)
    best_at = rng.integers(0, K, (B, steps), dtype=np.int32)
    return logits, back, tokv, best_at


def _pack(logits, back, tokv, best_at):
    return np.concatenate([a.reshape(-1).view(np.uint8) for a in (logits, back, tokv, best_at)] + [np.zeros(256, np.uint8)])


def _twin(lib, ws, B, V, steps, K, n, trun):
    buf = _pack(*ws)
    assert lib.msocr_attn_beam_workspace_bytes(B, steps, K, V) == buf.nbytes
    trun = np.ascontiguousarray(trun, dtype=np.int32)
    ids = np.full((B, n, steps), -7, dtype=np.int32)
    prob = np.full((B, n, steps), np.nan, dtype=np.float32)
    conf = np.full((B, n), np.nan, dtype=np.float32)
    logp = np.full((B, n), np.nan, dtype=np.float32)
    rc = lib.msocr_attn_beam_nbest_host(buf.ctypes.data, B, V, steps, K, n, EOS, trun.ctypes.data, ids.ctypes.data, prob.ctypes.data,
                                        conf.ctypes.data, logp.ctypes.data)
    assert rc == 0, rc
    return ids, prob, conf, logp


def _reference(ws, n, trun, steps):
    """The same read-out by a plain walk, every number in float64."""
    logits, back, tokv, best_at = ws
    B, _, K, V = logits.shape
    ids = np.full((B, n, steps), -1, dtype=np.int64)
    prob = np.zeros((B, n, steps))
    conf, logp = np.zeros((B, n)), np.zeros((B, n))
    for b in range(B):
        tr = int(trun[b])
        best = int(best_at[b, tr - 1])
        slots = [best] + [k for k in range(K) if k != best]  # rank 0 = the best slot, then the others in slot order
        for r in range(n):
            cur, lps = slots[r], np.zeros(tr)
            for t in range(tr - 1, -1, -1):
                ids[b, r, t] = tokv[b, t, cur]
                row = int(back[b, t, cur])
                x = logits[b, t, row].astype(np.float64)
                lps[t] = x[ids[b, r, t]] - (np.log(np.exp(x - x.max()).sum()) + x.max())
                cur = row
            prob[b, r, :tr] = np.exp(lps)
            conf[b, r] = prob[b, r, :tr].sum() / tr
            eos = np.flatnonzero(ids[b, r, :tr] == EOS)
            logp[b, r] = lps[: eos[0] + 1].sum() if len(eos) else lps.sum()
    return ids, prob, conf, logp


def _check(got, ref, what):
    ids, prob, conf, logp = got
    rids, rprob, rconf, rlogp = ref
    assert np.array_equal(ids, rids), what
    worst = 0.0
    for name, a, r in (("prob", prob, rprob), ("conf", conf, rconf), ("logp", logp, rlogp)):
        assert np.isfinite(a).all(), (what, name)
        err = np.abs(a.astype(np.float64) - r)
        assert (err <= RTOL * np.abs(r)).all(), (what, name, float((err / np.maximum(np.abs(r), 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(np.abs(r), 1e-300)).max()))
    print(f"[nbest-cpu] {what}: largest relative distance from float64 {worst:.2e}")


CASES = [
    # (id, B, V, steps, K, n, t_run): None = random in [1, steps]
    ("n1", 3, 7, 5, 4, 1, None),
    ("n2", 3, 7, 5, 4, 2, None),
    ("n4", 3, 7, 5, 4, 4, None),
    ("K1", 3, 7, 5, 1, 1, None),
    ("trun1", 3, 7, 5, 4, 4, 1),
    ("steps64", 2, 7, 64, 4, 4, 64),
    ("steps64-trun-below", 2, 7, 64, 4, 3, 41),
    ("V512-K16", 2, 512, 6, 16, 16, None),
]


@pytest.mark.parametrize("what,B,V,steps,K,n,tr", CASES, ids=[c[0] for c in CASES])
def test_host_twin_against_numpy_walk(lib, what, B, V, steps, K, n, tr):
    ws = _workspace(B, V, steps, K, seed=1000 + len(what) + steps * K)
    trun = np.random.default_rng(7).integers(1, steps + 1, B) if tr is None else np.full(B, tr)
    got = _twin(lib, ws, B, V, steps, K, n, trun)
    _check(got, _reference(ws, n, trun, steps), what)
    beyond = np.arange(steps)[None, None, :] >= np.asarray(trun)[:, None, None]
    assert (got[0][np.broadcast_to(beyond, got[0].shape)] == -1).all() and (got[1][np.broadcast_to(beyond, got[1].shape)] == 0).all()


def _planted():
    """B 3, V 7, steps 5, K 4 with the cases the rules are about, all at t_run = 5:
    row 0: rank 0 ends in EOS at the last step and rank 1 in PAD, on the same parent: two ranks, one text;
    row 1: rank 0 emits EOS at step 1 and ordinary tokens after it: the log-probability sum stops at step 1, the confidence does not;
    row 2: no EOS anywhere: the sum runs over every step."""
    B, V, steps, K = 3, 7, 5, 4
    logits, back, tokv, best_at = _workspace(B, V, steps, K, seed=5)
    tokv[tokv == EOS] = 3
    tokv[tokv == PAD] = 4
    best_at[:, steps - 1] = (2, 0, 1)
    # row 0: the ranks are the slots 2, 0, 1, 3
    back[0, 4, 2] = back[0, 4, 0] = 1
    tokv[0, 4, 2], tokv[0, 4, 0] = EOS, PAD
    # row 1: rank 0 = slot 0; its path at step 1
    cur = 0
    for t in range(4, 1, -1):
        cur = back[1, t, cur]
    tokv[1, 1, cur] = EOS
    return (logits, back, tokv, best_at), (B, V, steps, K)


def test_logp_stops_at_the_first_eos_and_confidence_does_not(lib):
    ws, (B, V, steps, K) = _planted()
    trun = np.full(B, steps)
    got = _twin(lib, ws, B, V, steps, K, K, trun)
    ref = _reference(ws, K, trun, steps)
    _check(got, ref, "planted")
    ids, prob, conf, logp = got
    assert ids[1, 0, 1] == EOS and (ids[1, 0, 2:] != EOS).all()
    lp = np.log(ref[1][1, 0])
    assert logp[1, 0] == pytest.approx(lp[:2].sum(), rel=RTOL) and abs(lp[2:].sum()) > 0.1  # the later steps would have shown
    assert conf[1, 0] == pytest.approx(ref[1][1, 0].mean(), rel=RTOL)
    assert not (ids[2] == EOS).any()
    assert np.allclose(logp[2], np.log(ref[1][2]).sum(axis=1), rtol=RTOL, atol=0)
    assert ids[0, 0, 4] == EOS and ids[0, 1, 4] == PAD and np.array_equal(ids[0, 0, :4], ids[0, 1, :4])


def test_trun_outside_the_steps_is_clamped(lib):
    """t_run 0 and below read as 1, above `steps` as `steps`: nothing outside the workspace is touched."""
    B, V, steps, K = 3, 7, 5, 4
    ws = _workspace(B, V, steps, K, seed=11)
    got = _twin(lib, ws, B, V, steps, K, K, [0, -5, 99])
    ref = _twin(lib, ws, B, V, steps, K, K, [1, 1, steps])
    for a, r in zip(got, ref):
        assert np.array_equal(a, r)


def test_host_twin_argument_errors(lib):
    B, V, steps, K, n = 2, 7, 5, 4, 2
    buf = _pack(*_workspace(B, 513, 65, 16, seed=3))  # large enough for every rejected shape below
    trun = np.ones(B, dtype=np.int32)
    ids = np.zeros((B, 16, 65), dtype=np.int32)
    prob = np.zeros((B, 16, 65), dtype=np.float32)
    conf, logp = np.zeros((B, 16), dtype=np.float32), np.zeros((B, 16), dtype=np.float32)
    ptrs = [buf.ctypes.data, trun.ctypes.data, ids.ctypes.data, prob.ctypes.data, conf.ctypes.data, logp.ctypes.data]

    def call(B=B, V=V, steps=steps, K=K, n=n, null=None):
        p = [None if i == null else v for i, v in enumerate(ptrs)]
        return lib.msocr_attn_beam_nbest_host(p[0], B, V, steps, K, n, EOS, p[1], p[2], p[3], p[4], p[5])

    assert call() == 0
    for i in range(len(ptrs)):
        assert call(null=i) == E_ARG, i
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(V=513), dict(steps=0), dict(steps=65), dict(K=0, n=1), dict(K=17, n=1), dict(n=0),
               dict(n=-1), dict(n=K + 1)):
        assert call(**kw) == E_ARG, kw
    assert call(V=512) == 0 and call(steps=64) == 0 and call(K=16, n=16) == 0 and call(n=K) == 0


# ------------------------------------------------------------------------------------------------ TRBA's host half
def _stub_trba():
    from manuscript_ocr_amd.recognizers import TRBA
    rec = TRBA.__new__(TRBA)  # no device: only the attributes `texts` reads
    rec.itos = ["<PAD>", "<SOS>", "<EOS>", "a", "b", "c", "d"]
    rec.pad_id, rec.sos_id, rec.eos_id, rec.blank_id = PAD, SOS, EOS, None
    return rec


def test_alternatives_drop_duplicates_and_keep_entry_zero(lib):
    rec = _stub_trba()
    ws, (B, V, steps, K) = _planted()
    trun = np.full(B, steps, dtype=np.int32)
    ids, _prob, conf, logp = _twin(lib, ws, B, V, steps, K, K, trun)
    alts = rec.alternatives(ids, trun, conf, logp)
    assert len(alts) == B
    best_texts = rec.texts(ids[:, 0], trun)
    for b in range(B):
        texts = rec.texts(ids[b], np.full(K, steps))
        assert alts[b][0] == {"text": best_texts[b], "confidence": float(conf[b, 0]), "logp": float(logp[b, 0])}
        assert [a["text"] for a in alts[b]] == list(dict.fromkeys(texts))  # first occurrences, in rank order
        kept = [texts.index(a["text"]) for a in alts[b]]
        assert [a["logp"] for a in alts[b]] == [float(logp[b, r]) for r in kept]
        assert [a["confidence"] for a in alts[b]] == [float(conf[b, r]) for r in kept]
    assert rec.texts(ids[0, :2], trun[:2])[0] == rec.texts(ids[0, :2], trun[:2])[1] and len(alts[0]) < K  # the EOS / PAD pair of row 0
    # t_run cuts the text as it cuts the word's own
    short = rec.alternatives(ids, np.full(B, 2), conf, logp)
    assert all(len(a["text"]) <= 2 for row in short for a in row)
    # entry 0 survives even when it is empty; confidences a rounding above 1 are clamped for the result objects
    one = rec.alternatives(np.array([[[EOS, 3], [EOS, 4], [3, EOS]]]), [2], np.array([[1.0000001, 0.5, 0.25]]), np.array([[-0.1, -0.2, -0.3]]))
    assert one == [[{"text": "", "confidence": 1.0, "logp": pytest.approx(-0.1)}, {"text": "a", "confidence": 0.25, "logp": pytest.approx(-0.3)}]]
    assert rec.alternatives(np.zeros((0, 3, 5), dtype=np.int32), [], np.zeros((0, 3)), np.zeros((0, 3))) == []


def test_n_best_argument_rules():
    from manuscript_ocr_amd.recognizers import TRBA
    TRBA._check_n_best(0, "greedy", 8)
    TRBA._check_n_best(8, "beam", 8)
    for bad in ((-1, "beam", 8), (1, "greedy", 8), (9, "beam", 8), (2, "beam", 1)):
        with pytest.raises(ValueError):
            TRBA._check_n_best(*bad)
    sig = inspect.signature(TRBA.predict)
    assert sig.parameters["n_best"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["n_best"].default == 0
    assert sig.parameters["return_chars"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(TRBA.recognize_finish).parameters["n_best"].default == 0
    assert inspect.signature(TRBA.recognize_canvases).parameters["n_best"].default == 0
    assert list(inspect.signature(TRBA.alternatives).parameters) == ["self", "alt_ids", "trun", "alt_conf", "alt_logp"]


def test_pipeline_switch_and_attach():
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors._types import AltWord, Block, CharWord, Page, Word
    pipe = Pipeline(detector=object(), recognizer=object())
    assert pipe.n_best == 0 and pipe._n_best() == 0
    pipe.n_best = 8
    assert pipe._n_best() == 8
    for bad in (9, -1):
        pipe.n_best = bad
        with pytest.raises(ValueError):
            pipe._n_best()
    poly = [(0.0, 0.0), (10.0, 0.0), (10.0, 5.0), (0.0, 5.0)]
    words = [Word(polygon=poly, detection_confidence=0.9, text=t, recognition_confidence=0.5) for t in ("ab", "c")]
    skipped = Word(polygon=poly, detection_confidence=0.8)  # too small for a crop: stays a plain Word
    alts = [[{"text": "ab", "confidence": 0.5, "logp": -1.0}, {"text": "ad", "confidence": 0.25, "logp": -2.5}],
            [{"text": "c", "confidence": 0.5, "logp": -0.5}]]
    chars = [[{"char": "a", "confidence": 0.5, "x": 1.0}, {"char": "b", "confidence": 0.5, "x": 6.0}], [{"char": "c", "confidence": 0.5, "x": 4.0}]]
    for with_chars in (False, True):
        page = Page(blocks=[Block(words=[words[0], skipped, words[1]])])
        before = page.model_dump()
        Pipeline._attach_details(words, [page], chars if with_chars else None, alts)
        got = page.blocks[0].words
        assert isinstance(got[0], AltWord) and isinstance(got[2], AltWord) and got[1] is skipped
        assert [a.text for a in got[0].alternatives] == ["ab", "ad"] and got[0].alternatives[1].logp == -2.5
        assert ["".join(c.char for c in w.chars) for w in (got[0], got[2])] == (["ab", "c"] if with_chars else ["", ""])
        assert page.model_dump() == before
    page = Page(blocks=[Block(words=list(words))])
    Pipeline._attach_details(words, [page], chars)  # char_details alone: CharWords, as before
    assert all(type(w) is CharWord for w in page.blocks[0].words)


def test_alternative_and_altword_validate():
    from pydantic import ValidationError

    from manuscript_ocr_amd.detectors._types import Alternative, AltWord, Block, CharWord, Page, Word
    a = Alternative(text="ab", confidence=0.25, logp=-3.5)
    assert (a.text, a.confidence, a.logp) == ("ab", 0.25, -3.5)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValidationError):
            Alternative(text="ab", confidence=bad, logp=0.0)
    with pytest.raises(ValidationError):
        Alternative(text="ab", confidence=0.5)  # logp is required
    poly = [(0.0, 0.0), (10.0, 0.0), (10.0, 5.0), (0.0, 5.0)]
    w = AltWord(polygon=poly, detection_confidence=0.9, text="ab", recognition_confidence=0.5,
                alternatives=[a, {"text": "ad", "confidence": 0.125, "logp": -4.0}])
    assert isinstance(w, CharWord) and isinstance(w, Word) and w.chars == [] and isinstance(w.alternatives[1], Alternative)
    assert AltWord(polygon=poly, detection_confidence=0.9).alternatives == []
    with pytest.raises(ValidationError):
        AltWord(polygon=poly, detection_confidence=0.9, alternatives=[{"text": "a", "confidence": 2.0, "logp": 0.0}])
    plain = Word(polygon=poly, detection_confidence=0.9, text="ab", recognition_confidence=0.5)
    assert set(Word.model_fields) == {"polygon", "detection_confidence", "text", "recognition_confidence"}
    assert Page(blocks=[Block(words=[w])]).model_dump() == Page(blocks=[Block(words=[plain])]).model_dump()
    assert "alternatives" in w.model_dump()


def test_header_exports_and_native_list_the_new_symbols(lib):
    from manuscript_ocr_amd import _native
    header = open(os.path.join(ROOT, "include", "msocr.h")).read()
    declared = set(re.findall(r"\b(msocr_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared, NEW_SYMBOLS - declared
    assert NEW_SYMBOLS <= set(_native.exported_symbols()), NEW_SYMBOLS - set(_native.exported_symbols())
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
