"""Nearest lexicon words by edit distance, on the device: msocr_edit_distance_pairs and msocr_lexicon_nearest
(csrc/lexicon_nearest.hip) against their host twins — which tests/test_lexicon_nearest_cpu.py holds to the textbook dynamic programme —
then the switch through TRBA.predict, Pipeline and TRBA.evaluate on test_gpu_nbest.py's pipeline fixture.  Integers, compared exactly.

(1) pairs on the length grid: device == host twin == DP.
(2) nearest: index and distance of every row and rank equal the host twin's, over B 1 / 37 / 300, lexicons of 1, 5, 1 000 and 20 011
    words (the last cut over several workgroups per row, asserted from the workspace size), V 194 and 512, k 1 / 3 / 8 / 16, bounds
    -1 / 0 / 2; rows of 62, 63 and 64 symbols against words of up to 63; the tie lexicon.
(3) A row's result does not depend on the other rows of its launch.  (4) A captured and replayed launch equals the eager one.
(5) TRBA.predict(suggest=...) with greedy, beam, lm, n_best and return_chars; (6) Pipeline.suggest; (7) TRBA.evaluate."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_charlm import _product_lm
from test_gpu_nbest import _pages_and_maps, _pipe
from test_lexicon_nearest_cpu import (csr, dp_pair, nearest_host, pair_grid, pairs_host, random_lexicon, rows_near, sorted_list,
                                      tie_lexicon)

pytestmark = pytest.mark.gpu

EOS, PAD = 2, 0
CONTENT = list(range(3, 60))


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _DevList:
    """A word list on the device, with its struct."""

    def __init__(self, begin, tok, by_length=False):
        from manuscript_ocr_amd import _native as nat
        self.begin, self.tok = _dev(begin), _dev(tok)
        self.wl = nat.WordList()
        if by_length:  # the kernel-friendly copy: stored in ascending (length, index) order, position p holds word order[p]
            begin, tok, order = sorted_list(begin, tok)
            self.begin, self.tok, self.order = _dev(begin), _dev(tok), _dev(order)
            self.wl.by_length = self.order.data_ptr()
        self.wl.word_begin, self.wl.word_tok, self.wl.n_words, self.wl.n_tok = self.begin.data_ptr(), self.tok.data_ptr(), len(begin) - 1, len(tok)


def _ws_bytes(B, n_words, k):
    from manuscript_ocr_amd import _native as nat
    return int(nat.lib().msocr_lexicon_nearest_ws_bytes(B, n_words, k))


def nearest_dev(ids_dev, trun_dev, V, blank, dl, k, bound, eos=EOS, pad=PAD):
    from manuscript_ocr_amd import _native as nat
    B, steps = ids_dev.shape
    idx = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    d = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty((max(_ws_bytes(B, dl.wl.n_words, k), 8),), dtype=torch.uint8, device="cuda")
    rc = nat.lib().msocr_lexicon_nearest(ids_dev.data_ptr(), trun_dev.data_ptr(), B, steps, V, eos, pad, blank, ctypes.byref(dl.wl), k, bound,
                                         idx.data_ptr(), d.data_ptr(), ws.data_ptr(), _stream())
    assert rc == 0, rc
    return idx, d


# ------------------------------------------------------------------------------------------------ (1) pairs
def test_pairs_equal_the_host_twin_and_the_dp(cuda):
    from manuscript_ocr_amd import _native as nat
    for V, eos, pad, a, ta, b, tb in pair_grid():
        B = len(a)
        out = [torch.full((B,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
        ad, bd, tad, tbd = _dev(a), _dev(b), _dev(ta), _dev(tb)
        rc = nat.lib().msocr_edit_distance_pairs(ad.data_ptr(), tad.data_ptr(), 64, bd.data_ptr(), tbd.data_ptr(), 64, B, V, eos, pad, -1,
                                                 *(o.data_ptr() for o in out), _stream())
        assert rc == 0
        d, la, lb = (o.cpu().numpy() for o in out)
        hd, hla, hlb = pairs_host(a, ta, b, tb, V, eos, pad, -1)
        assert (d == hd).all() and (la == hla).all() and (lb == hlb).all(), V
        assert d.tolist() == [dp_pair(x[:m], y[:n], V) for x, m, y, n in zip(a, ta, b, tb)], V
    # the text rule on the device: PAD and BLANK in the middle, EOS inside and outside t_run, ids outside [0, V)
    V, blank = 10, 9
    rows = np.array([[3, 0, 4, 9, 5, 6, 2, 7], [3, 4, 5, 6, 7, 7, 2, 7], [2] * 8, [3, -1, V, 2**31 - 1, 2, 2, 2, 2]], dtype=np.int64).astype(np.int32)
    trun = np.array([8, 4, 8, 8], dtype=np.int32)
    other = np.tile(np.array([3, 4, 5, 6, 2, 2, 2, 2], dtype=np.int32), (4, 1))
    out = [torch.full((4,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    rd, td, od, otd = _dev(rows), _dev(trun), _dev(other), _dev(np.full(4, 8))
    assert nat.lib().msocr_edit_distance_pairs(rd.data_ptr(), td.data_ptr(), 8, od.data_ptr(), otd.data_ptr(), 8, 4, V, EOS, PAD, blank,
                                               *(o.data_ptr() for o in out), _stream()) == 0
    got = [o.cpu().numpy().tolist() for o in out]
    assert got == [h.tolist() for h in pairs_host(rows, trun, other, np.full(4, 8), V, EOS, PAD, blank)]
    assert got == [[0, 0, 4, 3], [4, 4, 0, 4], [4, 4, 4, 4]]


# ------------------------------------------------------------------------------------------------ (2) nearest
_LEX = {}


def _lexicon(L, V):
    """(toks, lens, begin, tok, device list) of a seeded random lexicon of L words, lengths 1..16; with V = 512 a tenth of the tokens
    come from the top of the alphabet, V - 1 included."""
    if (L, V) not in _LEX:
        rng = np.random.default_rng(7 * L + V)
        content = CONTENT if V == 194 else CONTENT + list(range(506, 512))
        toks, lens = random_lexicon(rng, L, content)
        begin, tok = csr(toks, lens)
        _LEX[(L, V)] = (toks, lens, begin, tok, (_DevList(begin, tok), _DevList(begin, tok, by_length=True)), content)
    return _LEX[(L, V)]


def _from_k16(h16, k, bound):
    """The host twin's answer for (k, bound) from its answer for (16, no bound): the list is sorted by distance first, so the bound
    keeps a prefix of it and k another (tests/test_lexicon_nearest_cpu.py holds the twin itself to this for every k and bound)."""
    idx, d = h16[0][:, :k].copy(), h16[1][:, :k].copy()
    if bound >= 0:
        idx[d > bound], d[d > bound] = -1, -1
    return idx, d


def _check(ids, trun, V, blank, begin, tok, dls, k, bound, what, h16=None):
    """Both layouts of the list (in the original order, and with the by_length view) against the host twin."""
    hidx, hd = nearest_host(ids, trun, V, EOS, PAD, blank, begin, tok, k, bound) if h16 is None else _from_k16(h16, k, bound)
    for dl in dls if isinstance(dls, tuple) else (dls,):
        idx, d = nearest_dev(_dev(ids), _dev(trun), V, blank, dl, k, bound)
        idx, d = idx.cpu().numpy(), d.cpu().numpy()
        bad = np.argwhere((idx != hidx) | (d != hd))
        assert not len(bad), (what, dl.wl.by_length is not None, bad[:5].tolist(), idx[bad[0][0]].tolist(), hidx[bad[0][0]].tolist(),
                              d[bad[0][0]].tolist(), hd[bad[0][0]].tolist())
    return idx, d


@pytest.mark.parametrize("L", [1, 5, 1000, 20011])
@pytest.mark.parametrize("V", [194, 512])
def test_nearest_equals_the_host_twin(cuda, L, V):
    toks, lens, begin, tok, dl, content = _lexicon(L, V)
    rng = np.random.default_rng(L + V)
    for B in (1, 37, 300):
        ids, trun = rows_near(rng, toks, lens, content, B, 25, EOS)
        if B > 1:
            ids[1, :3], trun[1] = [-1, V, 2**31 - 1], 7   # ids outside [0, V) in a row, and a t_run inside it
        h16 = nearest_host(ids, trun, V, EOS, PAD, -1, begin, tok, 16, -1)
        for k, bound in [(k, bd) for k in (1, 3, 8, 16) for bd in (-1, 0, 2)]:
            # the twin itself is called where that is cheap, and for two of the twelve everywhere; else its k = 16 answer is cut
            direct = L * B <= 37000 or (k, bound) in ((3, -1), (16, 2))
            idx, d = _check(ids, trun, V, -1, begin, tok, dl, k, bound, (L, V, B, k, bound), None if direct else h16)
            assert ((idx >= 0) == (d >= 0)).all() and (idx < L).all()
            if bound < 0:
                assert ((idx >= 0).sum(axis=1) == min(k, L)).all()
    if L == 20011:  # one row spans several workgroups, for every B of this test: the slices' keys go through the workspace
        for B in (1, 37, 300):
            assert _ws_bytes(B, L, 3) >= 2 * B * 3 * 8, B
        assert _ws_bytes(7680, L, 3) == 0  # ... and a full bench step needs none: one workgroup per row


def test_nearest_long_rows_and_the_tie_lexicon(cuda):
    V = 194
    rng = np.random.default_rng(5)
    toks, lens = random_lexicon(rng, 200, CONTENT, max_len=63)
    lens[:6] = [63, 63, 62, 62, 61, 1]
    begin, tok = csr(toks, lens)
    dl = (_DevList(begin, tok), _DevList(begin, tok, by_length=True))
    ids = np.asarray(CONTENT)[rng.integers(0, len(CONTENT), (12, 64))].astype(np.int32)
    trun = np.array([62, 63, 64] * 4, dtype=np.int32)
    for b in range(6):  # near copies of the long words: a shifted copy, a copy with two substitutions
        n = int(lens[b])
        ids[b, :] = np.resize(toks[b, :n], 64)
        ids[b, 1:min(n + 1, 64)] = toks[b, :min(n, 63)]
    ids[6, :63] = toks[0, :63]
    ids[6, [5, 40]] = CONTENT[0], CONTENT[1]
    for k, bound in ((1, -1), (3, -1), (8, 2), (16, -1), (3, 0)):
        _check(ids, trun, V, -1, begin, tok, dl, k, bound, ("long", k, bound))
    # blank_id given: the symbol is removed from the rows before they are compared
    _check(ids, trun, V, CONTENT[3], begin, tok, dl, 3, -1, "long, blank")

    content = list(range(3, 23))
    toks, lens, base = tie_lexicon(content)
    begin, tok = csr(toks, lens)
    dl = (_DevList(begin, tok), _DevList(begin, tok, by_length=True))
    ids = np.full((3, 25), EOS, dtype=np.int32)
    ids[0, :6], ids[1, :6], ids[2, :5] = base, base[:2] + [content[0] if base[2] != content[0] else content[1]] + base[3:], base[1:]
    trun = np.full(3, 25, dtype=np.int32)
    for k in (1, 3, 8, 16):
        for bound in (-1, 0, 1, 2):
            idx, d = _check(ids, trun, V, -1, begin, tok, dl, k, bound, ("ties", k, bound))
    idx, d = _check(ids, trun, V, -1, begin, tok, dl, 16, -1, "ties")
    assert d[0, 0] == 0 and (d[0, 1:] == 1).all() and (np.diff(idx[0, 1:]) > 0).all()


# ------------------------------------------------------------------------------------------------ (3) independence, (4) capture
def test_a_rows_result_does_not_depend_on_its_launch(cuda):
    toks, lens, begin, tok, dl, content = _lexicon(20011, 194)
    ids, trun = rows_near(np.random.default_rng(9), toks, lens, content, 37, 25, EOS)
    assert _ws_bytes(1, 20011, 8) // (8 * 8) != _ws_bytes(37, 20011, 8) // (37 * 8 * 8)  # the two launches cut the lexicon differently
    for one in dl:
        idx, d = (t.cpu().numpy() for t in nearest_dev(_dev(ids), _dev(trun), 194, -1, one, 8, -1))
        for b in (0, 17, 36):
            i1, d1 = (t.cpu().numpy() for t in nearest_dev(_dev(ids[b:b + 1]), _dev(trun[b:b + 1]), 194, -1, one, 8, -1))
            assert (i1[0] == idx[b]).all() and (d1[0] == d[b]).all(), b


def test_a_captured_launch_equals_the_eager_one(cuda):
    from manuscript_ocr_amd.recognizers import Lexicon
    itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(ord("a") + i) for i in range(26)]
    rng = np.random.default_rng(21)
    words = sorted({"".join(itos[3 + int(c)] for c in rng.integers(0, 26, int(rng.integers(1, 9)))) for _ in range(3000)})
    lex = Lexicon(words, itos, 25)
    ids = rows_near(rng, *_padded(lex), list(range(3, 29)), 64, 25, EOS)[0]
    ids_dev, trun_dev = _dev(ids), _dev(np.full(64, 25))
    eager = [t.cpu().numpy() for t in lex.nearest_device(ids_dev, trun_dev, 3, 2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lex.nearest_device(ids_dev, trun_dev, 3, 2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lex.nearest_device(ids_dev, trun_dev, 3, 2)
    ids_dev.copy_(_dev(ids[::-1].copy()))   # other inputs in the captured buffers: a replay must compute, not remember
    graph.replay()
    flipped = [t.cpu().numpy() for t in out]
    assert (flipped[0] == eager[0][::-1]).all() and (flipped[1] == eager[1][::-1]).all()
    ids_dev.copy_(_dev(ids))
    graph.replay()
    again = [t.cpu().numpy() for t in out]
    assert (again[0] == eager[0]).all() and (again[1] == eager[1]).all()
    hidx, hd = lex.nearest(ids, None, 3, 2)
    assert (hidx == eager[0]).all() and (hd == eager[1]).all() and (hd >= 0).any() and (hd < 0).any()
    # Lexicon.nearest on a device: host arrays and device tensors
    for given in (ids, ids_dev):
        didx, dd = lex.nearest(given, None, 3, 2, device="cuda")
        assert (didx == hidx).all() and (dd == hd).all()


def _padded(lex):
    lens = np.diff(lex.word_begin)
    toks = np.zeros((len(lens), 16), dtype=np.int64)
    for i, (b, n) in enumerate(zip(lex.word_begin[:-1], lens)):
        toks[i, :n] = lex.word_tok[b:b + n]
    return toks, lens


# ------------------------------------------------------------------------------------------------ (5) - (7) through the product
@pytest.fixture(scope="module")
def product(cuda):
    """test_gpu_nbest.py's pipeline, its two pages, the words' host crops and a lexicon built from the beam decode's own readings
    plus seeded near misses of them."""
    from manuscript_ocr_amd.recognizers import Lexicon
    pipe = _pipe()
    rec = pipe.recognizer
    pages, mo = _pages_and_maps()
    off = pipe.predict_batch(pages, _maps_override=mo)
    crops = [pipe._extract_word_image(arr, np.array(w.polygon, dtype=np.int32)) for page, arr in zip(off, pages)
             for w in page.blocks[0].words if w.text is not None]
    read = [r["text"] for r in rec.predict(crops)] + [r["text"] for r in rec.predict(crops, mode="greedy")]
    rng = np.random.default_rng(2)
    symbols = [s for s in rec.itos if len(s) == 1 and not s.isspace()]
    near = [t[:p] + symbols[int(rng.integers(len(symbols)))] + t[p + 1:] for t in read if t for p in rng.integers(0, len(t), 3)]
    lex = Lexicon(near[::2] + read + near[1::2], rec.stoi, rec.max_length, strict=False)
    assert len(lex) > len(set(read)) >= 4
    return pipe, pages, mo, off, crops, lex


@pytest.fixture(scope="module")
def product_lm(product):
    return _product_lm(product[0].recognizer)


def test_predict_suggest(product, product_lm):
    from manuscript_ocr_amd.recognizers import Lexicon
    pipe, pages, mo, off, crops, lex = product
    rec = pipe.recognizer
    lm = product_lm
    n_checked = 0
    for kw in (dict(mode="greedy"), dict(), dict(lm=lm, lm_weight=0.8), dict(n_best=3), dict(return_chars=True),
               dict(return_chars=True, n_best=3, lm=lm)):
        plain = rec.predict(crops, **kw)
        for k, bound in ((3, None), (16, 1), (1, 0)):
            got = rec.predict(crops, suggest=lex, suggest_k=k, suggest_max_distance=bound, **kw)
            assert len(got) == len(plain)
            for g, p in zip(got, plain):
                assert set(g) == set(p) | {"suggestions"}
                assert {f: v for f, v in g.items() if f != "suggestions"} == p, kw   # bit for bit: the decode is untouched
                assert g["suggestions"] == lex.suggestions(*lex.nearest_texts([g["text"]], k, bound))[0], (kw, g["text"])
                assert len(g["suggestions"]) <= k and all(bound is None or s["distance"] <= bound for s in g["suggestions"])
                if 0 < len(g["text"]) < rec.max_length and "lm" not in kw:
                    # the lexicon holds every plain reading: a lookup that ignored the row could not return each word itself
                    first = g["suggestions"][0]
                    assert (first["text"], first["distance"]) == (g["text"], 0) and lex.words[first["lexicon_index"]] == g["text"]
                    n_checked += 1
    assert n_checked >= 4 * 3 * 4
    assert len({r["text"] for r in rec.predict(crops)}) >= 4  # distinct words: "itself first" is not one constant answer
    # refusals
    crop = crops[:1]
    other = Lexicon(["ab"], ["<PAD>", "<SOS>", "<EOS>", "a", "b"], rec.max_length)
    with pytest.raises(ValueError, match="charset"):
        rec.predict(crop, suggest=other)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be"):
            rec.predict(crop, suggest=lex, suggest_k=bad)
    with pytest.raises(ValueError, match="max_distance"):
        rec.predict(crop, suggest=lex, suggest_max_distance=-1)
    with pytest.raises(ValueError, match="suggest together with a lexicon"):
        rec.predict(crop, suggest=lex, lexicon=lex)
    assert rec.predict([], suggest=lex) == []


def _named(pages):
    return [[w for blk in p.blocks for w in blk.words if w.text is not None] for p in pages]


def _plain_key(pages):
    return [[(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for blk in p.blocks for w in blk.words] for p in pages]


def test_pipeline_suggest(product, product_lm):
    from manuscript_ocr_amd.detectors._types import CharWord, Suggestion, SuggestLmWord, SuggestWord, Word
    pipe, pages, mo, off, crops, lex = product
    rec = pipe.recognizer
    assert pipe.suggest is None and pipe.suggest_k == 3 and pipe.suggest_max_distance is None
    assert all(type(w) is Word for p in off for w in p.blocks[0].words)

    def check(on, base, cls, k, bound):
        assert _plain_key(on) == _plain_key(base)
        assert [p.model_dump() for p in on] == [p.model_dump() for p in base]
        n = 0
        for p in on:
            for blk in p.blocks:
                for w in blk.words:
                    if w.text is None:
                        assert type(w) is Word
                        continue
                    assert type(w) is cls and all(type(s) is Suggestion for s in w.suggestions)
                    assert [s.model_dump() for s in w.suggestions] == lex.suggestions(*lex.nearest_texts([w.text], k, bound))[0]
                    n += 1
        assert n == sum(len(ws) for ws in _named(base)) > 0

    pipe.suggest = lex
    try:
        on = pipe.predict_batch(pages, _maps_override=mo)
        check(on, off, SuggestWord, 3, None)
        assert all(w.suggestions[0].distance == 0 and w.suggestions[0].text == w.text for ws in _named(on) for w in ws if w.text)
        assert all(w.alternatives == [] and w.chars == [] for ws in _named(on) for w in ws)
        # the switches are read at submit
        pipe.suggest_k, pipe.suggest_max_distance = 5, 1
        h = pipe.submit_batch(pages, _maps_override=mo)
        pipe.suggest, pipe.suggest_k, pipe.suggest_max_distance = None, 3, None
        check(pipe.collect_batch(h), off, SuggestWord, 5, 1)
        pipe.suggest = lex
        # with the other switches
        for switch, value in (("char_details", True), ("n_best", 3), ("rectify_crops", True), ("group_lines", True), ("device_order", False)):
            keep = getattr(pipe, switch)
            setattr(pipe, switch, value)
            on = pipe.predict_batch(pages, _maps_override=mo)
            pipe.suggest = None
            base = pipe.predict_batch(pages, _maps_override=mo)
            pipe.suggest = lex
            setattr(pipe, switch, keep)
            check(on, base, SuggestWord, 3, None)
            if switch == "char_details":
                assert all("".join(c.char for c in w.chars) == w.text for ws in _named(on) for w in ws)
            if switch == "n_best":
                assert all(w.alternatives[0].text == w.text for ws in _named(on) for w in ws)
                assert [[w.alternatives for w in ws] for ws in _named(on)] == [[w.alternatives for w in ws] for ws in _named(base)]
        pipe.lm, pipe.lm_weight = product_lm, 0.8
        on = pipe.predict_batch(pages, _maps_override=mo)
        pipe.suggest = None
        base = pipe.predict_batch(pages, _maps_override=mo)
        pipe.suggest = lex
        pipe.lm, pipe.lm_weight = None, 0.5
        check(on, base, SuggestLmWord, 3, None)
        assert [[w.lm_logp for w in ws] for ws in _named(on)] == [[w.lm_logp for w in ws] for ws in _named(base)]
        # the generic route asks predict for them
        pipe.native_fast_path = False
        page = pipe.predict(pages[0])
        pipe.native_fast_path = True
        named = [w for w in page.blocks[0].words if w.text is not None]
        assert named and all(type(w) is SuggestWord for w in named)  # the detector's own boxes: other crops, other words
        assert all([s.model_dump() for s in w.suggestions] == lex.suggestions(*lex.nearest_texts([w.text]))[0] for w in named)
        # refusals at submit
        pipe.lexicon = lex
        with pytest.raises(ValueError, match="suggest together with a lexicon"):
            pipe.submit_batch(pages, _maps_override=mo)
        pipe.lexicon = None
        pipe.suggest_k = 17
        with pytest.raises(ValueError, match="k must be"):
            pipe.submit_batch(pages, _maps_override=mo)
        pipe.suggest_k = 3
    finally:
        pipe.suggest, pipe.suggest_k, pipe.suggest_max_distance, pipe.lexicon, pipe.lm, pipe.lm_weight = None, 3, None, None, None, 0.5
        pipe.native_fast_path = True
    again = pipe.predict_batch(pages, _maps_override=mo)
    assert _plain_key(again) == _plain_key(off) and [p.model_dump() for p in again] == [p.model_dump() for p in off]
    assert not any(isinstance(w, CharWord) for p in again for w in p.blocks[0].words)


def test_pipeline_suggest_on_a_replayed_graph(product, monkeypatch):
    """use_graphs=True: the lookup runs behind the captured decode, on the ids the replay's workspace is finalised to."""
    from manuscript_ocr_amd.detectors._types import SuggestWord
    _, pages, mo, _, _, lex = product
    pipe = _pipe(use_graphs=True)
    grec = pipe.recognizer
    pipe.stream_sets = 1
    pages_dev = torch.from_numpy(np.stack(pages)).cuda()
    seen, finish = [], grec.recognize_finish

    def spy(handle, *a, **kw):
        seen.append((handle.graph_inst is not None, kw.get("suggest") is not None))
        return finish(handle, *a, **kw)

    monkeypatch.setattr(grec, "recognize_finish", spy)
    base = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    pipe.suggest = lex
    on = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen == [(False, False), (True, True)], seen
    assert _plain_key(on) == _plain_key(base)
    words = [w for ws in _named(on) for w in ws]
    assert words and all(type(w) is SuggestWord for w in words)
    assert all([s.model_dump() for s in w.suggestions] == lex.suggestions(*lex.nearest_texts([w.text]))[0] for w in words)


def test_evaluate(product):
    pipe, pages, mo, off, crops, lex = product
    rec = pipe.recognizer
    for kw in (dict(), dict(mode="greedy")):
        read = [r["text"] for r in rec.predict(crops, **kw)]
        ev = rec.evaluate(crops, read, **kw)
        assert ev["n"] == len(crops) and ev["texts"] == read
        assert (ev["distances"] == 0).all() and ev["accuracy"] == 1.0 and ev["cer_mean"] == 0.0 and ev["cer_micro"] == 0.0
        assert ev["ref_lengths"].tolist() == [len(t) for t in read]
        symbols = [s for s in rec.itos if len(s) == 1 and not s.isspace()]
        other = lambda c: symbols[0] if c != symbols[0] else symbols[1]
        # one known edit each: a substitution in a text of odd length, an appended symbol otherwise (also for an empty text)
        edited = [other(t[0]) + t[1:] if len(t) % 2 else t + symbols[2] for t in read]
        assert all(len(t) <= rec.max_length for t in edited)
        ev = rec.evaluate(crops, edited, **kw)
        assert (ev["distances"] == 1).all() and ev["accuracy"] == 0.0 and ev["texts"] == read
        assert ev["ref_lengths"].tolist() == [len(t) for t in edited]
        assert ev["cer_micro"] == len(read) / sum(len(t) for t in edited)
        assert ev["cer_mean"] == pytest.approx(np.mean([1 / len(t) for t in edited]), rel=1e-12)
    from manuscript_ocr_amd.recognizers import edit_distances
    assert edit_distances(read, edited, rec.stoi, device="cuda").tolist() == edit_distances(read, edited, rec.stoi).tolist() == [1] * len(read)
    with pytest.raises(ValueError):
        rec.evaluate(crops, read[:-1])
    with pytest.raises(TypeError):
        rec.evaluate(crops, read, n_best=3)
