"""Nearest lexicon words by confusion-weighted edit distance, on the device: msocr_lexicon_nearest_weighted
(csrc/lexicon_nearest.hip) against its host twin — which tests/test_lexicon_nearest_weighted_cpu.py holds to the textbook weighted
dynamic programme — then the switch through TRBA.predict and Pipeline on test_gpu_lexicon_nearest.py's product fixture.  Integers,
compared exactly.

(1) index and distance of every row and rank equal the host twin's: lexicons of 1, 5, 1 000 and 20 011 words with 63-token words among
    them, V 194 (costs 1..9: ties are common) and 512 (costs 1..255), k 1 / 3 / 16, no bound and a bound, B from 1 (the lexicon cut over
    many workgroups) to 2 000 (one workgroup per row); rows of 0, 1, 63 and 64 symbols, symbols outside [0, V), lexicon words.
(2) The length-bound cases and the 64 * 255 case of the CPU tests.  (3) A row's result does not depend on the other rows of its launch.
(4) A captured and replayed launch equals the eager one.  (5) TRBA.predict(suggest=..., suggest_costs=...); (6) Pipeline.suggest_costs."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_lexicon_nearest import _DevList, _dev, _from_k16, _named, _padded, _plain_key, _stream, _ws_bytes, product  # noqa: F401
from test_lexicon_nearest_cpu import csr, rows_near
from test_lexicon_nearest_weighted_cpu import hard_cases, random_costs, weighted_host

pytestmark = pytest.mark.gpu

EOS, PAD = 2, 0
CONTENT = list(range(3, 40))


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


class _DevCosts:
    """Cost tables on the device, with their struct."""

    def __init__(self, costs):
        from manuscript_ocr_amd import _native as nat
        self.t = [torch.from_numpy(a).cuda() for a in (costs.sub, costs.dele, costs.ins)]
        self.struct = costs.fill(nat.EditCostsTable(), *(t.data_ptr() for t in self.t))


def weighted_dev(ids_dev, trun_dev, V, blank, dl, dc, k, bound):
    from manuscript_ocr_amd import _native as nat
    B, steps = ids_dev.shape
    idx = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    d = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    n_ws = int(nat.lib().msocr_lexicon_nearest_weighted_ws_bytes(B, dl.wl.n_words, k))
    assert n_ws == _ws_bytes(B, dl.wl.n_words, k)
    ws = torch.empty((max(n_ws, 8),), dtype=torch.uint8, device="cuda")
    rc = nat.lib().msocr_lexicon_nearest_weighted(ids_dev.data_ptr(), trun_dev.data_ptr(), B, steps, V, EOS, PAD, blank, ctypes.byref(dl.wl),
                                                  ctypes.byref(dc.struct), k, bound, idx.data_ptr(), d.data_ptr(), ws.data_ptr(), _stream())
    assert rc == 0, rc
    return idx.cpu().numpy(), d.cpu().numpy()


_LEX = {}


def _lexicon(L, V):
    """A seeded random lexicon of L words over a small share of the charset, lengths 1..16 and, from five words on, two of 63 tokens
    and one of 62; with V = 512 tokens from the top of the alphabet take part.  Both device layouts, the costs, and their device copy."""
    if (L, V) not in _LEX:
        rng = np.random.default_rng(11 * L + V)
        content = CONTENT if V == 194 else CONTENT + list(range(508, 512))
        lens = rng.integers(1, 17, L)
        if L >= 5:
            lens[[0, L // 2, L - 1]] = 63, 62, 63
        toks = np.asarray(content)[rng.integers(0, len(content), (L, 63))]
        begin, tok = csr(toks, lens)
        costs = random_costs(rng, V, hi=9 if V == 194 else 255)
        _LEX[(L, V)] = (toks, lens, begin, tok, (_DevList(begin, tok), _DevList(begin, tok, by_length=True)), content, costs, _DevCosts(costs))
    return _LEX[(L, V)]


def _rows(rng, toks, lens, content, B, V):
    """B rows of 64 steps: rows_near's mix of edited lexicon words and free draws, then rows of 0, 1, 63 and 64 symbols, symbols
    outside [0, V), a t_run inside a row and lexicon words as they are, the longest included."""
    ids, trun = rows_near(rng, toks, lens, content, B, 64, EOS, max_len=16)
    free = lambda n: np.asarray(content)[rng.integers(0, len(content), n)]
    special = [([], 64), (free(1), 64), (free(63), 63), (free(64), 64), (toks[0, :lens[0]], 64), (toks[-1, :lens[-1]], 64),
               ([-1, V, 2**31 - 1] + list(toks[0, :5]), 64), (free(30), 7)]
    for b, (s, t) in zip(range(B - 1, -1, -1), special):   # from the back; B = 1 gets the empty row
        ids[b] = EOS
        ids[b, :len(s)] = np.asarray(s, dtype=np.int64).astype(np.int32)
        trun[b] = t
    return ids, trun


def _check(ids, trun, V, blank, begin, tok, dls, costs, dc, k, bound, what, h16=None):
    hidx, hd = weighted_host(ids, trun, V, EOS, PAD, blank, begin, tok, costs, k, bound) if h16 is None else _from_k16(h16, k, bound)
    for dl in dls:
        idx, d = weighted_dev(_dev(ids), _dev(trun), V, blank, dl, dc, k, bound)
        bad = np.argwhere((idx != hidx) | (d != hd))
        assert not len(bad), (what, dl.wl.by_length is not None, bad[:5].tolist(), idx[bad[0][0]].tolist(), hidx[bad[0][0]].tolist(),
                              d[bad[0][0]].tolist(), hd[bad[0][0]].tolist())
    return idx, d


# ------------------------------------------------------------------------------------------------ (1) device == host twin
@pytest.mark.parametrize("L", [1, 5, 1000, 20011])
@pytest.mark.parametrize("V", [194, 512])
def test_weighted_nearest_equals_the_host_twin(cuda, L, V):
    toks, lens, begin, tok, dls, content, costs, dc = _lexicon(L, V)
    rng = np.random.default_rng(L + V)
    ties = 0
    for B in {1: (1, 37), 5: (1, 37, 2000), 1000: (1, 37), 20011: (1, 37)}[L]:
        ids, trun = _rows(rng, toks, lens, content, B, V)
        h16 = weighted_host(ids, trun, V, EOS, PAD, -1, begin, tok, costs, 16, -1)
        bounds = (-1, 0, int(np.median(h16[1][h16[1] >= 0])))
        for k, bound in [(k, bd) for k in (1, 3, 16) for bd in bounds]:
            direct = L * B <= 37000 or (k, bound) == (3, bounds[2])   # else the twin's k = 16 answer is cut to (k, bound)
            idx, d = _check(ids, trun, V, -1, begin, tok, dls, costs, dc, k, bound, (L, V, B, k, bound), None if direct else h16)
            assert ((idx >= 0) == (d >= 0)).all() and (idx < L).all()
            if bound < 0:
                assert ((idx >= 0).sum(axis=1) == min(k, L)).all()
        if B > 1:
            _check(ids, trun, V, content[3], begin, tok, dls, costs, dc, 3, -1, (L, V, B, "blank"))   # blank_id given: removed from the rows
            assert (h16[1][:, 0] == 0).any() and (h16[1][:, 0] > 0).any()                        # lexicon words and others among the rows
        ties += int((h16[1][:, 1:] == h16[1][:, :-1])[h16[1][:, 1:] >= 0].sum())
    if L >= 1000 and V == 194:
        assert ties > 20   # equal distances between different words: the index decides
    if L == 20011:   # B = 1 and 37 cut the lexicon over several workgroups per row; one workgroup per row from B = 1024 on
        assert _ws_bytes(1, L, 3) >= 2 * 3 * 8 and _ws_bytes(37, L, 3) >= 2 * 37 * 3 * 8
    if L == 5:
        assert _ws_bytes(2000, L, 16) == 0 and _ws_bytes(1, L, 16) == 0


# ------------------------------------------------------------------------------------------------ (2) the hard cases
def test_length_bound_and_largest_distance_on_the_device(cuda):
    for name, V, eos, pad, ids, trun, begin, tok, costs, k, bound, want_i, want_d in hard_cases():
        assert (eos, pad) == (EOS, PAD)
        dc = _DevCosts(costs)
        for dl in (_DevList(begin, tok), _DevList(begin, tok, by_length=True)):
            idx, d = weighted_dev(_dev(ids), _dev(trun), V, -1, dl, dc, k, bound)
            assert idx.tolist() == want_i and d.tolist() == want_d, (name, dl.wl.by_length is not None)
    # the first case behind a long list of words that set a threshold first, in 1 024 equal rows so that one workgroup walks the whole
    # list of a row in several passes: the length test then runs against a k-th best distance, not against "nothing yet"
    name, V, eos, pad, ids, trun, begin, tok, costs, k, bound, want_i, want_d = hard_cases()[0]
    lens = np.diff(begin)
    words = [tok[s:s + n] for s, n in zip(begin[:-1], lens)]
    filler = [np.array([4, 4])] * 700               # "bb" 700 times in front: distance 510 each
    begin2, tok2 = csr(filler + words, [2] * 700 + list(lens))
    dc = _DevCosts(costs)
    ids, trun = np.tile(ids, (1024, 1)), np.tile(trun, 1024)
    assert _ws_bytes(1024, 705, 3) == 0
    for dl in (_DevList(begin2, tok2), _DevList(begin2, tok2, by_length=True)):
        idx, d = weighted_dev(_dev(ids), _dev(trun), V, -1, dl, dc, 3, -1)
        assert (idx == [701, 0, 1]).all() and (d == [6, 510, 510]).all(), dl.wl.by_length is not None
        hidx, hd = weighted_host(ids, trun, V, EOS, PAD, -1, begin2, tok2, costs, 3, -1)
        assert (idx == hidx).all() and (d == hd).all()


def test_unknown_below_every_delete_behind_a_threshold(cuda):
    """`unknown` = 1 under tables of 255: a row of "ab" and six symbols outside the charset reaches "ab" at 6.  With the word behind
    700 others in one workgroup's walk, the length test runs against the k-th best distance, and through Lexicon.nearest_texts."""
    from test_lexicon_nearest_weighted_cpu import unknown_cases
    name, V, eos, pad, ids, trun, begin, tok, costs, k, bound, want_i, want_d = unknown_cases()[0]
    lens = np.diff(begin)
    words = [tok[s:s + n] for s, n in zip(begin[:-1], lens)]
    begin2, tok2 = csr([np.array([5, 6])] * 700 + words, [2] * 700 + list(lens))   # 700 words at 2 * 255 + 6 = 516 in front
    dc = _DevCosts(costs)
    ids, trun = np.tile(ids, (1024, 1)), np.tile(trun, 1024)
    assert _ws_bytes(1024, 703, 3) == 0
    for bound in (-1, 6):
        hidx, hd = weighted_host(ids[:2], trun[:2], V, EOS, PAD, -1, begin2, tok2, costs, 3, bound)
        assert hidx[0].tolist() == ([700, 701, 0] if bound < 0 else [700, -1, -1]) and hd[0].tolist()[:1] == [6]
        for dl in (_DevList(begin2, tok2), _DevList(begin2, tok2, by_length=True)):
            idx, d = weighted_dev(_dev(ids), _dev(trun), V, -1, dl, dc, 3, bound)
            assert (idx == hidx[0]).all() and (d == hd[0]).all(), (bound, dl.wl.by_length is not None)
    from manuscript_ocr_amd.recognizers import EditCosts, Lexicon
    itos = ["<PAD>", "<SOS>", "<EOS>"] + list("abcdefgh")
    V = len(itos)
    sub = np.full((V, V), 255)
    np.fill_diagonal(sub, 0)
    ec = EditCosts(sub, np.full(V, 255), np.full(V, 255), itos, unknown=1)
    lex = Lexicon(["cd"] * 1 + ["ef", "gh", "ab"], itos, 25)
    rows = ["aЖbЖЖЖЖЖ"] * 3
    want = lex.nearest_texts(rows, k=2, max_distance=6, costs=ec)
    got = lex.nearest_texts(rows, k=2, max_distance=6, costs=ec, device="cuda")
    assert want[0].tolist() == [[3, -1]] * 3 and want[1].tolist() == [[6, -1]] * 3
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


# ------------------------------------------------------------------------------------------------ (3) independence, (4) capture
def test_a_rows_result_does_not_depend_on_its_launch(cuda):
    toks, lens, begin, tok, dls, content, costs, dc = _lexicon(20011, 194)
    ids, trun = _rows(np.random.default_rng(9), toks, lens, content, 37, 194)
    assert _ws_bytes(1, 20011, 8) // (8 * 8) != _ws_bytes(37, 20011, 8) // (37 * 8 * 8)  # the two launches cut the lexicon differently
    for dl in dls:
        idx, d = weighted_dev(_dev(ids), _dev(trun), 194, -1, dl, dc, 8, -1)
        for b in (0, 17, 33, 36):
            i1, d1 = weighted_dev(_dev(ids[b:b + 1]), _dev(trun[b:b + 1]), 194, -1, dl, dc, 8, -1)
            assert (i1[0] == idx[b]).all() and (d1[0] == d[b]).all(), b


def _letters():
    from manuscript_ocr_amd.recognizers import EditCosts, Lexicon
    itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(ord("a") + i) for i in range(26)]
    rng = np.random.default_rng(21)
    words = sorted({"".join(itos[3 + int(c)] for c in rng.integers(0, 26, int(rng.integers(1, 9)))) for _ in range(3000)})
    lex = Lexicon(words, itos, 25)
    V = len(itos)
    sub = rng.integers(1, 13, (V, V))
    np.fill_diagonal(sub, 0)
    return lex, EditCosts(sub, rng.integers(1, 13, V), rng.integers(1, 13, V), itos), rng


def test_a_captured_launch_equals_the_eager_one(cuda):
    lex, costs, rng = _letters()
    ids = rows_near(rng, *_padded(lex), list(range(3, 29)), 64, 25, EOS)[0]
    ids_dev, trun_dev = _dev(ids), _dev(np.full(64, 25))
    eager = [t.cpu().numpy() for t in lex.nearest_device(ids_dev, trun_dev, 3, 9, costs)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lex.nearest_device(ids_dev, trun_dev, 3, 9, costs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lex.nearest_device(ids_dev, trun_dev, 3, 9, costs)
    ids_dev.copy_(_dev(ids[::-1].copy()))   # other inputs in the captured buffers: a replay must compute, not remember
    graph.replay()
    flipped = [t.cpu().numpy() for t in out]
    assert (flipped[0] == eager[0][::-1]).all() and (flipped[1] == eager[1][::-1]).all()
    ids_dev.copy_(_dev(ids))
    graph.replay()
    again = [t.cpu().numpy() for t in out]
    assert (again[0] == eager[0]).all() and (again[1] == eager[1]).all()
    hidx, hd = lex.nearest(ids, None, 3, 9, costs=costs)
    assert (hidx == eager[0]).all() and (hd == eager[1]).all() and (hd >= 0).any() and (hd < 0).any()
    uidx, _ = lex.nearest(ids, None, 3, None)
    assert (uidx != lex.nearest(ids, None, 3, None, costs=costs)[0]).any()   # the costs change the ranking
    for given in (ids, ids_dev):   # Lexicon.nearest on a device: host arrays and device tensors
        didx, dd = lex.nearest(given, None, 3, 9, device="cuda", costs=costs)
        assert (didx == hidx).all() and (dd == hd).all()


# ------------------------------------------------------------------------------------------------ (5), (6) through the product
@pytest.fixture(scope="module")
def product_costs(product):
    from manuscript_ocr_amd.recognizers import EditCosts
    rec = product[0].recognizer
    V = len(rec.itos)
    rng = np.random.default_rng(6)
    sub = rng.integers(1, 41, (V, V))
    np.fill_diagonal(sub, 0)
    return EditCosts(sub, rng.integers(1, 41, V), rng.integers(1, 41, V), rec.stoi)


def test_predict_suggest_costs(product, product_costs):
    from manuscript_ocr_amd.recognizers import EditCosts
    pipe, pages, mo, off, crops, lex = product
    rec, costs = pipe.recognizer, product_costs
    differs = 0
    for kw in (dict(mode="greedy"), dict(), dict(n_best=3, return_chars=True)):
        for k, bound in ((3, None), (16, 30), (1, 0)):
            base = rec.predict(crops, suggest=lex, suggest_k=k, suggest_max_distance=bound, **kw)
            got = rec.predict(crops, suggest=lex, suggest_k=k, suggest_max_distance=bound, suggest_costs=costs, **kw)
            assert len(got) == len(base) == len(crops)
            want = lex.suggestions(*lex.nearest_texts([g["text"] for g in got], k, bound, costs=costs, device=None))
            for g, b, w in zip(got, base, want):
                assert set(g) == set(b)
                assert {f: v for f, v in g.items() if f != "suggestions"} == {f: v for f, v in b.items() if f != "suggestions"}, kw
                assert g["suggestions"] == w, (kw, k, bound, g["text"])
                assert len(w) <= k and all(bound is None or s["distance"] <= bound for s in w)
                differs += g["suggestions"] != b["suggestions"]
                if 0 < len(g["text"]) < rec.max_length:   # the lexicon holds every plain reading
                    assert (w[0]["text"], w[0]["distance"]) == (g["text"], 0)
    assert differs >= 6   # the weighted ranking is another one
    # refusals
    crop = crops[:1]
    with pytest.raises(ValueError, match="suggest_costs needs suggest"):
        rec.predict(crop, suggest_costs=costs)
    with pytest.raises(ValueError, match="charset"):
        rec.predict(crop, suggest=lex, suggest_costs=EditCosts.uniform(["<PAD>", "<SOS>", "<EOS>", "a", "b"]))
    assert rec.predict([], suggest=lex, suggest_costs=costs) == []


def test_pipeline_suggest_costs(product, product_costs):
    from manuscript_ocr_amd.detectors._types import Suggestion, SuggestWord
    pipe, pages, mo, off, crops, lex = product
    costs = product_costs
    assert pipe.suggest is None and pipe.suggest_costs is None
    off = pipe.predict_batch(pages[:1], _maps_override=tuple(m[:1] for m in mo))   # one small page
    pipe.suggest, pipe.suggest_costs = lex, costs
    try:
        on = pipe.predict_batch(pages[:1], _maps_override=tuple(m[:1] for m in mo))
        assert _plain_key(on) == _plain_key(off)
        words = [w for ws in _named(on) for w in ws]
        assert words and all(type(w) is SuggestWord and all(type(s) is Suggestion for s in w.suggestions) for w in words)
        for w in words:
            assert [s.model_dump() for s in w.suggestions] == lex.suggestions(*lex.nearest_texts([w.text], 3, None, costs=costs))[0]
        assert any([s.model_dump() for s in w.suggestions] != lex.suggestions(*lex.nearest_texts([w.text], 3, None))[0] for w in words)
        # the generic route hands the costs to predict
        pipe.native_fast_path = False
        page = pipe.predict(pages[0])
        pipe.native_fast_path = True
        named = [w for w in page.blocks[0].words if w.text is not None]
        assert named and all([s.model_dump() for s in w.suggestions] == lex.suggestions(*lex.nearest_texts([w.text], costs=costs))[0]
                             for w in named)
        pipe.suggest = None
        with pytest.raises(ValueError, match="suggest_costs needs"):
            pipe.submit_batch(pages[:1], _maps_override=tuple(m[:1] for m in mo))
    finally:
        pipe.suggest, pipe.suggest_costs, pipe.native_fast_path = None, None, True
    again = pipe.predict_batch(pages[:1], _maps_override=tuple(m[:1] for m in mo))
    assert [p.model_dump() for p in again] == [p.model_dump() for p in off]
