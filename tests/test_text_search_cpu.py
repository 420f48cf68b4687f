"""Approximate text search, host side: csrc/text_search.h through the host twin msocr_text_search_host and
msocr_text_search_select_host against yardsticks written here, the C ABI's refusals, recognizers.TextCorpus / search_texts on strings,
PageCorpus / Pipeline.search on hand-built Pages, and the header in a C++ program of its own under the address and
undefined-behaviour sanitizers (tests/native/text_search_fuzz.cpp).  No GPU.

The yardsticks: the plain Sellers table in NumPy (top row 0, first column i) for the ends and distances; for the starts the plain
GLOBAL table of the pattern against every substring that ends at the hit, all lengths at once; the selection rule restated in
Python.  Every comparison is integer equality.  tests/test_gpu_text_search.py imports the helpers of this file."""
import os
import subprocess

import numpy as np
import pytest

E_ARG = -1
MAX_V = 2048


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


def sellers_row(a, b, v):
    """s_0 .. s_n: the bottom row of the table with D[0][j] = 0, D[i][0] = i; a token outside [0, v) equals nothing"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = len(b)
    ar = np.arange(n + 1)
    prev = np.zeros(n + 1, dtype=np.int64)
    for i, x in enumerate(a.tolist()):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i + 1
        ne = (b != x).astype(np.int64) if 0 <= x < v else 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + ne)
        prev = np.minimum.accumulate(cur - ar) + ar
    return prev


def shortest_starts(a, b, v, ends, dists):
    """for every hit (end j, score s): j - l for the smallest l with ed(a, b[j - l .. j)) == s.  ed(a, x) = ed(reversed a, reversed
    x), so one global table of the reversed pattern against b[j-1], b[j-2], .. holds every length in its bottom row; the rows of
    all hits are computed side by side."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    ends, dists = np.asarray(ends, dtype=np.int64), np.asarray(dists, dtype=np.int64)
    if len(ends) == 0:
        return np.zeros(0, dtype=np.int64)
    m = len(a)
    width = int(min(ends.max(), m + dists.max()))
    at = ends[:, None] - 1 - np.arange(width)[None, :]         # b's index of the l-th symbol read backwards
    rev = np.where(at >= 0, b[np.maximum(at, 0)], -5)            # before the text: a token that equals nothing
    ar = np.arange(width + 1)[None, :]
    prev = np.broadcast_to(ar, (len(ends), width + 1)).astype(np.int64)
    for i in range(m):
        x = int(a[m - 1 - i])
        cur = np.empty_like(prev)
        cur[:, 0] = i + 1
        ne = (rev != x).astype(np.int64) if 0 <= x < v else 1
        cur[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + ne)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    ok = (prev == dists[:, None]) & (ar <= ends[:, None])
    assert ok.any(axis=1).all(), "a score that no substring attains"
    return ends - np.argmax(ok, axis=1)


def ref_hits(patterns, ks, texts, v):
    """the full canonical hit list [n, 5] (pattern, text, start, end, distance) by the yardsticks"""
    rows = []
    for q, (a, k) in enumerate(zip(patterns, ks)):
        for t, b in enumerate(texts):
            s = sellers_row(a, b, v)
            ends = np.nonzero(s[1:] <= k)[0] + 1
            dists = s[ends]
            starts = shortest_starts(a, b, v, ends, dists)
            rows += [(q, t, int(st), int(e), int(d)) for st, e, d in zip(starts, ends, dists)]
    return np.array(rows, dtype=np.int32).reshape(-1, 5)


def ref_select(hits):
    """the selection rule of include/msocr.h restated: canonical order; per (pattern, text) by (distance, end) ascending, a hit is
    kept iff [start, end) intersects no kept hit of the group"""
    hits = sorted(map(tuple, np.asarray(hits).reshape(-1, 5).tolist()), key=lambda h: (h[0], h[1], h[3]))
    groups = {}
    for h in hits:
        groups.setdefault((h[0], h[1]), []).append(h)
    out = []
    for group in groups.values():
        kept = []
        for h in sorted(group, key=lambda h: (h[4], h[3])):
            if all(h[3] <= g[2] or g[3] <= h[2] for g in kept):
                kept.append(h)
        out += kept
    return np.array(sorted(out, key=lambda h: (h[0], h[1], h[3])), dtype=np.int32).reshape(-1, 5)


def csr(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    tok = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(0, dtype=np.int32)])
    return tok, off


def host(patterns, ks, texts, v, capacity=None):
    """the host twin -> (hits [min(count, capacity), 5], count)"""
    from manuscript_ocr_amd import ops
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    return ops.text_search_host(pat_tok, pat_off, ks, txt_tok, txt_off, v, capacity=capacity)


def canonical(hits):
    hits = np.asarray(hits, dtype=np.int32).reshape(-1, 5)
    return hits[np.lexsort((hits[:, 3], hits[:, 1], hits[:, 0]))] if len(hits) else hits


def edited(rng, a, v, edits):
    """a copy of a with `edits` random substitutions, insertions or deletions"""
    a = list(np.asarray(a).tolist())
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(a), 1)))
        if op == 0 and a:
            a[at] = int(rng.integers(0, v))
        elif op == 1:
            a.insert(at, int(rng.integers(0, v)))
        elif a:
            del a[at]
    return a


def planted(rng, a, v, n, gap=40):
    """a random text of about n tokens with copies of a carrying 0, 1 and 2 edits planted in it"""
    parts, k = [], 0
    while sum(map(len, parts)) < n:
        parts.append(rng.integers(0, v, int(rng.integers(1, gap))).tolist())
        parts.append(edited(rng, a, v, k % 3))
        k += 1
    return np.array([x for p in parts for x in p], dtype=np.int32)


PATTERN_LENS = (1, 2, 31, 32, 33, 63, 64)


def bounds_of(m):
    return sorted({k for k in (0, 1, 2, m - 1) if 0 <= k < m})


@pytest.mark.parametrize("v", [2, 4, 60])
def test_host_twin_against_the_sellers_table(v):
    """every pattern length and bound against texts of 0, 1, m - 1, m, m + k and about 1000 tokens, the long one with planted copies"""
    rng = np.random.default_rng(200 + v)
    for m in PATTERN_LENS:
        for k in bounds_of(m):
            a = rng.integers(0, v, m).astype(np.int32)
            texts = [rng.integers(0, v + 1, n).astype(np.int32) for n in (0, 1, m - 1, m, m + k)]
            texts.append(planted(rng, a, v, 1000))
            texts.append(np.concatenate([a, a[: m // 2], a]))  # the pattern itself at the text's start and end
            got, count = host([a], [k], texts, v)
            want = ref_hits([a], [k], texts, v)
            assert count == len(want), (m, k)
            assert np.array_equal(got, want), (m, k)
            if k <= 2 and m > 2 * k:  # the start rule's bounds, and the planted copies are found
                assert len(want) and np.all(want[:, 3] - want[:, 2] >= m - want[:, 4]) and np.all(want[:, 3] - want[:, 2] <= m + want[:, 4])
                assert (want[want[:, 1] == 6][:, 4] == 0).sum() >= 2


def test_several_patterns_and_texts_come_in_canonical_order():
    rng = np.random.default_rng(9)
    v = 4
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (3, 1, 64, 7, 33)]
    ks = [1, 0, 20, 2, 5]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (50, 0, 200, 1, 0, 130)]
    got, count = host(patterns, ks, texts, v)
    want = ref_hits(patterns, ks, texts, v)
    assert count == len(want) > 100 and np.array_equal(got, want)
    assert np.array_equal(got, canonical(got)) and len({(h[0], h[1], h[3]) for h in got.tolist()}) == len(got)


@pytest.mark.parametrize("m,k,n", [(1, 0, 9), (5, 0, 5), (5, 2, 40), (64, 63, 200), (64, 0, 63), (33, 32, 100)])
def test_one_symbol_text_against_one_symbol_pattern(m, k, n):
    """every position from m - k on is a hit: the end j costs max(m - j, 0) edits, and the shortest substring that attains it is
    min(j, m) long"""
    got, count = host([np.zeros(m, dtype=np.int32)], [k], [np.zeros(n, dtype=np.int32)], 1)
    ends = list(range(max(m - k, 1), n + 1))
    assert count == len(ends)
    assert got.tolist() == [[0, 0, j - min(j, m), j, max(m - j, 0)] for j in ends]


def test_foreign_tokens_on_both_sides():
    """-1, v and 2^31 - 1 equal nothing, not even themselves, and are never an index"""
    v = 6
    big = 2**31 - 1
    a = np.array([0, -1, 2, v, 4, big, 1], dtype=np.int32)
    texts = [np.array([5, 0, -1, 2, v, 4, big, 1, 3], dtype=np.int32),       # the pattern, foreign tokens included: 3 mismatches
             np.array([0, 3, 2, 3, 4, 3, 1, -1, big, v], dtype=np.int32),
             np.array([big, -1, v, -2**31, v + 1], dtype=np.int32)]
    for k in (0, 3, 6):
        got, count = host([a], [k], texts, v)
        want = ref_hits([a], [k], texts, v)
        assert count == len(want) and np.array_equal(got, want), k
    got, _ = host([a], [3], texts, v)
    assert [0, 0, 1, 8, 3] in got.tolist() and [0, 1, 0, 7, 3] in got.tolist() and not (got[:, 1] == 2).any()
    rng = np.random.default_rng(4)
    wild = np.array([-1, v, big, -2**31, 1, 2, 3], dtype=np.int32)
    patterns = [wild[rng.integers(0, 7, m)] for m in (4, 33, 64)]
    texts = [wild[rng.integers(0, 7, n)] for n in (0, 70, 300)]
    got, count = host(patterns, [2, 20, 50], texts, v)
    assert np.array_equal(got, ref_hits(patterns, [2, 20, 50], texts, v))


def test_capacity_exact_count_and_canonical_prefix():
    rng = np.random.default_rng(12)
    v = 3
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (4, 9)]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (80, 0, 150)]
    full, count = host(patterns, [1, 3], texts, v)
    assert count == len(full) > 20
    for cap in (0, 1, count - 1, count, count + 5):
        part, c = host(patterns, [1, 3], texts, v, capacity=cap)
        assert c == count and np.array_equal(part, full[:cap])
    none, c = host([np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)], [0], [np.zeros(50, dtype=np.int32)], v, capacity=4)
    assert c == 0 and none.shape == (0, 5)
    # nothing behind hits_out[capacity] is written
    L = _lib()
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    ks = np.array([1, 3], dtype=np.int32)
    buf = np.full((7 + 3, 5), -7, dtype=np.int32)
    cnt = np.zeros(1, dtype=np.int64)
    assert L.msocr_text_search_host(pat_tok.ctypes.data, pat_off.ctypes.data, ks.ctypes.data, 2, txt_tok.ctypes.data, txt_off.ctypes.data, 3,
                                    v, buf.ctypes.data, 7, cnt.ctypes.data) == 0
    assert cnt[0] == count and np.array_equal(buf[:7], full[:7]) and (buf[7:] == -7).all()


def test_selection_periodic_and_plateau_cases():
    from manuscript_ocr_amd import ops
    # aaa in aaaaaa: the ends 3, 4, 5, 6 all cost 0; [0, 3) and [3, 6) are kept
    hits, count = host([[0, 0, 0]], [0], [[0] * 6], 2)
    assert count == 4 and hits.tolist() == [[0, 0, j - 3, j, 0] for j in (3, 4, 5, 6)]
    assert ops.text_search_select(hits).tolist() == [[0, 0, 0, 3, 0], [0, 0, 3, 6, 0]]
    # abcd against abcx at k = 1: ends 3 (abc, d deleted) and 4 (x for d) both cost 1; one hit is kept, the earlier end
    hits, count = host([[0, 1, 2, 3]], [1], [[0, 1, 2, 9]], 10)
    assert hits.tolist() == [[0, 0, 0, 3, 1], [0, 0, 0, 4, 1]]
    assert ops.text_search_select(hits).tolist() == [[0, 0, 0, 3, 1]]
    assert ops.text_search_select(np.zeros((0, 5), dtype=np.int32)).shape == (0, 5)


def test_selection_against_the_restated_rule():
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(33)
    v = 3
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (2, 5, 12, 40)]
    ks = [1, 2, 5, 30]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (0, 60, 333)] + [np.zeros(90, dtype=np.int32)]
    hits, _ = host(patterns, ks, texts, v)
    want = ref_select(hits)
    assert 0 < len(want) < len(hits)
    assert np.array_equal(ops.text_search_select(hits), want)
    assert np.array_equal(ops.text_search_select(hits[rng.permutation(len(hits))]), want)  # whatever order the device wrote them in
    assert np.array_equal(ops.text_search_select(want), want)
    L = _lib()
    assert L.msocr_text_search_select_host(None, 3) == E_ARG and L.msocr_text_search_select_host(hits.ctypes.data, -1) == E_ARG
    assert L.msocr_text_search_select_host(None, 0) == 0


def test_symbols_wrappers_and_constants():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    for name in ("msocr_text_search_ws_bytes", "msocr_text_search", "msocr_text_search_host", "msocr_text_search_select_host"):
        assert name in nat.exported_symbols() and hasattr(_lib(), name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "msocr.h")).read()
    for name, value in (("MSOCR_SEARCH_MAX_ALPHABET", ops.SEARCH_MAX_ALPHABET), ("MSOCR_SEARCH_MAX_PATTERN", ops.SEARCH_MAX_PATTERN),
                        ("MSOCR_SEARCH_SEGMENT", ops.SEARCH_SEGMENT)):
        assert f"#define {name} {value}\n" in header
    assert ops.SEARCH_MAX_ALPHABET == MAX_V and ops.SEARCH_MAX_PATTERN == 64 and ops.SEARCH_CAPACITY == 65536


def test_abi_refusals():
    """Everything here is refused before any launch: no GPU is touched."""
    L = _lib()
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    tok = np.zeros(4096, dtype=np.int32)
    hits = np.full((8, 5), -7, dtype=np.int32)
    cnt = np.full(1, -7, dtype=np.int64)
    wsbuf = np.zeros(1 << 16, dtype=np.int64)
    good = dict(pat_off=i32(0, 3, 67), k=i32(2, 63), txt_off=i32(5, 5, 300), v=60)

    def ws(pat_off, k, txt_off, v, Q=None, T=None):
        return L.msocr_text_search_ws_bytes(pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt_off.ctypes.data,
                                            len(txt_off) - 1 if T is None else T, v)

    def run_host(pat_off, k, txt_off, v, Q=None, T=None, cap=8, pat=tok.ctypes.data, txt=tok.ctypes.data, out=hits.ctypes.data,
                 count=cnt.ctypes.data):
        return L.msocr_text_search_host(pat, pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt, txt_off.ctypes.data,
                                        len(txt_off) - 1 if T is None else T, v, out, cap, count)

    def run_dev(pat_off, k, txt_off, v, Q=None, T=None, cap=8, ws_ptr=wsbuf.ctypes.data, ws_bytes=wsbuf.nbytes, pat=tok.ctypes.data,
                txt=tok.ctypes.data, out=hits.ctypes.data, count=cnt.ctypes.data):  # `tok` stands in for device memory: a refused call reads nothing
        return L.msocr_text_search(pat, pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt, txt_off.ctypes.data,
                                   len(txt_off) - 1 if T is None else T, v, out, cap, count, ws_ptr, ws_bytes, None)

    # the workspace formula of include/msocr.h
    need = ws(**good)
    assert need == (16 * 2 * 60 + 8 * 3 + 4 * 3 + 4 * 3 + 4 * 2 + 7) // 8 * 8
    assert ws(i32(0, 64), i32(63), i32(0, 2**31 - 1), MAX_V) == 16 * MAX_V + 16 + 8 + 8 + 4 + 4
    assert run_host(**good) == 0 and cnt[0] >= 0
    bad = [
        dict(good, pat_off=i32(0, 3, 2)),          # offsets that decrease: a length below 1
        dict(good, pat_off=i32(0, 3, 3)),          # an empty pattern
        dict(good, pat_off=i32(0, 3, 68)),         # a pattern of 65 tokens
        dict(good, pat_off=i32(-1, 3, 67)),        # a start below 0
        dict(good, txt_off=i32(5, 4, 300)),
        dict(good, txt_off=i32(-2, 5, 300)),
        dict(good, txt_off=i32(2**31 - 1, -2**31, 0)),
        dict(good, k=i32(3, 63)),                  # k == m
        dict(good, k=i32(2, 64)),
        dict(good, k=i32(-1, 63)),
        dict(good, v=0), dict(good, v=-5), dict(good, v=MAX_V + 1),
    ]
    for case in bad:
        assert ws(**case) == E_ARG, case
        assert run_host(**case) == E_ARG, case
        assert run_dev(**case) == E_ARG, case
    for kw in (dict(Q=-1), dict(T=-1)):
        assert ws(**good, **kw) == E_ARG and run_host(**good, **kw) == E_ARG and run_dev(**good, **kw) == E_ARG
    assert run_host(**good, cap=-1) == E_ARG and run_dev(**good, cap=-1) == E_ARG
    for null in ("pat", "txt", "out", "count"):
        assert run_host(**good, **{null: None}) == E_ARG and run_dev(**good, **{null: None}) == E_ARG, null
    assert L.msocr_text_search_ws_bytes(None, good["k"].ctypes.data, 2, good["txt_off"].ctypes.data, 2, 60) == E_ARG
    assert L.msocr_text_search_ws_bytes(good["pat_off"].ctypes.data, None, 2, good["txt_off"].ctypes.data, 2, 60) == E_ARG
    assert L.msocr_text_search_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 2, 60) == E_ARG
    assert run_dev(**good, ws_bytes=need - 1) == E_ARG                              # a workspace smaller than required
    assert run_dev(**good, ws_ptr=wsbuf.ctypes.data + 4, ws_bytes=wsbuf.nbytes - 4) == E_ARG  # misaligned
    assert run_dev(**good, ws_ptr=None) == E_ARG
    # no pattern or no text: MSOCR_OK with count 0, no workspace, the offsets of the empty side are not read
    cnt[0] = -7
    assert L.msocr_text_search_ws_bytes(None, None, 0, good["txt_off"].ctypes.data, 2, 60) == 0
    assert L.msocr_text_search_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 0, 60) == 0
    assert L.msocr_text_search_host(tok.ctypes.data, None, None, 0, tok.ctypes.data, good["txt_off"].ctypes.data, 2, 60, hits.ctypes.data, 8,
                                    cnt.ctypes.data) == 0 and cnt[0] == 0
    cnt[0] = -7
    assert L.msocr_text_search_host(tok.ctypes.data, good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, tok.ctypes.data, None, 0, 60,
                                    hits.ctypes.data, 8, cnt.ctypes.data) == 0 and cnt[0] == 0
    assert L.msocr_text_search_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 0, 0) == E_ARG  # v is still checked


# ------------------------------------------------------------------------------------------------ the Python layer
def test_text_corpus_and_search_texts_on_strings():
    from manuscript_ocr_amd.recognizers import TextCorpus, TextHit, search_texts
    texts = ["был Ивановъ, и Нванов тут", "", "Иванов", "никого"]
    hits = search_texts(["Иванов"], texts, max_distance=1)
    assert hits == [TextHit(0, 0, 4, 10, 0), TextHit(0, 0, 16, 21, 1), TextHit(0, 2, 0, 6, 0)]
    assert all(isinstance(h, TextHit) and texts[h.text][h.start:h.end] in ("Иванов", "ванов") for h in hits)
    corpus = TextCorpus(texts)
    assert len(corpus) == 4 and corpus.v == len(set("".join(texts))) and corpus.stoi["б"] == 0 and corpus.stoi["ы"] == 1
    assert corpus.search(["Иванов"], max_distance=1) == hits
    assert corpus.search(["Иванов"], max_distance=[1]) == hits
    assert corpus.search(["Иванов"], max_error_rate=0.2) == hits                  # floor(0.2 * 6) = 1
    assert corpus.search(["Иванов"], max_error_rate=0.1) == [h for h in hits if h.distance == 0]
    assert corpus.search(["И"], max_error_rate=5.0) == corpus.search(["И"], max_distance=0)  # k = min(floor(rate m), m - 1)
    # a character the corpus does not hold matches nothing: one edit
    assert corpus.search(["Иваzов"], max_distance=1) == [TextHit(0, 0, 4, 10, 1), TextHit(0, 2, 0, 6, 1)]
    assert corpus.search(["zzz"], max_distance=2) == [] and corpus.search([], max_distance=0) == []
    # overlapping=True: every end within the bound, canonical order
    every = corpus.search(["Иванов", "тут"], max_distance=1, overlapping=True)
    assert [h for h in every if h.text == 2] == [TextHit(0, 2, 0, 5, 1), TextHit(0, 2, 0, 6, 0)]
    assert every == sorted(every, key=lambda h: (h.pattern, h.text, h.end)) and len(every) > len(hits)
    assert [(h.pattern, h.text, h.distance) for h in every if h.pattern == 1 and h.distance == 0] == [(1, 0, 0)]
    # a two-word phrase and a name inside a longer token
    assert search_texts(["и Нванов"], texts, max_distance=0) == [TextHit(0, 0, 13, 21, 0)]
    assert search_texts(["x" * 64], ["y" + "x" * 70], max_distance=0, overlapping=True) == [TextHit(0, 0, j - 64, j, 0) for j in range(65, 72)]
    assert TextCorpus([]).search(["a"], max_distance=0) == [] and TextCorpus(["", ""]).search(["a"], max_distance=0) == []
    for bad in (dict(max_distance=None), dict(max_distance=1, max_error_rate=0.5), dict(max_distance=6), dict(max_distance=-1),
                dict(max_distance=[1, 1]), dict(max_error_rate=-0.5)):
        with pytest.raises(ValueError):
            corpus.search(["Иванов"], **bad)
    with pytest.raises(ValueError):
        corpus.search([""], max_distance=0)
    with pytest.raises(ValueError):
        corpus.search(["x" * 65], max_distance=0)
    with pytest.raises(TypeError):
        corpus.search([5], max_distance=0)
    with pytest.raises(TypeError):
        TextCorpus([["a"]])
    with pytest.raises(ValueError):
        TextCorpus(["".join(chr(0x4E00 + k) for k in range(MAX_V + 1))])
    assert TextCorpus(["".join(chr(0x4E00 + k) for k in range(MAX_V))]).search([chr(0x4E00 + MAX_V - 1)], max_distance=0) == \
        [TextHit(0, 0, MAX_V - 1, MAX_V, 0)]


def hand_pages():
    from manuscript_ocr_amd.detectors._types import Block, Page, Word
    W = lambda t: Word(polygon=[(0, 0), (1, 0), (1, 1), (0, 1)], detection_confidence=0.5, text=t)  # noqa: E731
    return [Page(blocks=[Block(words=[W("alpha"), W(None), W("beta"), W("")]), Block(words=[W("gamma"), W("delta")])]),
            Page(blocks=[]),
            Page(blocks=[Block(words=[W(None)]), Block(words=[W("betta"), W("gamma")])])]


def test_page_corpus_and_pipeline_search_on_hand_built_pages():
    from manuscript_ocr_amd import PageCorpus, Pipeline
    from manuscript_ocr_amd.detectors._types import SearchHit
    pages = hand_pages()
    corpus = PageCorpus(pages)
    assert corpus.texts == ["alpha beta gamma delta", "", "betta gamma"] and len(corpus) == 3
    hits = corpus.search(["lph", "pha  bet", " beta\tgamma ", "a", "ta ga"], max_distance=0)
    assert all(isinstance(h, SearchHit) for h in hits)
    by_query = lambda q: [(h.page, h.start, h.end, h.matched_text, h.words) for h in hits if h.query == q]  # noqa: E731
    assert by_query(0) == [(0, 1, 4, "lph", [(0, 0)])]                              # inside one word
    assert by_query(1) == [(0, 2, 9, "pha bet", [(0, 0), (0, 2)])]                  # across two words; the word without text is skipped
    assert by_query(2) == [(0, 6, 16, "beta gamma", [(0, 2), (1, 0)])]              # across a block boundary
    assert hits[1].query_text == "pha bet" and hits[2].query_text == "beta gamma"
    assert [(h.page, h.words) for h in hits if h.query == 3][:3] == [(0, [(0, 0)]), (0, [(0, 0)]), (0, [(0, 2)])]
    assert by_query(4) == [(0, 8, 13, "ta ga", [(0, 2), (1, 0)]), (2, 3, 8, "ta ga", [(1, 0), (1, 1)])]
    assert hits == sorted(hits, key=lambda h: (h.query, h.page, h.end))
    # a separator alone counts for no word: "a " matched at the end of "alpha " touches alpha only
    sep = corpus.search(["a b"], max_distance=0)
    assert [(h.page, h.start, h.end, h.words) for h in sep] == [(0, 4, 7, [(0, 0), (0, 2)])]
    assert corpus.words_of(0, 5, 6) == [] and corpus.words_of(0, 5, 7) == [(0, 2)] and corpus.words_of(0, 4, 6) == [(0, 0)]
    # one error: betta for beta
    near = corpus.search(["beta gamma"], max_distance=1)
    assert [(h.page, h.distance, h.matched_text, h.words) for h in near] == [(0, 0, "beta gamma", [(0, 2), (1, 0)]),
                                                                            (2, 1, "betta gamma", [(1, 0), (1, 1)])]
    assert corpus.search(["beta gamma"], max_error_rate=0.1) == near
    # Pipeline.search takes Pages as they are: neither the networks nor a GPU
    pipe = Pipeline.__new__(Pipeline)
    assert pipe.search(pages, ["beta gamma"], max_distance=1) == near
    assert pipe.search([], ["x"], max_distance=0) == [] and pipe.search(pages, [], max_distance=0) == []
    with pytest.raises(ValueError):
        pipe.search(pages, ["beta"], max_distance=1, max_error_rate=0.1)
    with pytest.raises(ValueError):
        pipe.search(pages, ["  "], max_distance=0)


def test_pipeline_search_sends_images_through_predict():
    from manuscript_ocr_amd import Pipeline
    from test_quad_match_cpu import StandInDetector, StandInRecognizer, rect
    det = [rect(10, 10, 50, 30), rect(104, 10, 144, 30), rect(10, 60, 50, 80), rect(120, 60, 160, 80)]
    img = np.full((140, 260, 3), 255, dtype=np.uint8)
    for k, q in enumerate(det):
        img[q[0][1]: q[2][1], q[0][0]: q[2][0]] = 10 + k
    pipe = Pipeline(detector=StandInDetector(det), recognizer=StandInRecognizer({10: "alpha", 11: "beta", 12: "", 13: "delta"}))
    page = pipe.predict(img)
    own = " ".join(w.text for b in page.blocks for w in b.words if w.text)
    hits = pipe.search([img, page], ["beta", "delt"], max_distance=0)
    assert [(h.query, h.page, h.matched_text) for h in hits] == [(0, 0, "beta"), (0, 1, "beta"), (1, 0, "delt"), (1, 1, "delt")]
    for h in hits:
        assert own[h.start:h.end] == h.matched_text and len(h.words) == 1
        b, w = h.words[0]
        assert h.matched_text in page.blocks[b].words[w].text


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/text_search.h (scan, segment window, start walk, host twin, argument check, selection) in a plain C++ program of its own
    (tests/native/text_search_fuzz.cpp) with the address and undefined-behaviour sanitizers: garbage tokens and offsets, every array
    in a heap block of its exact size, every result compared with a plain table.  Run as a child process; nothing is loaded into
    this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "text_search_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "text_search_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 400 checked 400")
