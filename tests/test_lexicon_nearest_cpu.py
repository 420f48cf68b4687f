"""Nearest lexicon words by edit distance, host side: csrc/edit_distance.h through the host twins
msocr_edit_distance_pairs_host / msocr_lexicon_nearest_host, the validator msocr_wordlist_check_host, the C ABI's rejections,
Lexicon.nearest_texts, recognizers.metrics, and the header once more in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/native/edit_distance_fuzz.cpp).  No GPU.

The yardstick is the textbook dynamic programme written here (dp_pair, and dp_lexicon vectorised over the lexicon with NumPy).  All
results are integers and compared exactly.  tests/test_gpu_lexicon_nearest.py imports the helpers of this file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

E_ARG = -1
PATTERN_LENS = [0, 1, 2, 31, 32, 33, 62, 63, 64]
WORD_LENS = [1, 31, 32, 33, 62, 63]
# (V, eos_id, pad_id): the content alphabet is [0, V) without the two; tokens 0 and V - 1 are content wherever they can be
ALPHABETS = [(2, 1, 1), (2, 0, 0), (4, 1, 2), (4, 2, 2), (512, 2, 1)]


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


# ------------------------------------------------------------------------------------------------ the reference
def text_of(row, trun, eos, pad, blank):
    """TRBA.texts' rule on one row of ids."""
    out = []
    for v in list(row)[:max(0, min(int(trun), len(row)))]:
        if v == eos:
            break
        if v == pad or (blank >= 0 and v == blank):
            continue
        out.append(int(v))
    return out


def dp_pair(a, b, V):
    """Levenshtein distance, unit costs, one DP row per symbol of a; a symbol outside [0, V) equals nothing."""
    n = len(b)
    b = np.asarray(b, dtype=np.int64).reshape(n)
    ar = np.arange(n + 1)
    prev = ar.copy()
    for i, x in enumerate(a, 1):
        match = (b == x) & (0 <= x < V)
        cur = np.concatenate([[i], np.minimum(prev[:-1] + ~match, prev[1:] + 1)])
        prev = np.minimum.accumulate(cur - ar) + ar  # cur[j] = min(cur[j], cur[j - 1] + 1)
    return int(prev[n])


def dp_lexicon(q, toks, lens, V):
    """The same against every word at once: toks [L, W] (anything behind a word's length), lens [L] -> distances [L]."""
    L, W = toks.shape
    ar = np.arange(W + 1)[None, :]
    prev = np.tile(ar, (L, 1))
    for i, x in enumerate(q, 1):
        match = (toks == x) & (0 <= x < V)
        cur = np.concatenate([np.full((L, 1), i), np.minimum(prev[:, :-1] + ~match, prev[:, 1:] + 1)], axis=1)
        prev = np.minimum.accumulate(cur - ar, axis=1) + ar
    return prev[np.arange(L), lens]


def nearest_ref(dist, k, max_distance):
    """The k smallest (distance, index), a full sort; -1 / -1 behind the last one kept."""
    order = np.lexsort((np.arange(len(dist)), dist))
    if max_distance >= 0:
        order = order[dist[order] <= max_distance]
    order = order[:k]
    idx, d = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32)
    idx[:len(order)], d[:len(order)] = order, dist[order]
    return idx, d


def nearest_ref_rows(ids, trun, eos, pad, blank, toks, lens, V, k, max_distance):
    out = [nearest_ref(dp_lexicon(text_of(r, t, eos, pad, blank), toks, lens, V), k, max_distance) for r, t in zip(ids, trun)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------------------------------------ fixtures and calls
def csr(toks, lens):
    begin = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=begin[1:])
    return begin, np.concatenate([t[:n] for t, n in zip(toks, lens)]).astype(np.int32)


def random_lexicon(rng, L, content, max_len=16):
    lens = rng.integers(1, max_len + 1, L)
    toks = np.asarray(content)[rng.integers(0, len(content), (L, max_len))]
    return toks, lens


def rows_near(rng, toks, lens, content, B, steps, eos, max_len=16):
    """B rows [B, steps]: lengths 0..max_len; half are lexicon words with 0-3 random edits, half independent draws.  EOS-filled, so
    the text is the row up to its length; t_run = steps."""
    ids = np.full((B, steps), eos, dtype=np.int32)
    for b in range(B):
        if b % 2 == 0:
            w = int(rng.integers(len(lens)))
            s = list(toks[w, :lens[w]])
            for _ in range(int(rng.integers(0, 4))):
                op, pos = rng.integers(3), int(rng.integers(0, len(s) + 1))
                if op == 0 and len(s) < max_len:
                    s.insert(pos, content[rng.integers(len(content))])
                elif op == 1 and s:
                    del s[min(pos, len(s) - 1)]
                elif s:
                    s[min(pos, len(s) - 1)] = content[rng.integers(len(content))]
        else:
            s = list(np.asarray(content)[rng.integers(0, len(content), b % (max_len + 1))])
        ids[b, :len(s)] = s[:steps]
    return ids, np.full(B, steps, dtype=np.int32)


def sorted_list(begin, tok):
    """The list stored in ascending (length, index) order: (begin, tok, order) with position p holding word order[p]."""
    lens = np.diff(begin)
    order = np.argsort(lens, kind="stable").astype(np.int32)
    words = [tok[begin[w]:begin[w + 1]] for w in order]
    b2 = np.zeros(len(order) + 1, dtype=np.int32)
    np.cumsum(lens[order], out=b2[1:])
    return b2, np.concatenate(words).astype(np.int32), order


def host_wordlist(begin, tok, by_length=None):
    from manuscript_ocr_amd import _native as nat
    wl = nat.WordList()
    wl.word_begin, wl.word_tok, wl.n_words, wl.n_tok = begin.ctypes.data, tok.ctypes.data, len(begin) - 1, len(tok)
    if by_length is not None:
        wl.by_length = by_length.ctypes.data
    return wl


def nearest_host(ids, trun, V, eos, pad, blank, begin, tok, k, max_distance, by_length=None):
    ids, trun = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(trun, dtype=np.int32)
    B, steps = ids.shape
    idx, d = np.full((B, k), -7, dtype=np.int32), np.full((B, k), -7, dtype=np.int32)
    wl = host_wordlist(begin, tok, by_length)
    rc = _lib().msocr_lexicon_nearest_host(ids.ctypes.data, trun.ctypes.data, B, steps, V, eos, pad, blank, ctypes.byref(wl), k,
                                           max_distance, idx.ctypes.data, d.ctypes.data)
    assert rc == 0, rc
    return idx, d


def pairs_host(a, ta, b, tb, V, eos, pad, blank):
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    ta, tb = np.ascontiguousarray(ta, dtype=np.int32), np.ascontiguousarray(tb, dtype=np.int32)
    B = len(a)
    out = [np.full(B, -7, dtype=np.int32) for _ in range(3)]
    rc = _lib().msocr_edit_distance_pairs_host(a.ctypes.data, ta.ctypes.data, a.shape[1], b.ctypes.data, tb.ctypes.data, b.shape[1], B, V,
                                               eos, pad, blank, *(o.ctypes.data for o in out))
    assert rc == 0, rc
    return out


def pair_grid():
    """The length grid as one batch per alphabet: (V, eos, pad, a [B, 64], ta, b [B, 64], tb).  The rows are bounded by t_run, not by
    an EOS (a 64-symbol row has no room for one); behind t_run they hold other content, which must not be read."""
    rng = np.random.default_rng(11)
    out = []
    for V, eos, pad in ALPHABETS:
        content = [v for v in range(V) if v not in (eos, pad)]
        a_rows, b_rows, ta, tb = [], [], [], []
        for m in PATTERN_LENS:
            for n in WORD_LENS + [64]:
                for near in (False, True):
                    a = np.asarray(content)[rng.integers(0, len(content), 64)]
                    b = np.asarray(content)[rng.integers(0, len(content), 64)]
                    if m:
                        a[[0, m - 1]] = content[0], content[-1]  # tokens 0 and V - 1 (where they are content) take part
                    if near and m:
                        b[:n] = np.resize(a[:m], n)
                        for _ in range(int(rng.integers(0, 4))):
                            b[rng.integers(n)] = content[rng.integers(len(content))]
                    a_rows.append(a), b_rows.append(b), ta.append(m), tb.append(n)
        out.append((V, eos, pad, np.stack(a_rows).astype(np.int32), np.array(ta, np.int32), np.stack(b_rows).astype(np.int32),
                    np.array(tb, np.int32)))
    return out


def tie_lexicon(content, length=6):
    """One word and all its single-substitution variants, shuffled: many candidates at distance 0, 1 and 2 of a row, so that the
    index decides."""
    rng = np.random.default_rng(3)
    base = list(np.asarray(content)[rng.integers(0, len(content), length)])
    words = [base] + [base[:p] + [c] + base[p + 1:] for p in range(length) for c in content if c != base[p]]
    words = [words[i] for i in rng.permutation(len(words))]
    return np.array(words, dtype=np.int64), np.full(len(words), length), base


# ------------------------------------------------------------------------------------------------ tests
def test_pairs_equal_the_dynamic_programme_on_the_length_grid():
    for V, eos, pad, a, ta, b, tb in pair_grid():
        d, la, lb = pairs_host(a, ta, b, tb, V, eos, pad, -1)
        assert (la == ta).all() and (lb == tb).all()
        want = np.array([dp_pair(x[:m], y[:n], V) for x, m, y, n in zip(a, ta, b, tb)])
        bad = np.flatnonzero(d != want)
        assert not len(bad), (V, [(int(ta[i]), int(tb[i]), int(d[i]), int(want[i])) for i in bad[:5]])
        assert len(set(want.tolist())) > (1 if V == 2 else 10)


def test_the_text_rule():
    V, eos, pad, blank = 10, 2, 0, 9
    word = [3, 4, 5, 6]
    rows = [
        ([3, 4, 5, 6, 2, 7, 7, 7], 8, [3, 4, 5, 6]),      # EOS inside t_run ends the text
        ([3, 4, 5, 6, 2, 7, 7, 7], 3, [3, 4, 5]),         # t_run before the EOS
        ([3, 4, 5, 6, 7, 7, 2, 7], 4, [3, 4, 5, 6]),      # EOS outside t_run: never reached
        ([3, 0, 4, 9, 5, 6, 2, 2], 8, [3, 4, 5, 6]),      # PAD and BLANK in the middle are dropped
        ([2, 2, 2, 2, 2, 2, 2, 2], 8, []),                # all EOS: the empty text
        ([3, 4, 5, 6, 7, 8, 3, 4], 8, [3, 4, 5, 6, 7, 8, 3, 4]),  # no EOS: all t_run ids
        ([3, -1, 5, 6, 2, 2, 2, 2], 8, [3, -1, 5, 6]),    # ids outside [0, V): symbols that equal nothing
        ([3, 4, V, 6, 2, 2, 2, 2], 8, [3, 4, V, 6]),
        ([3, 4, 5, 2**31 - 1, 2, 2, 2, 2], 8, [3, 4, 5, 2**31 - 1]),
        ([3, 4, 5, 6, 2, 2, 2, 2], 0, []),
        ([3, 4, 5, 6, 2, 2, 2, 2], -3, []),
        ([3, 4, 5, 6, 7, 2, 2, 2], 99, [3, 4, 5, 6, 7]),  # t_run beyond the row is the row
    ]
    ids = np.array([r[0] for r in rows], dtype=np.int64).astype(np.int32)
    trun = np.array([r[1] for r in rows], dtype=np.int32)
    for b, (row, t, want) in enumerate(rows):
        assert text_of(row, t, eos, pad, blank) == want, b
    other = np.tile(np.array(word + [eos] * 4, dtype=np.int32), (len(rows), 1))
    d, la, lb = pairs_host(ids, trun, other, np.full(len(rows), 8), V, eos, pad, blank)
    assert la.tolist() == [len(r[2]) for r in rows] and (lb == 4).all()
    assert d.tolist() == [dp_pair(r[2], word, V) for r in rows]
    assert d.tolist() == [0, 1, 0, 0, 4, 4, 1, 1, 1, 4, 4, 1]
    # blank_id = -1: 9 is then a symbol like any other
    d2, la2, _ = pairs_host(ids[3:4], trun[3:4], other[:1], [8], V, eos, pad, -1)
    assert la2.tolist() == [5] and d2.tolist() == [1]
    # an id outside [0, V) equals nothing, not even itself on the other side
    same = np.array([[3, -1, V, 2**31 - 1, 2]], dtype=np.int64).astype(np.int32)
    d3, _, _ = pairs_host(same, [5], same, [5], V, eos, pad, blank)
    assert d3.tolist() == [3]
    # ... and the same through the lookup: a one-word lexicon
    begin, tok = csr(np.array([word]), [4])
    idx, dist = nearest_host(ids, trun, V, eos, pad, blank, begin, tok, 1, -1)
    assert (idx == 0).all() and dist[:, 0].tolist() == d.tolist()


@pytest.mark.parametrize("L", [1, 5, 1000])
def test_nearest_equals_a_full_sort_of_the_dp_distances(L):
    V, eos, pad, blank = 194, 2, 0, -1
    content = list(range(3, 60))  # a small share of the charset: near misses and ties are common
    rng = np.random.default_rng(100 + L)
    toks, lens = random_lexicon(rng, L, content)
    begin, tok = csr(toks, lens)
    assert _lib().msocr_wordlist_check_host(begin.ctypes.data, tok.ctypes.data, L, len(tok), V, 63) == 0
    ids, trun = rows_near(rng, toks, lens, content, 37, 25, eos)
    dists = np.stack([dp_lexicon(text_of(r, t, eos, pad, blank), toks, lens, V) for r, t in zip(ids, trun)])
    for k in (1, 3, 8, 16):
        for bound in (0, 1, 2, -1):
            idx, d = nearest_host(ids, trun, V, eos, pad, blank, begin, tok, k, bound)
            want = [nearest_ref(row, k, bound) for row in dists]
            assert (idx == np.stack([w[0] for w in want])).all() and (d == np.stack([w[1] for w in want])).all(), (L, k, bound)
            # the list stored by length, with its permutation, and in any other order: the same answer in the original index
            for b2, t2, order in (sorted_list(begin, tok), _stored(begin, tok, rng.permutation(L).astype(np.int32))):
                i2, d2 = nearest_host(ids, trun, V, eos, pad, blank, b2, t2, k, bound, by_length=order)
                assert (i2 == idx).all() and (d2 == d).all(), (L, k, bound)
    if L == 1000:
        assert (dists.min(axis=1) == 0).sum() >= 3 and (dists.min(axis=1) > 2).sum() >= 3  # hits and out-of-vocabulary rows both occur


def _stored(begin, tok, order):
    lens = np.diff(begin)
    b2 = np.zeros(len(order) + 1, dtype=np.int32)
    np.cumsum(lens[order], out=b2[1:])
    return b2, np.concatenate([tok[begin[w]:begin[w + 1]] for w in order]).astype(np.int32), order


def test_lexicon_sorted_wordlist_is_the_same_list():
    from manuscript_ocr_amd.recognizers import Lexicon
    words = ["cat", "cart", "a", "category", "car", "b", "dog"]
    lex = Lexicon(words, ITOS, 25)
    begin, tok, order = lex.sorted_wordlist()
    assert order.tolist() == [2, 5, 0, 4, 6, 1, 3] and begin.tolist() == [0, 1, 2, 5, 8, 11, 15, 23]
    want = sorted_list(lex.word_begin, lex.word_tok)
    assert (begin == want[0]).all() and (tok == want[1]).all() and (order == want[2]).all()
    assert ["".join(ITOS[t] for t in tok[b:e]) for b, e in zip(begin[:-1], begin[1:])] == [words[i] for i in order]


def test_ties_go_to_the_smaller_index():
    V, eos, pad = 194, 2, 0
    content = list(range(3, 23))
    toks, lens, base = tie_lexicon(content)
    begin, tok = csr(toks, lens)
    other = base[:2] + [content[0] if base[2] != content[0] else content[1]] + base[3:]
    ids = np.full((3, 25), eos, dtype=np.int32)
    ids[0, :6], ids[1, :6], ids[2, :5] = base, other, base[1:]
    trun = np.full(3, 25, dtype=np.int32)
    dists = np.stack([dp_lexicon(text_of(r, 25, eos, pad, -1), toks, lens, V) for r in ids])
    assert (dists[0] == 1).sum() == len(lens) - 1 and (dists[1] == 1).sum() >= 19 and (dists[1] == 2).sum() > 50
    for k in (1, 3, 8, 16):
        for bound in (0, 1, 2, -1):
            idx, d = nearest_host(ids, trun, V, eos, pad, -1, begin, tok, k, bound)
            want = [nearest_ref(row, k, bound) for row in dists]
            assert (idx == np.stack([w[0] for w in want])).all() and (d == np.stack([w[1] for w in want])).all(), (k, bound)
    idx, d = nearest_host(ids, trun, V, eos, pad, -1, begin, tok, 16, -1)
    assert d[0, 0] == 0 and (d[0, 1:] == 1).all() and (np.diff(idx[0, 1:]) > 0).all()


def test_the_validator_refuses_every_single_corruption():
    V = 20
    lens = [3, 1, 5, 2]
    begin, tok = csr(np.arange(20).reshape(4, 5) % V, lens)
    chk = lambda b, t, n_words=4, n_tok=None, v=V, mx=5: _lib().msocr_wordlist_check_host(
        b.ctypes.data, t.ctypes.data, n_words, len(t) if n_tok is None else n_tok, v, mx)
    assert chk(begin, tok) == 0
    for i in range(len(begin)):
        for value in (int(begin[i]) - 1, int(begin[i]) + 1, int(begin[i]) - 100, int(begin[i]) + 100, 2**31 - 1, -2**31):
            b, delta = begin.copy(), value - int(begin[i])
            b[i] = value
            # moving an inner begin by one can leave a valid list of other word lengths only if both neighbours stay in 1..5
            ok = 0 < i < 4 and 1 <= int(b[i]) - int(b[i - 1]) <= 5 and 1 <= int(b[i + 1]) - int(b[i]) <= 5
            assert chk(b, tok) == (0 if ok else E_ARG), (i, delta)
    for i in range(len(tok)):
        for bad in (-1, V, 2**31 - 1, -2**31):
            t = tok.copy()
            t[i] = bad
            assert chk(begin, t) == E_ARG, (i, bad)
    assert chk(begin, tok, mx=4) == E_ARG           # a word longer than max_word_len
    assert chk(begin, tok, mx=64) == E_ARG          # max_word_len beyond 63
    assert chk(begin, tok, mx=0) == E_ARG
    assert chk(begin, tok, n_tok=len(tok) - 1) == E_ARG
    assert chk(begin, tok, n_words=0) == E_ARG
    assert chk(begin, tok, v=0) == E_ARG
    assert _lib().msocr_wordlist_check_host(None, tok.ctypes.data, 4, len(tok), V, 5) == E_ARG
    assert _lib().msocr_wordlist_check_host(begin.ctypes.data, None, 4, len(tok), V, 5) == E_ARG


def test_c_abi_rejections():
    lib = _lib()
    V, eos, pad = 20, 2, 0
    begin, tok = csr(np.arange(20).reshape(4, 5) % V, [3, 1, 5, 2])
    ids, trun = np.full((2, 8), eos, dtype=np.int32), np.full(2, 8, dtype=np.int32)
    idx, d = np.zeros((2, 16), dtype=np.int32), np.zeros((2, 16), dtype=np.int32)
    wl = host_wordlist(begin, tok)

    def call(ids_p=ids.ctypes.data, trun_p=trun.ctypes.data, B=2, steps=8, V=V, eos=eos, pad=pad, blank=-1, wl=wl, k=3, bound=-1,
             idx_p=idx.ctypes.data, d_p=d.ctypes.data):
        return lib.msocr_lexicon_nearest_host(ids_p, trun_p, B, steps, V, eos, pad, blank, None if wl is None else ctypes.byref(wl), k,
                                              bound, idx_p, d_p)
    assert call() == 0 and call(B=0) == 0 and call(k=16) == 0 and call(k=1) == 0 and call(blank=V - 1) == 0 and call(bound=0) == 0
    for kw in (dict(ids_p=None), dict(trun_p=None), dict(idx_p=None), dict(d_p=None), dict(wl=None), dict(B=-1), dict(steps=0),
               dict(steps=65), dict(V=0), dict(V=513), dict(k=0), dict(k=17), dict(bound=-2), dict(eos=-1), dict(eos=V), dict(pad=-1),
               dict(pad=V), dict(blank=-2), dict(blank=V)):
        assert call(**kw) == E_ARG, kw
    for field, val in (("word_begin", None), ("word_tok", None), ("n_words", 0), ("n_words", -1)):
        w2 = host_wordlist(begin, tok)
        setattr(w2, field, val)
        assert call(wl=w2) == E_ARG, field
    # the device entry points refuse the same before any launch (no GPU is touched: nothing is launched)
    assert lib.msocr_lexicon_nearest(None, trun.ctypes.data, 2, 8, V, eos, pad, -1, ctypes.byref(wl), 3, -1, idx.ctypes.data, d.ctypes.data,
                                     None, None) == E_ARG
    assert lib.msocr_lexicon_nearest(ids.ctypes.data, trun.ctypes.data, 2, 8, V, eos, pad, -1, ctypes.byref(wl), 17, -1, idx.ctypes.data,
                                     d.ctypes.data, None, None) == E_ARG
    assert lib.msocr_lexicon_nearest(ids.ctypes.data, trun.ctypes.data, 0, 8, V, eos, pad, -1, ctypes.byref(wl), 3, -1, idx.ctypes.data,
                                     d.ctypes.data, None, None) == 0
    assert lib.msocr_lexicon_nearest_ws_bytes(0, 10, 3) == 0 and lib.msocr_lexicon_nearest_ws_bytes(4, 0, 3) == E_ARG
    assert lib.msocr_lexicon_nearest_ws_bytes(4, 10, 0) == E_ARG and lib.msocr_lexicon_nearest_ws_bytes(4, 10, 17) == E_ARG
    assert lib.msocr_lexicon_nearest_ws_bytes(-1, 10, 3) == E_ARG and lib.msocr_lexicon_nearest_ws_bytes(1, 100000, 3) > 0

    out = [np.zeros(2, dtype=np.int32) for _ in range(3)]

    def pairs(a_p=ids.ctypes.data, ta_p=trun.ctypes.data, sa=8, b_p=ids.ctypes.data, tb_p=trun.ctypes.data, sb=8, B=2, V=V, eos=eos,
              pad=pad, blank=-1, o0=out[0].ctypes.data, o1=out[1].ctypes.data, o2=out[2].ctypes.data):
        return lib.msocr_edit_distance_pairs_host(a_p, ta_p, sa, b_p, tb_p, sb, B, V, eos, pad, blank, o0, o1, o2)
    assert pairs() == 0 and pairs(B=0) == 0
    for kw in (dict(a_p=None), dict(ta_p=None), dict(b_p=None), dict(tb_p=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(sa=0),
               dict(sa=65), dict(sb=0), dict(sb=65), dict(B=-1), dict(V=0), dict(V=513), dict(eos=V), dict(pad=-1), dict(blank=-2),
               dict(blank=V)):
        assert pairs(**kw) == E_ARG, kw
    assert lib.msocr_edit_distance_pairs(None, trun.ctypes.data, 8, ids.ctypes.data, trun.ctypes.data, 8, 2, V, eos, pad, -1,
                                         out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None) == E_ARG


ITOS = ["<PAD>", "<SOS>", "<EOS>"] + list("abcdefghijklmnopqrstuvwxyz") + ["<BLANK>"]


def test_lexicon_nearest_texts():
    from manuscript_ocr_amd.recognizers import Lexicon
    words = ["cat", "cart", "car", "dog", "cot", "a", "category"]
    lex = Lexicon(words, ITOS, 25)
    assert lex.word_begin.tolist() == [0, 3, 7, 10, 13, 16, 17, 25] and len(lex.word_tok) == 25
    assert [lex.word_tok[b:e].tolist() for b, e in zip(lex.word_begin[:-1], lex.word_begin[1:])] == \
           [[ITOS.index(c) for c in w] for w in words]
    idx, d = lex.nearest_texts(["cat", "cut", "", "doge", "cät", "categoryy"], k=3)
    assert idx.tolist() == [[0, 1, 2], [0, 4, 1], [5, 0, 2], [3, 4, 0], [0, 4, 1], [6, 0, 1]]
    assert d.tolist() == [[0, 1, 1], [1, 1, 2], [1, 3, 3], [1, 3, 4], [1, 1, 2], [1, 6, 6]]
    # a character outside the charset is a symbol that matches nothing: "ä" costs one substitution, whatever it is
    assert lex.nearest_texts(["cät"], k=2)[1].tolist() == lex.nearest_texts(["c中t"], k=2)[1].tolist() == [[1, 1]]
    assert lex.suggestions(*lex.nearest_texts(["cut"], k=8, max_distance=1)) == [
        [{"text": "cat", "lexicon_index": 0, "distance": 1}, {"text": "cot", "lexicon_index": 4, "distance": 1}]]
    assert lex.suggestions(*lex.nearest_texts(["zzzzzzzz"], k=2, max_distance=2)) == [[]]
    # ids with a t_run, as a decode returns them
    eos = ITOS.index("<EOS>")
    ids = np.array([[ITOS.index(c) for c in "cart"] + [eos, 5, 5]], dtype=np.int32)
    assert lex.nearest(ids, [7], k=1)[0].tolist() == [[1]] and lex.nearest(ids, [3], k=1)[0].tolist() == [[2]]
    assert lex.nearest(ids, k=1)[1].tolist() == [[0]]
    for kw in (dict(k=0), dict(k=17), dict(max_distance=-1)):
        with pytest.raises(ValueError):
            lex.nearest_texts(["cat"], **kw)
    with pytest.raises(ValueError):
        lex.nearest_texts(["x" * 65])


def test_metrics_by_hand():
    from manuscript_ocr_amd.recognizers import accuracy, character_error_rate, edit_distances
    stoi = {s: i for i, s in enumerate(ITOS)}
    refs = ["kitten", "flaw", "", "", "abc", "слово", "x" * 64]
    hyps = ["sitting", "lawn", "", "ab", "abc", "слова", "y" + "x" * 63]
    assert edit_distances(refs, hyps, stoi).tolist() == [3, 2, 0, 2, 0, 1, 1]
    assert edit_distances(refs, hyps).tolist() == [3, 2, 0, 2, 0, 1, 1]  # without a charset: characters compare by equality
    assert edit_distances([], []).tolist() == []
    assert character_error_rate("kitten", "sitting") == 3 / 6
    assert character_error_rate("", "ab") == float("inf") and character_error_rate("", "") == 0.0
    assert character_error_rate("abc", "") == 1.0
    assert accuracy(["a", "b", "c", "d"], ["a", "x", "c", ""]) == 0.5 and accuracy([], []) == 0.0
    with pytest.raises(ValueError):
        edit_distances(["a"], [])
    with pytest.raises(ValueError):
        edit_distances(["x" * 65], ["x"])


def test_header_under_the_sanitizers(tmp_path):
    """csrc/edit_distance.h in a plain C++ program of its own (tests/native/edit_distance_fuzz.cpp) with the address and
    undefined-behaviour sanitizers: corrupted word lists, garbage rows and t_run values, every array in a heap block of its exact
    size.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "edit_distance_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"),
                           os.path.join(root, "tests", "native", "edit_distance_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 3000 checked")
