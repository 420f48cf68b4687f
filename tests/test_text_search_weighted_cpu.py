"""Approximate text search under confusion-weighted costs, host side: csrc/text_search_weighted.h through the
host twin msocr_text_search_weighted_host against a plain table written here, the direction of the tables on a hand-worked case, uniform
costs against the unit-cost twin, the bound clamp, the C ABI's refusals, TextCorpus / PageCorpus / Pipeline.search with costs=, and the
header in a C++ program of its own under the address and undefined-behaviour sanitizers (tests/native/text_search_weighted_fuzz.cpp).
No GPU.  Every comparison is integer equality.  tests/test_gpu_text_search_weighted.py imports the helpers of this file."""
import os
import subprocess

import numpy as np
import pytest

from test_text_search_cpu import PATTERN_LENS, bounds_of, canonical, csr, hand_pages, planted
from test_text_search_cpu import host as unit_host

E_ARG = -1
MAX_V = 768
MAX_W = 256


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


def make_costs(sub, delete, insert, unknown):
    """an EditCosts over V anonymous symbols"""
    from manuscript_ocr_amd.recognizers import EditCosts
    V = len(delete)
    return EditCosts(sub, delete, insert, [f"<{k}>" for k in range(V)], unknown=unknown)


def random_costs(rng, V, top=9):
    """asymmetric tables: sub[a][b] != sub[b][a] for most pairs, del != ins"""
    sub = rng.integers(1, top + 1, (V, V))
    np.fill_diagonal(sub, 0)
    return make_costs(sub, rng.integers(1, top + 1, V), rng.integers(1, top + 1, V), int(rng.integers(1, top + 1)))


class Plain:
    """the contract of include/msocr.h restated in plain Python"""

    def __init__(self, costs, tok_class, v):
        self.sub, self.dele, self.ins = costs.sub.tolist(), costs.delete.tolist(), costs.insert.tolist()
        self.V, self.unknown, self.v, self.cls = costs.num_classes, costs.unknown, v, [int(c) for c in tok_class]

    def klass(self, t):
        if not 0 <= t < self.v:
            return -1
        return self.cls[t] if 0 <= self.cls[t] < self.V else -1

    def w_sub(self, t, p):
        if t == p and 0 <= t < self.v:
            return 0
        ct, cp = self.klass(t), self.klass(p)
        return self.sub[ct][cp] if ct >= 0 and cp >= 0 else self.unknown

    def w_del(self, t):
        return self.dele[self.klass(t)] if self.klass(t) >= 0 else self.unknown

    def w_ins(self, p):
        return self.ins[self.klass(p)] if self.klass(p) >= 0 else self.unknown

    def column(self, prev, t, a, top):
        """the column behind text token t from the column before it; top = its row-0 entry"""
        cur = [top]
        wd = self.w_del(t)
        for i, p in enumerate(a):
            cur.append(min(prev[i] + self.w_sub(t, p), prev[i + 1] + wd, cur[i] + self.w_ins(p)))
        return cur

    def first_column(self, a):
        col = [0]
        for p in a:
            col.append(col[-1] + self.w_ins(p))
        return col

    def global_distance(self, a, b):
        col = self.first_column(a)
        for t in b:
            col = self.column(col, t, a, col[0] + self.w_del(t))
        return col[-1]

    def by_definition(self, a, b, j):
        """(the least global_distance(a, b[s:j]) over 0 <= s <= j, the largest s that attains it): the forward tables of all starts
        side by side, row s of `cols` being the column of start s; after j steps row s holds global_distance(a, b[s:j])"""
        m = len(a)
        sub = np.array([[self.w_sub(t, p) for p in a] for t in b[:j]], dtype=np.int64).reshape(j, m)
        dele = np.array([self.w_del(t) for t in b[:j]], dtype=np.int64)
        ins = [self.w_ins(p) for p in a]
        cols = np.tile(np.array(self.first_column(a), dtype=np.int64), (j + 1, 1))
        for step in range(j):                       # start s reads b[s + step]; the starts s >= j - step are done
            n = j - step
            at = np.arange(n) + step
            old = cols[:n].copy()
            cols[:n, 0] = old[:, 0] + dele[at]
            for i in range(1, m + 1):
                cols[:n, i] = np.minimum(np.minimum(old[:, i - 1] + sub[at, i - 1], old[:, i] + dele[at]), cols[:n, i - 1] + ins[i - 1])
        final = cols[:, m]
        least = int(final.min())
        return least, int(np.nonzero(final == least)[0].max())

    def hits(self, patterns, ks, texts):
        rows = []
        for q, (a, k) in enumerate(zip(patterns, ks)):
            a = [int(x) for x in a]
            first = self.first_column(a)
            k = min(int(k), first[-1] - 1)
            for t, b in enumerate(texts):
                b = [int(x) for x in b]
                col = first
                for j in range(1, len(b) + 1):
                    col = self.column(col, b[j - 1], a, 0)
                    if col[-1] <= k:
                        least, start = self.by_definition(a, b, j)
                        assert least == col[-1], "the semi-global table and the definition disagree"
                        rows.append((q, t, start, j, col[-1]))
        return np.array(rows, dtype=np.int32).reshape(-1, 5)


def host(patterns, ks, texts, v, tok_class, costs, capacity=None):
    """the host twin -> (hits [min(count, capacity), 5], count)"""
    from manuscript_ocr_amd import ops
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    return ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, txt_off, v, tok_class, costs, capacity=capacity)


def noisy(rng, a, v, edits):
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


@pytest.mark.parametrize("V", [1, 7, 194])
def test_host_twin_against_the_plain_table(V):
    """asymmetric random tables, a class map that is not injective and has holes, foreign and garbage tokens on both sides, texts of
    0 to 200 tokens with noisy copies of the pattern"""
    rng = np.random.default_rng(700 + V)
    v = 12
    costs = random_costs(rng, V)
    if V > 1:
        assert (costs.sub != costs.sub.T).any() and (costs.delete != costs.insert).any()
    tok_class = rng.integers(0, V, v).astype(np.int32)
    tok_class[[3, 7]] = -1                      # corpus characters outside the charset
    tok_class[5] = tok_class[4]                 # two tokens of one class
    tok_class[9], tok_class[10] = V, -2**31     # garbage classes
    P = Plain(costs, tok_class, v)
    wild = np.array([-1, v, 2**31 - 1, -2**31], dtype=np.int32)
    seen = 0
    for m in (1, 8, 9, 64):
        a = rng.integers(0, v, m).astype(np.int32)
        if m >= 8:
            a[2], a[5] = -1, v + 3              # foreign tokens in the pattern
        full = P.first_column(a.tolist())[-1]
        for k in sorted({0, min(6, full - 1), min(14, full - 1)}):
            parts = [rng.integers(0, v, 30), noisy(rng, a, v, 1), rng.integers(0, v, 25), a, wild[rng.integers(0, 4, 6)], noisy(rng, a, v, 2)]
            long_text = np.concatenate([np.asarray(p, dtype=np.int32) for p in parts])[:200]
            texts = [np.zeros(0, dtype=np.int32), a[:1], a, np.concatenate([a, a]), long_text]
            got, count = host([a], [k], texts, v, tok_class, costs)
            want = P.hits([a], [k], texts)
            assert count == len(want) and np.array_equal(got, want), (m, k)
            assert (want[:, 2] < want[:, 3]).all()
            seen += len(want)
    assert seen >= 20
    # the walk's start against the definition itself: every start behind it gives another distance
    a = [0, 1, 4, 5, 2]
    b = rng.integers(0, 6, 60).tolist()
    want = P.hits([a], [P.first_column(a)[-1] - 1], [b])
    assert len(want) > 20
    for _q, _t, s, j, d in want.tolist():
        assert P.global_distance(a, b[s:j]) == d and all(P.global_distance(a, b[x:j]) != d for x in range(s + 1, j + 1))
        assert d == min(P.global_distance(a, b[x:j]) for x in range(j + 1))


def test_several_patterns_and_texts_come_in_canonical_order_and_capacity_holds():
    rng = np.random.default_rng(5)
    v, V = 5, 4
    costs = random_costs(rng, V, top=4)
    tok_class = np.array([0, 1, 2, 3, 1], dtype=np.int32)
    patterns = [rng.integers(0, v, m).astype(np.int32) for m in (3, 1, 40, 7)]
    ks = [3, 0, 30, 5]
    texts = [rng.integers(0, v, n).astype(np.int32) for n in (50, 0, 130, 1, 0)]
    full, count = host(patterns, ks, texts, v, tok_class, costs)
    want = Plain(costs, tok_class, v).hits(patterns, ks, texts)
    assert count == len(want) > 50 and np.array_equal(full, want) and np.array_equal(full, canonical(full))
    for cap in (0, 1, count - 1, count, count + 5):
        part, c = host(patterns, ks, texts, v, tok_class, costs, capacity=cap)
        assert c == count and np.array_equal(part, full[:cap])
    L = _lib()
    pat_tok, pat_off = csr(patterns)
    txt_tok, txt_off = csr(texts)
    kk = np.array(ks, dtype=np.int32)
    buf = np.full((7 + 3, 5), -7, dtype=np.int32)
    cnt = np.zeros(1, dtype=np.int64)
    assert L.msocr_text_search_weighted_host(pat_tok.ctypes.data, pat_off.ctypes.data, kk.ctypes.data, 4, txt_tok.ctypes.data,
                                             txt_off.ctypes.data, 5, v, tok_class.ctypes.data, costs.struct(None), buf.ctypes.data, 7,
                                             cnt.ctypes.data) == 0
    assert cnt[0] == count and np.array_equal(buf[:7], full[:7]) and (buf[7:] == -7).all()


def ivanov_costs():
    """и and н are confused one way only: a true и is often read as н (text н, pattern и: sub[н][и] = 1), never the reverse"""
    from manuscript_ocr_amd.recognizers import EditCosts
    charset = ["и", "н", "в", "а", "о", "ъ"]
    V = len(charset)
    sub = np.full((V, V), 9)
    np.fill_diagonal(sub, 0)
    sub[1, 0] = 1                               # reading the recognised н as the true и
    delete, insert = np.full(V, 9), np.full(V, 9)
    delete[5] = 2                               # a trailing ъ the recogniser added is cheap to drop; supplying one is dear
    return EditCosts(sub, delete, insert, charset, unknown=9)


def test_direction_of_the_tables_on_a_hand_worked_case():
    """tokens и н в а о ъ = 0..5.  Text нванов, query иванов: one substitution sub[н][и] = 1.  Text иванов, query нванов: the same
    edit the other way costs sub[и][н] = 9.  A transposed sub swaps the two results; swapped ins / del swap the ъ cases."""
    costs = ivanov_costs()
    v = 6
    cls = np.arange(v, dtype=np.int32)
    ivanov, nvanov = [0, 2, 3, 1, 4, 2], [1, 2, 3, 1, 4, 2]
    got, _ = host([ivanov], [1], [nvanov], v, cls, costs)
    assert got.tolist() == [[0, 0, 0, 6, 1]]
    got, _ = host([nvanov], [1], [ivanov], v, cls, costs)
    assert got.tolist() == []
    got, _ = host([nvanov], [9], [ivanov], v, cls, costs)
    assert got.tolist() == [[0, 0, 1, 6, 9]]     # supplying н in front of ванов costs 9 too: the shorter substring is reported
    # the text has a ъ too many: the end behind it costs del[ъ] = 2; the text lacks the pattern's ъ: ins[ъ] = 9
    got, _ = host([ivanov], [2], [ivanov + [5]], v, cls, costs)
    assert got.tolist() == [[0, 0, 0, 6, 0], [0, 0, 0, 7, 2]]
    got, _ = host([ivanov + [5]], [8], [ivanov], v, cls, costs)
    assert got.tolist() == []
    got, _ = host([ivanov + [5]], [9], [ivanov], v, cls, costs)
    assert got.tolist() == [[0, 0, 0, 6, 9]]
    # many cheap confusions are accepted where one implausible edit is not: two и read as н cost 2, one в read as о costs 9
    got, _ = host([[0, 2, 0, 2]], [2], [[1, 2, 1, 2], [0, 4, 0, 2]], v, cls, costs)
    assert got.tolist() == [[0, 0, 0, 4, 2]]


@pytest.mark.parametrize("v", [2, 4, 60])
@pytest.mark.parametrize("inside", [True, False])
def test_uniform_costs_are_the_unit_search(v, inside):
    """EditCosts.uniform(charset, 1): the records of msocr_text_search_host on the random cases of test_text_search_cpu, with the
    corpus characters inside the charset (no two of one class: those would match at the diagonal's 0) or all outside it"""
    from manuscript_ocr_amd.recognizers import EditCosts
    costs = EditCosts.uniform([f"<{k}>" for k in range(v + 3)], 1)
    tok_class = (np.arange(v) + 3).astype(np.int32) if inside else np.full(v, -1, dtype=np.int32)
    rng = np.random.default_rng(200 + v)
    for m in PATTERN_LENS:
        for k in bounds_of(m):
            a = rng.integers(0, v, m).astype(np.int32)
            texts = [rng.integers(0, v + 1, n).astype(np.int32) for n in (0, 1, m - 1, m, m + k)]
            texts.append(planted(rng, a, v, 1000))
            texts.append(np.concatenate([a, a[: m // 2], a]))
            want, count = unit_host([a], [k], texts, v)
            got, c = host([a], [k], texts, v, tok_class, costs)
            assert c == count and np.array_equal(got, want), (m, k)
    wild = np.array([-1, v, 2**31 - 1, -2**31, 0, 1, 1], dtype=np.int32)
    patterns = [wild[rng.integers(0, 7, m)] for m in (4, 33, 64)]
    texts = [wild[rng.integers(0, 7, n)] for n in (0, 70, 300)]
    want, count = unit_host(patterns, [2, 20, 50], texts, v)
    got, c = host(patterns, [2, 20, 50], texts, v, tok_class, costs)
    assert c == count > 0 and np.array_equal(got, want)


def test_the_bound_is_clamped_below_the_cost_of_the_whole_pattern():
    """a bound at or above D[m][0] would match the empty substring at every end: it is taken as D[m][0] - 1"""
    rng = np.random.default_rng(8)
    v = V = 4
    costs = random_costs(rng, V, top=3)
    cls = np.arange(v, dtype=np.int32)
    P = Plain(costs, cls, v)
    for m in (1, 2, 5):
        a = rng.integers(0, v, m).astype(np.int32)
        full = P.first_column(a.tolist())[-1]
        texts = [rng.integers(0, v, 80).astype(np.int32), np.zeros(0, dtype=np.int32)]
        at, _ = host([a], [full - 1], texts, v, cls, costs)
        for k in (full, full + 1, 150):
            got, count = host([a], [k], texts, v, cls, costs)
            assert count == len(got) and np.array_equal(got, at)
            assert (got[:, 2] < got[:, 3]).all() and (got[:, 4] < full).all()
        assert np.array_equal(at, P.hits([a], [full + 5], texts)) and len(at) > 0


def test_symbols_wrappers_and_constants():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "msocr.h")).read()
    for name in ("msocr_text_search_weighted_ws_bytes", "msocr_text_search_weighted", "msocr_text_search_weighted_host"):
        assert name in nat.exported_symbols() and hasattr(_lib(), name) and f" {name}(" in header
    for name, value in (("MSOCR_SEARCH_W_MAX_ALPHABET", ops.SEARCH_W_MAX_ALPHABET), ("MSOCR_SEARCH_W_MAX_WINDOW", ops.SEARCH_W_MAX_WINDOW)):
        assert f"#define {name} {value}\n" in header
    assert ops.SEARCH_W_MAX_ALPHABET == MAX_V and ops.SEARCH_W_MAX_WINDOW == MAX_W
    for name in ("text_search_weighted_into", "text_search_weighted", "text_search_weighted_host", "text_search_weighted_workspace_bytes"):
        assert callable(getattr(ops, name))


def test_abi_refusals():
    """Everything here is refused before any launch: no GPU is touched."""
    import ctypes

    from manuscript_ocr_amd import _native as nat
    L = _lib()
    i32 = lambda *x: np.array(x, dtype=np.int32)  # noqa: E731
    tok = np.zeros(4096, dtype=np.int32)
    cls = np.zeros(MAX_V, dtype=np.int32)
    hits = np.full((8, 5), -7, dtype=np.int32)
    cnt = np.full(1, -7, dtype=np.int64)
    wsbuf = np.zeros(1 << 12, dtype=np.int64)
    tab = np.ones(16, dtype=np.uint8)

    def struct(**kw):
        ec = nat.EditCostsTable()
        ec.sub = ec.del_ = ec.ins = tab.ctypes.data
        ec.V, ec.unknown, ec.min_ins, ec.min_del = 4, 6, 1, 3
        for name, value in kw.items():
            setattr(ec, name, value)
        return ec

    good = dict(pat_off=i32(0, 3, 67), k=i32(2, 3 * (MAX_W - 64) + 2), txt_off=i32(5, 5, 300), v=60, ec=struct())

    def ws(pat_off, k, txt_off, v, ec, Q=None, T=None):
        return L.msocr_text_search_weighted_ws_bytes(pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt_off.ctypes.data,
                                                     len(txt_off) - 1 if T is None else T, v, ctypes.pointer(ec) if ec is not None else None)

    def run_host(pat_off, k, txt_off, v, ec, Q=None, T=None, cap=8, pat=tok.ctypes.data, txt=tok.ctypes.data, klass=cls.ctypes.data,
                 out=hits.ctypes.data, count=cnt.ctypes.data):
        return L.msocr_text_search_weighted_host(pat, pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt, txt_off.ctypes.data,
                                                 len(txt_off) - 1 if T is None else T, v, klass, ctypes.pointer(ec) if ec is not None else None,
                                                 out, cap, count)

    def run_dev(pat_off, k, txt_off, v, ec, Q=None, T=None, cap=8, ws_ptr=wsbuf.ctypes.data, ws_bytes=wsbuf.nbytes, pat=tok.ctypes.data,
                txt=tok.ctypes.data, klass=cls.ctypes.data, out=hits.ctypes.data, count=cnt.ctypes.data):
        # host arrays stand in for device memory: a refused call reads nothing
        return L.msocr_text_search_weighted(pat, pat_off.ctypes.data, k.ctypes.data, len(k) if Q is None else Q, txt, txt_off.ctypes.data,
                                            len(txt_off) - 1 if T is None else T, v, klass, ctypes.pointer(ec) if ec is not None else None,
                                            out, cap, count, ws_ptr, ws_bytes, None)

    # the workspace formula of include/msocr.h; the second pattern's window is exactly the cap: 64 + (3 * 192 + 2) // 3 = 256
    need = ws(**good)
    assert need == (8 * 3 + 4 * 3 + 4 * 3 + 4 * 2 + 7) // 8 * 8
    assert run_host(**good) == 0 and cnt[0] >= 0
    bad = [
        dict(good, pat_off=i32(0, 3, 2)), dict(good, pat_off=i32(0, 3, 3)), dict(good, pat_off=i32(0, 3, 68)),
        dict(good, pat_off=i32(-1, 3, 67)),
        dict(good, txt_off=i32(5, 4, 300)), dict(good, txt_off=i32(-2, 5, 300)), dict(good, txt_off=i32(2**31 - 1, -2**31, 0)),
        dict(good, k=i32(-1, 5)), dict(good, k=i32(2, -2**31)),                         # k < 0
        dict(good, k=i32(2, 3 * (MAX_W - 64) + 3)),                                     # the window 257
        dict(good, k=i32(3 * (MAX_W - 3) + 3, 0)), dict(good, k=i32(2**31 - 1, 0)),
        dict(good, ec=struct(min_del=2)),                                               # a cheaper delete widens the same bound's window
        dict(good, ec=struct(unknown=2)),                                               # ... and so does a cheaper unknown
        dict(good, v=0), dict(good, v=-5), dict(good, v=MAX_V + 1),
        dict(good, ec=None), dict(good, ec=struct(sub=None)), dict(good, ec=struct(del_=None)), dict(good, ec=struct(ins=None)),
        dict(good, ec=struct(unknown=0)), dict(good, ec=struct(unknown=256)), dict(good, ec=struct(min_del=0)),
        dict(good, ec=struct(min_del=256)), dict(good, ec=struct(min_ins=0)), dict(good, ec=struct(min_ins=256)),
        dict(good, ec=struct(V=0)), dict(good, ec=struct(V=513)),
    ]
    for case in bad:
        assert ws(**case) == E_ARG, case
        assert run_host(**case) == E_ARG, case
        assert run_dev(**case) == E_ARG, case
    assert ws(**dict(good, k=i32(3, 500))) == need                                      # k >= m is a bound like any other
    assert ws(**dict(good, v=MAX_V)) == need and ws(**dict(good, ec=struct(V=512))) == need
    for kw in (dict(Q=-1), dict(T=-1)):
        assert ws(**good, **kw) == E_ARG and run_host(**good, **kw) == E_ARG and run_dev(**good, **kw) == E_ARG
    assert run_host(**good, cap=-1) == E_ARG and run_dev(**good, cap=-1) == E_ARG
    for null in ("pat", "txt", "klass", "out", "count"):
        assert run_host(**good, **{null: None}) == E_ARG and run_dev(**good, **{null: None}) == E_ARG, null
    ecp = ctypes.pointer(good["ec"])
    assert L.msocr_text_search_weighted_ws_bytes(None, good["k"].ctypes.data, 2, good["txt_off"].ctypes.data, 2, 60, ecp) == E_ARG
    assert L.msocr_text_search_weighted_ws_bytes(good["pat_off"].ctypes.data, None, 2, good["txt_off"].ctypes.data, 2, 60, ecp) == E_ARG
    assert L.msocr_text_search_weighted_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 2, 60, ecp) == E_ARG
    assert run_dev(**good, ws_bytes=need - 1) == E_ARG
    assert run_dev(**good, ws_ptr=wsbuf.ctypes.data + 4, ws_bytes=wsbuf.nbytes - 4) == E_ARG
    assert run_dev(**good, ws_ptr=None) == E_ARG
    # no pattern or no text: MSOCR_OK with count 0, no workspace, the offsets of the empty side are not read
    assert L.msocr_text_search_weighted_ws_bytes(None, None, 0, good["txt_off"].ctypes.data, 2, 60, ecp) == 0
    assert L.msocr_text_search_weighted_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 0, 60, ecp) == 0
    cnt[0] = -7
    assert L.msocr_text_search_weighted_host(tok.ctypes.data, None, None, 0, tok.ctypes.data, good["txt_off"].ctypes.data, 2, 60,
                                             cls.ctypes.data, ecp, hits.ctypes.data, 8, cnt.ctypes.data) == 0 and cnt[0] == 0
    assert L.msocr_text_search_weighted_ws_bytes(good["pat_off"].ctypes.data, good["k"].ctypes.data, 2, None, 0, 0, ecp) == E_ARG


# ------------------------------------------------------------------------------------------------ the Python layer
def test_text_corpus_search_with_costs():
    from manuscript_ocr_amd.recognizers import EditCosts, TextCorpus, TextHit, search_texts
    costs = ivanov_costs()
    assert costs.stoi == {"и": 0, "н": 1, "в": 2, "а": 3, "о": 4, "ъ": 5}
    texts = ["был нванов, и лванов тут", "", "ивановъ", "никого", "нвaнoв"]  # the last one with two Latin letters
    corpus = TextCorpus(texts)
    unit = corpus.search(["иванов"], max_distance=1)
    assert [(h.text, h.start, h.end, h.distance) for h in unit] == [(0, 5, 10, 1), (0, 15, 20, 1), (2, 0, 6, 0)]  # the shortest substring: ванов
    # weighted, bound 2: н for и is cheap, л for и is not (л lies outside the charset: unknown = 9); the added ъ costs 2 to drop
    hits = corpus.search(["иванов"], max_distance=2, costs=costs)
    assert hits == [TextHit(0, 0, 4, 10, 1), TextHit(0, 2, 0, 6, 0)]
    every = corpus.search(["иванов"], max_distance=2, costs=costs, overlapping=True)
    assert every == [TextHit(0, 0, 4, 10, 1), TextHit(0, 2, 0, 6, 0), TextHit(0, 2, 0, 7, 2)]
    assert search_texts(["иванов"], texts, max_distance=2, costs=costs) == hits
    assert corpus.search(["нванов"], max_distance=2, costs=costs) == [TextHit(0, 0, 4, 10, 0)]  # and not the other way round
    # the class map: cached per EditCosts, -1 outside the charset
    cls, dev = corpus.token_classes(costs)
    assert cls is dev and corpus.token_classes(costs)[0] is cls
    assert cls[corpus.stoi["н"]] == 1 and cls[corpus.stoi["л"]] == -1 and cls[corpus.stoi[" "]] == -1 and len(cls) == corpus.v
    # bounds: cost units, below what the whole pattern costs to supply (6 x 9 = 54); the rate is taken of that sum
    assert corpus.search(["иванов"], max_error_rate=0.04, costs=costs) == hits          # floor(0.04 * 54) = 2
    assert corpus.search(["иванов"], max_error_rate=0.01, costs=costs) == [TextHit(0, 2, 0, 6, 0)]
    assert len(corpus.search(["иванов"], max_distance=53, costs=costs)) >= 3
    assert corpus.search(["иванов"], max_error_rate=7.0, costs=costs) == corpus.search(["иванов"], max_distance=53, costs=costs)
    # a pattern character the corpus does not hold costs `unknown` and matches nothing: z z = 18 to supply, 9 to read a в as a z
    assert corpus.search(["zz"], max_distance=17, costs=costs, overlapping=True) == []
    assert [(h.start, h.end, h.distance) for h in corpus.search(["вz"], max_distance=9, costs=costs) if h.text == 2] == [(1, 2, 9), (5, 6, 9)]
    for bad in (dict(max_distance=54), dict(max_distance=-1), dict(max_distance=None), dict(max_distance=1, max_error_rate=0.5),
                dict(max_distance=[1, 1]), dict(max_error_rate=-0.5)):
        with pytest.raises(ValueError):
            corpus.search(["иванов"], costs=costs, **bad)
    with pytest.raises(ValueError, match="outside"):
        corpus.search(["zz"], max_distance=18, costs=costs)
    with pytest.raises(TypeError):
        corpus.search(["иванов"], max_distance=1, costs="unit")
    # the window: 64 characters and a bound of 193 at a cheapest delete of 1 span 257
    cheap = EditCosts.uniform(["x", "y"], 1)
    dear = EditCosts(np.array([[0, 4], [4, 0]]), np.array([1, 4]), np.array([4, 4]), ["x", "y"], unknown=4)
    long_corpus = TextCorpus(["y" + "x" * 300])
    assert len(long_corpus.search(["x" * 64], max_distance=63, costs=cheap, overlapping=True)) == 300
    assert len(long_corpus.search(["x" * 64], max_distance=192, costs=dear, overlapping=True)) == 300 - 15
    with pytest.raises(ValueError, match="span 257"):
        long_corpus.search(["x" * 64], max_distance=193, costs=dear)
    # more than 768 distinct characters: the unit search takes them, the weighted one does not
    wide = TextCorpus(["".join(chr(0x4E00 + k) for k in range(MAX_V + 1))])
    assert len(wide.search([chr(0x4E00)], max_distance=0)) == 1
    with pytest.raises(ValueError, match="distinct characters"):
        wide.search([chr(0x4E00)], max_distance=0, costs=cheap)
    assert TextCorpus(["".join(chr(0x4E00 + k) for k in range(MAX_V))]).search([chr(0x4E00 + MAX_V - 1)], max_distance=0, costs=cheap) == \
        [TextHit(0, 0, MAX_V - 1, MAX_V, 0)]
    # uniform costs 1: the unit search, whether the charset holds the characters or not
    for charset in (sorted(set("".join(texts))), ["q"]):
        one = EditCosts.uniform(charset, 1)
        for kw in (dict(max_distance=1), dict(max_distance=2, overlapping=True), dict(max_error_rate=0.34)):
            assert corpus.search(["иванов", "тут"], costs=one, **kw) == corpus.search(["иванов", "тут"], **kw)
    assert TextCorpus([]).search(["a"], max_distance=0, costs=cheap) == [] and corpus.search([], max_distance=0, costs=cheap) == []


def test_page_corpus_and_pipeline_search_with_costs():
    from manuscript_ocr_amd import PageCorpus, Pipeline
    from manuscript_ocr_amd.recognizers import EditCosts
    pages = hand_pages()  # "alpha beta gamma delta", "", "betta gamma"
    charset = sorted(set("alphabetagammadelta"))
    V = len(charset)
    sub = np.full((V, V), 8)
    np.fill_diagonal(sub, 0)
    delete, insert = np.full(V, 8), np.full(V, 8)
    delete[charset.index("t")] = 1  # a doubled t is cheap to drop
    costs = EditCosts(sub, delete, insert, charset, unknown=8)
    corpus = PageCorpus(pages)
    near = corpus.search(["beta gamma"], max_distance=1, costs=costs)
    assert [(h.page, h.distance, h.matched_text, h.words) for h in near] == [(0, 0, "beta gamma", [(0, 2), (1, 0)]),
                                                                            (2, 1, "betta gamma", [(1, 0), (1, 1)])]
    assert corpus.search(["betta"], max_distance=7, costs=costs) == corpus.search(["betta"], max_distance=0, costs=costs)  # supplying a t costs 8
    assert [h.matched_text for h in corpus.search(["betta"], max_distance=8, costs=costs)] == ["beta", "betta"]
    # the space between words lies outside the charset: a query that spans words still matches it at 0
    assert [(h.page, h.distance) for h in corpus.search([" beta\tgamma "], max_distance=0, costs=costs)] == [(0, 0)]
    pipe = Pipeline.__new__(Pipeline)
    assert pipe.search(pages, ["beta gamma"], max_distance=1, costs=costs) == near
    assert pipe.search(pages, ["beta gamma"], max_error_rate=0.02, costs=costs) == near  # floor(0.02 * 80) = 1
    assert pipe.search([], ["x"], max_distance=0, costs=costs) == []
    one = EditCosts.uniform(charset, 1)
    for q in (["beta gamma"], ["a", "ta ga"]):
        assert pipe.search(pages, q, max_distance=1 if len(q[0]) > 1 else 0, costs=one) == pipe.search(pages, q, max_distance=1 if len(q[0]) > 1 else 0)
    with pytest.raises(ValueError):
        pipe.search(pages, ["beta"], max_distance=32, costs=costs)


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/text_search_weighted.h (cost functions, host twin, start walk, profile entries, packed-key column step, argument check) in
    a plain C++ program of its own (tests/native/text_search_weighted_fuzz.cpp) with the address and undefined-behaviour sanitizers:
    garbage tokens, classes, offsets and tables, every array in a heap block of its exact size, every result compared with a plain
    table.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "text_search_weighted_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "text_search_weighted_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 400 checked 400")
