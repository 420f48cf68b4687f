"""Nearest lexicon words by confusion-weighted edit distance, host side: csrc/edit_distance_weighted.h through
the host twin msocr_lexicon_nearest_weighted_host, the validator msocr_edit_costs_check_host, the C ABI's rejections,
recognizers.EditCosts and Lexicon.nearest_texts(costs=...), and the header once more in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/native/edit_distance_weighted_fuzz.cpp).  No GPU.

The yardstick is the textbook weighted dynamic programme written here (dp_weighted_lexicon, vectorised over the lexicon with NumPy),
which shares nothing with the header.  All results are integers and compared exactly.  tests/test_gpu_lexicon_nearest_weighted.py
imports the helpers and the hard cases of this file."""
import ctypes
import math
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from test_lexicon_nearest_cpu import csr, host_wordlist, nearest_host, nearest_ref, random_lexicon, rows_near, text_of

E_ARG = -1
ROW_LENS = [0, 1, 2, 7, 63, 64]
WORD_LENS = [1, 2, 7, 62, 63]


def _lib():
    from manuscript_ocr_amd import _native as nat
    return nat.lib()


# ------------------------------------------------------------------------------------------------ the reference
def dp_weighted_lexicon(q, toks, lens, sub, dele, ins, V, unknown):
    """What turning the row q into each word costs: toks [L, W] (anything behind a word's length), lens [L] -> distances [L].
    D[i][j] over i symbols of q and j tokens of the word; a symbol outside [0, V) on either side costs `unknown` whatever the edit."""
    L, W = toks.shape
    toks = np.asarray(toks, dtype=np.int64)
    tok_ok = (toks >= 0) & (toks < V)
    safe = np.where(tok_ok, toks, 0)
    ins_c = np.where(tok_ok, np.asarray(ins, dtype=np.int64)[safe], unknown)                       # [L, W]
    P = np.concatenate([np.zeros((L, 1), dtype=np.int64), np.cumsum(ins_c, axis=1)], axis=1)       # D[0][j]
    prev = P.copy()
    for x in q:
        x = int(x)
        x_ok = 0 <= x < V
        del_c = int(dele[x]) if x_ok else unknown
        sub_c = np.where(tok_ok, np.asarray(sub, dtype=np.int64)[x if x_ok else 0][safe], unknown) if x_ok else np.full((L, W), unknown)
        base = np.concatenate([prev[:, :1] + del_c, np.minimum(prev[:, :-1] + sub_c, prev[:, 1:] + del_c)], axis=1)
        prev = np.minimum.accumulate(base - P, axis=1) + P   # cur[j] = min over j' <= j of base[j'] + the inserts of tokens j' .. j - 1
    return prev[np.arange(L), lens]


def dp_weighted_pair(a, b, sub, dele, ins, V, unknown):
    """The same for one pair, cell by cell (the check of the vectorised form)."""
    c_s = lambda x, y: int(sub[x][y]) if 0 <= x < V and 0 <= y < V else unknown
    c_d = lambda x: int(dele[x]) if 0 <= x < V else unknown
    c_i = lambda y: int(ins[y]) if 0 <= y < V else unknown
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        D[i][0] = D[i - 1][0] + c_d(a[i - 1])
    for j in range(1, len(b) + 1):
        D[0][j] = D[0][j - 1] + c_i(b[j - 1])
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j - 1] + c_s(a[i - 1], b[j - 1]), D[i - 1][j] + c_d(a[i - 1]), D[i][j - 1] + c_i(b[j - 1]))
    return D[len(a)][len(b)]


# ------------------------------------------------------------------------------------------------ fixtures and calls
class Costs:
    """Host cost tables with their msocr_edit_costs struct."""

    def __init__(self, sub, dele, ins, unknown, min_ins=None, min_del=None):
        from manuscript_ocr_amd import _native as nat
        self.sub = np.ascontiguousarray(sub, dtype=np.uint8)
        self.dele, self.ins = np.ascontiguousarray(dele, dtype=np.uint8), np.ascontiguousarray(ins, dtype=np.uint8)
        self.V, self.unknown = len(self.ins), int(unknown)
        self.min_ins = int(self.ins.min()) if min_ins is None else min_ins
        self.min_del = int(self.dele.min()) if min_del is None else min_del
        self.struct = self.fill(nat.EditCostsTable(), self.sub.ctypes.data, self.dele.ctypes.data, self.ins.ctypes.data)

    def fill(self, ec, sub_p, del_p, ins_p):
        ec.sub, ec.del_, ec.ins = sub_p, del_p, ins_p
        ec.V, ec.unknown, ec.min_ins, ec.min_del = self.V, self.unknown, self.min_ins, self.min_del
        return ec

    def check(self):
        return _lib().msocr_edit_costs_check_host(self.sub.ctypes.data, self.dele.ctypes.data, self.ins.ctypes.data, self.V, self.unknown,
                                                  self.min_ins, self.min_del)

    def dp(self, q, toks, lens):
        return dp_weighted_lexicon(q, toks, lens, self.sub, self.dele, self.ins, self.V, self.unknown)


def random_costs(rng, V, lo=1, hi=255, unknown=None):
    """Asymmetric tables: every entry drawn on its own; a zero diagonal."""
    sub = rng.integers(lo, hi + 1, (V, V))
    np.fill_diagonal(sub, 0)
    c = Costs(sub, rng.integers(lo, hi + 1, V), rng.integers(lo, hi + 1, V), int(rng.integers(lo, hi + 1)) if unknown is None else unknown)
    assert c.check() == 0 and (c.sub != c.sub.T).any()
    return c


def flat_costs(V, cost, unknown=None):
    sub = np.full((V, V), cost)
    np.fill_diagonal(sub, 0)
    return Costs(sub, np.full(V, cost), np.full(V, cost), cost if unknown is None else unknown)


def weighted_host(ids, trun, V, eos, pad, blank, begin, tok, costs, k, max_distance, by_length=None):
    ids, trun = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(trun, dtype=np.int32)
    B, steps = ids.shape
    idx, d = np.full((B, k), -7, dtype=np.int32), np.full((B, k), -7, dtype=np.int32)
    wl = host_wordlist(begin, tok, by_length)
    rc = _lib().msocr_lexicon_nearest_weighted_host(ids.ctypes.data, trun.ctypes.data, B, steps, V, eos, pad, blank, ctypes.byref(wl),
                                                    ctypes.byref(costs.struct), k, max_distance, idx.ctypes.data, d.ctypes.data)
    assert rc == 0, rc
    return idx, d


def weighted_ref_rows(ids, trun, eos, pad, blank, toks, lens, costs, k, max_distance):
    out = [nearest_ref(costs.dp(text_of(r, t, eos, pad, blank), toks, lens), k, max_distance) for r, t in zip(ids, trun)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def length_grid(rng, V, eos, pad, content):
    """A lexicon with words of every length of WORD_LENS and rows of every length of ROW_LENS, half of them near copies of a word; a
    few rows carry symbols outside [0, V), an EOS inside the row, or a t_run shorter than the row.  -> toks [L, 63], lens, ids [B, 64],
    trun.  Rows are bounded by t_run (a 64-symbol row has no room for an EOS); behind it they hold other content."""
    content = np.asarray(content)
    lens = np.array([n for n in WORD_LENS for _ in range(5)])
    toks = content[rng.integers(0, len(content), (len(lens), 63))]
    rows, trun = [], []
    for m in ROW_LENS:
        for n in WORD_LENS:
            for near in (False, True):
                a = content[rng.integers(0, len(content), 64)]
                if near and m:
                    w = int(np.flatnonzero(lens == n)[rng.integers(5)])
                    a[:m] = np.resize(toks[w, :n], m)
                    for _ in range(int(rng.integers(0, 4))):
                        a[rng.integers(m)] = content[rng.integers(len(content))]
                rows.append(a), trun.append(m)
    ids = np.stack(rows).astype(np.int64)
    trun = np.array(trun, dtype=np.int32)
    seven = np.flatnonzero(trun == 7)
    ids[seven[0], [1, 4]] = -1, V                     # symbols outside [0, V): each costs `unknown`
    ids[seven[1], 2] = 2**31 - 1
    ids[seven[2], 3] = eos                            # an EOS inside t_run ends the text at 3 symbols
    ids[seven[3], 5] = pad                            # a PAD inside is dropped
    long = np.flatnonzero(trun == 63)
    trun[long[0]], trun[long[1]] = 40, -2             # t_run shorter than the row's content, and a negative one
    ids[long[2], 10] = -1
    return toks, lens, ids.astype(np.int32), trun


def hard_cases():
    """The cases of tests 4 and 5 as (name, V, eos, pad, ids, trun, begin, tok, costs, k, max_distance, want_index, want_dist); the GPU
    test runs them on the device.  Tokens: PAD 0, SOS 1, EOS 2, a 3, b 4, x 5, then filler symbols."""
    V, eos, pad, a, b, x = 12, 2, 0, 3, 4, 5
    out = []
    # many cheap insertions win: "aa" -> "aaxxxxxx" costs 6 inserts of x at 1 each, "bb" two substitutions at 255 each
    words = [[b, b], [a, a] + [x] * 6, [b, b, b], [b] * 8, [6, 7]]
    begin, tok = csr([np.array(w + [0] * 8)[:8] for w in words], [len(w) for w in words])
    sub = np.full((V, V), 255)
    np.fill_diagonal(sub, 0)
    ins = np.full(V, 255)
    ins[x] = 1
    cheap_ins = Costs(sub, np.full(V, 255), ins, 255)
    assert cheap_ins.check() == 0 and cheap_ins.min_del == 255 and cheap_ins.min_ins == 1
    ids = np.full((1, 10), eos, dtype=np.int32)
    ids[0, :2] = a
    for k, bound, want_i, want_d in ((1, -1, [1], [6]), (1, 6, [1], [6]), (3, 6, [1, -1, -1], [6, -1, -1]), (1, 5, [-1], [-1]),
                                     (2, -1, [1, 0], [6, 510])):
        out.append((f"cheap inserts k={k} bound={bound}", V, eos, pad, ids, np.array([10], np.int32), begin, tok, cheap_ins, k, bound,
                    [want_i], [want_d]))
    # the mirror: many cheap deletions win: "aaxxxxxx" -> "aa" costs 6 deletes of x at 1 each
    words = [[b] * 8, [a, a], [b] * 7, [b, b], [6, 7, 8, 9, 10, 11, 6, 7]]
    begin, tok = csr([np.array(w + [0] * 8)[:8] for w in words], [len(w) for w in words])
    dele = np.full(V, 255)
    dele[x] = 1
    cheap_del = Costs(sub, dele, np.full(V, 255), 255)
    assert cheap_del.check() == 0 and cheap_del.min_ins == 255 and cheap_del.min_del == 1
    ids = np.full((1, 10), eos, dtype=np.int32)
    ids[0, :8] = [a, a] + [x] * 6
    for k, bound, want_i, want_d in ((1, -1, [1], [6]), (1, 6, [1], [6]), (1, 5, [-1], [-1]), (2, -1, [1, 3], [6, 2 * 255 + 6])):
        out.append((f"cheap deletes k={k} bound={bound}", V, eos, pad, ids, np.array([10], np.int32), begin, tok, cheap_del, k, bound,
                    [want_i], [want_d]))
    # 64 symbols against 63 tokens with nothing in common, every cost 255 -> 63 substitutions and a deletion, 64 * 255; so costs every
    # other word that shares nothing with the row, whatever its length: they tie and come back by index, not by length
    V2 = 194
    flat = flat_costs(V2, 255)
    words = [list(range(100, 163)), [7], list(range(70, 133)), list(range(101, 163))]
    begin, tok = csr([np.array(w + [0] * 63)[:63] for w in words], [len(w) for w in words])
    ids = np.full((1, 64), 50, dtype=np.int32)
    ids[0, ::2] = 51
    for k, want_i, want_d in ((1, [0], [16320]), (4, [0, 1, 2, 3], [16320, 16320, 16320, 16320])):
        out.append((f"largest k={k}", V2, eos, pad, ids, np.array([64], np.int32), begin, tok, flat, k, -1, [want_i], [want_d]))
    out += unknown_cases()
    return out


def unknown_cases():
    """`unknown` below every del and ins: a symbol outside [0, V) is then the cheapest thing to drop or to supply, and a length test
    on the minima of the two vectors alone would be no lower bound.  Same tuple as hard_cases."""
    V, eos, pad, a, b = 12, 2, 0, 3, 4
    costs = flat_costs(V, 255, unknown=1)
    assert costs.check() == 0 and costs.min_del == costs.min_ins == 255
    out = []
    # the row is "ab" and six characters outside the charset, dropped at 1 each
    words = [[a, b], [b, a], [5, 6, 7, 8, 9, 10, 11, 5]]
    begin, tok = csr([np.array(w + [0] * 8)[:8] for w in words], [len(w) for w in words])
    ids = np.full((1, 10), eos, dtype=np.int32)
    ids[0, :8] = [a, -1, b, V, -1, 2**31 - 1, -1, -1]
    for k, bound, want_i, want_d in ((1, 6, [0], [6]), (1, -1, [0], [6]), (3, -1, [0, 1, 2], [6, 261, 516]), (2, 5, [-1, -1], [-1, -1]),
                                     (3, 300, [0, 1, -1], [6, 261, -1])):   # "ba": b and a read from two of the six, a dropped
        out.append((f"unknown rows k={k} bound={bound}", V, eos, pad, ids, np.array([10], np.int32), begin, tok, costs, k, bound,
                    [want_i], [want_d]))
    # the mirror: the row is "ab", the word holds six tokens outside [0, V) (a list no Lexicon builds), supplied at 1 each
    words = [[b, a], [a, -1, b, V, -1, 2**31 - 1, -1, -1], [5, 6]]
    begin, tok = csr([np.array(w + [0] * 8, dtype=np.int64)[:8] for w in words], [len(w) for w in words])
    ids = np.full((1, 10), eos, dtype=np.int32)
    ids[0, :2] = [a, b]
    for k, bound, want_i, want_d in ((1, 6, [1], [6]), (2, -1, [1, 0], [6, 510]), (1, 5, [-1], [-1])):
        out.append((f"unknown words k={k} bound={bound}", V, eos, pad, ids, np.array([10], np.int32), begin, tok, costs, k, bound,
                    [want_i], [want_d]))
    return out


# ------------------------------------------------------------------------------------------------ tests
def test_the_vectorised_reference_equals_the_cell_by_cell_one():
    rng = np.random.default_rng(1)
    V = 9
    costs = random_costs(rng, V)
    toks = rng.integers(-1, V + 1, (40, 12))
    lens = rng.integers(1, 13, 40)
    for m in (0, 1, 5, 12):
        q = rng.integers(-1, V + 1, m)
        got = costs.dp(q, toks, lens)
        want = [dp_weighted_pair(list(q), list(t[:n]), costs.sub, costs.dele, costs.ins, V, costs.unknown) for t, n in zip(toks, lens)]
        assert got.tolist() == want, m


@pytest.mark.parametrize("V", [20, 194, 512])
def test_host_twin_equals_the_weighted_dp(V):
    eos, pad = 2, 0
    rng = np.random.default_rng(40 + V)
    content = list(range(3, 14)) + [V - 1]  # a small share of the charset (ties are common), token V - 1 included
    costs = random_costs(rng, V, hi=9)       # small costs: equal distances between different words occur
    toks, lens, ids, trun = length_grid(rng, V, eos, pad, content)
    begin, tok = csr(toks, lens)
    assert _lib().msocr_wordlist_check_host(begin.ctypes.data, tok.ctypes.data, len(lens), len(tok), V, 63) == 0
    for blank in (-1, content[2]):
        dists = np.stack([costs.dp(text_of(r, t, eos, pad, blank), toks, lens) for r, t in zip(ids, trun)])
        for k in (1, 3, 16):
            for bound in (-1, 0, 20):
                idx, d = weighted_host(ids, trun, V, eos, pad, blank, begin, tok, costs, k, bound)
                want = [nearest_ref(row, k, bound) for row in dists]
                wi, wd = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
                bad = np.argwhere((idx != wi) | (d != wd))
                assert not len(bad), (V, blank, k, bound, bad[:3].tolist(), idx[bad[0][0]].tolist(), wi[bad[0][0]].tolist(),
                                      d[bad[0][0]].tolist(), wd[bad[0][0]].tolist())
        if blank < 0:
            assert any(len(set(row.tolist())) < len(row) for row in dists)      # ties occur
            assert (dists.min(axis=1) == 0).any() and dists.max() > 63 * 2    # lexicon words among the rows, and far ones
    # full-range costs once: the distances of the long rows reach thousands
    wide = random_costs(rng, V)
    idx, d = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, wide, 16, -1)
    wi, wd = weighted_ref_rows(ids, trun, eos, pad, -1, toks, lens, wide, 16, -1)
    assert (idx == wi).all() and (d == wd).all() and d.max() > 3000
    # the list stored by length with its permutation: the same answer in the original index
    from test_lexicon_nearest_cpu import sorted_list
    b2, t2, order = sorted_list(begin, tok)
    i2, d2 = weighted_host(ids, trun, V, eos, pad, -1, b2, t2, wide, 16, -1, by_length=order)
    assert (i2 == idx).all() and (d2 == d).all()


@pytest.mark.parametrize("L", [1, 5, 1000])
def test_unit_costs_reproduce_the_unit_cost_lookup(L):
    from manuscript_ocr_amd.recognizers import EditCosts
    V, eos, pad = 194, 2, 0
    itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(0x400 + i) for i in range(V - 3)]
    ec = EditCosts.uniform(itos, cost=1)
    assert ec.unknown == 1 and ec.num_classes == V and ec.min_ins == ec.min_del == 1
    costs = Costs(ec.sub, ec.delete, ec.insert, ec.unknown)
    content = list(range(3, 60))
    rng = np.random.default_rng(100 + L)
    toks, lens = random_lexicon(rng, L, content)
    begin, tok = csr(toks, lens)
    ids, trun = rows_near(rng, toks, lens, content, 37, 25, eos)
    ids[1, :3], trun[1] = [-1, V, 2**31 - 1], 7
    for k in (1, 3, 16):
        for bound in (-1, 0, 2):
            idx, d = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, costs, k, bound)
            uidx, ud = nearest_host(ids, trun, V, eos, pad, -1, begin, tok, k, bound)
            assert (idx == uidx).all() and (d == ud).all(), (L, k, bound)


def test_direction():
    V, eos, pad, a, b, c = 8, 2, 0, 3, 4, 5
    sub = np.full((V, V), 250)
    np.fill_diagonal(sub, 0)
    sub[a, b], sub[b, a] = 1, 200
    dele, ins = np.full(V, 120), np.full(V, 120)   # a deletion and an insertion together cost more than any substitution above
    dele[c], ins[c] = 7, 9        # dropping a recognised "c" costs 7, supplying a missing "c" costs 9
    costs = Costs(sub, dele, ins, 250)
    assert costs.check() == 0
    one = lambda row, word: int(weighted_host(np.array([row + [eos] * (4 - len(row))]), [4], V, eos, pad, -1, *csr([np.array(word + [0] * 4)], [len(word)]),
                                              costs, 1, -1)[1][0, 0])
    assert one([a], [b]) == 1 and one([b], [a]) == 200         # sub[recognised][lexicon]
    assert one([b, c], [b]) == 7 and one([c, b], [b]) == 7      # the row is one symbol longer: it pays del of that symbol
    assert one([b], [b, c]) == 9 and one([b], [c, b]) == 9      # the row is one shorter: it pays ins of the missing one
    assert one([], [c]) == 9 and one([], [c, b]) == 129 and one([a], [b, b]) == 121 and one([c, c, c], [c]) == 14


def test_length_bound_and_largest_distance():
    for name, V, eos, pad, ids, trun, begin, tok, costs, k, bound, want_i, want_d in hard_cases():
        idx, d = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, costs, k, bound)
        assert idx.tolist() == want_i and d.tolist() == want_d, name
        # and the expectation itself against the dynamic programme
        lens = np.diff(begin)
        toks = np.zeros((len(lens), 63), dtype=np.int64)
        for i, (s, n) in enumerate(zip(begin[:-1], lens)):
            toks[i, :n] = tok[s:s + n]
        wi, wd = weighted_ref_rows(ids, trun, eos, pad, -1, toks, lens, costs, k, bound)
        assert wi.tolist() == want_i and wd.tolist() == want_d, name


def test_ties_and_bounds():
    V, eos, pad = 30, 2, 0
    rng = np.random.default_rng(8)
    content = list(range(3, 9))
    sub = np.full((V, V), 10)
    np.fill_diagonal(sub, 0)
    sub[3, 4], sub[4, 3], sub[5, 6] = 4, 6, 4
    costs = Costs(sub, np.full(V, 5), np.full(V, 5), 10)   # two deletes, two inserts and one substitution cost the same
    assert costs.check() == 0
    toks, lens = random_lexicon(rng, 400, content, max_len=5)
    begin, tok = csr(toks, lens)
    ids, trun = rows_near(rng, toks, lens, content, 24, 8, eos, max_len=5)
    dists = np.stack([costs.dp(text_of(r, t, eos, pad, -1), toks, lens) for r, t in zip(ids, trun)])
    in_lexicon = dists.min(axis=1) == 0
    assert in_lexicon.any() and not in_lexicon.all()
    for k in (1, 3, 16):
        for bound in (-1, 0, 4, 5, 10, 11):
            idx, d = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, costs, k, bound)
            want = [nearest_ref(row, k, bound) for row in dists]
            assert (idx == np.stack([w[0] for w in want])).all() and (d == np.stack([w[1] for w in want])).all(), (k, bound)
            if bound >= 0:
                assert d.max() <= bound
    idx, d = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, costs, 16, -1)
    same = (d[:, 1:] == d[:, :-1])
    assert same.any() and (idx[:, 1:][same] > idx[:, :-1][same]).all()         # equal distances: ascending index
    idx0, d0 = weighted_host(ids, trun, V, eos, pad, -1, begin, tok, costs, 1, 0)   # max_distance 0: exactly the rows in the lexicon
    assert ((idx0[:, 0] >= 0) == in_lexicon).all() and (d0[in_lexicon] == 0).all() and (d0[~in_lexicon] == -1).all()


def test_the_validator_refuses_every_single_violation():
    V = 6
    rng = np.random.default_rng(2)
    good = random_costs(rng, V)

    def chk(sub=good.sub, dele=good.dele, ins=good.ins, v=V, unknown=good.unknown, min_ins=good.min_ins, min_del=good.min_del):
        ptr = lambda a: None if a is None else a.ctypes.data
        return _lib().msocr_edit_costs_check_host(ptr(sub), ptr(dele), ptr(ins), v, unknown, min_ins, min_del)
    assert chk() == 0
    for i in range(V):                       # a non-zero diagonal entry
        s = good.sub.copy()
        s[i, i] = 1
        assert chk(sub=s) == E_ARG, i
    for i in range(V):                       # a zero off-diagonal, ins or del entry
        for j in range(V):
            if i != j:
                s = good.sub.copy()
                s[i, j] = 0
                assert chk(sub=s) == E_ARG, (i, j)
        for name in ("dele", "ins"):
            v = getattr(good, name).copy()
            v[i] = 0
            assert chk(**{name: v}) == E_ARG, (name, i)
    for delta in (-1, 1):                    # wrong minima
        assert chk(min_ins=good.min_ins + delta) == E_ARG and chk(min_del=good.min_del + delta) == E_ARG
    for bad in (0, -1, 256, 2**31 - 1):      # unknown outside 1..255
        assert chk(unknown=bad) == E_ARG, bad
    assert chk(unknown=1) == 0 and chk(unknown=255) == 0
    for bad in (0, -1, 513):                 # V outside 1..512 (the arrays are never read)
        assert chk(v=bad) == E_ARG, bad
    assert chk(sub=None) == E_ARG and chk(dele=None) == E_ARG and chk(ins=None) == E_ARG
    big = flat_costs(512, 3)
    assert big.check() == 0
    one = Costs(np.zeros((1, 1)), [4], [5], 9)
    assert one.check() == 0


def test_c_abi_rejections():
    from manuscript_ocr_amd import _native as nat
    lib = _lib()
    V, eos, pad = 20, 2, 0
    begin, tok = csr(np.arange(20).reshape(4, 5) % V, [3, 1, 5, 2])
    ids, trun = np.full((2, 8), eos, dtype=np.int32), np.full(2, 8, dtype=np.int32)
    idx, d = np.zeros((2, 16), dtype=np.int32), np.zeros((2, 16), dtype=np.int32)
    wl = host_wordlist(begin, tok)
    costs = random_costs(np.random.default_rng(4), V)

    def call(ids_p=ids.ctypes.data, trun_p=trun.ctypes.data, B=2, steps=8, V=V, eos=eos, pad=pad, blank=-1, wl=wl, ec=costs.struct, k=3,
             bound=-1, idx_p=idx.ctypes.data, d_p=d.ctypes.data):
        return lib.msocr_lexicon_nearest_weighted_host(ids_p, trun_p, B, steps, V, eos, pad, blank, None if wl is None else ctypes.byref(wl),
                                                       None if ec is None else ctypes.byref(ec), k, bound, idx_p, d_p)
    assert call() == 0 and call(B=0) == 0 and call(k=16) == 0 and call(k=1) == 0 and call(blank=V - 1) == 0 and call(bound=0) == 0
    for kw in (dict(ids_p=None), dict(trun_p=None), dict(idx_p=None), dict(d_p=None), dict(wl=None), dict(B=-1), dict(steps=0),
               dict(steps=65), dict(V=0), dict(V=513), dict(k=0), dict(k=17), dict(bound=-2), dict(eos=-1), dict(eos=V), dict(pad=-1),
               dict(pad=V), dict(blank=-2), dict(blank=V), dict(ec=None), dict(V=V - 1)):
        assert call(**kw) == E_ARG, kw
    for field, val in (("word_begin", None), ("word_tok", None), ("n_words", 0), ("n_words", -1)):
        w2 = host_wordlist(begin, tok)
        setattr(w2, field, val)
        assert call(wl=w2) == E_ARG, field
    for field, val in (("sub", None), ("del_", None), ("ins", None), ("V", V + 1), ("unknown", 0), ("unknown", 256), ("min_ins", 0),
                       ("min_ins", 256), ("min_del", 0), ("min_del", 256)):
        e2 = costs.fill(nat.EditCostsTable(), costs.sub.ctypes.data, costs.dele.ctypes.data, costs.ins.ctypes.data)
        setattr(e2, field, val)
        assert call(ec=e2) == E_ARG, field
    # the device entry point refuses the same before any launch (no GPU is touched: nothing is launched)
    dev = lambda ids_p=ids.ctypes.data, B=2, k=3, ec=costs.struct: lib.msocr_lexicon_nearest_weighted(
        ids_p, trun.ctypes.data, B, 8, V, eos, pad, -1, ctypes.byref(wl), None if ec is None else ctypes.byref(ec), k, -1, idx.ctypes.data,
        d.ctypes.data, None, None)
    assert dev(ids_p=None) == E_ARG and dev(k=17) == E_ARG and dev(ec=None) == E_ARG and dev(B=0) == 0
    for args in ((0, 10, 3), (4, 0, 3), (4, 10, 0), (4, 10, 17), (-1, 10, 3), (1, 100000, 3), (37, 20011, 16), (7680, 20011, 3)):
        assert lib.msocr_lexicon_nearest_weighted_ws_bytes(*args) == lib.msocr_lexicon_nearest_ws_bytes(*args), args


ITOS4 = ["<PAD>", "<SOS>", "<EOS>", "a", "b", "c", "d"]


def _cost(p, unit=32, floor=1e-4):
    return unit if p <= 0 else min(max(int(round(unit * math.log(p) / math.log(floor))), 1), unit)


def test_edit_costs_from_confusions_by_hand():
    from manuscript_ocr_amd.recognizers import EditCosts, error_breakdown
    conf = Counter({("a", "b"): 30, ("c", None): 5, (None, "d"): 2,
                    ("a", "ж"): 7, ("ж", "a"): 7, (None, "ж"): 3, ("ж", None): 3, ("<EOS>", "a"): 4, ("b", "<PAD>"): 4})
    ref_counts = {"a": 100, "b": 50, "c": 40, "d": 10, "ж": 1000, "<EOS>": 1000}
    ec = EditCosts.from_confusions(conf, ref_counts, ITOS4)
    V = 7
    sub = np.full((V, V), 32)
    np.fill_diagonal(sub, 0)
    dele, ins = np.full(V, 32), np.full(V, 32)
    sub[4, 3] = _cost(30 / 100)     # true a read as b: the lookup meets b and must reach a -> sub[b][a]
    ins[5] = _cost(5 / 40)          # c was dropped: the lookup supplies it
    dele[6] = _cost(2 / 200)        # d was added (relative to all 200 reference tokens of the charset): the lookup drops it
    assert (sub[4, 3], ins[5], dele[6]) == (4, 7, 16)
    assert ec.sub.dtype == np.uint8 and (ec.sub == sub).all() and (ec.delete == dele).all() and (ec.insert == ins).all()
    assert ec.unknown == 32 and ec.min_ins == 7 and ec.min_del == 16 and ec.sub[3, 4] == 32    # unobserved: unit; not symmetric
    # the clamps: an edit seen every time costs 1, one rarer than `floor` costs `unit`, another unit scales
    ec2 = EditCosts.from_confusions({("a", "b"): 100, ("c", "d"): 1}, {"a": 100, "c": 10**6}, ITOS4, unit=200, floor=1e-3)
    assert ec2.sub[4, 3] == 1 and ec2.sub[6, 5] == 200 and ec2.unknown == 200 and ec2.delete.tolist() == [200] * V
    assert EditCosts.from_confusions({("a", "b"): 10}, {"a": 100}, ITOS4, unit=200, floor=1e-3).sub[4, 3] == _cost(0.1, 200, 1e-3) == 67
    # from_pairs: error_breakdown on the pairs, the reference tokens counted
    refs, hyps = ["abcd", "aabd", "cab"], ["abbd", "abd", "cabd"]
    bd = error_breakdown(refs, hyps)["confusions"]
    assert bd and {type(k) for k in bd} == {tuple}
    want = EditCosts.from_confusions(bd, Counter("".join(refs)), ITOS4)
    got = EditCosts.from_pairs(refs, hyps, ITOS4)
    assert (got.sub == want.sub).all() and (got.delete == want.delete).all() and (got.insert == want.insert).all()
    assert (got.sub != np.where(np.eye(V, dtype=bool), 0, 32)).any() or (got.insert != 32).any() or (got.delete != 32).any()
    # refusals
    with pytest.raises(ValueError):
        EditCosts(np.ones((V, V)), dele, ins, ITOS4)            # a non-zero diagonal
    with pytest.raises(ValueError):
        EditCosts(sub, dele, ins[:-1], ITOS4)
    with pytest.raises(ValueError):
        EditCosts(sub, dele, ins, ITOS4, unknown=0)
    with pytest.raises(ValueError):
        EditCosts.from_confusions(conf, ref_counts, ITOS4, unit=256)
    st = ec.to(None)[3]
    assert (st.V, st.unknown, st.min_ins, st.min_del) == (7, 32, 7, 16) and ec.to(None) is ec.to(None)
    assert ctypes.addressof(ec.struct(None).contents) == ctypes.addressof(st)


def test_lexicon_nearest_texts_with_costs():
    from manuscript_ocr_amd.recognizers import EditCosts, Lexicon
    itos = ["<PAD>", "<SOS>", "<EOS>"] + list("ИЛРНваночи")
    # the recogniser reads И as Н four times in ten; it never confuses Л or Р with Н
    costs = EditCosts.from_confusions({("И", "Н"): 400, ("Н", "И"): 350, ("в", None): 3}, {"И": 1000, "Н": 1000, "в": 900}, itos)
    cheap = _cost(0.4)
    assert cheap == 3 and costs.sub[itos.index("Н"), itos.index("И")] == cheap
    words = ["Иванов", "Лванов", "Рванов"]
    lex = Lexicon(words, itos, 25)
    rows = ["Нванов", "Лванов"]
    idx, d = lex.nearest_texts(rows, k=3, costs=costs)
    assert idx.tolist() == [[0, 1, 2], [1, 0, 2]] and d.tolist() == [[cheap, 32, 32], [0, 32, 32]]
    uidx, ud = lex.nearest_texts(rows, k=3)
    assert uidx.tolist() == [[0, 1, 2], [1, 0, 2]] and ud.tolist() == [[1, 1, 1], [0, 1, 1]]   # the tie, in index order
    # the same lexicon in another order: the unit-cost tie follows the index, the weighted ranking follows the confusions
    rev = Lexicon(words[::-1], itos, 25)
    assert rev.nearest_texts(rows[:1], k=3)[0].tolist() == [[0, 1, 2]]
    assert [s["text"] for s in rev.suggestions(*rev.nearest_texts(rows[:1], k=3, costs=costs))[0]] == ["Иванов", "Рванов", "Лванов"]
    assert lex.suggestions(*lex.nearest_texts(rows[:1], k=3, max_distance=cheap, costs=costs)) == [
        [{"text": "Иванов", "lexicon_index": 0, "distance": cheap}]]
    # a character outside the charset costs `unknown` = unit; ids with a t_run go the same way
    assert lex.nearest_texts(["Xванов"], k=1, costs=costs)[1].tolist() == [[32]]
    ids, trun = lex.encode_rows(rows)
    i2, d2 = lex.nearest(ids, trun, k=3, costs=costs)
    assert (i2 == idx).all() and (d2 == d).all()
    # uniform costs of 1 are the unit-cost lookup
    u1 = EditCosts.uniform(itos)
    assert [a.tolist() for a in lex.nearest_texts(rows, k=3, costs=u1)] == [uidx.tolist(), ud.tolist()]
    assert lex.nearest_texts(rows, k=3, costs=EditCosts.uniform(itos, cost=5))[1].tolist() == [[5, 5, 5], [0, 5, 5]]
    with pytest.raises(ValueError, match="charset"):
        lex.nearest_texts(rows, costs=EditCosts.uniform(itos + ["я"]))
    with pytest.raises(TypeError):
        lex.nearest_texts(rows, costs=costs.sub)


def test_header_under_the_sanitizers(tmp_path):
    """csrc/edit_distance_weighted.h in a plain C++ program of its own (tests/native/edit_distance_weighted_fuzz.cpp) with the address
    and undefined-behaviour sanitizers: corrupted word lists, garbage rows and t_run values, arbitrary cost tables, every array in a
    heap block of its exact size; the column DP and the query-profile form against a full-table DP.  Run as a child process; nothing
    is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("the ROCm clang++ is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "edit_distance_weighted_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"),
                           os.path.join(root, "tests", "native", "edit_distance_weighted_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 1500 checked")
