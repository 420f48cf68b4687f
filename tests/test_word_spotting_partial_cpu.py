"""Partial word spotting (include/msocr.h, "word spotting", "Subsequence distance") without a GPU: the host
twin msocr_dtw_subsequence_host against yardsticks written here in plain NumPy f64 over the definition, cell by cell; every refusal
of the C ABI; WordIndex.spot(..., partial=True) on hand-built features; and csrc/word_spotting.h in a plain C++ program under the
address and undefined-behaviour sanitizers (tests/native/word_spotting_partial_fuzz.cpp).

The yardsticks: `yard_cost` (the local costs of one pair in f64), `yard_sub_table` (the table S and the start column every cell
carries, with the tie rules of the definition: diagonal, then upper, then left; optionally pinned to one start column), `yard_sub`
(d and the span: the smallest end that attains the minimum) and `yard_pinned` (the cost of the best path from (0, s) to
(Lq - 1, e), divided by Lq).  tests/test_gpu_word_spotting_partial.py imports them.

Tolerances.  From the SAME f32 unit frames the host twin is the f64 table rounded to f32 once: a path has at most Lq + Ln - 1 cells
of cost at most 2, so d <= 2 (Lq + Ln) / Lq and the rounding moves it by at most 2 (Lq + Ln) / Lq 2^-24 (`tol_same`; the f64
sums' own error, ~1e-13, is covered by an added 1e-12).  From the same RAW frames it additionally carries the f32 unit frames' error:
`bound_sub`, derived in tests/test_gpu_word_spotting_partial.py.

Spans on random data are held to the VALIDITY criterion, never to equality (near-ties may legitimately fall differently):
0 <= s <= e < Ln, and the best path pinned to that start and end costs, per query frame, at most d_yard + the tolerance."""
import os
import subprocess

import numpy as np
import pytest

from test_word_spotting_cpu import EPS, bound, full_gate, random_words, same_bits, yard_unit


# ------------------------------------------------------------------------------------------------ yardsticks
def yard_cost(u, Lu, v, Lv):
    return 1.0 - np.asarray(u[:Lu], dtype=np.float64) @ np.asarray(v[:Lv], dtype=np.float64).T


def yard_sub_table(C, pin=None):
    """the definition, cell by cell, in f64 -> (S, start); pin: only this column of row 0 may begin a path"""
    Lq, Ln = C.shape
    S = np.full((Lq, Ln), np.inf)
    st = np.full((Lq, Ln), -1, dtype=np.int64)
    for j in range(Ln):
        if pin is None or j == pin:
            S[0, j], st[0, j] = C[0, j], j          # a free start; row 0 takes no left step
    for i in range(1, Lq):
        for j in range(Ln):
            best, b = (S[i - 1, j - 1], st[i - 1, j - 1]) if j else (np.inf, -1)   # the diagonal predecessor wins ties,
            if S[i - 1, j] < best:
                best, b = S[i - 1, j], st[i - 1, j]                                # then the upper,
            if j and S[i, j - 1] < best:
                best, b = S[i, j - 1], st[i, j - 1]                                # then the left
            S[i, j], st[i, j] = C[i, j] + best, b
    return S, st


def yard_sub(C):
    """-> d, (start, end): the smallest end column that attains the minimum of the last row"""
    S, st = yard_sub_table(C)
    e = int(np.argmin(S[-1]))                       # the first of equal minima
    return S[-1, e] / C.shape[0], (int(st[-1, e]), e + 1)


def yard_pinned(C, s, e):
    S, _ = yard_sub_table(C, pin=s)
    return S[-1, e] / C.shape[0]


def bound_sub(H, Lq, Ln):
    """The bound of the subsequence distance against the f64 yardstick, from raw frames: the global distance's bound times
    (Lq + Ln) / Lq (tests/test_gpu_word_spotting_partial.py derives it)."""
    return bound(H, Lq, Ln) * (Lq + Ln) / Lq


def tol_same(Lq, Ln):
    return 2.0 * (Lq + Ln) / Lq * EPS + 1e-12


def check_pairs(d, span, uq, ql, lo, hi, uc, cl, tol, what, scale=1.0):
    """every pair of a result against the yardstick over the unit frames uq / uc (f64, or the f32 ones the twin saw): the gate, d
    within tol(Lq, Ln), the span by the validity criterion with scale * tol -> the largest error / tolerance seen"""
    worst = 0.0
    for q in range(len(ql)):
        for n in range(len(cl)):
            Lq, Ln = int(ql[q]), int(cl[n])
            if not (1 <= Lq and 1 <= Ln and lo[q] <= Ln <= hi[q]):
                assert d[q, n] == np.inf and span[q, n].tolist() == [-1, -1], (what, q, n)
                continue
            C = yard_cost(uq[q], Lq, uc[n], Ln)
            want, _ = yard_sub(C)
            t = tol(Lq, Ln)
            assert abs(d[q, n] - want) <= t, (what, q, n, float(d[q, n]), want, t)
            worst = max(worst, abs(d[q, n] - want) / t)
            s, e = (int(x) for x in span[q, n])
            assert 0 <= s < e <= Ln, (what, q, n, s, e, Ln)
            assert yard_pinned(C, s, e - 1) <= want + scale * t, (what, q, n, s, e)
    return worst


def yard_sub_all(uq, ql, uc, cl, pin=None):
    """`yard_sub_table` for all pairs at once: loops over the cells, NumPy across the pairs (held to the cell-by-cell form below).
    uq [Q, T, H], uc [N, T, H] unit frames with zeros behind the lengths (cells outside Lq x Ln are then computed too, and never
    looked at: a cell depends on cells of smaller indices only); pin [Q, N]: the one start column of every pair -> S, start
    [Q, N, rows, cols] over the rows and columns any pair needs"""
    uq, uc = np.asarray(uq, dtype=np.float64), np.asarray(uc, dtype=np.float64)
    Q, T, H = uq.shape
    N = uc.shape[0]
    rows, cols = int(np.max(ql)), int(np.max(cl))
    # cell-major, [i, j, Q, N]: every step below works on contiguous [Q, N] planes
    C = 1.0 - np.ascontiguousarray((uq.reshape(Q * T, H) @ uc.reshape(N * T, H).T).reshape(Q, T, N, T).transpose(1, 3, 0, 2))
    S = np.full((rows, cols, Q, N), np.inf)
    st = np.full((rows, cols, Q, N), -1, dtype=np.int64)
    for j in range(cols):
        ok = np.ones((Q, N), dtype=bool) if pin is None else np.asarray(pin) == j
        S[0, j] = np.where(ok, C[0, j], np.inf)
        st[0, j] = np.where(ok, j, -1)
    for i in range(1, rows):
        for j in range(cols):
            if j:
                best, b = S[i - 1, j - 1], st[i - 1, j - 1]
            else:
                best, b = np.full((Q, N), np.inf), np.full((Q, N), -1, dtype=np.int64)
            take = S[i - 1, j] < best
            best, b = np.where(take, S[i - 1, j], best), np.where(take, st[i - 1, j], b)
            if j:
                take = S[i, j - 1] < best
                best, b = np.where(take, S[i, j - 1], best), np.where(take, st[i, j - 1], b)
            S[i, j], st[i, j] = C[i, j] + best, b
    return S.transpose(2, 3, 0, 1), st.transpose(2, 3, 0, 1)


def yard_sub_results(S, st, ql, cl):
    """-> d [Q, N], span [Q, N, 2] of every pair from the tables of `yard_sub_all`"""
    ql, cl = np.asarray(ql, dtype=np.int64), np.asarray(cl, dtype=np.int64)
    Q, N = S.shape[:2]
    qi, ni = np.arange(Q)[:, None], np.arange(N)[None, :]
    last = np.where(np.arange(S.shape[3])[None, None, :] < cl[None, :, None], S[qi, ni, (ql - 1)[:, None]], np.inf)
    e = np.argmin(last, axis=2)                     # the first of equal minima
    d = last[qi, ni, e] / ql[:, None]
    return d, np.stack([st[qi, ni, (ql - 1)[:, None], e], e + 1], axis=2)


def check_all(d, span, fq, ql, lo, hi, fc, cl, what, scale=2.0, words=256):
    """A whole [Q, N] result (lengths inside [1, T]) against the f64 yardstick from the same raw frames: +inf and (-1, -1) exactly
    where the gate says so; elsewhere d within bound_sub and the span valid: inside its word, and the best path pinned to it within
    scale * bound_sub of the optimum.  The yardstick runs over the corpus in slices of `words` words, so that its tables stay
    small.  -> the largest error / bound"""
    ql, cl, lo, hi = (np.asarray(a, dtype=np.int64) for a in (ql, cl, lo, hi))
    H = fq.shape[2]
    uq = yard_unit(fq, ql)
    ok = (cl[None, :] >= lo[:, None]) & (cl[None, :] <= hi[:, None])
    assert np.array_equal(np.isposinf(d), ~ok) and not np.isnan(d).any(), what
    assert (span[~ok] == -1).all(), what
    s, e = span[..., 0].astype(np.int64), span[..., 1].astype(np.int64)
    assert ((0 <= s) & (s < e) & (e <= cl[None, :]))[ok].all(), what
    lim = bound_sub(H, ql[:, None], cl[None, :]).astype(np.float64)
    want, pinned = np.empty(d.shape), np.empty(d.shape)
    qi = np.arange(len(ql))[:, None]
    for at in range(0, len(cl), words):
        w = slice(at, at + words)
        uc = yard_unit(fc[w], cl[w])
        want[:, w], _ = yard_sub_results(*yard_sub_all(uq, ql, uc, cl[w]), ql, cl[w])
        S, _ = yard_sub_all(uq, ql, uc, cl[w], pin=np.where(ok[:, w], s[:, w], 0))
        pinned[:, w] = S[qi, np.arange(S.shape[1])[None, :], (ql - 1)[:, None], np.where(ok[:, w], e[:, w] - 1, 0)] / ql[:, None]
    err = np.where(ok, np.abs(np.where(ok, d, 0.0) - want), 0.0)
    worst = float((err / lim).max()) if ok.any() else 0.0
    print(f"{what}: worst error / bound {worst:.4f} (error {float(err.max()):.3e}); worst (pinned - optimum) / bound "
          f"{float(np.where(ok, (pinned - want) / lim, 0.0).max()):.4f}")
    assert (err <= lim).all(), (what, float(err.max()), worst)
    assert (pinned <= want + scale * lim)[ok].all(), what
    return worst


def onehot(symbols, T, H, scale=3.0):
    """one word of mutually orthogonal one-hot frames: frame t = scale * e_symbols[t]; NaN behind the length"""
    f = np.full((T, H), np.nan, dtype=np.float32)
    f[:len(symbols)] = 0.0
    f[np.arange(len(symbols)), symbols] = scale
    return f


def exact_cases(T=12, H=64):
    """(name, query symbols, word symbols, d, span): costs are exactly 0 or 1 on every route, so d and the span are EQUAL.
    The spans are what the definition's tie rules give (worked by hand, and held to the yardstick in the test): with every frame
    twice the match loses the first of the first pair (the diagonal predecessor wins the tie at the start) and the second of the
    last pair (the smallest end), so a copy of 4 frames doubled spans 6 frames, not 8."""
    return [
        ("a copy inside junk", [1, 2, 3, 4], [10, 11, 1, 2, 3, 4, 12, 13], 0.0, (2, 6)),
        ("the copy with every frame twice", [1, 2, 3, 4], [10, 1, 1, 2, 2, 3, 3, 4, 4, 11], 0.0, (2, 8)),
        ("one substituted frame", [1, 2, 3, 4], [10, 1, 2, 9, 4, 11], 1 / 4, (1, 5)),
        ("tie: [a] in [a, a]", [1], [1, 1], 0.0, (0, 1)),
        ("tie: [a, a] in [a, a, a]", [1, 1], [1, 1, 1], 0.0, (0, 1)),
        ("two places: the first end", [1, 2], [9, 1, 2, 8, 1, 2], 0.0, (1, 3)),
        ("Lq > Ln, a stretched query", [1, 1, 2, 2, 3], [1, 2, 3], 0.0, (0, 3)),
        ("Lq > Ln, nothing in common", [1, 2, 3, 4, 5, 6, 7], [8, 9], 1.0, (0, 1)),
        ("a query of one frame", [1], [2, 1, 3], 0.0, (1, 2)),
        ("a word of one frame", [1, 2, 3], [2], 2 / 3, (0, 1)),
        ("one frame each, equal", [5], [5], 0.0, (0, 1)),
        ("one frame each, orthogonal", [5], [6], 1.0, (0, 1)),
        ("full length", list(range(T)), list(range(T)), 0.0, (0, T)),
    ]


def exact_arrays(T=12, H=64):
    cases = exact_cases(T, H)
    fq = np.stack([onehot(c[1], T, H) for c in cases])
    fc = np.stack([onehot(c[2], T, H, 0.25) for c in cases])
    ql = np.array([len(c[1]) for c in cases], dtype=np.int32)
    cl = np.array([len(c[2]) for c in cases], dtype=np.int32)
    return cases, fq, ql, fc, cl


def host_from_raw(fq, ql, lo, hi, fc, cl):
    from manuscript_ocr_amd import ops
    return ops.dtw_subsequence_host(ops.frame_normalize_host(fq, ql), ql, lo, hi, ops.frame_normalize_host(fc, cl), cl)


def nan_behind(feat, lengths):
    for n in range(len(lengths)):
        feat[n, max(int(lengths[n]), 0):] = np.nan
    return feat


# ------------------------------------------------------------------------------------------------ (a) exact cases
def test_exact_cases_on_one_hot_frames():
    cases, fq, ql, fc, cl = exact_arrays()
    T = fq.shape[1]
    d, span = host_from_raw(fq, ql, *full_gate(len(ql), T), fc, cl)
    uq, uc = yard_unit(fq, ql), yard_unit(fc, cl)
    for k, (name, _q, _w, want_d, want_span) in enumerate(cases):
        yd, yspan = yard_sub(yard_cost(uq[k], ql[k], uc[k], cl[k]))
        assert (yd, yspan) == (want_d, want_span), name            # the hand-worked value is the yardstick's
        assert d[k, k] == np.float32(want_d) and tuple(span[k, k].tolist()) == want_span, (name, float(d[k, k]), span[k, k].tolist())
    # ... and every other pairing of these queries and words equals the yardstick too: exact costs leave no near-ties
    for q in range(len(ql)):
        for n in range(len(cl)):
            yd, yspan = yard_sub(yard_cost(uq[q], ql[q], uc[n], cl[n]))
            assert d[q, n] == np.float32(yd) and tuple(span[q, n].tolist()) == yspan, (q, n)


# ------------------------------------------------------------------------------------------------ (b) random frames
@pytest.mark.parametrize("T", [1, 2, 33, 64])
def test_host_twin_against_the_yardstick(T):
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(100 + T)
    H = 64
    edge = sorted({1, min(2, T), max(T - 1, 1), T})
    fq, ql = random_words(rng, len(edge), T, H, edge)
    fc, cl = random_words(rng, len(edge) + 3, T, H, edge + list(rng.integers(1, T + 1, 3)))
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo, hi = full_gate(len(ql), T)
    uq, uc = ops.frame_normalize_host(fq, ql), ops.frame_normalize_host(fc, cl)
    d, span = ops.dtw_subsequence_host(uq, ql, lo, hi, uc, cl)
    assert np.isfinite(d).all() and d.dtype == np.float32 and span.dtype == np.int32 and span.shape == d.shape + (2,)
    # from the same f32 unit frames: the f64 table rounded once
    check_pairs(d, span, uq, ql, lo, hi, uc, cl, tol_same, f"T {T}, same unit frames")
    # from the same raw frames: the unit frames' own error on top
    check_pairs(d, span, yard_unit(fq, ql), ql, lo, hi, yard_unit(fc, cl), cl, lambda a, b: bound_sub(H, a, b), f"T {T}, raw frames")


def test_the_yardstick_against_brute_force():
    """the table against the definition taken literally on a tiny case: every monotone path with steps (1, 1), (1, 0), (0, 1) from
    any (0, s) to any (Lq - 1, e) that takes no step along row 0, enumerated"""
    rng = np.random.default_rng(7)
    C = rng.random((3, 4))

    def paths(i, j):
        if i == 0:
            yield C[0, j]
            return
        for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            if pj >= 0:
                for p in paths(pi, pj):
                    yield p + C[i, j]

    for e in range(4):
        S, _ = yard_sub_table(C)
        assert S[2, e] == pytest.approx(min(paths(2, e)), abs=1e-12)
    d, (s, e) = yard_sub(C)
    assert d == pytest.approx(min(min(paths(2, j)) for j in range(4)) / 3, abs=1e-12)
    assert yard_pinned(C, s, e - 1) == pytest.approx(d, abs=1e-12)


def test_the_vectorised_yardstick_is_the_cell_by_cell_one():
    rng = np.random.default_rng(11)
    T, H = 7, 64
    fq, ql = random_words(rng, 3, T, H, [1, 7, 4])
    fc, cl = random_words(rng, 5, T, H, [7, 1, 2, 5, 3])
    uq, uc = yard_unit(fq, ql), yard_unit(fc, cl)
    d, span = yard_sub_results(*yard_sub_all(uq, ql, uc, cl), ql, cl)
    pin = rng.integers(0, cl[None, :].repeat(3, axis=0))
    Sp, _ = yard_sub_all(uq, ql, uc, cl, pin=pin)
    for q in range(3):
        for n in range(5):
            C = yard_cost(uq[q], ql[q], uc[n], cl[n])
            wd, wspan = yard_sub(C)
            assert d[q, n] == pytest.approx(wd, abs=1e-14) and tuple(span[q, n]) == wspan
            for e in range(cl[n]):
                assert Sp[q, n, ql[q] - 1, e] / ql[q] == pytest.approx(yard_pinned(C, pin[q, n], e), abs=1e-14)


# ------------------------------------------------------------------------------------------------ (c) the gate and the ABI
def test_length_gate_zero_frames_and_empty_calls():
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(6)
    T, H = 12, 64
    fq, ql = random_words(rng, 1, T, H, [6])
    fc, cl = random_words(rng, 6, T, H, [2, 3, 6, 9, 10, 12])
    uq, uc = ops.frame_normalize_host(fq, ql), ops.frame_normalize_host(fc, cl)
    d, span = ops.dtw_subsequence_host(uq, ql, [3], [9], uc, cl)     # at len_lo, at len_hi, one outside each
    assert np.isfinite(d[0]).tolist() == [False, True, True, True, False, False]
    assert (span[0, [0, 4, 5]] == -1).all() and (span[0, 1:4, 0] >= 0).all()
    open_d, open_span = ops.dtw_subsequence_host(uq, ql, [1], [T], uc, cl)
    assert same_bits(d[0, 1:4], open_d[0, 1:4]) and np.array_equal(span[0, 1:4], open_span[0, 1:4])
    d, span = ops.dtw_subsequence_host(uq, ql, [7], [8], uc, cl)
    assert np.isinf(d).all() and (span == -1).all()
    # zero-norm and non-finite frames cost 1 against everything and leave no NaN
    fq, ql = random_words(rng, 2, T, H, [4, 3])
    fc, cl = random_words(rng, 3, T, H, [4, 6, 1])
    fq[0, 1] = 0.0
    fq[1, 0, 3] = np.nan
    fc[1, 2, 0] = -np.inf
    fc[2, 0] = 0.0
    d, span = host_from_raw(fq, ql, *full_gate(2, T), fc, cl)
    assert np.isfinite(d).all()
    check_pairs(d, span, yard_unit(fq, ql), ql, *full_gate(2, T), yard_unit(fc, cl), cl, lambda a, b: bound_sub(H, a, b), "zero frames")
    assert d[0, 2] == np.float32(1.0) and d[1, 2] == np.float32(1.0)    # a one-frame zero word: Lq cells of cost 1, over Lq
    assert span[:, 2].tolist() == [[0, 1], [0, 1]]
    # N = 0 and Q = 0
    cl = np.array([2, 3, 6, 9, 10, 12], dtype=np.int32)
    d, span = ops.dtw_subsequence_host(uq[:0], cl[:0], cl[:0], cl[:0], uc, cl)
    assert d.shape == (0, 6) and span.shape == (0, 6, 2)
    d, span = ops.dtw_subsequence_host(uq, [6], [1], [T], uc[:0], cl[:0])
    assert d.shape == (1, 0) and span.shape == (1, 0, 2)


def test_symbols_and_abi_refusals():
    """Everything here is refused before any launch: no GPU is touched, the device entry point included."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    for name in ("msocr_dtw_subsequence", "msocr_dtw_subsequence_host"):
        assert name in nat.exported_symbols() and hasattr(nat.lib(), name)
    assert callable(ops.dtw_subsequence) and callable(ops.dtw_subsequence_host)
    L = nat.lib()
    E_ARG = -1
    T, H = 4, 64
    f = np.zeros((2, T, H), dtype=np.float32)
    ln = np.array([1, 4], dtype=np.int32)
    lo, hi = np.array([1, 1], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    dist = np.zeros((2, 2), dtype=np.float32)
    span = np.zeros((2, 2, 2), dtype=np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    big = np.zeros((2, 65, 64), dtype=np.float32)
    # shapes: T = 0 / 65, H = 0 / 32 / 96 / 576, negative counts, N T H >= 2^31 (only sizes are read), on either side
    for (N, t, h) in ((2, 0, H), (2, 65, H), (2, T, 0), (2, T, 32), (2, T, 96), (2, T, 576), (-1, T, H), (1 << 16, 64, 512)):
        assert L.msocr_dtw_subsequence_host(p(big), p(ln), p(lo), p(hi), 2, p(big), p(ln), N, t, h, p(dist), p(span)) == E_ARG
        assert L.msocr_dtw_subsequence(p(big), p(ln), p(lo), p(hi), 2, p(big), p(ln), N, t, h, p(dist), p(span), None) == E_ARG
        assert L.msocr_dtw_subsequence_host(p(big), p(ln), p(lo), p(hi), N, p(big), p(ln), 2, t, h, p(dist), p(span)) == E_ARG
        assert L.msocr_dtw_subsequence(p(big), p(ln), p(lo), p(hi), N, p(big), p(ln), 2, t, h, p(dist), p(span), None) == E_ARG
    # null pointers, the span among them
    args = [p(f), p(ln), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist), p(span)]
    assert L.msocr_dtw_subsequence_host(*args) == 0
    for k in (0, 1, 2, 3, 5, 6, 10, 11):
        bad = list(args)
        bad[k] = None
        assert L.msocr_dtw_subsequence_host(*bad) == E_ARG
        assert L.msocr_dtw_subsequence(*bad, None) == E_ARG
    # unit frames that are not 16-byte aligned (device route)
    raw = np.zeros(2 * T * H + 1, dtype=np.float32)
    off = raw[1:] if raw.ctypes.data % 16 == 0 else raw[:-1]
    assert off.ctypes.data % 16 != 0
    assert L.msocr_dtw_subsequence(p(off), p(ln), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist), p(span), None) == E_ARG
    assert L.msocr_dtw_subsequence(p(f), p(ln), p(lo), p(hi), 2, p(off), p(ln), 2, T, H, p(dist), p(span), None) == E_ARG
    # lengths outside [1, T] and len_lo > len_hi (the host twin can read them)
    for bad_len in ([0, 4], [1, 5], [-3, 1]):
        b = np.array(bad_len, dtype=np.int32)
        assert L.msocr_dtw_subsequence_host(p(f), p(b), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist), p(span)) == E_ARG
        assert L.msocr_dtw_subsequence_host(p(f), p(ln), p(lo), p(hi), 2, p(f), p(b), 2, T, H, p(dist), p(span)) == E_ARG
    assert L.msocr_dtw_subsequence_host(p(f), p(ln), p(hi), p(lo), 2, p(f), p(ln), 2, T, H, p(dist), p(span)) == E_ARG
    # nothing to do is fine, and launches nothing
    assert L.msocr_dtw_subsequence_host(p(f), p(ln), p(lo), p(hi), 0, p(f), p(ln), 2, T, H, p(dist), p(span)) == 0
    assert L.msocr_dtw_subsequence_host(p(f), p(ln), p(lo), p(hi), 2, p(f), p(ln), 0, T, H, p(dist), p(span)) == 0
    assert L.msocr_dtw_subsequence(p(f), p(ln), p(lo), p(hi), 0, p(f), p(ln), 2, T, H, p(dist), p(span), None) == 0
    assert L.msocr_dtw_subsequence(p(f), p(ln), p(lo), p(hi), 2, p(f), p(ln), 0, T, H, p(dist), p(span), None) == 0


# ------------------------------------------------------------------------------------------------ (d) WordIndex
def stem_index(device=None):
    """Twelve words of T = 16, H = 64 on two pages.  Word 7 holds word 1's six frames at columns 4 .. 9 between frames of its own;
    word 9 is word 1 again."""
    from manuscript_ocr_amd import WordIndex
    rng = np.random.default_rng(8)
    T, H = 16, 64
    lens = [5, 6, 3, 8, 16, 1, 2, 13, 12, 6, 9, 4]
    ids = [(0, 0, w) for w in range(6)] + [(1, 0, w) for w in range(3)] + [(1, 1, w) for w in range(3)]
    feat, lens = random_words(rng, 12, T, H, lens)
    feat[7, 4:10] = feat[1, :6]
    feat[9] = feat[1]
    texts = [f"w{i}" if i % 2 else None for i in range(12)]
    return WordIndex.from_features(feat, lens, ids, texts=texts, device=device), feat, lens, ids, texts


def part_rows(per_query):
    """what a caller sees of the hits, the distance as its f32 bits"""
    return [[(type(h).__name__, h.query, h.page, h.block, h.word, h.rank, h.text, np.float32(h.distance).tobytes(), h.frame_start,
              h.frame_end, h.fraction) for h in hits] for hits in per_query]


def check_stem_index(index, feat, lens, ids, texts):
    """the asserts on `stem_index` that hold on the host and on the device alike"""
    from manuscript_ocr_amd.detectors._types import PartSpotHit, SpotHit
    H, T = 64, 16
    hits = index.spot([(0, 0, 1), (1, 1, 2)], k=12, max_length_ratio=2.0, partial=True)
    assert len(hits) == 2 and all(type(h) is PartSpotHit and isinstance(h, SpotHit) for hs in hits for h in hs)
    first = hits[0]
    # the query of 6 frames finds itself, its copy and the word that contains it: distance about 0, the spans exactly
    # (a planted copy's diagonal costs ~1e-7 a frame, any other path ~1 a frame: no near-tie)
    top = {(h.page, h.block, h.word): h for h in first[:3]}
    assert sorted(top) == [(0, 0, 1), (1, 0, 1), (1, 1, 0)]
    for ref, (a, b, L) in (((0, 0, 1), (0, 6, 6)), ((1, 1, 0), (0, 6, 6)), ((1, 0, 1), (4, 10, 13))):
        h = top[ref]
        assert (h.frame_start, h.frame_end) == (a, b) and h.fraction == (a / L, b / L) and abs(h.distance) <= bound_sub(H, 6, L)
    assert first[3].distance > 0.1
    assert [h.rank for h in first] == list(range(len(first))) and all(h.query == 0 for h in first)
    assert [h.distance for h in first] == sorted(h.distance for h in first)
    assert top[(1, 1, 0)].text == "w9" and top[(0, 0, 1)].text == "w1"
    # the gate of the partial route: ceil(L / r) .. T.  A query of 6 frames meets words of 3 .. 16 frames: all but words 5 and 6
    assert sorted(h.word + 100 * h.page + 10 * h.block for h in first) == sorted(w + 100 * p + 10 * b for (p, b, w), L in zip(ids, lens) if L >= 3)
    everything = index.spot([(0, 0, 1)], k=256, max_length_ratio=None, partial=True)[0]
    assert sorted((h.page, h.block, h.word) for h in everything) == sorted(ids)
    # against the yardstick: every hit within the bound, its span valid
    unit = yard_unit(feat, lens)
    for q, ref in enumerate([(0, 0, 1), (1, 1, 2)]):
        row = ids.index(ref)
        for h in hits[q]:
            n = ids.index((h.page, h.block, h.word))
            C = yard_cost(unit[row], lens[row], unit[n], lens[n])
            want, _ = yard_sub(C)
            lim = bound_sub(H, lens[row], lens[n])
            assert abs(h.distance - want) <= lim and 0 <= h.frame_start < h.frame_end <= lens[n]
            assert yard_pinned(C, h.frame_start, h.frame_end - 1) <= want + 2 * lim
            assert h.fraction == (h.frame_start / lens[n], h.frame_end / lens[n])
    # queries as frames, and partial=False is the call without the argument, with its type
    by_frames = index.spot_features(feat[[1]], lens[[1]], k=12, partial=True)
    assert part_rows(by_frames) == part_rows([first])
    plain, flagged = index.spot([(0, 0, 1), (1, 1, 2)], k=5), index.spot([(0, 0, 1), (1, 1, 2)], k=5, partial=False)
    assert all(type(h) is SpotHit for hs in flagged for h in hs)
    assert [[h.model_dump() for h in hs] for hs in plain] == [[h.model_dump() for h in hs] for hs in flagged]
    assert [[h.model_dump() for h in hs] for hs in index.spot_features(feat[[1]], lens[[1]], k=5, partial=False)] == \
           [[h.model_dump() for h in hs] for hs in index.spot_features(feat[[1]], lens[[1]], k=5)]
    assert index.spot([], partial=True) == []


def test_word_index_partial():
    check_stem_index(*stem_index())


def partial_in_blocks_and_in_one(monkeypatch, device):
    """The words of test_word_spotting_cpu.words_for_blocks in an index of one block and in one of blocks of 5, 5, 5, 5, 3 with
    the 7 queries cut into 5 + 2: the same PartSpotHits, distances bit for bit and spans equal -> the hits without a gate"""
    from manuscript_ocr_amd import WordIndex, _spotting
    from test_word_spotting_cpu import words_for_blocks
    feat, lens, ids, texts, fq, ql = words_for_blocks()
    T, H = feat.shape[1:]

    def build():
        index, at = WordIndex(None, device=device), 0
        for n in (3, 9, 11):
            index.add_features(feat[at:at + n], lens[at:at + n], ids[at:at + n], texts[at:at + n])
            at += n
        return index

    refs = [ids[21], ids[3], ids[17], ids[0], ids[22], ids[20]]

    def ask(index):
        return [index.spot_features(fq, ql, k=23, max_length_ratio=None, partial=True), index.spot_features(fq, ql, k=4, partial=True),
                index.spot(refs, k=6, partial=True), index.spot(refs + [ids[9]], k=256, max_length_ratio=1.5, partial=True)]

    one = build()
    want = ask(one)
    assert [int(u.shape[0]) for u, _ in one._blocks] == [23]
    monkeypatch.setattr(_spotting, "_LIMIT", 5 * T * H)
    cut = build()
    got = ask(cut)
    assert [int(u.shape[0]) for u, _ in cut._blocks] == [5, 5, 5, 5, 3]
    for g, w in zip(got, want):
        assert part_rows(g) == part_rows(w)
    everything = got[0]
    assert all(sorted(h.word for h in hits) == list(range(23)) for hits in everything)
    # word 17 is word 3 again and query 2 is its frames: the tie across the block edge goes to the word that entered first,
    # both with the span of the whole word; a reference into the last block finds itself with span [0, L)
    for hits in (everything[2], got[2][1], got[2][2]):
        assert [(h.word, h.rank) for h in hits[:2]] == [(3, 0), (17, 1)] and hits[0].distance == hits[1].distance
        assert all((h.frame_start, h.frame_end, h.fraction) == (0, lens[3], (0.0, 1.0)) for h in hits[:2])
    for q, n in ((0, 21), (4, 22), (5, 20)):
        h = got[2][q][0]
        assert h.word == n and abs(h.distance) <= bound_sub(H, lens[n], lens[n]) and (h.frame_start, h.frame_end) == (0, lens[n])
    return everything


def test_word_index_partial_in_several_blocks(monkeypatch):
    from test_word_spotting_cpu import words_for_blocks
    everything = partial_in_blocks_and_in_one(monkeypatch, None)
    feat, lens, _ids, _texts, fq, ql = words_for_blocks()
    uq, uc = yard_unit(fq, ql), yard_unit(feat, lens)
    for q, hits in enumerate(everything):
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        for h in hits:
            want, _ = yard_sub(yard_cost(uq[q], ql[q], uc[h.word], lens[h.word]))
            assert abs(h.distance - want) <= bound_sub(64, ql[q], lens[h.word])


def test_types_and_signatures():
    import inspect
    from manuscript_ocr_amd import Pipeline, WordIndex
    from manuscript_ocr_amd.detectors._types import PartSpotHit, SpotHit
    assert issubclass(PartSpotHit, SpotHit)
    assert set(PartSpotHit.model_fields) - set(SpotHit.model_fields) == {"frame_start", "frame_end", "fraction"}
    assert "query" in PartSpotHit.model_fields["distance"].description.lower()
    for fn in (WordIndex.spot, WordIndex.spot_features, Pipeline.spot):
        assert inspect.signature(fn).parameters["partial"].default is False


# ------------------------------------------------------------------------------------------------ (e) the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """The subsequence part of csrc/word_spotting.h (the argument check, the f64 table with its start columns and tie rules, the
    gate) in a plain C++ program of its own (tests/native/word_spotting_partial_fuzz.cpp) with the address and undefined-behaviour
    sanitizers: garbage lengths, non-finite features, every array in a heap block of its exact size, every result compared with a
    plain full table.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no clang++ with sanitizer runtimes here")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "word_spotting_partial_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "word_spotting_partial_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 300 checked 300")
