"""Word spotting (include/msocr.h, "word spotting") without a GPU: the host twins msocr_frame_normalize_host,
msocr_dtw_distances_host and msocr_topk_smallest_host against yardsticks written here in plain NumPy f64 over the definition, every
refusal of the C ABI, WordIndex on hand-built features, and csrc/word_spotting.h in a plain C++ program under the address and
undefined-behaviour sanitizers (tests/native/word_spotting_fuzz.cpp).

The yardsticks: `yard_unit` (u = x / ||x|| in f64; the zero frame where the squared norm is not finite, overflows f32 or is below
FLT_MIN), `yard_pair` (the table of the definition, cell by cell), `yard_all` (the same for all pairs at once: loops over the
cells, NumPy across the pairs; held to `yard_pair` below) and `yard_topk` (a stable sort of the finite entries).  tests/
test_gpu_word_spotting.py imports them."""
import os
import subprocess

import numpy as np
import pytest

EPS = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------ yardsticks
def yard_unit(feat, lengths, dtype=np.float64):
    """[N, T, H] raw frames -> unit frames in `dtype`; frames t >= len are zeros and their input is not looked at"""
    feat = np.asarray(feat)
    N, T, H = feat.shape
    out = np.zeros((N, T, H), dtype=dtype)
    for n in range(N):
        for t in range(int(lengths[n])):
            x = feat[n, t].astype(dtype)
            with np.errstate(all="ignore"):
                ss = float(np.sum(x * x, dtype=dtype))
            if np.isfinite(ss) and FLT_MIN <= ss <= FLT_MAX:
                out[n, t] = x / np.sqrt(dtype(ss))
    return out


def yard_pair(u, Lu, v, Lv):
    """the definition, cell by cell, in f64: u [>= Lu, H], v [>= Lv, H] unit frames -> d"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    D = np.full((Lu, Lv), np.inf)
    for i in range(Lu):
        for j in range(Lv):
            c = 1.0 - float(np.dot(u[i], v[j]))
            if i == 0 and j == 0:
                best = 0.0
            else:
                best = min(D[i - 1, j - 1] if i and j else np.inf, D[i - 1, j] if i else np.inf, D[i, j - 1] if j else np.inf)
            D[i, j] = c + best
    return D[Lu - 1, Lv - 1] / (Lu + Lv)


def yard_all(qu, ql, lo, hi, cu, cl, dtype=np.float64):
    """all pairs at once in `dtype`: qu [Q, T, H], cu [N, T, H] unit frames (zeros behind the lengths) -> d [Q, N], +inf where the
    word's length lies outside [lo[q], hi[q]]"""
    qu, cu = np.asarray(qu, dtype=dtype), np.asarray(cu, dtype=dtype)
    Q, T, H = qu.shape
    N = cu.shape[0]
    ql, cl, lo, hi = (np.asarray(a, dtype=np.int64) for a in (ql, cl, lo, hi))
    out = np.full((Q, N), np.inf, dtype=dtype)
    if Q == 0 or N == 0:
        return out
    C = dtype(1.0) - (qu.reshape(Q * T, H) @ cu.reshape(N * T, H).T).reshape(Q, T, N, T).transpose(0, 2, 1, 3)  # [Q, N, i, j]
    D = np.full((Q, N, T, T), np.inf, dtype=dtype)
    for i in range(T):
        for j in range(T):
            if i == 0 and j == 0:
                D[:, :, 0, 0] = C[:, :, 0, 0]
                continue
            best = np.full((Q, N), np.inf, dtype=dtype)
            if i and j:
                best = np.minimum(best, D[:, :, i - 1, j - 1])
            if i:
                best = np.minimum(best, D[:, :, i - 1, j])
            if j:
                best = np.minimum(best, D[:, :, i, j - 1])
            D[:, :, i, j] = C[:, :, i, j] + best
    last = D[np.arange(Q)[:, None], np.arange(N)[None, :], (ql - 1)[:, None], (cl - 1)[None, :]]
    d = last / (ql[:, None] + cl[None, :]).astype(dtype)
    ok = (cl[None, :] >= lo[:, None]) & (cl[None, :] <= hi[:, None])
    out[ok] = d[ok]
    return out


def yard_topk(dist, k):
    dist = np.asarray(dist, dtype=np.float32)
    Q, N = dist.shape
    idx = np.full((Q, k), -1, dtype=np.int32)
    val = np.full((Q, k), np.inf, dtype=np.float32)
    for q in range(Q):
        fin = np.flatnonzero(np.isfinite(dist[q]))
        order = fin[np.argsort(dist[q, fin], kind="stable")][:k]  # a stable sort: equal values (-0.0 == 0.0) keep ascending index
        idx[q, :len(order)] = order
        val[q, :len(order)] = dist[q, order]
    return idx, val


def bound(H, Lq, Ln):
    """The bound of the distance against the f64 yardstick, from raw frames (tests/test_gpu_word_spotting.py derives it)."""
    return (3 * H + 2 * (Lq + Ln) + 16) * EPS


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_words(rng, N, T, H, lengths=None):
    feat = rng.standard_normal((N, T, H)).astype(np.float32)
    if lengths is None:
        lengths = rng.integers(1, T + 1, N)
    return feat, np.asarray(lengths, dtype=np.int32)


def full_gate(Q, T):
    return np.ones(Q, dtype=np.int32), np.full(Q, T, dtype=np.int32)


def host_from_raw(fq, ql, lo, hi, fc, cl):
    from manuscript_ocr_amd import ops
    return ops.dtw_distances_host(ops.frame_normalize_host(fq, ql), ql, lo, hi, ops.frame_normalize_host(fc, cl), cl)


# ------------------------------------------------------------------------------------------------ the yardsticks themselves
def test_yard_all_is_yard_pair():
    rng = np.random.default_rng(1)
    fq, ql = random_words(rng, 3, 6, 64, [1, 6, 4])
    fc, cl = random_words(rng, 5, 6, 64, [6, 1, 2, 5, 3])
    uq, uc = yard_unit(fq, ql), yard_unit(fc, cl)
    lo, hi = np.array([1, 2, 1], dtype=np.int32), np.array([6, 5, 3], dtype=np.int32)
    got = yard_all(uq, ql, lo, hi, uc, cl)
    for q in range(3):
        for n in range(5):
            if lo[q] <= cl[n] <= hi[q]:
                assert got[q, n] == pytest.approx(yard_pair(uq[q], ql[q], uc[n], cl[n]), abs=1e-15)
            else:
                assert got[q, n] == np.inf


# ------------------------------------------------------------------------------------------------ normalisation
def test_normalize_host_lengths_and_the_zero_rule():
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(2)
    for H in (64, 256, 512):
        feat, lengths = random_words(rng, 6, 5, H, [5, 4, 1, 5, 5, 5])
        feat[0, 1] = 0.0                       # no direction
        feat[0, 2, 7] = np.nan
        feat[3, 0, H - 1] = np.inf
        feat[3, 1] = 1e30                      # the squared norm overflows f32
        feat[3, 2] = 1e-30                     # ... and here lies below FLT_MIN
        feat[4, 3] *= 1e18
        feat[4, 4] *= 1e-18
        feat[1, 4:] = np.nan                   # behind the length: never read
        feat[2, 1:] = np.inf
        unit = ops.frame_normalize_host(feat, lengths)
        assert np.isfinite(unit).all()
        for n, t in ((0, 1), (0, 2), (3, 0), (3, 1), (3, 2)):
            assert not unit[n, t].any()
        for n in range(6):
            assert not unit[n, lengths[n]:].any()
        want = yard_unit(feat, lengths)
        nz = np.abs(want).sum(axis=2) > 0
        assert np.array_equal(nz, np.abs(unit).sum(axis=2) > 0)
        norm = np.sqrt((unit.astype(np.float64) ** 2).sum(axis=2))
        assert np.abs(norm[nz] - 1.0).max() <= (H + 4) * EPS
        assert np.abs(unit - want).max() <= (H + 4) * EPS


# ------------------------------------------------------------------------------------------------ distances
def test_identities():
    """a sequence against itself and against a copy with every frame repeated twice: d <= bound; mutually orthogonal one-hot frames:
    d = max(Lq, Ln) / (Lq + Ln) exactly (every cell costs 1 and the cheapest path has max(Lq, Ln) cells)"""
    rng = np.random.default_rng(3)
    H, T = 64, 24
    for L in (1, 2, 7, 12):
        feat = np.zeros((2, T, H), dtype=np.float32)
        x = rng.standard_normal((L, H)).astype(np.float32)
        feat[0, :L] = x
        feat[1, :2 * L] = np.repeat(x, 2, axis=0)
        lens = np.array([L, 2 * L], dtype=np.int32)
        d = host_from_raw(feat[:1], lens[:1], *full_gate(1, T), feat, lens)
        assert abs(d[0, 0]) <= bound(H, L, L)
        assert abs(d[0, 1]) <= bound(H, L, 2 * L)
    for Lq, Ln in ((1, 1), (1, 9), (9, 1), (5, 8), (24, 24), (24, 3)):
        q = np.zeros((1, T, H), dtype=np.float32)
        c = np.zeros((1, T, H), dtype=np.float32)
        q[0, np.arange(Lq), np.arange(Lq)] = 3.0          # e_0 .. e_{Lq-1}
        c[0, np.arange(Ln), 32 + np.arange(Ln)] = 0.25    # e_32 .. : orthogonal to all of them
        d = host_from_raw(q, [Lq], *full_gate(1, T), c, [Ln])
        assert d[0, 0] == np.float32(max(Lq, Ln) / (Lq + Ln))


def test_host_twin_against_the_yardstick():
    """random frames over T in {1, 2, 33, 64} with lengths 1, 2, T - 1, T on both sides: the host twin is the definition in f64
    from its own f32 unit frames, so it sits within the unit frames' error of the yardstick from raw frames"""
    rng = np.random.default_rng(4)
    for T in (1, 2, 33, 64):
        H = 64
        edge = sorted({1, min(2, T), max(T - 1, 1), T})
        fq, ql = random_words(rng, len(edge), T, H, edge)
        fc, cl = random_words(rng, len(edge) + 3, T, H, edge + list(rng.integers(1, T + 1, 3)))
        for f, l in ((fq, ql), (fc, cl)):
            for n in range(len(l)):
                f[n, l[n]:] = np.nan               # never read
        got = host_from_raw(fq, ql, *full_gate(len(ql), T), fc, cl)
        want = yard_all(yard_unit(fq, ql), ql, *full_gate(len(ql), T), yard_unit(fc, cl), cl)
        assert np.isfinite(got).all()
        for q in range(len(ql)):
            for n in range(len(cl)):
                assert abs(got[q, n] - want[q, n]) <= bound(H, ql[q], cl[n])
        # and from the SAME f32 unit frames the twin is the f64 table rounded once
        from manuscript_ocr_amd import ops
        uq, uc = ops.frame_normalize_host(fq, ql), ops.frame_normalize_host(fc, cl)
        same = yard_all(uq, ql, *full_gate(len(ql), T), uc, cl)
        assert np.abs(got - same).max() <= 4 * EPS


def test_zero_and_non_finite_frames_cost_one():
    rng = np.random.default_rng(5)
    T, H = 6, 64
    fq, ql = random_words(rng, 2, T, H, [4, 3])
    fc, cl = random_words(rng, 3, T, H, [4, 6, 1])
    fq[0, 1] = 0.0
    fq[1, 0, 3] = np.nan
    fc[1, 2, 0] = -np.inf
    fc[2, 0] = 0.0                                  # a word that is one zero frame: costs 1 against everything
    got = host_from_raw(fq, ql, *full_gate(2, T), fc, cl)
    want = yard_all(yard_unit(fq, ql), ql, *full_gate(2, T), yard_unit(fc, cl), cl)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= bound(H, T, T)
    # against the one-frame zero word every cell costs exactly 1: D = Lq, d = Lq / (Lq + 1)
    assert got[0, 2] == np.float32(4 / 5) and got[1, 2] == np.float32(3 / 4)


def test_length_gate():
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd._spotting import length_bounds
    rng = np.random.default_rng(6)
    T, H = 12, 64
    fq, ql = random_words(rng, 1, T, H, [6])
    fc, cl = random_words(rng, 6, T, H, [2, 3, 6, 9, 10, 12])
    uq, uc = ops.frame_normalize_host(fq, ql), ops.frame_normalize_host(fc, cl)
    got = ops.dtw_distances_host(uq, ql, [3], [9], uc, cl)
    assert np.array_equal(np.isfinite(got[0]), [False, True, True, True, False, False])
    open_gate = ops.dtw_distances_host(uq, ql, [1], [T], uc, cl)
    assert np.array_equal(got[0, 1:4], open_gate[0, 1:4])
    assert np.isinf(ops.dtw_distances_host(uq, ql, [7], [8], uc, cl)).all()
    # the Python layer's bounds: ceil(L / r), floor(L r), clipped into [1, T]
    lo, hi = length_bounds([6, 1, 5, 12], 2.0, T)
    assert lo.tolist() == [3, 1, 3, 6] and hi.tolist() == [12, 2, 10, 12]
    lo, hi = length_bounds([6, 5], 1.5, T)
    assert lo.tolist() == [4, 4] and hi.tolist() == [9, 7]
    lo, hi = length_bounds([6, 5], None, T)
    assert lo.tolist() == [1, 1] and hi.tolist() == [T, T]
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            length_bounds([3], bad, T)


# ------------------------------------------------------------------------------------------------ selection
def test_topk_host_against_the_stable_sort():
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(7)
    inf = np.float32(np.inf)
    rows = [
        rng.standard_normal(40).astype(np.float32),
        np.full(40, 0.5, dtype=np.float32),                                     # all equal: ties by index
        np.full(40, inf, dtype=np.float32),                                     # nothing finite
        np.where(np.arange(40) % 7 == 3, rng.random(40), np.inf).astype(np.float32),   # six finite entries
        np.array([0.0, -0.0] * 20, dtype=np.float32),                           # -0.0 == 0.0: index order, signs kept
        np.where(np.arange(40) % 3 == 0, np.nan, rng.integers(0, 4, 40)).astype(np.float32),
        np.concatenate([[-np.inf, np.inf, np.nan], rng.integers(-2, 2, 37)]).astype(np.float32),
    ]
    dist = np.stack(rows)
    for k in (1, 5, 6, 7, 40, 41, 256):
        idx, val = ops.topk_smallest_host(dist, k)
        widx, wval = yard_topk(dist, k)
        assert np.array_equal(idx, widx)
        assert same_bits(val, wval)
    idx, val = ops.topk_smallest_host(dist, 6)
    assert idx[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert idx[2].tolist() == [-1] * 6 and np.isinf(val[2]).all()
    assert idx[3].tolist() == sorted(idx[3].tolist(), key=lambda i: dist[3, i]) and (idx[3] % 7 == 3).all()
    assert idx[4].tolist() == [0, 1, 2, 3, 4, 5] and np.signbit(val[4]).tolist() == [False, True] * 3
    # N = 0 and Q = 0
    idx, val = ops.topk_smallest_host(np.zeros((3, 0), dtype=np.float32), 4)
    assert idx.shape == (3, 4) and (idx == -1).all() and np.isinf(val).all()
    idx, val = ops.topk_smallest_host(np.zeros((0, 9), dtype=np.float32), 4)
    assert idx.shape == (0, 4)


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbols_wrappers_and_constants():
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    for name in ("msocr_frame_normalize", "msocr_frame_normalize_host", "msocr_dtw_distances", "msocr_dtw_distances_host",
                 "msocr_topk_smallest", "msocr_topk_smallest_host"):
        assert name in nat.exported_symbols()
        assert hasattr(nat.lib(), name)
    assert (ops.SPOT_MAX_T, ops.SPOT_MAX_H, ops.SPOT_MAX_K) == (64, 512, 256)
    assert ops.SPOT_TILE >= 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msocr.h")).read()
    for name, value in (("MSOCR_SPOT_MAX_T", ops.SPOT_MAX_T), ("MSOCR_SPOT_MAX_H", ops.SPOT_MAX_H), ("MSOCR_SPOT_MAX_K", ops.SPOT_MAX_K),
                        ("MSOCR_SPOT_TILE", ops.SPOT_TILE)):
        assert f"#define {name} {value}\n" in header


def test_abi_refusals():
    """Everything here is refused before any launch: no GPU is touched, the device entry points included."""
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    E_ARG = -1
    T, H = 4, 64
    f = np.zeros((2, T, H), dtype=np.float32)
    out = np.zeros((2, T, H), dtype=np.float32)
    ln = np.array([1, 4], dtype=np.int32)
    lo, hi = np.array([1, 1], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    dist = np.zeros((2, 2), dtype=np.float32)
    idx = np.zeros((2, 256), dtype=np.int32)
    val = np.zeros((2, 256), dtype=np.float32)
    p = lambda a: a.ctypes.data  # noqa: E731
    big = np.zeros((2, 65, 64), dtype=np.float32)

    # shapes: T = 0 / 65, H = 0 / 32 / 96 / 576, negative counts, N T H >= 2^31 (only sizes are read)
    for (N, t, h) in ((2, 0, H), (2, 65, H), (2, T, 0), (2, T, 32), (2, T, 96), (2, T, 576), (-1, T, H), (1 << 16, 64, 512)):
        assert L.msocr_frame_normalize_host(p(big), p(ln), N, t, h, p(big)) == E_ARG
        assert L.msocr_frame_normalize(p(big), p(ln), N, t, h, p(big), None) == E_ARG
        assert L.msocr_dtw_distances_host(p(big), p(ln), p(lo), p(hi), 2, p(big), p(ln), N, t, h, p(dist)) == E_ARG
        assert L.msocr_dtw_distances(p(big), p(ln), p(lo), p(hi), 2, p(big), p(ln), N, t, h, p(dist), None) == E_ARG
        assert L.msocr_dtw_distances_host(p(big), p(ln), p(lo), p(hi), N, p(big), p(ln), 2, t, h, p(dist)) == E_ARG
        assert L.msocr_dtw_distances(p(big), p(ln), p(lo), p(hi), N, p(big), p(ln), 2, t, h, p(dist), None) == E_ARG
    # null pointers
    assert L.msocr_frame_normalize_host(None, p(ln), 2, T, H, p(out)) == E_ARG
    assert L.msocr_frame_normalize_host(p(f), None, 2, T, H, p(out)) == E_ARG
    assert L.msocr_frame_normalize_host(p(f), p(ln), 2, T, H, None) == E_ARG
    assert L.msocr_frame_normalize(p(f), p(ln), 2, T, H, None, None) == E_ARG
    args = [p(f), p(ln), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist)]
    assert L.msocr_dtw_distances_host(*args) == 0
    for k in (0, 1, 2, 3, 5, 6, 10):
        bad = list(args)
        bad[k] = None
        assert L.msocr_dtw_distances_host(*bad) == E_ARG
        assert L.msocr_dtw_distances(*bad, None) == E_ARG
    # unit frames that are not 16-byte aligned (device route)
    raw = np.zeros(2 * T * H + 1, dtype=np.float32)
    off = raw[1:] if raw.ctypes.data % 16 == 0 else raw[:-1]
    assert off.ctypes.data % 16 != 0
    assert L.msocr_dtw_distances(p(off), p(ln), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist), None) == E_ARG
    # lengths outside [1, T] and len_lo > len_hi (the host twin can read them)
    for bad_len in ([0, 4], [1, 5], [-3, 1]):
        b = np.array(bad_len, dtype=np.int32)
        assert L.msocr_dtw_distances_host(p(f), p(b), p(lo), p(hi), 2, p(f), p(ln), 2, T, H, p(dist)) == E_ARG
        assert L.msocr_dtw_distances_host(p(f), p(ln), p(lo), p(hi), 2, p(f), p(b), 2, T, H, p(dist)) == E_ARG
    assert L.msocr_dtw_distances_host(p(f), p(ln), p(hi), p(lo), 2, p(f), p(ln), 2, T, H, p(dist)) == E_ARG
    # the selection: k = 0 / 257, negative counts, null pointers
    for (Q, N, k) in ((2, 2, 0), (2, 2, 257), (2, 2, -1), (-1, 2, 1), (2, -1, 1)):
        assert L.msocr_topk_smallest_host(p(dist), Q, N, k, p(idx), p(val)) == E_ARG
        assert L.msocr_topk_smallest(p(dist), Q, N, k, p(idx), p(val), None) == E_ARG
    assert L.msocr_topk_smallest_host(None, 2, 2, 1, p(idx), p(val)) == E_ARG
    assert L.msocr_topk_smallest_host(p(dist), 2, 2, 1, None, p(val)) == E_ARG
    assert L.msocr_topk_smallest_host(p(dist), 2, 2, 1, p(idx), None) == E_ARG
    assert L.msocr_topk_smallest(p(dist), 2, 2, 1, None, p(val), None) == E_ARG
    # nothing to do is fine: no word, no query
    assert L.msocr_dtw_distances_host(p(f), p(ln), p(lo), p(hi), 0, p(f), p(ln), 2, T, H, p(dist)) == 0
    assert L.msocr_dtw_distances_host(p(f), p(ln), p(lo), p(hi), 2, p(f), p(ln), 0, T, H, p(dist)) == 0
    assert L.msocr_frame_normalize_host(p(f), p(ln), 0, T, H, p(out)) == 0


# ------------------------------------------------------------------------------------------------ WordIndex
def hand_index(device=None):
    """twelve words on two pages: word (1, 0, 2) is word (0, 0, 1) with every frame repeated twice, (1, 1, 0) is (0, 0, 1) again"""
    from manuscript_ocr_amd import WordIndex
    rng = np.random.default_rng(8)
    T, H = 16, 64
    lens = [5, 6, 3, 8, 16, 1, 2, 7, 12, 6, 9, 4]
    ids = [(0, 0, w) for w in range(6)] + [(1, 0, w) for w in range(3)] + [(1, 1, w) for w in range(3)]
    feat, lens = random_words(rng, 12, T, H, lens)
    feat[8, :12] = np.repeat(feat[1, :6], 2, axis=0)
    feat[9] = feat[1]
    texts = [f"w{i}" if i % 2 else None for i in range(12)]
    return WordIndex.from_features(feat, lens, ids, texts=texts, device=device), feat, lens, ids, texts


def test_word_index_from_features_and_spot():
    from manuscript_ocr_amd.detectors._types import SpotHit
    index, feat, lens, ids, texts = hand_index()
    assert len(index) == 12 and index.device is None and index.pages == 2
    assert index.nbytes == 12 * (16 * 64 * 4 + 4)
    unit = yard_unit(feat, lens)
    # a reference query finds itself at rank 0 with distance about 0; its copy and its stretched copy follow
    hits = index.spot([(0, 0, 1), (1, 1, 2)], k=4, max_length_ratio=2.0)
    assert len(hits) == 2 and all(isinstance(h, SpotHit) for h in hits[0])
    first = hits[0]
    # (the three distances are rounding noise around 0, so their order among themselves says nothing, but for the identical copy:
    # equal frames give equal bits, and the tie goes to the word that entered first)
    where = [(h.page, h.block, h.word) for h in first[:3]]
    assert sorted(where) == [(0, 0, 1), (1, 0, 2), (1, 1, 0)] and where.index((0, 0, 1)) < where.index((1, 1, 0))
    assert all(abs(h.distance) <= bound(64, 6, 12) for h in first[:3]) and first[3].distance > 0.1
    assert [h.rank for h in first] == [0, 1, 2, 3] and all(h.query == 0 for h in first)
    assert {(h.word, h.text) for h in first[:3]} == {(1, "w1"), (0, "w9"), (2, None)}
    assert (hits[1][0].page, hits[1][0].block, hits[1][0].word) == (1, 1, 2) and hits[1][0].query == 1
    # ordering: ascending distance, the gate respected, against the yardstick
    for q, ref in enumerate([(0, 0, 1), (1, 1, 2)]):
        row = ids.index(ref)
        lo, hi = -(-int(lens[row]) // 2), min(2 * int(lens[row]), 16)
        want = yard_all(unit[row:row + 1], lens[row:row + 1], [lo], [hi], unit, lens)[0]
        got = hits[q]
        assert [h.distance for h in got] == sorted(h.distance for h in got)
        for h in got:
            n = ids.index((h.page, h.block, h.word))
            assert lo <= lens[n] <= hi and abs(h.distance - want[n]) <= bound(64, lens[row], lens[n])
        assert len(got) == min(4, int(np.isfinite(want).sum()))
    # max_length_ratio=None compares with everything; k beyond the index returns every word once
    everything = index.spot([(0, 0, 5)], k=256, max_length_ratio=None)[0]
    assert sorted((h.page, h.block, h.word) for h in everything) == sorted(ids)
    gated = index.spot([(0, 0, 5)], k=256, max_length_ratio=2.0)[0]       # one frame: words of 1 .. 2 frames
    assert sorted((h.page, h.block, h.word) for h in gated) == [(0, 0, 5), (1, 0, 0)]
    # queries as frames
    by_frames = index.spot_features(feat[[1]], lens[[1]], k=4)
    assert [(h.page, h.block, h.word) for h in by_frames[0]] == [(h.page, h.block, h.word) for h in first]
    # the index grows; ids stay distinct; shapes must agree; an image query needs a recogniser
    index.add_features(feat[:1], lens[:1], [(2, 0, 0)])
    assert len(index) == 13 and index.pages == 3
    assert (lambda h: (h.page, h.word))(index.spot([(2, 0, 0)], k=1)[0][0]) == (0, 0)   # its twin entered first
    with pytest.raises(ValueError):
        index.add_features(feat[:1], lens[:1], [(0, 0, 0)])
    with pytest.raises(ValueError):
        index.add_features(np.zeros((1, 8, 64), dtype=np.float32), [1], [(5, 0, 0)])
    with pytest.raises(KeyError):
        index.spot([(9, 9, 9)])
    with pytest.raises(TypeError):
        index.spot([np.zeros((20, 40, 3), dtype=np.uint8)])
    for bad_k in (0, 257):
        with pytest.raises(ValueError):
            index.spot([(0, 0, 0)], k=bad_k)
    assert index.spot([]) == []


def words_for_blocks():
    """23 words of T = 6, H = 64 and 7 queries.  Word 17 is word 3 again and query 2 is the same frames, so that its two nearest
    words tie bit for bit; with five words to a block they lie in blocks 0 and 3."""
    rng = np.random.default_rng(9)
    T, H = 6, 64
    feat, lens = random_words(rng, 23, T, H)
    feat[17], lens[17] = feat[3], lens[3]
    ids = [(n // 10, n % 2, n) for n in range(23)]
    texts = [f"w{n}" if n % 3 else None for n in range(23)]
    fq, ql = random_words(rng, 7, T, H, [6, 1, 3, 5, 2, 6, 4])
    fq[2], ql[2] = feat[3], lens[3]
    return feat, lens, ids, texts, fq, ql


def hit_rows(per_query):
    """what a caller sees of the hits, the distance as its f32 bits"""
    return [[(h.query, h.page, h.block, h.word, h.rank, h.text, np.float32(h.distance).tobytes()) for h in hits] for hits in per_query]


def spot_in_blocks_and_in_one(monkeypatch, device):
    """The words of `words_for_blocks` enter an index in pieces of 3, 9 and 11, once under the default limit of a native call (one
    block, one call) and once with room for five words per call: blocks of 5, 5, 5, 5, 3, joined from the pieces across their
    edges, and the 7 queries cut into 5 + 2.  Both indexes answer the same questions, by frames and by reference (a word of the last
    block, both tied words), and must give the same hits: ids, ranks, texts, and distances bit for bit.
    -> the hits of the frame queries without a length gate, k = 23, from the index in blocks"""
    from manuscript_ocr_amd import WordIndex, _spotting
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
        return [index.spot_features(fq, ql, k=23, max_length_ratio=None), index.spot_features(fq, ql, k=4), index.spot(refs, k=6),
                index.spot(refs + [ids[9]], k=256, max_length_ratio=1.5)]

    one = build()
    want = ask(one)
    assert [int(u.shape[0]) for u, _ in one._blocks] == [23]
    monkeypatch.setattr(_spotting, "_LIMIT", 5 * T * H)
    cut = build()
    got = ask(cut)
    assert [int(u.shape[0]) for u, _ in cut._blocks] == [5, 5, 5, 5, 3] and len(cut) == 23
    assert [int(l.shape[0]) for _, l in cut._blocks] == [5, 5, 5, 5, 3]
    for g, w in zip(got, want):
        assert hit_rows(g) == hit_rows(w)
    everything = got[0]
    assert all(len(hits) == 23 for hits in everything)                       # no gate: every word once, whichever block holds it
    assert all(sorted(h.word for h in hits) == list(range(23)) for hits in everything)
    # the tie across the block edge: the word that entered first wins, from the frames and from either reference
    for hits in (everything[2], got[2][1], got[2][2]):
        assert [(h.word, h.rank) for h in hits[:2]] == [(3, 0), (17, 1)] and hits[0].distance == hits[1].distance
        assert abs(hits[0].distance) <= bound(H, lens[3], lens[3]) < 0.01 < hits[2].distance
    # a reference into the last block (frames_of walks the blocks) finds itself
    for q, n in ((0, 21), (4, 22), (5, 20)):
        assert got[2][q][0].word == n and abs(got[2][q][0].distance) <= bound(H, lens[n], lens[n])
    return everything


def test_word_index_in_several_blocks(monkeypatch):
    """The host route of an index and a query set beyond one native call: the first test in which
    WordIndex._pack begins a second block and joins pieces across block edges, in which frames_of walks past the first block, and in
    which spot_features joins the [Q', n] parts of several calls, here 2 x 5, into one [Q, N] array."""
    everything = spot_in_blocks_and_in_one(monkeypatch, None)
    feat, lens, _ids, _texts, fq, ql = words_for_blocks()
    want = yard_all(yard_unit(fq, ql), ql, *full_gate(7, 6), yard_unit(feat, lens), lens)
    for q, hits in enumerate(everything):
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        for h in hits:
            assert abs(h.distance - want[q, h.word]) <= bound(64, ql[q], lens[h.word])


def test_empty_index_and_exports():
    import manuscript_ocr_amd
    from manuscript_ocr_amd import Pipeline, WordIndex
    from manuscript_ocr_amd.recognizers import TRBA
    assert "WordIndex" in manuscript_ocr_amd.__all__
    empty = WordIndex()
    assert len(empty) == 0 and empty.nbytes == 0
    assert empty.spot_features(np.zeros((2, 4, 64), dtype=np.float32), [1, 2]) == [[], []]
    for name in ("index_words", "spot"):
        assert callable(getattr(Pipeline, name))
    for name in ("embed", "embed_canvases"):
        assert callable(getattr(TRBA, name))
    with pytest.raises(TypeError):
        Pipeline(detector=object(), recognizer=object()).index_words([], pages=[])


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_header_under_the_sanitizers(tmp_path):
    """csrc/word_spotting.h (the frame rule, the f32 sum's order, the f64 table, the gate, the ordering key and the selection, with
    the checks every entry point makes) in a plain C++ program of its own (tests/native/word_spotting_fuzz.cpp) with the address and
    undefined-behaviour sanitizers: garbage lengths, non-finite features, every array in a heap block of its exact size, every
    result compared with a plain table and a plain sort.  Run as a child process; nothing is loaded into this one."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no clang++ with sanitizer runtimes here")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "word_spotting_fuzz"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "manuscript_ocr_amd", "csrc"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "word_spotting_fuzz.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("rounds 300 checked 300")
