"""Word spotting on the MI355X (include/msocr.h, "word spotting"): msocr_frame_normalize and
msocr_dtw_distances against the f64 yardsticks of tests/test_word_spotting_cpu.py, msocr_topk_smallest against its host twin bit for
bit, and a WordIndex built through Pipeline on a synthetic page.

The bound of the distance, derived and not fitted.  Both sides start from the same raw f32 frames.
  * For unit vectors any f32 summation order of <u, v> errs by at most gamma_H <= H 2^-24 (|sum |u_k v_k|| <= 1 by Cauchy-Schwarz).
  * The device's unit frames are off the true ones by at most (H + 4) 2^-24 in length and direction each (the f32 sum of squares,
    the root, the quotient), which moves <u, v> by at most (H + 4) 2^-24 per operand.
  * So a local cost errs by at most (3 H + 8) 2^-24.  A warping path visits at most Lq + Ln - 1 cells and d divides the path's sum
    by Lq + Ln, so the costs' share of the error of d stays below (3 H + 8) 2^-24; the minimum over paths of perturbed sums moves
    by no more than the largest perturbation of a path.
  * The table's own f32 additions: at most Lq + Ln - 1 of them on a path, each rounding a value <= 2 (Lq + Ln) relatively by
    2^-24; divided by Lq + Ln that is at most 2 (Lq + Ln) 2^-24, and the subtraction 1 - acc and the division add a few 2^-24.
  |d_dev - d_f64| <= (3 H + 2 (Lq + Ln) + 16) 2^-24.
The device forms the products with the exact f32 matrix instruction, so there is no split-operand term.  A wrong frame, a length off
by one or a padded row leaking into the table lands orders of magnitude above this (costs differ by ~1 / (Lq + Ln)).

Beside every assert the ratio of the device's largest error to that of a NumPy f32 evaluation of the same case is printed
(DESIGN.md section 4.25 records it); it is not asserted."""
import numpy as np
import pytest
import torch

from test_word_spotting_cpu import (EPS, bound, full_gate, random_words, same_bits, spot_in_blocks_and_in_one, words_for_blocks, yard_all,
                                    yard_topk, yard_unit)

pytestmark = pytest.mark.gpu

CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import _native as nat
    nat.lib()
    return torch.device("cuda")


def tile():
    from manuscript_ocr_amd import ops
    return ops.SPOT_TILE


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def device_from_raw(fq, ql, lo, hi, fc, cl):
    from manuscript_ocr_amd import ops
    qlen, clen = dev(ql, np.int32), dev(cl, np.int32)
    uq, uc = ops.frame_normalize(dev(fq), qlen), ops.frame_normalize(dev(fc), clen)
    d = ops.dtw_distances(uq, qlen, dev(lo, np.int32), dev(hi, np.int32), uc, clen)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def nan_behind(feat, lengths):
    for n in range(len(lengths)):
        feat[n, lengths[n]:] = np.nan      # never written by the caller, never read by the kernels
    return feat


def yard_sliced(qu, ql, lo, hi, cu, cl, dtype=np.float64, words=256):
    """yard_all over the corpus in slices of `words` words, so that its [Q, n, T, T] table stays small; a pair's value does not
    depend on the slice it is in"""
    if len(cl) <= words:
        return yard_all(qu, ql, lo, hi, cu, cl, dtype)
    return np.concatenate([yard_all(qu, ql, lo, hi, cu[s:s + words], cl[s:s + words], dtype) for s in range(0, len(cl), words)], axis=1)


def check_against_yardstick(fq, ql, lo, hi, fc, cl, what):
    H = fq.shape[2]
    got = device_from_raw(fq, ql, lo, hi, fc, cl)
    want = yard_sliced(yard_unit(fq, ql), ql, lo, hi, yard_unit(fc, cl), cl)
    f32 = yard_sliced(yard_unit(fq, ql, np.float32), ql, lo, hi, yard_unit(fc, cl, np.float32), cl, np.float32)
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, want, 0)), 0.0)
    lim = bound(H, np.asarray(ql)[:, None], np.asarray(cl)[None, :])
    if fin.any():
        e32 = float(np.where(fin, np.abs(np.where(fin, f32, 0) - np.where(fin, want, 0)), 0.0).max())
        print(f"{what}: device err {err.max():.3e}, worst err/bound {float((err / lim).max()):.3f}, "
              f"NumPy-f32 err {e32:.3e}, device / NumPy-f32 {err.max() / e32 if e32 else float('nan'):.2f}")
    assert (err <= lim).all(), (what, float(err.max()), float((err / lim).max()))
    return got, want


# ------------------------------------------------------------------------------------------------ msocr_frame_normalize
@pytest.mark.parametrize("H", [64, 256, 512])
def test_frame_normalize(cuda, H):
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(20 + H)
    T = 7
    feat, lengths = random_words(rng, 9, T, H, [7, 4, 1, 7, 7, 7, 2, 6, 7])   # 63 frames: the last workgroup is partial
    feat[0, 1] = 0.0
    feat[0, 2, 7] = np.nan
    feat[3, 0, H - 1] = np.inf
    feat[3, 1] = 1e30
    feat[3, 2] = 1e-30
    feat[4, 3] *= 1e18
    feat[4, 4] *= 1e-18
    nan_behind(feat, lengths)
    unit = ops.frame_normalize(dev(feat), dev(lengths)).cpu().numpy()
    assert np.isfinite(unit).all()
    for n, t in ((0, 1), (0, 2), (3, 0), (3, 1), (3, 2)):
        assert not unit[n, t].any()
    for n in range(9):
        assert not unit[n, lengths[n]:].any()
    want = yard_unit(feat, lengths)
    nz = np.abs(want).sum(axis=2) > 0
    assert np.array_equal(nz, np.abs(unit).sum(axis=2) > 0)
    norm = np.sqrt((unit.astype(np.float64) ** 2).sum(axis=2))
    print(f"H {H}: | ||u|| - 1 | max {np.abs(norm[nz] - 1.0).max():.3e}, bound {(H + 4) * EPS:.3e}")
    assert np.abs(norm[nz] - 1.0).max() <= (H + 4) * EPS
    assert np.abs(unit - want).max() <= (H + 4) * EPS
    # the host twin sums in the same order
    assert np.abs(unit - ops.frame_normalize_host(feat, lengths)).max() <= 2 * EPS
    # in place, and lengths outside [0, T] are clamped
    x = dev(feat)
    assert ops.frame_normalize(x, dev(lengths), out=x) is x and same_bits(x.cpu().numpy(), unit)
    odd = ops.frame_normalize(dev(feat[:2]), dev(np.array([-5, T + 9], dtype=np.int32))).cpu().numpy()
    assert not odd[0].any() and same_bits(odd[1, :lengths[1]], unit[1, :lengths[1]]) and not np.isfinite(feat[1, lengths[1]:]).any()
    assert ops.frame_normalize(dev(feat[:0]), dev(lengths[:0])).shape == (0, T, H)


# ------------------------------------------------------------------------------------------------ msocr_dtw_distances
@pytest.mark.parametrize("H", [64, 256, 512])
@pytest.mark.parametrize("T", [1, 2, 33, 64])
def test_dtw_grid_of_shapes(cuda, T, H):
    """lengths 1, 2, T - 1, T on both sides and ragged lengths inside one tile, 3 tiles + 7 words, NaN behind every length"""
    rng = np.random.default_rng(1000 * T + H)
    edge = sorted({1, min(2, T), max(T - 1, 1), T})
    N = 3 * tile() + 7
    fq, ql = random_words(rng, len(edge), T, H, edge)
    fc, cl = random_words(rng, N, T, H, (edge + list(rng.integers(1, T + 1, N)))[:N])
    nan_behind(fq, ql), nan_behind(fc, cl)
    check_against_yardstick(fq, ql, *full_gate(len(ql), T), fc, cl, f"T {T} H {H}")


@pytest.mark.parametrize("T,H", [(33, 256), (64, 64)])
@pytest.mark.parametrize("Q", [1, 3, 65])
def test_dtw_counts_around_the_tile(cuda, Q, T, H):
    rng = np.random.default_rng(7 * Q + T)
    t = tile()
    for N in sorted({1, max(t - 1, 1), t, t + 1, 3 * t + 7}):
        fq, ql = random_words(rng, Q, T, H)
        fc, cl = random_words(rng, N, T, H)
        ql[0], cl[-1] = T, T
        nan_behind(fq, ql), nan_behind(fc, cl)
        lo, hi = np.maximum(ql // 2, 1).astype(np.int32), np.minimum(ql * 2, T).astype(np.int32)
        check_against_yardstick(fq, ql, lo, hi, fc, cl, f"Q {Q} N {N} T {T} H {H}")


def test_dtw_gate_and_identities(cuda):
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(5)
    T, H = 33, 256
    t = tile()
    N = 2 * t + 3
    # the only admissible word is the last one; then nothing is admissible
    fq, ql = random_words(rng, 2, T, H, [10, 20])
    fc, cl = random_words(rng, N, T, H, [5] * (N - 1) + [12])
    nan_behind(fq, ql), nan_behind(fc, cl)
    got, _ = check_against_yardstick(fq, ql, [12, 12], [12, 33], fc, cl, "only the last word")
    assert np.isinf(got[:, :-1]).all() and np.isfinite(got[:, -1]).all()
    got, _ = check_against_yardstick(fq, ql, [6, 13], [11, 33], fc, cl, "nothing admissible")
    assert np.isinf(got).all()
    # at len_lo, at len_hi and one outside each
    fc, cl = random_words(rng, 4, T, H, [4, 5, 9, 10])
    got, _ = check_against_yardstick(fq[:1], ql[:1], [5], [9], nan_behind(fc, cl), cl, "gate edges")
    assert np.array_equal(np.isfinite(got[0]), [False, True, True, False])
    # a length outside [1, T] cannot be refused on the device: its pairs are gated out
    cl_bad = np.array([0, 5, T + 1, -7], dtype=np.int32)
    ql_bad = np.array([10, 0], dtype=np.int32)
    uq = ops.frame_normalize(dev(fq), dev(ql_bad))
    uc = ops.frame_normalize(dev(np.nan_to_num(fc)), dev(cl_bad))
    d = ops.dtw_distances(uq, dev(ql_bad), dev([1, 1], np.int32), dev([T, T], np.int32), uc, dev(cl_bad)).cpu().numpy()
    assert np.array_equal(np.isfinite(d), [[False, True, False, False], [False] * 4])
    # itself, a copy with every frame twice, orthogonal one-hot frames, zero and non-finite frames
    L = 16
    x = rng.standard_normal((L, H)).astype(np.float32)
    fc = np.full((4, T, H), np.nan, dtype=np.float32)
    fc[0, :L] = x
    fc[1, :2 * L] = np.repeat(x, 2, axis=0)
    fc[2, :T] = 0.0
    fc[2, np.arange(T), np.arange(T)] = 2.0
    fc[3, :3] = x[:3]
    fc[3, 1] = 0.0
    fc[3, 2, 5] = np.inf
    cl = np.array([L, 2 * L, T, 3], dtype=np.int32)
    fq = np.full((2, T, H), np.nan, dtype=np.float32)
    fq[0, :L] = x
    fq[1, :9] = 0.0
    fq[1, np.arange(9), 100 + np.arange(9)] = 0.5
    ql = np.array([L, 9], dtype=np.int32)
    got, _ = check_against_yardstick(fq, ql, *full_gate(2, T), fc, cl, "identities")
    assert abs(got[0, 0]) <= bound(H, L, L) and abs(got[0, 1]) <= bound(H, L, 2 * L)
    assert got[1, 2] == np.float32(T / (9 + T))      # every cell costs exactly 1
    # no query, no word
    e = ops.dtw_distances(uq[:0], dev(ql_bad[:0]), dev(ql_bad[:0]), dev(ql_bad[:0]), uc, dev(cl_bad))
    assert e.shape == (0, 4)
    e = ops.dtw_distances(uq, dev(ql_bad), dev(ql_bad), dev(ql_bad), uc[:0], dev(cl_bad[:0]))
    assert e.shape == (2, 0)


# ------------------------------------------------------------------------------------------------ launch geometry
# msocr_dtw_distances sizes its grid from the CU count: tiles of 4 words by `rows` query rows, about four workgroups per CU, and a
# workgroup walks the queries q = blockIdx.y, blockIdx.y + rows, ..  At the sizes above rows = Q, one query per workgroup.  The tests
# below read the CU count, restate the host's formula and assert the geometry they are there for, so on a part with another CU
# count they either still enter their path or fail and say so.
def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def grid_rows(Q, N, cu):
    """gridDim.y of ws_dtw_kernel as msocr_dtw_distances sets it"""
    tiles = -(-N // tile())
    return max(1, min(Q, 65535, -(-4 * cu // tiles)))


def check_rows_alone(fq, ql, lo, hi, fc, cl, got, what):
    """Row q of the batched result against a call that holds query q alone (its workgroups then handle it first, on a fresh LDS
    tile and fresh wavefront registers): nothing in a pair's arithmetic depends on the query its workgroup handled before, so the
    two agree bit for bit."""
    from manuscript_ocr_amd import ops
    qlen, clen, lo_d, hi_d = dev(ql, np.int32), dev(cl, np.int32), dev(lo, np.int32), dev(hi, np.int32)
    uq, uc = ops.frame_normalize(dev(fq), qlen), ops.frame_normalize(dev(fc), clen)
    alone = torch.cat([ops.dtw_distances(uq[q:q + 1], qlen[q:q + 1], lo_d[q:q + 1], hi_d[q:q + 1], uc, clen) for q in range(len(ql))])
    torch.cuda.synchronize()
    alone = alone.cpu().numpy()
    bad = np.argwhere(alone.view(np.uint32) != got.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), [(float(got[q, n]), float(alone[q, n])) for q, n in bad[:8]])


def test_dtw_one_grid_row_walks_all_queries(cuda):
    """rows = 1, the geometry of any index of real size: the first test in which a workgroup of ws_dtw_kernel takes a second trip of
    `for (q = blockIdx.y; q < Q; q += gridDim.y)`, so the first to reuse a wave's LDS cost tile for the next query (the
    ws_wave_lds_order() at the loop's head) and to reset d1 / up_prev between queries.  Query lengths T, 1, T - 1, 2, T: a short
    query follows a long one on the same tile, whose cells outside Lq x Ln are the long one's.  The gates skip pairs between
    computed ones (the `continue` arm leaves the tile as it was).  16 cu words of ragged lengths, NaN behind every length."""
    cu = cu_count()
    T, H, Q = 8, 64, 5
    N = 16 * cu
    assert grid_rows(Q, N, cu) == 1
    rng = np.random.default_rng(61)
    fq, ql = random_words(rng, Q, T, H, [T, 1, T - 1, 2, T])
    fc, cl = random_words(rng, N, T, H, (list(range(1, T + 1)) + list(rng.integers(1, T + 1, N)))[:N])
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo, hi = np.array([1, 1, 4, 1, 3], dtype=np.int32), np.array([T, 4, T, 2, T], dtype=np.int32)
    got, _ = check_against_yardstick(fq, ql, lo, hi, fc, cl, f"rows 1: Q {Q} N {N} T {T} H {H}")
    for n in (2, 5, N - 1):      # words of 3 and of 6 frames: skipped pairs between computed ones
        L = int(cl[n])
        assert np.isfinite(got[:, n]).tolist() == [lo[q] <= L <= hi[q] for q in range(Q)]
    assert np.isfinite(got[:, 2]).tolist() == [True, True, False, False, True]
    assert np.isfinite(got[:, 5]).tolist() == [True, False, True, False, True]
    check_rows_alone(fq, ql, lo, hi, fc, cl, got, "rows 1")


@pytest.mark.parametrize("T,H", [(33, 256), (64, 64)])
def test_dtw_a_few_queries_per_workgroup(cuda, T, H):
    """1 < rows < Q: a workgroup of ws_dtw_kernel handles the queries blockIdx.y, blockIdx.y + rows, ..: the stride of the query
    loop is neither 1 nor Q.  At (33, 256) the tile's pitch is T + 1, at (64, 64) it is T and all 64 lanes are rows of the
    wavefront; 4 cu + 3 words, so the last tile is partial.  The reuse of the tile and of the wavefront registers as in the test
    above, at two blocks of the cost tile per side."""
    cu = cu_count()
    Q, N = 9, 4 * cu + 3
    rows = grid_rows(Q, N, cu)
    assert 1 < rows < Q, (rows, cu)
    rng = np.random.default_rng(62 + T)
    fq, ql = random_words(rng, Q, T, H, [T, 1, T - 1, 2, T, T // 2 + 1, 5, T // 2, 9])
    fc, cl = random_words(rng, N, T, H)
    cl[:4] = [T, 1, T - 1, 2]
    cl[-1] = T
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo, hi = np.maximum(ql // 2, 1).astype(np.int32), np.minimum(ql * 2, T).astype(np.int32)
    lo[4], hi[4] = 1, T
    got, _ = check_against_yardstick(fq, ql, lo, hi, fc, cl, f"rows {rows}: Q {Q} N {N} T {T} H {H}")
    assert np.isinf(got).any() and np.isfinite(got[4]).all()
    check_rows_alone(fq, ql, lo, hi, fc, cl, got, f"rows {rows} T {T}")


def test_dtw_many_queries_one_partial_tile(cuda):
    """rows < Q with a single tile of three words: the fourth wave of every workgroup returns before the query loop while the other
    three take two trips of it (the kernel has no block-wide barrier for it to miss)."""
    cu = cu_count()
    T, H, N = 2, 64, 3
    Q = 4 * cu + 5
    rows = grid_rows(Q, N, cu)
    assert rows < Q, (rows, cu)
    rng = np.random.default_rng(63)
    fq, ql = random_words(rng, Q, T, H)
    fc, cl = random_words(rng, N, T, H, [2, 1, 2])
    nan_behind(fq, ql), nan_behind(fc, cl)
    lo = np.ones(Q, dtype=np.int32)
    hi = np.where(np.arange(Q) % 7 == 3, 1, T).astype(np.int32)
    got, _ = check_against_yardstick(fq, ql, lo, hi, fc, cl, f"rows {rows}: Q {Q} N {N} T {T} H {H}")
    assert np.isfinite(got[:, 1]).all() and np.array_equal(np.isfinite(got[:, 0]), hi == T)


def test_frame_normalize_beyond_one_trip_of_the_grid(cuda):
    """The first test in which ws_normalize_kernel takes a second trip of its grid-stride loop (f += stride): the grid is capped at
    32 cu workgroups of 4 frames, and N T frames lie above 128 cu.  Ragged lengths with 0 and T among them, NaN behind them, and a
    zero frame, non-finite frames and overflowing frames among the words behind frame 128 cu: the second trip sees the zero rule
    and the frames behind a length too.  The asserts are those of test_frame_normalize."""
    from manuscript_ocr_amd import ops
    cu = cu_count()
    T, H = 7, 64
    first = -(-128 * cu // T)            # the first word whose frames all lie in the second trip
    N = first + 5
    assert N * T > 128 * cu and first * T >= 128 * cu
    rng = np.random.default_rng(64)
    feat, lengths = random_words(rng, N, T, H, rng.integers(0, T + 1, N))
    lengths[:3] = [T, 0, 3]
    lengths[first:] = [T, T, 0, 4, T]
    special = []
    for w in (0, first):
        feat[w, 1] = 0.0
        feat[w, 2, 7] = np.nan
        feat[w, 3, H - 1] = np.inf
        feat[w, 4] = 1e30
        feat[w, 5] = 1e-30
        feat[w + (N - 1 - first if w else 2), 1] *= 1e18      # words of T and of 3 frames: finite, far from 1
        special += [(w, t) for t in (1, 2, 3, 4, 5)]
    feat[first + 1, 6] *= 1e-18
    nan_behind(feat, lengths)
    unit = ops.frame_normalize(dev(feat), dev(lengths)).cpu().numpy()
    assert np.isfinite(unit).all()
    for n, t in special:
        assert not unit[n, t].any()
    behind = np.arange(T)[None, :] >= lengths[:, None]
    assert not unit[behind].any()
    want = yard_unit(feat, lengths)
    nz = np.abs(want).sum(axis=2) > 0
    assert np.array_equal(nz, np.abs(unit).sum(axis=2) > 0)
    assert nz[first:].sum() == 3 * T - 5 + 4 and nz[first + 4, 1] and nz[first + 1, 6]
    norm = np.sqrt((unit.astype(np.float64) ** 2).sum(axis=2))
    err = np.abs(unit - want).max()
    print(f"second trip, N {N} T {T} H {H}: | ||u|| - 1 | max {np.abs(norm[nz] - 1.0).max():.3e}, |u - yardstick| max {err:.3e}, "
          f"bound {(H + 4) * EPS:.3e}, worst err/bound {err / ((H + 4) * EPS):.3f}")
    assert np.abs(norm[nz] - 1.0).max() <= (H + 4) * EPS
    assert err <= (H + 4) * EPS
    host = ops.frame_normalize_host(feat, lengths)
    print(f"second trip: device against the host twin {np.abs(unit - host).max():.3e}, bound {2 * EPS:.3e}")
    assert np.abs(unit - host).max() <= 2 * EPS


# ------------------------------------------------------------------------------------------------ msocr_topk_smallest
def same_as_host_topk(dist, k):
    from manuscript_ocr_amd import ops
    idx, val = ops.topk_smallest(dev(dist), k)
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    hidx, hval = ops.topk_smallest_host(dist, k)
    assert np.array_equal(idx, hidx), (k, dist.shape)
    assert same_bits(val, hval), (k, dist.shape)
    return idx, val


def test_topk_on_device_distances(cuda):
    rng = np.random.default_rng(31)
    T, H = 33, 64
    fq, ql = random_words(rng, 5, T, H)
    fc, cl = random_words(rng, 300, T, H)
    fc[150:160] = fc[10:20]                      # equal words: equal bits, ties by index
    cl[150:160] = cl[10:20]
    lo, hi = np.maximum(ql // 2, 1).astype(np.int32), np.minimum(ql * 2, T).astype(np.int32)
    dist = device_from_raw(fq, ql, lo, hi, fc, cl)
    assert np.isinf(dist).any() and np.isfinite(dist).any()
    for k in (1, 7, 64, 256):
        idx, val = same_as_host_topk(dist, k)
        widx, wval = yard_topk(dist, k)
        assert np.array_equal(idx, widx) and same_bits(val, wval)


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 1000, 70001])
def test_topk_constructed(cuda, N):
    rng = np.random.default_rng(40 + N)
    inf = np.float32(np.inf)
    rows = [
        rng.standard_normal(N).astype(np.float32),
        np.full(N, 0.5, dtype=np.float32),                                           # all equal
        np.full(N, inf, dtype=np.float32),                                           # nothing finite
        np.where(np.arange(N) % 7 == 3, rng.random(N), np.inf).astype(np.float32),
        np.where(np.arange(N) % 2 == 0, 0.0, -0.0).astype(np.float32),               # -0.0 == 0.0
        rng.integers(-3, 4, N).astype(np.float32),                                   # many ties around the k-th value
        np.where(rng.random(N) < 0.3, np.nan, rng.integers(0, 3, N)).astype(np.float32),
        np.concatenate([[-np.inf, np.inf, np.nan], -rng.random(max(N - 3, 0))])[:N].astype(np.float32),
        (rng.integers(0, 2, N) * np.float32(1e-45)).astype(np.float32),              # subnormals and zeros
    ]
    dist = np.stack(rows)
    for k in (1, 3, 256):
        idx, val = same_as_host_topk(dist, k)
        widx, wval = yard_topk(dist, k)
        assert np.array_equal(idx, widx) and same_bits(val, wval)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def rec(cuda):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


def test_embed(cuda, rec):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers._trba.transforms import FRAME_STRIDE
    crops = [np.ascontiguousarray(x) for x in synth.synth_crops(1, 5, 32, 100)]
    crops[1] = np.ascontiguousarray(crops[1][:, :60])     # padding on the canvas: fewer frames
    crops[2] = np.ascontiguousarray(crops[2][:, :7])
    feat, lengths = rec.embed(crops)
    T = feat.shape[1]
    assert feat.shape == (5, T, 256) and feat.dtype == torch.float32 and feat.is_cuda and lengths.dtype == np.int32
    assert lengths.tolist() == [min(T, w // FRAME_STRIDE + 1) for w in (100, 60, 7, 100, 100)]
    same, _ = rec.model.encode(torch.from_numpy(rec._canvases(crops)).cuda())
    assert torch.equal(feat, same)
    one, l1 = rec.embed(crops[1])
    assert one.shape == (1, T, 256) and l1.tolist() == [lengths[1]]
    none, l0 = rec.embed([])
    assert none.shape[0] == 0 and len(l0) == 0


def test_word_index_in_several_blocks_on_the_device(cuda, monkeypatch):
    """The device route of an index and a query set beyond one native call: the first test to enter the `else` arm of
    WordIndex.spot_features, which fills one [Q, N] array from a launch per (query piece, block), here 2 x 5, over blocks that
    WordIndex._pack joined with torch.cat across the pieces' edges.  The same hits as the index in one block, distances bit for
    bit (tests/test_word_spotting_cpu.py holds the host route to the same), and the distances within `bound` of the yardstick."""
    everything = spot_in_blocks_and_in_one(monkeypatch, "cuda")
    feat, lens, _ids, _texts, fq, ql = words_for_blocks()
    T, H = feat.shape[1:]
    want = yard_all(yard_unit(fq, ql), ql, *full_gate(len(ql), T), yard_unit(feat, lens), lens)
    worst = 0.0
    for q, hits in enumerate(everything):
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        for h in hits:
            lim = bound(H, ql[q], lens[h.word])
            worst = max(worst, abs(h.distance - want[q, h.word]) / lim)
            assert abs(h.distance - want[q, h.word]) <= lim
    print(f"index in blocks of 5, 5, 5, 5, 3: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("rectify", [False, True])
def test_word_index_through_the_pipeline(cuda, rec, rectify):
    from manuscript_ocr_amd import Pipeline, WordIndex, synth
    from manuscript_ocr_amd._spotting import length_bounds
    from manuscript_ocr_amd.detectors import EAST
    H, W = 224, 320
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda"), rec)
    pipe.rectify_crops = rectify
    img, rects = synth.synth_page(41, H, W)
    score, geo = synth.synth_maps(rects, (H, W), (H // 4, W // 4), 41)
    page = pipe.predict_batch([img], _maps_override=(torch.from_numpy(score)[None].cuda(), torch.from_numpy(geo)[None].cuda()))[0]
    index = pipe.index_words([img, img], pages=[page, page])
    assert isinstance(index, WordIndex) and index.rectify_crops == rectify and index.pages == 2
    words = page.blocks[0].words
    n = len(index) // 2
    assert n >= 4 and len(index) + index.skipped == 2 * len(words)
    assert index.ids[:n] == [(0, b, w) for (_, b, w) in index.ids[n:]] and all(p == 1 for (p, _, _) in index.ids[n:])
    T, Hd = index.T, index.H
    assert index.nbytes == len(index) * (T * Hd * 4 + 4)

    # the f64 yardstick over the same raw frames: the index's own cut, embedded once more (the encoder is deterministic)
    kept = [words[w] for (_, _, w) in index.ids[:n]]
    canv, new_w, rows = index._cut(np.ascontiguousarray(img), kept)
    assert rows == list(range(n))
    raw, lens = rec.embed_canvases(canv, new_w)
    raw = np.concatenate([raw.cpu().numpy()] * 2)
    lens = np.concatenate([lens] * 2)
    unit = yard_unit(raw, lens)
    k = 5
    refs = [index.ids[j] for j in (0, n - 1, n + 1)]
    got = index.spot(refs, k=k)
    lo, hi = length_bounds([lens[index.ids.index(r)] for r in refs], 2.0, T)
    for q, ref in enumerate(refs):
        row = index.ids.index(ref)
        want = yard_all(unit[row:row + 1], lens[row:row + 1], lo[q:q + 1], hi[q:q + 1], unit, lens)[0]
        hits = got[q]
        lim = [bound(Hd, lens[row], lens[index.ids.index((h.page, h.block, h.word))]) for h in hits]
        # a reference query finds itself (or its identical twin of the other page copy, which entered first) at rank 0, distance ~ 0
        assert (hits[0].block, hits[0].word) == ref[1:] and hits[0].page == 0 and abs(hits[0].distance) <= lim[0]
        assert (hits[1].block, hits[1].word) == ref[1:] and hits[1].page == 1 and hits[1].distance == hits[0].distance
        assert [h.rank for h in hits] == list(range(len(hits))) and len(hits) == min(k, int(np.isfinite(want).sum()))
        assert [h.distance for h in hits] == sorted(h.distance for h in hits)
        kth = np.sort(want[np.isfinite(want)])[len(hits) - 1]
        for h, b in zip(hits, lim):
            i = index.ids.index((h.page, h.block, h.word))
            assert abs(h.distance - want[i]) <= b
            assert want[i] <= kth + 2 * b
            assert h.text == words[h.word].text
        print(f"rectify {rectify} query {ref}: distances {[round(h.distance, 6) for h in hits]}")

    # a query by a crop of the page: through Pipeline.spot with the word's polygon (cut the pipeline's way: the index's own canvas)
    w0 = index.ids[1][2]
    # (one canvas through the encoder alone need not give the bits it gives inside a page's batch, so: about 0, not equal)
    by_polygon = pipe.spot(index, [(img, words[w0].polygon), index.ids[1]], k=k)
    assert [(h.page, h.word) for h in by_polygon[0][:2]] == [(0, w0), (1, w0)] == [(h.page, h.word) for h in by_polygon[1][:2]]
    assert abs(by_polygon[0][0].distance) <= bound(Hd, T, T) and by_polygon[0][0].query == 0 and by_polygon[1][0].query == 1
    # ... and as a word image: the word's window of the page, embedded as TRBA.embed embeds an image
    p = np.array(words[w0].polygon, dtype=np.int32)
    (x0, y0), (x1, y1) = p.min(0), p.max(0)
    window = np.ascontiguousarray(img[max(0, y0):min(H, y1), max(0, x0):min(W, x1)])
    by_image = index.spot([window], k=k)[0]
    print(f"rectify {rectify} image query: {[((h.page, h.word), round(h.distance, 6)) for h in by_image]}")
    assert (0, w0) in [(h.page, h.word) for h in by_image]
    if not rectify:  # the host's ResizeAndPadA is the device crop's, byte for byte: the same frames as the indexed word's
        assert by_image[0].word == w0 and abs(by_image[0].distance) <= bound(Hd, T, T)
