"""Skew-aware reading order (Pipeline.deskew), the part that needs no GPU: the host twins
msocr_page_skew_host and msocr_deskew_boxes_host against a NumPy / Python restatement of the definition written from its text
(include/msocr.h; the canonical corner order is the restatement of tests/test_quad_crop_cpu.py), what the definition means on
rotated pages, the generic route of Pipeline with stand-in plugins, and the C ABI's symbol lists.

Everything is integer arithmetic (Python ints in the restatement: no width to overflow) or f64 in the written order: every
comparison is for equality, except the recovered angle, whose bound follows from the per-word rint and is computed from the page.

tests/test_gpu_deskew.py takes the restatement and the page builders from this module.
"""
import math
import os
import re

import numpy as np
import pytest

import test_quad_crop_cpu as qc
import test_text_lines_cpu as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
F32 = np.float32
NAN = float("nan")


# ================================================================================================ the restatement
def ref_vote(quad):
    """quad [4,2] as stored -> (qx, qy) as Python ints, or None when the word does not vote."""
    c = qc.ref_canonical(np.asarray(quad, dtype=F32).reshape(4, 2))
    if c is None:
        return None
    p = [(float(x), float(y)) for x, y in c]
    dx, dy = (p[1][0] - p[0][0]) + (p[2][0] - p[3][0]), (p[1][1] - p[0][1]) + (p[2][1] - p[3][1])
    rx, ry = (p[3][0] - p[0][0]) + (p[2][0] - p[1][0]), (p[3][1] - p[0][1]) + (p[2][1] - p[1][1])
    qx, qy, px, py = (int(np.rint(8.0 * v)) for v in (dx, dy, rx, ry))
    if not (0 < qx < 2 ** 23 and abs(qy) <= qx and qx * qx + qy * qy >= px * px + py * py):
        return None
    return qx, qy


def ref_skew(quads):
    """quads [n,4,2] -> (skew int64 [4] = {S2x, S2y, m, applied}, cs f64 [2])."""
    votes = [v for v in (ref_vote(q) for q in np.asarray(quads, dtype=F32).reshape(-1, 4, 2)) if v is not None]
    s1x, s1y = sum(v[0] for v in votes), sum(v[1] for v in votes)
    near = [v for v in votes if 4 * abs(s1x * v[1] - s1y * v[0]) <= s1x * v[0] + s1y * v[1]]
    s2x, s2y, m = sum(v[0] for v in near), sum(v[1] for v in near), len(near)
    applied = m >= 8 and s2x > 0 and abs(s2y) <= s2x and 256 * abs(s2y) > s2x
    c, s = 1.0, 0.0
    if applied:
        nrm = math.sqrt(float(s2x) * float(s2x) + float(s2y) * float(s2y))
        c, s = float(s2x) / nrm, float(s2y) / nrm
    return np.array([s2x, s2y, m, int(applied)], dtype=np.int64), np.array([c, s], dtype=np.float64)


def trunc_boxes(quads):
    """The words' own integer boxes: np.int32 truncation of the corners, min / max."""
    p = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    with np.errstate(invalid="ignore"):
        p = p.astype(np.int32)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1).astype(np.int32).reshape(-1, 4)


def ref_boxes(quads, page_hw, skew, cs):
    """The ordering boxes [n,4] int32."""
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    out = trunc_boxes(q)
    if not skew[3]:
        return out
    c, s = float(cs[0]), float(cs[1])
    hx, hy = 0.5 * float(page_hw[1]), 0.5 * float(page_hw[0])
    fl = lambda v: int(min(max(math.floor(v), -2 ** 31), 2 ** 31 - 1))
    for k, w in enumerate(q):
        if not np.isfinite(w).all():
            continue
        xs, ys = [], []
        for x, y in w:
            u, v = float(x) - hx, float(y) - hy
            xs.append((c * u + s * v) + hx)
            ys.append((c * v - s * u) + hy)
        out[k] = [fl(min(xs)), fl(min(ys)), fl(max(xs)), fl(max(ys))]
    return out


def check_twins(quads, page_hw=(3000, 2000)):
    """Both twins on `quads` against the restatement -> (skew, cs, boxes) of the twins."""
    from manuscript_ocr_amd import ops
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    skew, cs = ops.page_skew_host(q)
    es, ec = ref_skew(q)
    assert skew.dtype == np.int64 and cs.dtype == np.float64
    assert np.array_equal(skew, es), (skew, es)
    assert np.array_equal(cs, ec), (cs, ec)
    boxes = ops.deskew_boxes_host(q, page_hw, skew, cs)
    assert boxes.dtype == np.int32 and np.array_equal(boxes, ref_boxes(q, page_hw, skew, cs))
    if not skew[3]:
        assert np.array_equal(boxes, trunc_boxes(q)) and cs.tolist() == [1.0, 0.0]
    return skew, cs, boxes


def deskewed_lines(quads, page_hw):
    """The definition's order and lines through the twins: (order, line, records with the words' own boxes united, skew)."""
    from manuscript_ocr_amd import ops
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    skew, cs = ops.page_skew_host(q)
    order, line, recs = ops.reading_lines_host(ops.deskew_boxes_host(q, page_hw, skew, cs))
    own = trunc_boxes(q)[order]
    recs = recs.copy()
    for r in recs:
        seg = own[r[0]:r[0] + r[1]]
        r[2:4], r[4:6] = seg[:, :2].min(axis=0), seg[:, 2:].max(axis=0)
    return order, line, recs, skew


# ================================================================================================ pages
def rect(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float64)


def turn(pts, deg, centre):
    """Points [..., 2] turned by deg about centre; y points down, so a positive angle makes a line descend to the right."""
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    d = np.asarray(pts, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    return np.stack([c * d[..., 0] - s * d[..., 1], s * d[..., 0] + c * d[..., 1]], axis=-1) + np.asarray(centre, dtype=np.float64)


def rising(width, rise, n=8, h=30.0):
    """n words of the given width in a column whose two horizontal edges both rise by `rise`."""
    return np.stack([np.array([[100.0, 100.0 + 60 * k], [100.0 + width, 100.0 + 60 * k + rise], [100.0 + width, 130.0 + 60 * k + rise],
                               [100.0, 130.0 + 60 * k]]) for k in range(n)]).astype(F32)


def grid_page(rows, cols, deg, page_hw, word_wh=(170.0, 30.0), pitch=(230.0, 60.0), jitter_deg=0.0, seed=0, shuffle=True):
    """rows x cols words on a grid centred on the page, turned rigidly by deg about the page centre, every word turned by a further
    U(-jitter_deg, jitter_deg) about its own centre, in shuffled detector order.  -> (quads [n,4,2] f32, true_order [n]: the word
    at every position of the line-major reading order)."""
    rng = np.random.default_rng([SEED, rows, cols, seed])
    H, W = page_hw
    x0 = 0.5 * W - 0.5 * ((cols - 1) * pitch[0] + word_wh[0])
    y0 = 0.5 * H - 0.5 * ((rows - 1) * pitch[1] + word_wh[1])
    quads = []
    for r in range(rows):
        for c in range(cols):
            q = rect(x0 + c * pitch[0], y0 + r * pitch[1], *word_wh)
            q = turn(q, rng.uniform(-jitter_deg, jitter_deg) if jitter_deg else 0.0, q.mean(axis=0))
            quads.append(turn(q, deg, (0.5 * W, 0.5 * H)))
    quads = np.asarray(quads)
    perm = rng.permutation(len(quads)) if shuffle else np.arange(len(quads))
    true_order = np.empty(len(quads), dtype=np.int64)
    true_order[:] = np.argsort(perm)  # position p of the line-major order holds grid word p, stored at index argsort(perm)[p]
    return quads[perm].astype(F32), true_order


def text_page_quads(deg, page_hw=(3000, 1200)):
    """The 1190-word text page of tests/test_text_lines_cpu.py as rectangles, turned rigidly by deg about the page centre."""
    b = np.asarray(tl.text_page(), dtype=np.float64)
    q = np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], axis=1) + 0.25
    return turn(q, deg, (0.5 * page_hw[1], 0.5 * page_hw[0])).astype(F32)


WIDE_HW = (34000, 300000)


def wide_page(deg=1.0, n=1024):
    """n words 280 000 px wide, one per line, on a page 300 000 px wide: qx = 4.48e6 per word, the sums pass 2^32."""
    q = np.stack([rect(10000.0, 1000.0 + 30 * k, 280000.0, 20.0) for k in range(n)])
    rng = np.random.default_rng([SEED, 77])
    return turn(q, deg, (0.5 * WIDE_HW[1], 0.5 * WIDE_HW[0]))[rng.permutation(n)].astype(F32)


# ================================================================================================ 1. the twins
def test_empty_page_and_single_word():
    skew, cs, boxes = check_twins(np.zeros((0, 4, 2)))
    assert skew.tolist() == [0, 0, 0, 0] and cs.tolist() == [1.0, 0.0] and boxes.shape == (0, 4)
    skew, cs, boxes = check_twins([turn(rect(100.5, 200.5, 160, 30), 5.0, (180, 215))])
    assert skew[2] == 1 and skew[3] == 0 and skew[0] > 0 and skew[1] > 0
    from manuscript_ocr_amd import _native as nat
    out, c2 = np.zeros(4, dtype=np.int64), np.zeros(2)
    assert nat.lib().msocr_page_skew_host(None, 0, out.ctypes.data, c2.ctypes.data) == 0 and c2.tolist() == [1.0, 0.0]
    assert nat.lib().msocr_page_skew_host(None, 1, out.ctypes.data, c2.ctypes.data) == -1
    assert nat.lib().msocr_page_skew_host(None, 0, None, c2.ctypes.data) == -1
    assert nat.lib().msocr_page_skew_host(None, -1, out.ctypes.data, c2.ctypes.data) == -1
    assert nat.lib().msocr_deskew_boxes_host(None, 0, 0, 10, out.ctypes.data, c2.ctypes.data, None) == -1


def test_seven_words_identity_eight_applied():
    q, _ = grid_page(4, 2, 3.0, (1000, 1000))
    skew, cs, boxes = check_twins(q[:7], (1000, 1000))
    assert skew[2] == 7 and skew[3] == 0
    skew, cs, boxes = check_twins(q, (1000, 1000))
    assert skew[2] == 8 and skew[3] == 1 and cs[0] < 1.0 and cs[1] > 0.0
    assert not np.array_equal(boxes, trunc_boxes(q))
    assert abs(math.degrees(math.atan2(skew[1], skew[0])) - 3.0) < 0.01
    # a word that does not vote beside seven that do: still the identity
    tall = turn(rect(500, 500, 20, 90), 3.0, (500, 500)).astype(F32)
    skew, _cs, _b = check_twins(np.concatenate([q[:7], tall[None]]), (1000, 1000))
    assert skew[2] == 7 and skew[3] == 0


def test_dead_zone_edge():
    skew, cs, _ = check_twins(rising(256.0, 1.0))
    assert skew.tolist() == [32768, 128, 8, 0] and cs.tolist() == [1.0, 0.0]
    skew, cs, boxes = check_twins(rising(256.0, 1.0625))
    assert skew.tolist() == [32768, 136, 8, 1] and cs[1] > 0.0
    assert not np.array_equal(boxes, trunc_boxes(rising(256.0, 1.0625)))
    skew, _cs, _b = check_twins(rising(256.0, -1.0625))
    assert skew.tolist() == [32768, -136, 8, 1]


def test_windings_and_start_corners():
    q, _ = grid_page(3, 4, -4.0, (1000, 1400), jitter_deg=1.0)
    base = check_twins(q, (1000, 1400))
    assert base[0][3] == 1 and base[0][2] == 12
    for start in range(4):
        for backwards in (False, True):
            idx = [(start + k) % 4 for k in range(4)]
            idx = idx[::-1] if backwards else idx
            got = check_twins(q[:, idx], (1000, 1400))
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]), (start, backwards)


def test_words_that_do_not_vote():
    """A bow-tie, a NaN corner, a tall word, a word of qx >= 2^23 and two words at 88 degrees leave the sums as they are; the word
    with the NaN corner keeps its own box."""
    H, W = 1200, 2000
    q, _ = grid_page(3, 4, 3.0, (H, W))
    base, _cs, bb = check_twins(q, (H, W))
    assert base[3] == 1 and base[2] == 12
    w = rect(300, 700, 170, 30)
    bow = turn(w[[0, 1, 3, 2]], 3.0, (1000, 600))
    nan = turn(w, 3.0, (1000, 600)).copy()
    nan[2, 1] = NAN
    tall = turn(rect(900, 800, 25, 80), 3.0, (1000, 600))
    huge = rect(-300000.0, 900.0, 600000.0, 30.0)  # 16 * 600000 = 9.6e6 >= 2^23
    steep = [turn(rect(1500 + 80 * k, 300, 170, 30), 88.0, (1585 + 80 * k, 315)) for k in range(2)]
    for name, extra in (("bow-tie", [bow]), ("nan", [nan]), ("tall", [tall]), ("huge", [huge]), ("88 degrees", steep)):
        for e in extra:
            assert ref_vote(e) is None, name
        skew, cs, boxes = check_twins(np.concatenate([q, np.asarray(extra, dtype=F32)]), (H, W))
        assert np.array_equal(skew, base) and np.array_equal(boxes[:len(q)], bb), name
        if name == "nan":
            assert np.array_equal(boxes[-1], trunc_boxes(np.asarray(extra, dtype=F32))[0])
    assert ref_vote(rect(0.0, 900.0, 524287.0, 30.0)) == (8388592, 0) and ref_vote(rect(0.0, 900.0, 524288.0, 30.0)) is None


def test_outliers_leave_the_second_pass_unchanged():
    """Two words at 33 degrees beside a page at 3: they vote in the first pass, fall outside atan(1/4) of it and leave S2 exactly."""
    H, W = 1200, 2000
    q, _ = grid_page(4, 5, 3.0, (H, W), jitter_deg=1.0)
    base, _cs, _b = check_twins(q, (H, W))
    out = np.asarray([turn(rect(200 + 900 * k, 1000, 170, 30), 33.0, (285 + 900 * k, 1015)) for k in range(2)], dtype=F32)
    assert all(ref_vote(o) is not None for o in out)
    skew, _cs, _b = check_twins(np.concatenate([out[:1], q, out[1:]]), (H, W))
    assert base[3] == 1 and base[2] == 20 and np.array_equal(skew, base)


def test_sums_past_two_to_the_32_and_shuffled_input():
    q = wide_page()
    skew, cs, boxes = check_twins(q, WIDE_HW)
    assert skew[2] == 1024 and skew[3] == 1 and skew[0] > 2 ** 32 and skew[1] > 2 ** 24
    assert abs(math.degrees(math.atan2(skew[1], skew[0])) - 1.0) < 1e-3
    rng = np.random.default_rng([SEED, 5])
    p = rng.permutation(len(q))
    s2, c2, b2 = check_twins(q[p], WIDE_HW)
    assert np.array_equal(s2, skew) and np.array_equal(c2, cs) and np.array_equal(b2, boxes[p])
    q, _ = grid_page(6, 8, 5.0, (1200, 2000), jitter_deg=1.0)
    a, b = check_twins(q, (1200, 2000)), check_twins(q[rng.permutation(len(q))], (1200, 2000))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_recovery_on_rotated_rectangles():
    """Exact rectangles turned rigidly: atan2(S2y, S2x) is the angle up to 0.5 / (16 w_min) rad, the per-word rint of a direction
    16 w long (w_min = the page's shortest word); measured worst case over these 40 pages: printed."""
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng([SEED, 9])
    worst = 0.0
    for page in range(40):
        deg = float(rng.uniform(-8.0, 8.0))
        n = int(rng.integers(8, 60))
        ws = rng.uniform(40.0, 300.0, size=n)
        q = np.stack([rect(rng.uniform(100, 1500), rng.uniform(100, 1000), w, rng.uniform(18, 36)) for w in ws])
        skew, _cs = ops.page_skew_host(turn(q, deg, (1000, 600)).astype(F32))
        assert skew[2] == n
        err = abs(math.atan2(skew[1], skew[0]) - math.radians(deg))
        bound = 0.5 / (16.0 * float(ws.min()))
        worst = max(worst, math.degrees(err))
        assert err <= bound, (page, deg, err, bound)
    print(f"deskew recovery: worst error {worst:.5f} degrees over 40 pages")


# ================================================================================================ 2. the order
def skewed_text(deg=3.0, rows=6, cols=8, seed=1):
    return grid_page(rows, cols, deg, (1200, 2000), jitter_deg=1.0, seed=seed), (1200, 2000)


def test_deskewed_order_is_line_major_where_the_plain_order_is_not():
    from manuscript_ocr_amd import ops
    (q, true_order), hw = skewed_text()
    plain, _l, plain_recs = tl.check_twin(trunc_boxes(q))
    assert not np.array_equal(plain, true_order), "the plain order of the skewed page is expected to be wrong"
    assert int((plain != true_order).sum()) >= 24 and len(plain_recs) != 6
    skew, cs, boxes = check_twins(q, hw)
    assert skew[3] == 1 and abs(math.degrees(math.atan2(skew[1], skew[0])) - 3.0) < 0.2
    tl.check_twin(boxes)  # the twin's order on the ordering boxes is the reference's
    order, line, recs, _s = deskewed_lines(q, hw)
    assert np.array_equal(order, true_order)
    assert recs[:, :2].tolist() == [[8 * k, 8] for k in range(6)] and line.tolist() == [k // 8 for k in range(48)]
    own = trunc_boxes(q)
    for first, count, x0, y0, x1, y1 in recs.tolist():
        seg = own[order[first:first + count]]
        assert (x0, y0, x1, y1) == (seg[:, 0].min(), seg[:, 1].min(), seg[:, 2].max(), seg[:, 3].max())
    # the same page upright: inside the dead zone nothing moves
    (q0, t0), _hw = grid_page(6, 8, 0.0, hw, seed=1), hw
    s0, _c0, b0 = check_twins(q0, hw)
    assert s0[3] == 0 and np.array_equal(ops.reading_lines_host(b0)[0], t0) and np.array_equal(b0, trunc_boxes(q0))


@pytest.mark.parametrize("deg", [-3.0, 2.0, 5.0, 8.0])
def test_deskewed_order_over_angles(deg):
    (q, true_order), hw = skewed_text(deg, seed=int(deg) + 10)
    order, _line, recs, skew = deskewed_lines(q, hw)
    assert skew[3] == 1 and np.array_equal(order, true_order) and len(recs) == 6


# ================================================================================================ 3. the generic route of Pipeline
class StandInDetector:
    def __init__(self, quads, conf=0.9):
        self.quads = quads

    def predict(self, image, vis=False, profile=False):
        from manuscript_ocr_amd.detectors._types import Block, Page, Word
        words = [Word(polygon=[[float(x), float(y)] for x, y in q], detection_confidence=0.9) for q in self.quads]
        self.words = words
        return {"page": Page(blocks=[Block(words=words)]), "vis_image": None, "score_map": None, "geo_map": None}


class StandInRecognizer:
    def predict(self, images):
        return [{"text": f"w{i}", "confidence": 0.5} for i in range(len(images))]


def _pipe(quads, **switches):
    from manuscript_ocr_amd import Pipeline
    p = Pipeline(detector=StandInDetector(quads), recognizer=StandInRecognizer())
    assert vars(p)["deskew"] is False, "declared in __init__, off by default"
    for k, v in switches.items():
        setattr(p, k, v)
    return p


def _polys(page):
    return [w.polygon for b in page.blocks for w in b.words]


def test_pipeline_deskew_generic_route():
    from manuscript_ocr_amd.detectors._types import Block, Page, SkewPage, TextLine
    (q, true_order), hw = skewed_text()
    img = np.zeros(hw + (3,), dtype=np.uint8)
    off = _pipe(q).predict(img)
    assert type(off) is Page and _polys(off) != [[tuple(map(float, pt)) for pt in q[k]] for k in true_order]
    p = _pipe(q, deskew=True)
    on = p.predict(img)
    assert type(on) is SkewPage and isinstance(on, Page) and len(on.blocks) == 1 and type(on.blocks[0]) is Block
    skew, _cs = ref_skew(q)
    assert on.skew_deg == math.degrees(math.atan2(int(skew[1]), int(skew[0]))) and abs(on.skew_deg - 3.0) < 0.2
    assert [id(w) for w in on.blocks[0].words] == [id(p.detector.words[k]) for k in true_order], "the same word objects, line-major"
    assert sorted(map(str, _polys(on))) == sorted(map(str, _polys(off))), "the same polygons, permuted"
    assert [w.text for w in on.blocks[0].words] == [f"w{i}" for i in range(48)]
    from pydantic import BaseModel

    class Book(BaseModel):
        pages: list[Page]

    dumped = Book(pages=[on]).model_dump()["pages"][0]
    assert "skew_deg" not in dumped and dumped == Page(blocks=on.blocks).model_dump(), "declared as a Page, a SkewPage dumps as a Page"
    assert on.model_dump()["skew_deg"] == on.skew_deg
    # with group_lines: the lines of the deskewed frame, their boxes in page coordinates
    lines = _pipe(q, deskew=True, group_lines=True).predict(img)
    assert type(lines) is SkewPage and lines.skew_deg == on.skew_deg
    assert [type(b) for b in lines.blocks] == [TextLine] * 6 and [len(b.words) for b in lines.blocks] == [8] * 6
    assert _polys(lines) == _polys(on)
    _o, _l, recs, _s = deskewed_lines(q, hw)
    assert [b.bbox for b in lines.blocks] == [tuple(r[2:]) for r in recs.tolist()]
    # the switch off again: today's page
    again = _pipe(q, deskew=False).predict(img)
    assert type(again) is Page and _polys(again) == _polys(off) and again.model_dump() == off.model_dump()


def test_pipeline_deskew_upright_and_axis_aligned_pages_keep_their_order():
    from manuscript_ocr_amd.detectors._types import SkewPage
    hw = (1200, 2000)
    q, _t = grid_page(6, 8, 0.1, hw, seed=3)  # inside the dead zone
    img = np.zeros(hw + (3,), dtype=np.uint8)
    off, on = _pipe(q).predict(img), _pipe(q, deskew=True).predict(img)
    assert type(on) is SkewPage and on.skew_deg == 0.0 and _polys(on) == _polys(off)
    t = trunc_boxes(skewed_text()[0][0]).astype(np.float64)  # the AABBs of a skewed page: rectangles, zero by construction
    rects = np.stack([t[:, [0, 1]], t[:, [2, 1]], t[:, [2, 3]], t[:, [0, 3]]], axis=1)
    off, on = _pipe(rects).predict(img), _pipe(rects, deskew=True).predict(img)
    assert type(on) is SkewPage and on.skew_deg == 0.0 and _polys(on) == _polys(off)
    raw = _pipe(skewed_text()[0][0], deskew=True).predict(img, recognize_text=False)
    assert not isinstance(raw, SkewPage), "no reading order is applied there: the switch has no effect"


# ================================================================================================ 4. the C ABI
def test_new_symbols_in_header_bindings_and_library():
    import __graft_entry__ as g
    g.build()
    from manuscript_ocr_amd import _native, ops
    header = open(os.path.join(ROOT, "include", "msocr.h")).read()
    declared = set(re.findall(r"\b(msocr_[a-z0-9_]+)\s*\(", header))
    for name in ("msocr_reading_order_deskew", "msocr_reading_order_deskew_workspace_bytes", "msocr_page_skew_host", "msocr_deskew_boxes_host"):
        assert name in declared and name in _native.exported_symbols() and hasattr(_native.lib(), name), name
    L = _native.lib()
    for n, mc in ((1, 1), (3, 300), (2, 16384), (2, 20000)):
        cap = min(mc, 16384)
        assert L.msocr_reading_order_deskew_workspace_bytes(n, mc) == L.msocr_reading_order_workspace_bytes(n, mc) + n * 16 * cap
    assert L.msocr_reading_order_deskew_workspace_bytes(0, 5) == 0
    assert all(hasattr(ops, f) for f in ("reading_order_deskew", "page_skew_host", "deskew_boxes_host"))
