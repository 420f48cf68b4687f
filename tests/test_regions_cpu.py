"""Column-aware reading order (Pipeline.columns), the part that needs no GPU: the host twin
msocr_reading_regions_host against a Python restatement of the XY-cut written from the text of include/msocr.h, the layout pages the
feature exists for, the generic route of Pipeline with stand-in plugins, and the C ABI's symbol lists and refusals.

The yardstick.  `ref_regions` restates the definition with Python ints and floats on the oracle's resolve_intersections and
sort_boxes_reading_order (oracle/pipeline_glue.py): the cut is recursive as the header words it, and inside every leaf the flattened
lines are pinned to the oracle's sort_boxes_reading_order on the leaf's shrunk boxes before anything is compared against them.
Everything is integer or f64 arithmetic in one written order, so every comparison here is for equality.

tests/test_gpu_regions.py takes `ref_regions`, `check_regions_twin` and the page builders from this module.
"""
import math
import os
import re

import numpy as np
import pytest

import test_deskew_cpu as dk
import test_text_lines_cpu as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
INF = float("inf")
NAN = float("nan")
INT_MIN = -2 ** 31
DEFAULTS = (2.0, 1.5, 3.0)  # col_gap_ratio, row_gap_ratio, col_min_height_ratio
MAX_DEPTH = 6


# ================================================================================================ the restatement
def ref_cut(S, ratios=DEFAULTS):
    """Shrunk boxes (tuples of Python ints) -> the leaves of the XY-cut in depth-first order, each a list of ascending indices."""
    n = len(S)
    avg_h = float(sum(s[3] - s[1] for s in S)) / float(n)
    gx, gy, mh = ratios[0] * avg_h, ratios[1] * avg_h, ratios[2] * avg_h
    leaves = []

    def walk(words, lo, hi, g):
        segs, run = [], None
        for i in sorted(words, key=lambda i: (S[i][lo], i)):
            if run is None or float(S[i][lo] - run) >= g:
                segs.append([])
            segs[-1].append(i)
            run = S[i][hi] if run is None else max(run, S[i][hi])
        return segs

    def cut(words, depth):
        if depth == MAX_DEPTH or len(words) == 1:
            leaves.append(sorted(words))
            return
        segs = [words]
        if float(max(S[i][3] for i in words) - min(S[i][1] for i in words)) >= mh:
            segs = walk(words, 0, 2, gx)
        if len(segs) == 1:
            segs = walk(words, 1, 3, gy)
        if len(segs) == 1:
            leaves.append(sorted(words))
            return
        for seg in segs:
            cut(seg, depth + 1)

    cut(list(range(n)), 0)
    return leaves


def leaf_lines(boxes, y_tol_ratio, x_gap_ratio):
    """The lines of sort_boxes_reading_order on `boxes` (taken as they are), as tests/test_text_lines_cpu.py::lines_of groups them."""
    avg_h = np.mean([b[3] - b[1] for b in boxes])
    lines = []
    for b in sorted(boxes, key=lambda b: (b[1] + b[3]) / 2):
        cy = (b[1] + b[3]) / 2
        for ln in lines:
            line_cy = np.mean([(v[1] + v[3]) / 2 for v in ln])
            if abs(cy - line_cy) <= avg_h * y_tol_ratio and (b[0] - max(v[2] for v in ln)) <= avg_h * x_gap_ratio:
                ln.append(b)
                break
        else:
            lines.append([b])
    lines.sort(key=lambda ln: np.mean([(b[1] + b[3]) / 2 for b in ln]))
    for ln in lines:
        ln.sort(key=lambda b: b[0])
    return lines


def _records(spans, boxes, order):
    recs, pos = [], 0
    for count in spans:
        a = np.array([boxes[k] for k in order[pos:pos + count]], dtype=np.int64)
        recs.append([pos, count, a[:, 0].min(), a[:, 1].min(), a[:, 2].max(), a[:, 3].max()])
        pos += count
    return np.array(recs, dtype=np.int32).reshape(-1, 6)


def ref_regions(boxes, y_tol_ratio=0.6, x_gap_ratio=INF, ratios=DEFAULTS):
    """boxes -> (order [n], line [n], line records [L,6], region [n], region records [R,6]) int32 by the definition."""
    from oracle import pipeline_glue as G
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if not boxes:
        e, r = np.zeros(0, dtype=np.int32), np.zeros((0, 6), dtype=np.int32)
        return e, e, r, e, r
    S = G.resolve_intersections(boxes)
    back = dict(zip(S, boxes))
    first = {}
    for k, b in enumerate(boxes):
        first.setdefault(b, k)
    order, line, region, line_spans, region_spans = [], [], [], [], []
    for leaf in ref_cut(S, ratios):
        mine = [S[i] for i in leaf]
        lines = leaf_lines(mine, y_tol_ratio, x_gap_ratio)
        flat = [b for ln in lines for b in ln]
        assert flat == G.sort_boxes_reading_order(mine, y_tol_ratio, x_gap_ratio), "leaf_lines does not flatten to the oracle"
        for ln in lines:
            line += [len(line_spans)] * len(ln)
            line_spans.append(len(ln))
        region += [len(region_spans)] * len(flat)
        region_spans.append(len(flat))
        order += [first[back[s]] for s in flat]
    i32 = lambda v: np.array(v, dtype=np.int32)
    return i32(order), i32(line), _records(line_spans, boxes, order), i32(region), _records(region_spans, boxes, order)


def regions_host(boxes, y_tol_ratio=0.6, x_gap_ratio=INF, ratios=DEFAULTS):
    from manuscript_ocr_amd import ops
    return ops.reading_regions_host(np.asarray(boxes, dtype=np.int64).astype(np.int32).reshape(-1, 4), y_tol_ratio, x_gap_ratio, *ratios)


def check_regions_twin(boxes, y_tol_ratio=0.6, x_gap_ratio=INF, ratios=DEFAULTS, reference=True):
    """msocr_reading_regions_host on `boxes`: sound in structure (lines and regions tile the positions, a line lies in one region,
    the boxes are the unions NumPy forms) and, with `reference`, equal to `ref_regions`.  Returns the twin's five arrays."""
    order, line, lrecs, region, rrecs = got = regions_host(boxes, y_tol_ratio, x_gap_ratio, ratios)
    assert all(a.dtype == np.int32 for a in got) and lrecs.shape[1:] == (6,) and rrecs.shape[1:] == (6,)
    tl.check_structure(boxes, order, line, lrecs)
    tl.check_structure(boxes, order, region, rrecs)
    for first, count in lrecs[:, :2].tolist():
        assert len(set(region[first:first + count].tolist())) == 1, "a line spans two regions"
    if reference:
        for g, e, what in zip(got, ref_regions(boxes, y_tol_ratio, x_gap_ratio, ratios), ("order", "line", "lines", "region", "regions")):
            assert np.array_equal(g, e), (what, g.tolist()[:40], e.tolist()[:40])
    return got


# ================================================================================================ pages
def layout_page(cols=2, lines=20, per_line=4, stagger=0, heading=False, footer=False, seed=0, gutter=120, shuffle=True):
    """A page of `cols` columns of `lines` lines of `per_line` words 40 x 20 at pitch 56 x 36 (word space 16, line space 16), the
    columns `gutter` apart and column c lowered by c * stagger; `heading` / `footer`: one line of words across the whole width, 60
    above / below the body.  All heights are 20, so avg_h = 20, gx = 40, gy = 30, mh = 60 with the default ratios.  Left edges are
    jittered by up to 3.  -> (boxes [n,4] in shuffled detector order, truth [n]: the index of the word at every position of the
    column-major reading order)."""
    rng = np.random.default_rng([SEED, cols, lines, per_line, stagger, int(heading), int(footer), seed])
    col_w = per_line * 56 - 16
    width = cols * col_w + (cols - 1) * gutter
    top = 100 if heading else 20
    b = []
    if heading:
        b += [[30 + 56 * k, 20, 30 + 56 * k + 40, 40] for k in range((width + 16) // 56)]
    for c in range(cols):
        for ln in range(lines):
            for k in range(per_line):
                x, y = 30 + c * (col_w + gutter) + 56 * k + int(rng.integers(0, 4)), top + 36 * ln + c * stagger
                b.append([x, y, x + 40 - 3, y + 20])
    if footer:
        y = top + 36 * (lines - 1) + (cols - 1) * stagger + 20 + 60
        b += [[30 + 56 * k, y, 30 + 56 * k + 40, y + 20] for k in range((width + 16) // 56)]
    b = np.array(b, dtype=np.int64)
    perm = rng.permutation(len(b)) if shuffle else np.arange(len(b))
    return b[perm], np.argsort(perm)


LAYOUTS = {
    "two aligned columns": dict(cols=2, lines=20, per_line=4),
    "two staggered columns": dict(cols=2, lines=20, per_line=4, stagger=18),
    "a heading over two columns": dict(cols=2, lines=20, per_line=4, heading=True),
    "a heading over two columns with a footer": dict(cols=2, lines=19, per_line=4, heading=True, footer=True, stagger=18),
    "three columns": dict(cols=3, lines=16, per_line=4, stagger=7),
    "a four-column spread": dict(cols=4, lines=13, per_line=4, stagger=11),
}


def two_paragraphs():
    """One column, two paragraphs of 6 lines of 5 words, 50 apart: two regions, and the plain order already is the truth."""
    b, _t = layout_page(cols=1, lines=6, per_line=5, seed=5, shuffle=False)
    low = b.copy()
    low[:, [1, 3]] += 6 * 36 - 16 + 50
    both = np.concatenate([b, low])
    return both[np.random.default_rng([SEED, 77]).permutation(len(both))]


def column_pair(gap, lines=3, pitch=25, second_dy=0):
    """Two columns of `lines` single 40 x 20 words at line pitch `pitch`, `gap` apart; the second column lowered by second_dy."""
    return [[0, pitch * k, 40, pitch * k + 20] for k in range(lines)] + [[40 + gap, pitch * k + second_dy, 80 + gap, pitch * k + 20 + second_dy]
                                                                         for k in range(lines)]


def edge_pages():
    """The `>=` edges with all heights 20 (avg_h = 20: gx = 40, gy = 30, mh = 60 exactly) -> name: (boxes, regions expected)."""
    return {
        "column gap 40 cuts": (column_pair(40), 2),
        "column gap 39 does not": (column_pair(39), 1),
        "row gap 30 cuts": ([[0, 0, 40, 20], [50, 0, 90, 20], [0, 50, 40, 70], [50, 50, 90, 70]], 2),
        "row gap 29 does not": ([[0, 0, 40, 20], [50, 0, 90, 20], [0, 49, 40, 69], [50, 49, 90, 69]], 1),
        "height 60 allows the vertical cut": (column_pair(100, lines=2, pitch=40), 2),
        "height 59 does not": (column_pair(100, lines=2, pitch=39), 1),
    }


def nested_page(depth):
    """A stacked pair of words 50 apart (a horizontal cut would part them) inside `depth` nested cuts that alternate, the outermost
    vertical: every cut splits off a column of words left of the rest (100 away, spanning its height at line space 5) or a row of
    words above it (100 away, spanning its width at word space 5).  All heights 20."""
    b = [[0, 0, 40, 20], [0, 70, 40, 90]]
    for k in range(depth):
        a = np.array(b)
        x0, y0, x1, y1 = a[:, 0].min(), a[:, 1].min(), a[:, 2].max(), a[:, 3].max()
        if (depth - 1 - k) % 2 == 0:  # vertical
            b += [[x0 - 140, y, x0 - 100, y + 20] for y in range(y0, y1, 25)]
        else:
            b += [[x, y0 - 120, x + 40, y0 - 100] for x in range(x0, x1, 45)]
    return b


def nan_corner_page():
    """A two-column page with a word whose box lies at INT_MIN in x0 (a NaN corner truncates to INT_MIN), one whose whole x extent
    does, and one at INT_MIN in y: the walks meet differences that do not fit int32."""
    b, _t = layout_page(cols=2, lines=4, per_line=3, seed=9)
    return b.tolist() + [[INT_MIN, 500, 500, 520], [INT_MIN, 400, INT_MIN, 420], [700, INT_MIN, 740, INT_MIN + 20]]


# ================================================================================================ 1. the twin against the restatement
def test_empty_page_one_word_and_a_pair():
    order, line, lrecs, region, rrecs = check_regions_twin([])
    assert len(order) == 0 and lrecs.shape == (0, 6) and rrecs.shape == (0, 6)
    order, line, lrecs, region, rrecs = check_regions_twin([[5, 6, 70, 30]])
    assert order.tolist() == [0] and region.tolist() == [0] and rrecs.tolist() == [[0, 1, 5, 6, 70, 30]] == lrecs.tolist()
    # two words each side of a gap on one line: a band one line high is never split at its word spaces
    order, line, lrecs, region, rrecs = check_regions_twin([[500, 0, 560, 20], [0, 0, 60, 20]])
    assert order.tolist() == [1, 0] and len(rrecs) == 1 and len(lrecs) == 1
    # ... and the same two with room below them: two columns
    order, line, lrecs, region, rrecs = check_regions_twin([[500, 0, 560, 20], [0, 0, 60, 20], [500, 40, 560, 60], [0, 40, 60, 60]])
    assert order.tolist() == [1, 3, 0, 2] and region.tolist() == [0, 0, 1, 1] and line.tolist() == [0, 1, 2, 3]
    assert rrecs.tolist() == [[0, 2, 0, 0, 60, 60], [2, 2, 500, 0, 560, 60]]


@pytest.mark.parametrize("name", list(edge_pages()))
def test_threshold_edges(name):
    boxes, nreg = edge_pages()[name]
    assert len(check_regions_twin(boxes)[4]) == nreg


def test_depth_limit_leaves_the_innermost_pair_uncut():
    # 5 cuts: the pair is a region at depth 5 and is parted;  6: the innermost cut is horizontal and parts row, word and word at
    # once;  7: the region at depth 6 holds the seventh part and the pair, and is a leaf
    for depth, nreg in ((5, 7), (6, 8), (7, 7)):
        boxes = nested_page(depth)
        order, line, lrecs, region, rrecs = check_regions_twin(boxes)
        assert len(rrecs) == nreg, (depth, rrecs.tolist())
        pair = [region[order.tolist().index(k)] for k in (0, 1)]
        assert (pair[0] == pair[1]) == (depth == 7), depth
    assert len(rrecs) == 7 and rrecs[-1, 1] > 2, "seven nested cuts: the seventh is not made, its part stays with the pair"


def test_nan_corner_duplicates_and_infinite_ratios():
    order, line, lrecs, region, rrecs = check_regions_twin(nan_corner_page())
    assert len(rrecs) >= 3 and rrecs[:, 2].min() == INT_MIN and rrecs[:, 3].min() == INT_MIN
    # duplicates: two positions name word 0, and equal shrunk boxes land in one region (two columns of two lines 38 apart: four)
    far = [[x + 900, y, x1 + 900, y1] for x, y, x1, y1 in tl.duplicate_page()]
    order, line, lrecs, region, rrecs = check_regions_twin(tl.duplicate_page() + far)
    assert order.tolist() == [0, 0, 1, 3, 4, 5, 5, 6, 8, 9] and region.tolist() == [0] * 3 + [1] * 2 + [2] * 3 + [3] * 2
    from manuscript_ocr_amd import ops
    for boxes in (layout_page()[0], two_paragraphs(), nested_page(7), tl.duplicate_page()):
        for ratios in ((INF, INF, 3.0), (INF, INF, INF), (2.0, INF, INF)):
            order, line, lrecs, region, rrecs = check_regions_twin(boxes, ratios=ratios)
            po, pl, pr = ops.reading_lines_host(np.asarray(boxes, dtype=np.int32))
            assert np.array_equal(order, po) and np.array_equal(line, pl) and np.array_equal(lrecs, pr) and len(rrecs) == 1
            assert rrecs[0, :2].tolist() == [0, len(boxes)]


def test_shuffled_input_gives_the_same_reading():
    for kw in LAYOUTS.values():
        plain, _t = layout_page(shuffle=False, **kw)
        shuffled, _t = layout_page(**kw)
        a, b = regions_host(plain), regions_host(shuffled)
        assert np.array_equal(plain[a[0]], shuffled[b[0]]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_envelope_pages():
    for name, boxes in tl.envelope_pages().items():
        check_regions_twin(boxes)
        check_regions_twin(boxes, 0.6, tl.TIE_GAP, (0.5, 0.25, 1.0))
    check_regions_twin(tl.tie_page(), 0.6, tl.TIE_GAP)
    for boxes in tl.golden_cases():
        check_regions_twin(boxes)


# ================================================================================================ 2. the layout pages
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_pages_read_column_by_column(name):
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd.detectors import _east
    boxes, truth = layout_page(**LAYOUTS[name])
    plain = ops.reading_lines_host(boxes.astype(np.int32))[0]
    wrong = int((plain != truth).sum())
    print(f"{name}: {len(boxes)} words, the plain order is wrong at {wrong}")
    assert wrong > len(boxes) // 2, "the page-wide line rule reads across the gutter: why the feature exists"
    order, line, lrecs, region, rrecs = check_regions_twin(boxes)
    assert np.array_equal(order, truth), "column-major truth"
    kw = LAYOUTS[name]
    assert len(rrecs) == kw["cols"] + int(kw.get("heading", False)) + int(kw.get("footer", False))
    py, reg = _east.utils.sort_boxes_reading_order_regions([tuple(b) for b in boxes.tolist()], return_regions=True)
    assert py == [tuple(b) for b in boxes[truth].tolist()] and reg == region.tolist(), "the Python function gives the same reading"


def test_single_column_pages_keep_the_plain_order():
    from manuscript_ocr_amd import ops
    boxes = tl.text_page()
    order, line, lrecs, region, rrecs = check_regions_twin(boxes, reference=False)  # 1190 words: the oracle's sweep is slow
    po, pl, pr = ops.reading_lines_host(np.asarray(boxes, dtype=np.int32))
    assert len(rrecs) == 1 and np.array_equal(order, po) and np.array_equal(line, pl) and np.array_equal(lrecs, pr) and len(pr) == 70
    boxes = two_paragraphs()
    order, line, lrecs, region, rrecs = check_regions_twin(boxes)
    assert len(rrecs) == 2 and rrecs[:, 1].tolist() == [30, 30] and np.array_equal(order, ops.reading_lines_host(boxes.astype(np.int32))[0])


# ================================================================================================ 3. the generic route of Pipeline
def _rects(boxes):
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    return np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], axis=1) + 0.25


def _union(words):
    p = np.array([w.polygon for w in words]).astype(np.int32)
    return (*p.min(axis=(0, 1)).tolist(), *p.max(axis=(0, 1)).tolist())


def test_pipeline_columns_generic_route():
    from manuscript_ocr_amd import Pipeline, ops
    from manuscript_ocr_amd.detectors._types import Block, Page, Region, RegionLine, TextLine
    assert issubclass(Region, Block) and issubclass(RegionLine, TextLine)
    boxes, truth = layout_page(cols=2, lines=6, per_line=3, heading=True, seed=2)
    q = _rects(boxes)
    img = np.zeros((400, 600, 3), dtype=np.uint8)
    p0 = dk._pipe(q)
    assert vars(p0)["columns"] is False and p0.column_params == dict(zip(("col_gap_ratio", "row_gap_ratio", "col_min_height_ratio"), DEFAULTS))
    off = p0.predict(img)
    want = [[tuple(map(float, pt)) for pt in q[k]] for k in truth]
    assert type(off) is Page and dk._polys(off) != want
    p = dk._pipe(q, columns=True)
    on = p.predict(img)
    assert type(on) is Page and [type(b) for b in on.blocks] == [Region] * 3 and [b.index for b in on.blocks] == [0, 1, 2]
    assert [len(b.words) for b in on.blocks] == [len(boxes) - 36, 18, 18] and dk._polys(on) == want
    assert [id(w) for b in on.blocks for w in b.words] == [id(p.detector.words[k]) for k in truth], "the same word objects"
    assert [b.bbox for b in on.blocks] == [_union(b.words) for b in on.blocks]
    assert [w.text for b in on.blocks for w in b.words] == [f"w{i}" for i in range(len(boxes))], "the crops follow the order"
    assert "bbox" not in on.model_dump()["blocks"][0] and "index" not in on.model_dump()["blocks"][0]
    assert on.model_dump() == Page(blocks=[Block(words=b.words) for b in on.blocks]).model_dump(), "a Region dumps as a Block"
    assert p.get_text(on).count("\n") == 2
    # with group_lines: RegionLines, region-major
    lines = dk._pipe(q, columns=True, group_lines=True).predict(img)
    assert [type(b) for b in lines.blocks] == [RegionLine] * 13 and [b.region for b in lines.blocks] == [0] + [1] * 6 + [2] * 6
    assert dk._polys(lines) == want and [b.bbox for b in lines.blocks] == [_union(b.words) for b in lines.blocks]
    assert lines.model_dump() == Page(blocks=[Block(words=b.words) for b in lines.blocks]).model_dump()
    # other ratios reach the cut; a bad one is refused
    one = dk._pipe(q, columns=True, column_params={"col_gap_ratio": INF, "row_gap_ratio": INF}).predict(img)
    assert len(one.blocks) == 1 and one.blocks[0].index == 0 and dk._polys(one) == dk._polys(off)
    for bad in ({"col_gap_ratio": -1.0}, {"row_gap_ratio": NAN}, {"gap": 1.0}):
        with pytest.raises(ValueError):
            dk._pipe(q, columns=True, column_params=bad).predict(img)
    # the switch off: today's page, and where no reading order is applied the switch has no effect
    again = dk._pipe(q, columns=False).predict(img)
    assert type(again.blocks[0]) is Block and again.model_dump() == off.model_dump()
    raw = dk._pipe(q, columns=True).predict(img, recognize_text=False)
    assert len(raw.blocks) == 1 and type(raw.blocks[0]) is Block
    # a page of one region keeps the plain order
    single = _rects(tl.text_page(lines=6, per_line=5))
    a, b = dk._pipe(single).predict(img), dk._pipe(single, columns=True).predict(img)
    assert len(b.blocks) == 1 and type(b.blocks[0]) is Region and dk._polys(a) == dk._polys(b)
    assert b.model_dump() == a.model_dump()


def test_pipeline_columns_with_deskew_on_a_turned_two_column_page():
    from manuscript_ocr_amd.detectors._types import Region, RegionLine, SkewPage
    boxes, truth = layout_page(cols=2, lines=20, per_line=4, gutter=64, seed=3)  # 3 degrees shear 720 px of column by 38: no band
    hw = (900, 700)
    q = dk.turn(_rects(boxes), 3.0, (0.5 * hw[1], 0.5 * hw[0])).astype(np.float32)
    img = np.zeros(hw + (3,), dtype=np.uint8)
    want = [[tuple(map(float, pt)) for pt in q[k]] for k in truth]
    assert dk._polys(dk._pipe(q, columns=True).predict(img)) != want, "in the page frame no empty band of 40 is left between the columns"
    on = dk._pipe(q, columns=True, deskew=True).predict(img)
    assert type(on) is SkewPage and abs(on.skew_deg - 3.0) < 0.2 and [type(b) for b in on.blocks] == [Region, Region]
    assert dk._polys(on) == want and [b.bbox for b in on.blocks] == [_union(b.words) for b in on.blocks]
    lines = dk._pipe(q, columns=True, deskew=True, group_lines=True).predict(img)
    assert type(lines) is SkewPage and [type(b) for b in lines.blocks] == [RegionLine] * 40
    assert [b.region for b in lines.blocks] == [0] * 20 + [1] * 20 and [len(b.words) for b in lines.blocks] == [4] * 40
    assert dk._polys(lines) == want and [b.bbox for b in lines.blocks] == [_union(b.words) for b in lines.blocks]


def test_pipeline_columns_splits_blocks_block_major():
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors._types import Region
    left, _t = layout_page(cols=2, lines=3, per_line=2, seed=4)
    words = lambda b: [tl._word(*[float(v) for v in bx]) for bx in b.tolist()]
    p = Pipeline(detector=tl.StandInDetector([words(left), [], words(left + [0, 300, 0, 300])]), recognizer=tl.StandInRecognizer())
    p.columns = True
    page = p.predict(np.zeros((500, 500, 3), dtype=np.uint8))
    assert [type(b) for b in page.blocks] == [Region] * 4 and [b.index for b in page.blocks] == [0, 1, 2, 3]
    assert [len(b.words) for b in page.blocks] == [6, 6, 6, 6] and page.blocks[2].bbox[1] >= 300


# ================================================================================================ 4. the C ABI
def test_new_symbols_refusals_and_workspace_size():
    import __graft_entry__ as g
    g.build()
    from manuscript_ocr_amd import _native, ops
    header = open(os.path.join(ROOT, "include", "msocr.h")).read()
    declared = set(re.findall(r"\b(msocr_[a-z0-9_]+)\s*\(", header))
    for name in ("msocr_reading_order_regions", "msocr_reading_order_regions_workspace_bytes", "msocr_reading_order_region_rows",
                 "msocr_reading_regions_host"):
        assert name in declared and name in _native.exported_symbols() and hasattr(_native.lib(), name), name
    L = _native.lib()
    assert [L.msocr_reading_order_region_rows(n) for n in (1, 200, 256, 257, 16400)] == [1, 200, 256, 256, 256]
    for n, mc in ((1, 1), (3, 300), (2, 16384), (2, 20000)):
        cap = min(mc, 16384)
        assert L.msocr_reading_order_regions_workspace_bytes(n, mc) == L.msocr_reading_order_deskew_workspace_bytes(n, mc) + n * 4 * (-(-3 * cap // 4) * 4)
    assert L.msocr_reading_order_regions_workspace_bytes(0, 5) == 0
    assert all(hasattr(ops, f) for f in ("reading_order_regions", "reading_regions_host", "column_ratios", "ReadingRegions"))
    b = np.array([[0, 0, 10, 10], [50, 0, 60, 10]], dtype=np.int32)
    o, ln, lr, rg, rr = (np.full(s, -7, dtype=np.int32) for s in (2, 2, (2, 6), 2, (2, 6)))
    nl, nr = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    call = lambda ratios, outs: L.msocr_reading_regions_host(ptr(b), 2, 0.6, INF, *ratios, *outs)
    full = [ptr(o), ptr(ln), ptr(lr), ptr(nl), ptr(rg), ptr(rr), ptr(nr)]
    assert call(DEFAULTS, full) == 0 and nl[0] == 1 and nr[0] == 1
    for k in range(3):
        for bad in (NAN, -1.0, -INF):
            ratios = list(DEFAULTS)
            ratios[k] = bad
            assert call(ratios, full) == -1, (k, bad)
        ratios = list(DEFAULTS)
        ratios[k] = INF
        assert call(ratios, full) == 0
    for miss in range(7):
        outs = list(full)
        outs[miss] = None
        assert call(DEFAULTS, outs) == -1, miss
    assert L.msocr_reading_regions_host(None, 0, 0.6, INF, *DEFAULTS, None, None, None, ptr(nl), None, None, ptr(nr)) == 0 and nr[0] == 0
    assert L.msocr_reading_regions_host(None, -1, 0.6, INF, *DEFAULTS, *full) == -1
    with pytest.raises(ValueError):
        ops.column_ratios({"col_gap_ratio": NAN})
    assert ops.column_ratios({"row_gap_ratio": INF}) == (2.0, INF, 3.0)
