"""Text lines as a result (Pipeline.group_lines), the part that needs no GPU: the host twin msocr_reading_lines_host against a
Python restatement of the line grouping, the generic route of Pipeline with stand-in plugins, and the C ABI's symbol lists.

The yardstick.  The reference's sort_boxes_reading_order builds the lines and returns only the flattened list, and so does its
restatement in oracle/pipeline_glue.py.  `lines_of` below restates the grouping once more and returns the lines; `expected` asserts
on every input that the flattening equals oracle.pipeline_glue.sort_boxes_reading_order_with_resolutions before anything is compared
against it.  Everything is integer or f64 arithmetic in the reference's written order, so every comparison here is for equality.

tests/test_gpu_text_lines.py takes `lines_of`, `expected`, `check_twin` and the page builders from this module.
"""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261017
INF = float("inf")


# ================================================================================================ the restatement
def lines_of(boxes, y_tol_ratio=0.6, x_gap_ratio=np.inf):
    """Integer boxes -> the text lines of sort_boxes_reading_order_with_resolutions, each a list of ORIGINAL boxes: intersections
    resolved by the oracle, grouping / line sort / word sort as the oracle's sort_boxes_reading_order writes them, boxes mapped
    back through dict(zip(shrunk, boxes))."""
    from oracle import pipeline_glue as G
    boxes = [tuple(int(v) for v in b) for b in boxes]
    shrunk = G.resolve_intersections(boxes)
    back = dict(zip(shrunk, boxes))
    if not shrunk:
        return []
    avg_h = np.mean([b[3] - b[1] for b in shrunk])
    lines = []
    for b in sorted(shrunk, key=lambda b: (b[1] + b[3]) / 2):
        cy = (b[1] + b[3]) / 2
        for ln in lines:
            line_cy = np.mean([(v[1] + v[3]) / 2 for v in ln])
            last_x1 = max(v[2] for v in ln)
            if abs(cy - line_cy) <= avg_h * y_tol_ratio and (b[0] - last_x1) <= avg_h * x_gap_ratio:
                ln.append(b)
                break
        else:
            lines.append([b])
    lines.sort(key=lambda ln: np.mean([(b[1] + b[3]) / 2 for b in ln]))
    for ln in lines:
        ln.sort(key=lambda b: b[0])
    return [[back[b] for b in ln] for ln in lines]


def expected(boxes, y_tol_ratio=0.6, x_gap_ratio=np.inf):
    """boxes -> (order [n], line [n], records [L,6]) int32 from `lines_of`, after pinning its flattening to the oracle.  order is
    the first-equal-word re-match of the pipeline; a record is {first, count, union of the line's boxes}."""
    from oracle import pipeline_glue as G
    boxes = [tuple(int(v) for v in b) for b in boxes]
    lines = lines_of(boxes, y_tol_ratio, x_gap_ratio)
    flat = [b for ln in lines for b in ln]
    assert flat == G.sort_boxes_reading_order_with_resolutions(boxes, y_tol_ratio, x_gap_ratio), "lines_of does not flatten to the oracle"
    first = {}
    for k, b in enumerate(boxes):
        first.setdefault(b, k)
    order = np.array([first[b] for b in flat], dtype=np.int32)
    line = np.array([li for li, ln in enumerate(lines) for _ in ln], dtype=np.int32)
    recs, pos = [], 0
    for ln in lines:
        a = np.array(ln, dtype=np.int64)
        recs.append([pos, len(ln), a[:, 0].min(), a[:, 1].min(), a[:, 2].max(), a[:, 3].max()])
        pos += len(ln)
    return order, line, np.array(recs, dtype=np.int32).reshape(-1, 6)


def host_order(boxes, y_tol_ratio=0.6, x_gap_ratio=INF):
    from manuscript_ocr_amd import _native as nat
    b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    order = np.empty(len(b), dtype=np.int32)
    assert nat.lib().msocr_reading_order_host(b.ctypes.data, len(b), y_tol_ratio, x_gap_ratio, order.ctypes.data) == 0
    return order


def check_structure(boxes, order, line, recs):
    """What holds for every page, whatever reference is at hand: line starts at 0 and steps by 0 or 1, the records' spans tile
    [0, n) in line order, and every box is the union NumPy forms from `order`."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    n = len(b)
    assert len(order) == n and len(line) == n
    if n == 0:
        assert len(recs) == 0
        return
    assert line[0] == 0 and set(np.diff(line).tolist()) <= {0, 1} and line[-1] == len(recs) - 1
    pos = 0
    for li, (first, count, x0, y0, x1, y1) in enumerate(recs.tolist()):
        assert first == pos and count >= 1, (li, first, count)
        assert (line[first:first + count] == li).all()
        w = b[order[first:first + count]]
        assert (x0, y0, x1, y1) == (w[:, 0].min(), w[:, 1].min(), w[:, 2].max(), w[:, 3].max()), li
        pos += count
    assert pos == n


def check_twin(boxes, y_tol_ratio=0.6, x_gap_ratio=INF, reference=True):
    """msocr_reading_lines_host on `boxes`: equal to msocr_reading_order_host in the order, sound in structure and, with
    `reference`, equal to `expected`.  Returns the twin's (order, line, records)."""
    from manuscript_ocr_amd import ops
    order, line, recs = ops.reading_lines_host(np.asarray(boxes, dtype=np.int32).reshape(-1, 4), y_tol_ratio, x_gap_ratio)
    assert order.dtype == line.dtype == recs.dtype == np.int32 and recs.shape[1:] == (6,)
    assert np.array_equal(order, host_order(boxes, y_tol_ratio, x_gap_ratio))
    check_structure(boxes, order, line, recs)
    if reference:
        eo, el, er = expected(boxes, y_tol_ratio, x_gap_ratio)
        assert np.array_equal(order, eo) and np.array_equal(line, el) and np.array_equal(recs, er)
    return order, line, recs


# ================================================================================================ pages
def golden_cases():
    return [c["boxes"] for c in json.load(open(os.path.join(ROOT, "tests", "golden", "pipeline_glue.json")))]


def random_boxes(rng, n, H=600, W=900):
    x0, y0 = rng.integers(0, W, size=n), rng.integers(0, H, size=n)
    w, h = rng.integers(0, 120, size=n), rng.integers(0, 40, size=n)
    b = np.stack([x0, y0, x0 + w, y0 + h], 1)
    if n > 8:
        b[n // 2], b[n - 1] = b[0], b[1]
    return b.tolist()


def envelope_pages():
    """The pages of tests/test_host_cpu.py::test_reading_order_host_twin_equals_python_glue_on_envelope_pages, rebuilt: boxes that
    never stop shrinking (all 50 sweeps), negative coordinates, zero height (NaN gap: every box a line, lines tie on mean cy),
    boxes that collapse to duplicate shrunk boxes, boxes across the page edges, the pair-capacity clique and a shuffled word grid."""
    rng = np.random.default_rng([SEED, 44])
    pages = {}
    neg = []
    for k in range(20):
        x, y = -40 * k - 12, -30 * (k % 5) - 9
        neg += [[x, y, -1, -1], [x - 3, y - 2, -1, -1]]
    pages["fifty_sweeps"] = neg + random_boxes(rng, 40)
    pages["negative_fractions"] = ([[-int(a) - 3, -int(b) - 2, int(c), int(d)] for a, b, c, d in rng.integers(0, 60, size=(60, 4))]
                                   + [[-90, -50, -30, -20], [-9, -9, 0, 0], [-1, -1, 1, 1]])
    pages["zero_height"] = [[int(x), int(y), int(x) + int(w), int(y)] for x, y, w in rng.integers(0, 400, size=(80, 3))]
    dup = []
    for k in range(12):
        x, y = 150 * (k % 4) + 7, 90 * (k // 4) + 3
        dup += [[x, y, x + 100, y + 50], [x, y, x + 101, y + 51]]
    pages["duplicate_shrunk"] = dup + random_boxes(rng, 30)
    H, W = 600, 900
    pages["page_edges"] = ([[-20, 100, 30, 140], [W - 25, 200, W + 40, 240], [300, -15, 380, 25], [400, H - 10, 470, H + 30], [-30, -20, 50, 40],
                            [W - 10, H - 10, W + 10, H + 10], [-80, 50, -10, 90], [100, -70, 160, -8], [-60, -50, -10, -5], [W + 5, 10, W + 60, 50],
                            [10, H + 3, 70, H + 40], [-5, -5, W + 5, H + 5], [-W - 50, 300, -W - 5, 340], [500, -H - 40, 560, -H - 2]]
                           + random_boxes(rng, 25))
    clique = [[2 * i, 2 * i, 600 + 2 * i, 400 + 2 * i] for i in range(107)]
    for k in range(25):
        x = 3000 + 100 * k
        clique += [[x, 0, x + 50, 30], [x + 20, 10, x + 70, 40]]
    pages["clique"] = clique
    i = np.arange(298)
    grid = np.stack([10 + 80 * (i % 5), 5 + 30 * (i // 5), 60 + 80 * (i % 5), 25 + 30 * (i // 5)], 1)
    pages["word_grid"] = grid[np.random.default_rng(3).permutation(298)].tolist()
    return pages


def duplicate_page():
    """Words 0 and 2 are the same box (of zero height, so that they intersect nothing and keep their place): the dict keeps one
    original and the re-match takes the first word equal to it, so two positions of the order name word 0.  avg_h = 18, tol = 10.8:
    centre y 25, 25, 27 form the first line, 95 and 97 the second."""
    return [[10, 25, 90, 25], [100, 12, 180, 42], [10, 25, 90, 25], [12, 80, 95, 110], [100, 82, 170, 112]]


# x_gap_ratio = 1: a word further right of its line than one average height opens a new line, so two lines share a centre y
TIE_GAP = 1.0


def tie_page():
    """avg_h = 20, gap = 20: word 1 starts 450 right of word 0 -> a second line at the same centre y; word 2 joins the first
    (10 right of it).  The two lines tie on mean cy = 10; creation order decides: (0, 2) then (1).  A third line below."""
    return [[0, 0, 50, 20], [500, 0, 550, 20], [60, 0, 100, 20], [5, 60, 45, 80]]


def text_page(lines=70, per_line=17, seed=SEED):
    """lines x per_line words at 60-pixel pitch in rows 40 pixels apart, every corner jittered by +-3 pixels, shuffled."""
    rng = np.random.default_rng([seed, lines, per_line])
    r, c = np.divmod(np.arange(lines * per_line), per_line)
    j = rng.integers(-3, 4, size=(lines * per_line, 4))
    b = np.stack([10 + 60 * c, 10 + 40 * r, 10 + 60 * c + 44, 10 + 40 * r + 24], 1) + j
    return b[rng.permutation(len(b))].tolist()


# ================================================================================================ 1. the host twin
def test_lines_of_flattens_to_the_reference_generated_goldens():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "pipeline_glue.json")))
    assert len(cases) == 9
    for c in cases:
        assert [list(b) for ln in lines_of(c["boxes"]) for b in ln] == c["sorted_res"]


def test_reading_lines_host_on_golden_cases():
    seen = []
    for boxes in golden_cases():
        _o, _l, recs = check_twin(boxes)
        seen.append((len(boxes), len(recs)))
    assert min(seen) == (0, 0) and max(n for n, _ in seen) == 66 and max(L for _, L in seen) == 14, seen


def test_reading_lines_host_on_envelope_pages():
    for name, boxes in envelope_pages().items():
        order, _line, recs = check_twin(boxes)
        if name == "zero_height":
            assert len(recs) == len(boxes), "NaN gap: every box is a line"
            assert len({b[1] for b in boxes}) < len(boxes), "regime: lines that tie on mean cy"
        if name == "duplicate_shrunk":
            assert len(set(order.tolist())) < len(order), "a later original replaces an earlier one"
        if name == "word_grid":
            assert len(recs) == 60 and recs[:-1, 1].tolist() == [5] * 59 and recs[-1, 1] == 3


def test_reading_lines_host_duplicates_ties_and_empty_page():
    order, line, recs = check_twin(duplicate_page())
    assert order.tolist() == [0, 0, 1, 3, 4] and line.tolist() == [0, 0, 0, 1, 1]
    assert recs.tolist() == [[0, 3, 10, 12, 180, 42], [3, 2, 12, 80, 170, 112]]
    order, line, recs = check_twin(tie_page(), 0.6, TIE_GAP)
    assert order.tolist() == [0, 2, 1, 3] and line.tolist() == [0, 0, 1, 2]
    assert recs.tolist() == [[0, 2, 0, 0, 100, 20], [2, 1, 500, 0, 550, 20], [3, 1, 5, 60, 45, 80]]
    order, line, recs = check_twin([])
    assert len(order) == 0 and len(line) == 0 and recs.shape == (0, 6)
    from manuscript_ocr_amd import _native as nat
    nl = np.full(1, -7, dtype=np.int32)
    assert nat.lib().msocr_reading_lines_host(None, 0, 0.6, INF, None, None, None, nl.ctypes.data) == 0 and nl[0] == 0
    assert nat.lib().msocr_reading_lines_host(None, 0, 0.6, INF, None, None, None, None) == -1
    assert nat.lib().msocr_reading_lines_host(None, -1, 0.6, INF, None, None, None, nl.ctypes.data) == -1


def test_reading_lines_host_on_the_text_page():
    boxes = text_page()
    _o, _l, recs = check_twin(boxes)
    assert len(boxes) == 1190 and len(recs) == 70 and (recs[:, 1] == 17).all()


# ================================================================================================ 2. the generic route of Pipeline
def _word(x0, y0, x1, y1, conf=0.9):
    from manuscript_ocr_amd.detectors._types import Word
    return Word(polygon=[[x0, y0], [x1, y0], [x1, y1], [x0, y1]], detection_confidence=conf)


def _three_lines():
    """Three lines of 3, 2 and 1 words in shuffled detector order; the corners carry fractions that np.int32 truncates."""
    return [_word(210.6, 12.2, 300.9, 50.7), _word(10.5, 60.5, 100.5, 95.5), _word(10.9, 10.9, 100.2, 50.2), _word(20.3, 110.8, 90.1, 140.4),
            _word(110.4, 11.6, 200.8, 49.3), _word(120.7, 61.2, 230.6, 96.9)]


class StandInDetector:
    """The detector stand-in of tests/test_pipeline_api.py, restated: a fresh Page per call from lists of words per block."""

    def __init__(self, blocks):
        self.blocks = blocks

    def predict(self, image, vis=False, profile=False):
        from manuscript_ocr_amd.detectors._types import Block, Page
        return {"page": Page(blocks=[Block(words=list(ws)) for ws in self.blocks]), "vis_image": None, "score_map": None, "geo_map": None}


class StandInRecognizer:
    def predict(self, images):
        return [{"text": f"word{i + 1}", "confidence": 0.9 - i * 0.05} for i in range(len(images))]


IMG = np.zeros((160, 400, 3), dtype=np.uint8)


def _pipe(blocks, group_lines):
    from manuscript_ocr_amd import Pipeline
    p = Pipeline(detector=StandInDetector(blocks), recognizer=StandInRecognizer())
    assert vars(p)["group_lines"] is False
    p.group_lines = group_lines
    return p


def _flat(page):
    return [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for b in page.blocks for w in b.words]


def test_pipeline_group_lines_generic_route():
    from manuscript_ocr_amd.detectors._types import Block, Page, TextLine
    words = _three_lines()
    off = _pipe([words], False).predict(IMG)
    assert len(off.blocks) == 1 and type(off.blocks[0]) is Block
    p = _pipe([words], True)
    on = p.predict(IMG)
    assert isinstance(on, Page) and len(on.blocks) == 3, "one block per text line"
    assert all(type(b) is TextLine for b in on.blocks)
    assert [len(b.words) for b in on.blocks] == [3, 2, 1]
    assert _flat(on) == _flat(off) and len(_flat(on)) == 6
    assert [b.bbox for b in on.blocks] == [(10, 10, 300, 50), (10, 60, 230, 96), (20, 110, 90, 140)]
    assert [[w.text for w in b.words] for b in on.blocks] == [["word1", "word2", "word3"], ["word4", "word5"], ["word6"]]
    assert p.get_text(on) == "word1 word2 word3\nword4 word5\nword6"
    assert "bbox" not in on.model_dump()["blocks"][0], "a default dump serialises a TextLine as a Block"
    assert on.model_dump() == Page(blocks=[Block(words=b.words) for b in on.blocks]).model_dump()
    # where the reference applies no reading order the switch has no effect
    raw = _pipe([words], True).predict(IMG, recognize_text=False)
    assert len(raw.blocks) == 1 and type(raw.blocks[0]) is Block and [w.polygon for w in raw.blocks[0].words] == [w.polygon for w in words]


def test_pipeline_group_lines_splits_blocks_block_major():
    from manuscript_ocr_amd.detectors._types import TextLine
    words = _three_lines()
    second = [_word(300.5, 20.5, 380.5, 50.5), _word(305.5, 70.5, 390.5, 100.5), _word(210.5, 21.5, 290.5, 51.5)]
    blocks = [words[:3], [], second]  # two words of line 1 and one of line 2, an empty block, two more lines
    off = _pipe(blocks, False).predict(IMG)
    on = _pipe(blocks, True).predict(IMG)
    assert [len(b.words) for b in off.blocks] == [3, 0, 3]
    assert all(type(b) is TextLine for b in on.blocks)
    assert [len(b.words) for b in on.blocks] == [2, 1, 2, 1], "block-major, the empty block yields no line"
    assert _flat(on) == _flat(off)
    assert [b.bbox for b in on.blocks] == [(10, 10, 300, 50), (10, 60, 100, 95), (210, 20, 380, 51), (305, 70, 390, 100)]
    empty = _pipe([[]], True).predict(IMG)
    assert empty.blocks == []


def test_pipeline_group_lines_keeps_the_word_objects():
    """The words of the lines are the objects of the reordered block, not copies."""
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.detectors._types import Block, Page
    words = _three_lines()
    page = Page(blocks=[Block(words=words)])
    p = Pipeline(detector=StandInDetector([words]), recognizer=StandInRecognizer())
    recs = []
    p._order_and_crop(page, IMG, recs)
    ordered = list(page.blocks[0].words)
    p._split_lines(page, recs)
    assert [id(w) for b in page.blocks for w in b.words] == [id(w) for w in ordered]


# ================================================================================================ 3. the C ABI
def test_new_symbols_in_header_bindings_and_library():
    import __graft_entry__ as g
    g.build()
    from manuscript_ocr_amd import _native
    header = open(os.path.join(ROOT, "include", "msocr.h")).read()
    declared = set(re.findall(r"\b(msocr_[a-z0-9_]+)\s*\(", header))
    for name in ("msocr_reading_order_lines", "msocr_reading_order_line_rows", "msocr_reading_lines_host"):
        assert name in declared and name in _native.exported_symbols() and hasattr(_native.lib(), name), name
    rows = _native.lib().msocr_reading_order_line_rows
    assert [rows(n) for n in (1, 300, 4096, 4097, 16400)] == [1, 300, 4096, 4096, 4096]
