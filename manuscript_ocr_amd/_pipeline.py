"""Pipeline — drop-in for the reference orchestration
(/root/reference/src/manuscript/_pipeline.py:17-221): detect -> reading-order sort -> crop ->
recognise -> annotate, behind the same duck-typed plugin protocol
(docs/PIPELINE_API.md: detector.predict(image, vis=False, profile=...) -> {"page"}|tuple|Page,
recognizer.predict(List[np.ndarray]) -> [{"text","confidence"}|(text, conf)|other]).

`pipeline.char_details = True` (this package's extension, native path only): recognised words come back as CharWords with
per-symbol confidence and x position (detectors/_types.py).

`pipeline.rectify_crops = True` (this package's extension, absent by default): the recogniser's crops are cut ALONG the detected
quadrilaterals instead of from their axis-aligned windows (useful with EAST(axis_aligned_output=False)).
The recognised words and their order do not change, only the pixels the recogniser sees.  Native path: the device kernel
msocr_quad_crop writes the recogniser's canvases directly.  Every other route (foreign plugins, profile=True, native_fast_path =
False) cuts on the host in `_extract_word_image`.  With this package's TRBA as the recogniser it hands over the word's finished
img_h x img_w canvas from the host twin msocr_quad_crop_host, the device route's bytes, which the recogniser's ResizeAndPadA passes
through unchanged: the pages equal the device route's.  A foreign recogniser, whose canvas is not known, gets the rectified region
at its natural size and resizes it itself, so that route resamples twice.

`pipeline.group_lines = True` (this package's extension, absent by default): every block the pipeline puts into reading order comes
back as its text lines, one TextLine (detectors/_types.py) per line in reading order, holding exactly the words at the line's
positions.  The lines are the ones the reading order is built from (y_tol_ratio = 0.6, x_gap_ratio = inf),
nothing is estimated anew; `get_text` then returns one row per line.  Where the reference applies no reading order the switch has
no effect: `recognize_text=False`, on the generic route and on the batch route, returns the detector's blocks in detector order.

`pipeline.n_best = n` (this package's extension, 0 = off by default; n <= 8, the beam width the pipeline decodes with): recognised
words come back as AltWords (detectors/_types.py) whose `alternatives` are the n best final hypotheses of the recogniser's beam search
in its own order, duplicates of an earlier text dropped, entry 0 the word's own text and confidence.  They are
read out of the workspace the decode leaves behind: the decode itself, and with it every other field of the pages, does not change.
Works on the native batch path with every other switch, and on the generic route when the recogniser is this package's TRBA; a
foreign recogniser is not asked for alternatives.

`pipeline.lexicon = Lexicon(words, recognizer.stoi, recognizer.max_length)` (this package's extension, None = off by default): the
recogniser's beam search is constrained to the lexicon's words; recognised words come back as LexWords
(detectors/_types.py) whose `text` is a lexicon word and whose `lexicon_index` is its index in `lexicon.words`.  Combines with
char_details, rectify_crops, group_lines and n_best (the alternatives are then lexicon words too).  The detector's "words" carry their
punctuation: a lexicon of bare word forms forbids "слово," — the caller supplies the forms to admit.  Captured graphs are not provided
for this route: with a `use_graphs` recogniser a batch is refused at submit (ValueError).  A foreign recogniser is not asked.

`pipeline.lm = CharLM.from_texts(texts, recognizer.stoi)` with `pipeline.lm_weight` (this package's extension, None = off by default;
the weight's default 0.5 is a placeholder, not a tuned value): the recogniser's beam search is fused with a character n-gram language
model, for open-vocabulary text; recognised words come back as LmWords (detectors/_types.py) whose `lm_logp`
is the language model's unweighted log-probability of `text`; confidences stay the model's.  Combines with char_details,
rectify_crops, group_lines and n_best (every alternative then carries its own lm_logp).  With a `use_graphs` recogniser, or with
`lexicon` also set, a batch is refused at submit (ValueError).  A foreign recogniser is not asked.

`pipeline.suggest = Lexicon(words, recognizer.stoi, recognizer.max_length)` with `pipeline.suggest_k` (1..16, default 3) and
`pipeline.suggest_max_distance` (None = no bound) (this package's extension, None = off by default): approximate dictionary lookup
(with `pipeline.suggest_costs = EditCosts(...)` under confusion-weighted costs, distances then in cost units)
behind the open decode; recognised words come back as SuggestWords (SuggestLmWords when `lm` is also set;
detectors/_types.py) whose `suggestions` are the suggest_k lexicon words nearest to `text` by Levenshtein distance, with their
distances.  The decode is untouched: text and confidences are what the same batch gives without the switch.  Combines with
char_details, n_best, rectify_crops, group_lines, lm and a `use_graphs` recogniser (the lookup runs behind the decode, on its device
ids).  With `lexicon` also set a batch is refused at submit (ValueError).  A foreign recogniser is not asked.

`pipeline.deskew = True` (this package's extension, absent by default; needs EAST(axis_aligned_output=False)): the page's skew is
estimated from the detected quadrilaterals, and the reading order and the text lines are computed in the deskewed frame (DESIGN.md
section 4.19).  Only the permutation of the words and the line spans change: the word polygons, the crop windows, the recogniser's
inputs and the TextLine boxes stay in page coordinates, computed from the original boxes.  The page comes back as a SkewPage
(detectors/_types.py) whose `skew_deg` is the estimate, 0.0 where no rotation was applied (fewer than 8 words that vote, or a skew
inside the dead zone of 0.22 degrees: an upright page keeps its order bit for bit).  With axis-aligned detector output every word
is a rectangle, the estimate is zero by construction and the switch is a no-op.  The threshold of 8 words and the 14-degree gate of
the second pass are placeholders, not tuned values.  Combines with group_lines, rectify_crops, char_details, n_best, lexicon, lm and
suggest, which all sit behind the order; `score_page` takes the words as given.  Where the reference applies no reading order
(`recognize_text=False`) the switch has no effect.

`pipeline.columns = True` (this package's extension, absent by default): the page is cut into regions at its wide empty vertical and
horizontal bands (an XY-cut) ahead of the line rule, so an open book, a two-column register or a heading above
two columns is read column by column instead of straight across the gutter.  `pipeline.column_params` holds the three ratios of the
cut (col_gap_ratio, row_gap_ratio, col_min_height_ratio, in units of the page's mean word height): placeholders, not tuned values.
Every reading-ordered block comes back as its Regions (detectors/_types.py), with `group_lines` as RegionLines; both dump as a
Block.  With `deskew` the cut runs in the deskewed frame.  Combines with rectify_crops, char_details, n_best, lexicon, lm and suggest,
which all sit behind the order.  A page without a wide empty band is one region and keeps its order bit for bit.

`pipeline.score_page(image, page)` (this package's extension): the forced decode of a page whose words already carry a `text`
(an edition, a keyed-in ground truth): how well every text fits its word image and where its symbols sit.

`process_batch` is broken upstream (it calls a non-existent `self.process`, _pipeline.py:187);
here it is the per-image `predict`.  `predict_batch` is the MI355X fast path: when detector and
recogniser are this package's EAST/TRBA it runs the detector once for all pages and the
recogniser once for all crops of all pages (results identical to per-page predict).
"""
import contextlib
import gc
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch
from PIL import Image

from . import _native as nat
from . import ingest, ops
from .detectors import EAST, read_image, sort_boxes_reading_order_with_resolutions, visualize_page
from .recognizers import TRBA


@contextlib.contextmanager
def _gc_paused():
    """The batch path creates ~10^5 small container objects per step (Words, polygons, result rows); with the cyclic GC
    enabled, generation-2 passes over them land in the middle of the enqueue path (measured ~10 ms per group).  Nothing
    here forms reference cycles, so reference counting alone frees everything; the collector's state is restored on exit."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _reading_order(aabbs_i32):
    """Indices of the words in reading order: sort_boxes_reading_order_with_resolutions + the reference's "first word with an
    equal box" re-match (_pipeline.py:113-121), evaluated by the host helper msocr_reading_order_host (same arithmetic)."""
    boxes = np.ascontiguousarray(aabbs_i32, dtype=np.int32)
    order = np.empty(len(boxes), dtype=np.int32)
    nat.check(nat.lib().msocr_reading_order_host(boxes.ctypes.data, len(boxes), 0.6, float("inf"), order.ctypes.data), "reading_order_host")
    return order.tolist()


_NO_LINES = np.empty((0, 6), dtype=np.int32)  # the line records of a block without words


def _word_aabb(word):
    poly = np.array(word.polygon, dtype=np.int32)  # float -> int32 truncation (reference :106)
    x_min, y_min = np.min(poly, axis=0)
    x_max, y_max = np.max(poly, axis=0)
    return (x_min, y_min, x_max, y_max), poly


def _word_quads(words):
    """[n,8] f32 corners of the words as stored; a polygon that is not four points gets NaN corners (it does not vote and keeps its box)."""
    q = np.full((len(words), 8), np.nan, dtype=np.float32)
    for k, w in enumerate(words):
        if len(w.polygon) == 4:
            q[k] = np.asarray(w.polygon, dtype=np.float32).reshape(8)
    return q


def _page_skew(page):
    """deskew: the skew of a page from the quads of all its words -> (skew, cs, skew_deg) (ops.page_skew_host); skew_deg is for
    reporting only, 0.0 where the rotation is not applied."""
    skew, cs = ops.page_skew_host(_word_quads([w for block in page.blocks for w in block.words]))
    return skew, cs, (float(np.degrees(np.arctan2(float(skew[1]), float(skew[0])))) if skew[3] else 0.0)


def _ordering_boxes(words, aabbs_i32, page_hw, skew, cs):
    """deskew: the boxes the reading order sees, [n,4] int32: the words' own boxes where the rotation is not applied, else the boxes
    of the rotated corners (ops.deskew_boxes_host); a word without four finite corners keeps its own box."""
    aabbs = np.ascontiguousarray(aabbs_i32, dtype=np.int32).reshape(-1, 4)
    if not skew[3] or not len(aabbs):
        return aabbs
    quads = _word_quads(words)
    boxes = ops.deskew_boxes_host(quads, page_hw, skew, cs)
    plain = ~np.isfinite(quads).all(axis=1)
    boxes[plain] = aabbs[plain]
    return boxes


def _page_frame_records(recs, order, aabbs_i32):
    """deskew: line records of the ordering boxes -> the same spans with x0..y1 = the union of the ORIGINAL boxes of the words at
    the line's positions."""
    at_pos = np.ascontiguousarray(aabbs_i32, dtype=np.int32).reshape(-1, 4)[np.asarray(order, dtype=np.int64)]
    out = np.array(recs, dtype=np.int32).reshape(-1, 6)
    for r in out:
        seg = at_pos[r[0]:r[0] + r[1]]
        r[2:4], r[4:6] = seg[:, :2].min(axis=0), seg[:, 2:].max(axis=0)
    return out


@dataclass(slots=True)
class _Group:
    """One group of consecutive pages of a batch, with the same fields on both routes; what a route does not produce stays None."""
    lo: int
    hi: int
    stream: Any                      # crops + recogniser
    det_stream: Any                  # detector, reading order, the small uploads
    det: Any                         # the detector's Detection
    det_event: Any                   # the detector outputs (and descriptors) of this group are complete
    ro: Any = None                   # ops.ReadingOrder of the group's pages (device_order)
    rl: Any = None                   # ops.ReadingLines behind it (group_lines)
    qd: Any = None                   # [pages,max_cand,12] device quad descriptors behind it (rectify_crops)
    sk: Any = None                   # ops.PageSkew behind it (deskew)
    rg: Any = None                   # ops.ReadingRegions behind it (columns)
    device_ordered: bool = False     # advance_batch took the device route: Page / Word assembly is collect_batch's
    words: Optional[list] = None     # the Words that got a crop, in crop order
    spans: List[List[int]] = field(default_factory=list)  # per page [first crop, crops]
    handle: Any = None               # the recogniser's handle; None = no crops
    desc_host: Any = None            # crop descriptors int32 [M,8]: numpy on the host route,
    desc_dev: Any = None             # ... a device tensor on the device route (kept only for char_details)
    qdesc_host: Any = None           # quad descriptors int32 [M,12] (rectify_crops), likewise
    qdesc_dev: Any = None


@dataclass(slots=True)
class _Batch:
    """Handle of submit_batch -> advance_batch -> collect_batch."""
    arrays: list                     # per page: the host pixels, or a zero-stride placeholder of the right shape
    pages_dev: Any                   # [N,H,W,3] u8 on the device
    main: Any                        # the caller's stream
    groups: List[_Group]
    recognize_text: bool
    profile: bool
    rectify: bool                    # rectify_crops as it was at submit
    line_recs: Optional[dict]        # group_lines as it was at submit: page index -> per block its [L,6] line records; None = off
    n_best: int                      # n_best as it was at submit
    lexicon: Any                     # lexicon as it was at submit; None = the open search
    lm: Any                          # lm as it was at submit; None = the model's own scores
    lm_weight: float                 # lm_weight as it was at submit
    ingest_pending: Any              # the device JPEG stages' deferred verdict, read in advance_batch
    resubmit: Callable[[], "_Batch"]  # the same batch again through the host JPEG decoder
    pages: Optional[list] = None     # set by advance_batch (which makes it idempotent), filled by both stages
    tm: Optional[Dict[str, float]] = None  # host seconds per stage -> Pipeline.last_profile
    suggest: Optional[tuple] = None  # (suggest, suggest_k, suggest_max_distance, suggest_costs) as they were at submit; None = off
    skews: Optional[dict] = None     # deskew as it was at submit: page index -> skew_deg; None = off
    region_recs: Optional[dict] = None  # columns as it was at submit: page index -> per block its [R,6] region records; None = off
    ratios: Optional[tuple] = None   # column_params as they were at submit: the three ratios of the cut; None = off

    def replace_with(self, other):
        """Become `other` (the corrupt-JPEG resubmission) while staying the object the caller holds."""
        for name in self.__slots__:
            setattr(self, name, getattr(other, name))


class Pipeline:
    def __init__(self, detector: Optional[EAST] = None, recognizer: Optional[TRBA] = None, min_text_size: int = 5):
        self.detector = detector if detector is not None else EAST()
        self.recognizer = recognizer if recognizer is not None else TRBA()
        self.min_text_size = min_text_size
        # Switches: plain attributes, set after construction (the constructor keeps the reference's signature).  DESIGN.md section 7c.
        self.native_fast_path = True       # predict() of this package's plugins goes through predict_batch; False = generic route (test hook)
        self.device_ingest = True          # JPEG files are decoded on the device (ingest.py); False = read_image on the host (test hook)
        self.device_entropy = None         # Huffman stage: None = ingest's policy, True / False force the device stages / host pool (tests, bench.py)
        self.device_order = True           # reading order + crop descriptors on the device; False = on the host (test hook)
        self.rectify_crops = False         # crops cut along the detected quadrilaterals (user extension, see the module docstring)
        self.char_details = False          # recognised words come back as CharWords with per-symbol details (user extension)
        self.group_lines = False           # every reading-ordered block comes back as its text lines, one TextLine each (user extension)
        self.deskew = False                # reading order and text lines in the deskewed frame, SkewPages come back (user extension)
        self.columns = False               # the page is cut into regions ahead of the line rule, Regions / RegionLines come back (user extension)
        self.column_params = dict(ops.COLUMN_PARAMS)  # the three ratios of that cut; placeholders, not tuned values
        self.n_best = 0                    # > 0: recognised words come back as AltWords with the beam search's n best readings (user extension)
        self.lexicon = None                # a recognizers.Lexicon: the beam search is constrained to its words, LexWords come back (user extension)
        self.lm = None                     # a recognizers.CharLM: the beam search is fused with it, LmWords come back (user extension)
        self.lm_weight = 0.5               # weight of the language model's log-probabilities; a placeholder, not a tuned value
        self.suggest = None                # a recognizers.Lexicon: every word gets its nearest lexicon words, SuggestWords come back (user extension)
        self.suggest_k = 3                 # suggestions per word, 1..16
        self.suggest_max_distance = None   # drop suggestions further away than this many edits; None = no bound
        self.suggest_costs = None          # a recognizers.EditCosts: rank the suggestions by the confusion-weighted distance (needs suggest)
        self.serialize_streams = False     # every group on the caller's stream: same launches, no overlap (profiling aid, bench.py)
        self.stream_sets = 2               # batches that may be in flight at once, each on its own set of streams (bench.py, tests)
        self.det_stream_priority = True    # detector streams are created at high priority; False = normal (profiling aid)
        self.upload_on_det_stream = True   # host route: the small blocking uploads ride the detector stream (bench.py A/B)
        self._stream_sets, self._det_stream_sets, self._set_idx = [], [], 0  # submit_batch's streams, per set one per group
        self._copy_stream = None           # collect_batch's read-back stream

    # ------------------------------------------------------------------------------------- helpers
    @staticmethod
    def _page_of(det_out):
        if isinstance(det_out, dict):
            page = det_out.get("page")
        elif isinstance(det_out, tuple):
            page = det_out[0]
        else:
            page = det_out
        if page is None:
            raise RuntimeError("Detector did not return a Page result.")
        return page

    def _order_and_crop(self, page, image_array, line_recs=None, skew=None, region_recs=None, ratios=None):
        """_pipeline.py:102-137: reorder every block in reading order, collect crops of words >= min_text_size.
        `line_recs` (a list, group_lines): gets every block's line records from the host twin on the same AABBs; the order stays the
        Python function's (tests/test_host_cpu.py pins the two orders to be equal).  `skew` (deskew): the page's (skew, cs) with the
        rotation applied: order and lines come from the host twins on the ordering boxes, the records' boxes from the words' own.
        `region_recs` (a list) and `ratios` (columns): order, lines and every block's region records come from
        msocr_reading_regions_host, on the ordering boxes where `skew` is given."""
        words, crops = [], []
        for block in page.blocks:
            boxes = [_word_aabb(w)[0] for w in block.words]
            if ratios is not None:
                if block.words:
                    seen = boxes if skew is None else _ordering_boxes(block.words, boxes, image_array.shape[:2], *skew)
                    order, _line, recs, _region, rrecs = ops.reading_regions_host(seen, 0.6, float("inf"), *ratios)
                    recs, rrecs = _page_frame_records(recs, order, boxes), _page_frame_records(rrecs, order, boxes)
                    block.words = [block.words[k] for k in order.tolist()]
                else:
                    recs = rrecs = _NO_LINES
                region_recs.append(rrecs)
                if line_recs is not None:
                    line_recs.append(recs)
                boxes = None
            elif skew is not None and block.words:
                order, _line, recs = ops.reading_lines_host(_ordering_boxes(block.words, boxes, image_array.shape[:2], *skew))
                if line_recs is not None:
                    line_recs.append(_page_frame_records(recs, order, boxes))
                block.words = [block.words[k] for k in order.tolist()]
                boxes = None
            elif line_recs is not None:
                line_recs.append(ops.reading_lines_host(np.array(boxes, dtype=np.int32).reshape(-1, 4))[2])
            if boxes is not None:
                first = {}
                for k, bx in enumerate(boxes):  # first equal word wins, as the reference's tuple comparison (:113-121)
                    first.setdefault(tuple(int(v) for v in bx), k)
                block.words = [block.words[first[tuple(int(v) for v in bx)]] for bx in sort_boxes_reading_order_with_resolutions(boxes)]
            for word in block.words:
                (x0, y0, x1, y1), poly = _word_aabb(word)
                if (x1 - x0) >= self.min_text_size and (y1 - y0) >= self.min_text_size:
                    region = self._extract_word_image(image_array, poly, quad=word.polygon)
                    if region is not None and region.size > 0:
                        words.append(word)
                        crops.append(region)
        return words, crops

    @staticmethod
    def _assign(words, results):
        for word, result in zip(words, results):
            if isinstance(result, dict):
                text, confidence = result.get("text", ""), result.get("confidence", None)
            elif isinstance(result, tuple) and len(result) == 2:
                text, confidence = result
            else:
                text, confidence = (str(result) if result is not None else ""), None
            word.text = text
            word.recognition_confidence = confidence

    _BEAM_SIZE = 8  # the width the recogniser is called with: its default

    def _n_best(self):
        """The `n_best` switch for a call that recognises with this package's TRBA."""
        n = int(self.n_best)
        if not 0 <= n <= self._BEAM_SIZE:
            raise ValueError(f"Pipeline.n_best must be between 0 and {self._BEAM_SIZE}, the recogniser's beam width, got {n}")
        return n

    # ------------------------------------------------------------------------------------- API
    def predict(self, image: Union[str, np.ndarray, Image.Image], recognize_text: bool = True, vis: bool = False,
                profile: bool = False):
        if (isinstance(self.detector, EAST) and isinstance(self.recognizer, TRBA) and recognize_text and not profile
                and self.native_fast_path):
            # both plugins are this package's: same result through the device path (crops cut, resized and padded on the
            # device from the uploaded page, one recogniser pass) — tests/test_gpu_pipeline.py pins batch == per-page
            page = self.predict_batch([image])[0]  # a JPEG path is decoded on the device (ingest.py), arrays are uploaded
            if vis:
                pil = image if isinstance(image, Image.Image) else Image.fromarray(read_image(image))
                return page, visualize_page(pil, page, show_order=True)
            return page
        start = time.time()
        t0 = time.time()
        page = self._page_of(self.detector.predict(image, vis=False, profile=profile))
        if profile:
            print(f"Detection: {time.time() - t0:.3f}s")
        if not recognize_text:
            if vis:
                arr = read_image(image)
                pil = image if isinstance(image, Image.Image) else Image.fromarray(arr)
                return page, visualize_page(pil, page, show_order=False)
            return page
        t0 = time.time()
        image_array = read_image(image)
        if profile:
            print(f"Load image for crops: {time.time() - t0:.3f}s")
        t0 = time.time()
        line_recs = [] if self.group_lines else None
        skew = _page_skew(page) if self.deskew else None
        ratios = ops.column_ratios(self.column_params) if self.columns else None
        region_recs = [] if ratios is not None else None
        words, crops = self._order_and_crop(page, image_array, line_recs, skew[:2] if skew is not None and skew[0][3] else None,
                                            region_recs, ratios)
        if profile:
            print(f"Extract {len(crops)} crops: {time.time() - t0:.3f}s")
        if crops:
            t0 = time.time()
            n_best = self._n_best() if isinstance(self.recognizer, TRBA) else 0  # a foreign recogniser is not asked
            lexicon = self.lexicon if isinstance(self.recognizer, TRBA) else None
            lm = self.lm if isinstance(self.recognizer, TRBA) else None
            suggest = self.suggest if isinstance(self.recognizer, TRBA) else None
            suggest_costs = self.suggest_costs if isinstance(self.recognizer, TRBA) else None
            extra = {**({"n_best": n_best} if n_best else {}), **({"lexicon": lexicon} if lexicon is not None else {}),
                     **({"lm": lm, "lm_weight": self.lm_weight} if lm is not None else {}),
                     **({"suggest": suggest, "suggest_k": self.suggest_k, "suggest_max_distance": self.suggest_max_distance}
                        if suggest is not None else {}),
                     **({"suggest_costs": suggest_costs} if suggest_costs is not None else {})}
            results = self.recognizer.predict(crops, **extra)
            if profile:
                print(f"Recognition: {time.time() - t0:.3f}s")
            self._assign(words, [results[i] for i in range(len(words))])
            if n_best or lexicon is not None or lm is not None or suggest is not None:
                self._attach_details(words, [page], alts=[results[i]["alternatives"] for i in range(len(words))] if n_best else None,
                                     lex_idx=None if lexicon is None else [results[i]["lexicon_index"] for i in range(len(words))],
                                     lm_logp=None if lm is None else [results[i]["lm_logp"] for i in range(len(words))],
                                     suggestions=None if suggest is None else [results[i]["suggestions"] for i in range(len(words))])
        if region_recs is not None:
            self._split_regions(page, region_recs, line_recs)
        elif line_recs is not None:
            self._split_lines(page, line_recs)
        if skew is not None:
            page = self._skew_page(page, skew[2])
        if profile:
            print(f"Pipeline total: {time.time() - start:.3f}s")
        if vis:
            pil = image if isinstance(image, Image.Image) else Image.fromarray(image_array)
            return page, visualize_page(pil, page, show_order=True)
        return page

    def _order_boxes(self, page, line_recs=None, deskew_hw=None, region_recs=None, ratios=None):
        """Reading-order reorder of every block (in place) + AABBs of the words that pass min_text_size.
        Same semantics as _pipeline.py:102-133 of the reference, vectorised.  `line_recs` (a list, group_lines): order and line
        records of every block then come from msocr_reading_lines_host, and the records are appended to it.  `deskew_hw` (the page's
        (H, W), deskew): the order and the lines are those of the ordering boxes of the deskewed frame, everything else stays the
        original boxes'; returns the page's skew_deg as a third value.  `region_recs` (a list) and `ratios` (columns): order, lines
        and every block's region records come from msocr_reading_regions_host."""
        words, boxes = [], []
        skew = _page_skew(page) if deskew_hw is not None else None
        for block in page.blocks:
            if not block.words:
                if line_recs is not None:
                    line_recs.append(_NO_LINES)
                if region_recs is not None:
                    region_recs.append(_NO_LINES)
                continue
            # AABBs of all words at once: np.array(polygon, int32) truncates toward zero (_pipeline.py:106)
            polys = np.array([w.polygon for w in block.words], dtype=np.float64).astype(np.int32)
            mins, maxs = polys.min(axis=1), polys.max(axis=1)
            aabbs = [(a[0], a[1], b[0], b[1]) for a, b in zip(mins, maxs)]
            own = np.concatenate([mins, maxs], axis=1)
            seen = _ordering_boxes(block.words, own, deskew_hw, skew[0], skew[1]) if skew is not None and skew[0][3] else own
            if ratios is not None:
                order, _line, recs, _region, rrecs = ops.reading_regions_host(seen, 0.6, float("inf"), *ratios)
                order = order.tolist()
                region_recs.append(rrecs if seen is own else _page_frame_records(rrecs, order, own))
                if line_recs is not None:
                    line_recs.append(recs if seen is own else _page_frame_records(recs, order, own))
            elif line_recs is None:
                order = _reading_order(seen)
            else:
                order, _line, recs = ops.reading_lines_host(seen)
                order = order.tolist()
                line_recs.append(recs if seen is own else _page_frame_records(recs, order, own))
            old_words = block.words
            block.words = [old_words[k] for k in order]
            for k in order:
                x0, y0, x1, y1 = aabbs[k]
                if (x1 - x0) >= self.min_text_size and (y1 - y0) >= self.min_text_size:
                    words.append(old_words[k])
                    boxes.append((x0, y0, x1, y1))
        if skew is not None:
            return words, boxes, skew[2]
        return words, boxes

    def predict_batch(self, images: List[Union[str, np.ndarray]], recognize_text: bool = True, profile: bool = False,
                      pages_dev=None, sub_batches: int = 0, _maps_override=None):
        """Pages -> list of Pages, same results as per-page `predict`.  Pages of different sizes are processed as one group per
        size (the word crops are cut from the ORIGINAL pages, which only stack when they are equally sized; the detector alone
        batches any mix: EAST.predict_batch), results returned in input order.

        MI355X fast path (detector and recogniser are this package's EAST / TRBA): the pages are uploaded once,
        word crops are cut, resized and padded ON THE DEVICE from the resident pages (no host crop, no per-crop upload)
        and the recogniser runs over all crops of a sub-batch at once — while the decode run lengths that enter the
        confidences still follow the reference's per-page / per-`batch_size` chunking.  The batch is processed as
        `sub_batches` groups on separate HIP streams in a software pipeline, so the host stages of one group (box
        filters, reading order, crop descriptors) overlap the device work of the others.
        `pages_dev`: optional [N,H,W,3] u8 device tensor already holding `images` (benchmarks: inputs resident in HBM).
        = collect_batch(submit_batch(...)); call the two halves yourself to overlap consecutive batches."""
        if not (isinstance(self.detector, EAST) and isinstance(self.recognizer, TRBA)):
            return [self.predict(im, recognize_text=recognize_text, profile=profile) for im in images]
        if pages_dev is None and len(images) > 1:
            shapes = [self._shape_of(im) for im in images]
            if len(set(shapes)) > 1:
                # ragged batch: every size group's detector work is enqueued before the first group is collected
                groups = {}
                for i, sh in enumerate(shapes):
                    groups.setdefault(sh, []).append(i)
                def maps_of(idx):  # injected maps (tests / benchmarks) follow their pages
                    if _maps_override is None:
                        return None
                    sel = torch.tensor(idx, device=_maps_override[0].device)
                    return (_maps_override[0].index_select(0, sel), _maps_override[1].index_select(0, sel))
                handles = []
                for idx in groups.values():
                    mo = maps_of(idx)  # kept alive in `handles` until the group is collected: the detector streams read it asynchronously
                    handles.append((idx, self.submit_batch([images[i] for i in idx], recognize_text, profile, None, sub_batches, mo), mo))
                out = [None] * len(images)
                for idx, h, _mo in handles:
                    for i, pg in zip(idx, self.collect_batch(h)):
                        out[i] = pg
                return out
        return self.collect_batch(self.submit_batch(images, recognize_text, profile, pages_dev, sub_batches, _maps_override))

    @staticmethod
    def _shape_of(im):
        """(height, width) of a page as read_image / the device ingest return it, without decoding it twice: arrays know theirs,
        files are asked through PIL's header parse — the stored size, swapped when the Exif orientation (tag 0x0112) is 5..8."""
        if isinstance(im, np.ndarray):
            return tuple(im.shape[:2])
        try:
            with Image.open(im) as f:
                if f.getexif().get(0x0112) in (5, 6, 7, 8):
                    return (f.width, f.height)
                return (f.height, f.width)
        except Exception:
            return tuple(read_image(im).shape[:2])

    def submit_batch(self, images, recognize_text: bool = True, profile: bool = False, pages_dev=None, sub_batches: int = 0,
                     _maps_override=None, _device_entropy=None):
        """Stage 1 of `predict_batch`: upload (if needed) and enqueue every group's detector work; returns a handle
        without synchronising.  Consecutive submits alternate between two sets of streams, so the detector work of
        batch i+1 can be enqueued before `collect_batch` of batch i and fills the device while batch i drains."""
        if not (isinstance(self.detector, EAST) and isinstance(self.recognizer, TRBA)):
            raise TypeError("submit_batch/collect_batch need this package's EAST and TRBA plugins")
        det, n_best, lexicon, lm, lm_weight = self.detector, self._n_best(), self.lexicon, self.lm, self.lm_weight
        if lm is not None:
            self.recognizer._check_lm(lm, lm_weight, "beam", lexicon)
            if self.recognizer.use_graphs:
                raise ValueError("Pipeline.lm with a use_graphs recogniser: captured graphs are not provided for the decode fused with a "
                                 "language model; construct the recogniser without use_graphs")
        if lexicon is not None:
            self.recognizer._check_lexicon(lexicon, "beam")
            if self.recognizer.use_graphs:
                raise ValueError("Pipeline.lexicon with a use_graphs recogniser: captured graphs are not provided for the lexicon-constrained "
                                 "decode; construct the recogniser without use_graphs")
        suggest = None if self.suggest is None else (self.suggest, self.suggest_k, self.suggest_max_distance, self.suggest_costs)
        if suggest is not None:
            self.recognizer._check_suggest(*suggest[:3], lexicon, "beam", suggest[3])
        elif self.suggest_costs is not None:
            raise ValueError("Pipeline.suggest_costs needs Pipeline.suggest: the costs weight a lexicon lookup, they start none")
        # image ingest: a JPEG file is decoded ON THE DEVICE (Huffman stage + reconstruction, ingest.py) — the page's
        # pixels never exist on the host, `arrays` then only carries the shape; everything else goes through read_image
        dec, ingest_pending = [None] * len(images), None
        # Which Huffman stage: ingest's policy (the per-interval kernel for short restart intervals, the self-synchronising stage
        # for long ones and for files without restart markers; `pipeline.device_entropy = True / False` forces the device stages /
        # the host pool).
        # From files, same box: device stage 79.5-80.1, host pool 78.2-79.2 pages/s against 83.0 resident.
        if _device_entropy is None:
            _device_entropy = self.device_entropy
        ing = torch.cuda.current_stream()
        with torch.cuda.stream(ing):
            if pages_dev is None and self.device_ingest:
                # the device stages' verdict on corrupt streams (and the pages the self-synchronising stage declined) is read in
                # advance_batch (ingest.check_pending), not here
                dec, ingest_pending = ingest.read_images_device(list(images), det.device, device_entropy=_device_entropy, defer_status=True)
            arrays = [np.broadcast_to(np.uint8(0), tuple(t.shape)) if t is not None else read_image(im) for im, t in zip(images, dec)]
            if len({a.shape for a in arrays}) != 1:
                raise ValueError("predict_batch needs equally sized pages")
            N = len(arrays)
            if pages_dev is None:
                if not any(t is not None for t in dec):
                    pages_dev = torch.from_numpy(np.ascontiguousarray(np.stack(arrays))).to(det.device)
                else:
                    pages_dev = torch.stack([t if t is not None else torch.from_numpy(np.ascontiguousarray(a)).to(det.device)
                                             for t, a in zip(dec, arrays)])
        # groups per batch.  Round 1 needed 8 groups of 2 pages to hide its host stages behind other groups' device work; with the
        # reading order on the device and Page assembly off the enqueue path, larger launch sequences win (bigger GEMM M, fewer
        # launches): 16 pages measured 44.0 / 45.4 / 45.7 pages/s at 8 / 4 / 2 groups with 4 hardware queues and 36.3 / 46.8 / 48.1
        # with 8; one group ties two at lower memory, two keeps a second detector sequence in flight
        nsub = sub_batches or (2 if N >= 8 else 1)
        nsub = max(1, min(nsub, N))
        H, W = arrays[0].shape[:2]
        bounds = [(N * k // nsub, N * (k + 1) // nsub) for k in range(nsub)]
        main = torch.cuda.current_stream()
        if self.serialize_streams:  # profiling aid: same launches, no cross-stream kernel overlap
            streams = det_streams = [main] * nsub
        else:
            # Two stream sets alternate between consecutive batches.  Per group: a HIGH-priority stream for the detector and a
            # normal one for crops + recogniser.  Detection is the short head of a group's work and the host needs its boxes
            # before it can enqueue the long recogniser tail: with equal priorities the detector kernels of batch i+1 share the
            # chip fairly with the recogniser of batch i and finish together with it, so the next recogniser work is enqueued
            # only when the device has already drained (measured: 5 % idle); at high priority they overtake it.
            nsets = max(1, int(self.stream_sets))  # batches that may be in flight at once
            # Every stream keeps its own allocator pool (stream-ordered reuse without waiting for the device), so reserved memory
            # grows with the number of streams in flight x the per-page activation footprint: measured 96 GB at 16 pages x
            # 1536 x 2048 with two stream sets = 1.9 KB per page pixel.  When two sets would not fit comfortably (configs[4]:
            # 16 pages x 3072 x 4096 -> 380 GB) consecutive batches share ONE set of streams: half the memory, still
            # stream-ordered, a little less overlap between batches — instead of an allocator that thrashes at the 288 GB limit.
            if nsets > 1 and 1900.0 * N * H * W > 0.6 * torch.cuda.get_device_properties(pages_dev.device).total_memory:
                nsets = 1
            if len(self._stream_sets) != nsets:
                self._stream_sets, self._det_stream_sets, self._set_idx = [[] for _ in range(nsets)], [[] for _ in range(nsets)], 0
            self._set_idx = (self._set_idx + 1) % nsets
            pool, dpool = self._stream_sets[self._set_idx], self._det_stream_sets[self._set_idx]
            hi_prio = -1 if self.det_stream_priority else 0
            while len(pool) < nsub:
                pool.append(torch.cuda.Stream())
                dpool.append(torch.cuda.Stream(priority=hi_prio))
            streams, det_streams = pool[:nsub], dpool[:nsub]
        rec, rectify, group_lines, groups = self.recognizer, bool(self.rectify_crops), bool(self.group_lines), []
        deskew = bool(self.deskew)
        ratios = ops.column_ratios(self.column_params) if self.columns else None
        for (lo, hi), st, dst in zip(bounds, streams, det_streams):
            if dst is not main:
                dst.wait_stream(main)
            with torch.cuda.stream(dst):
                mo = None if _maps_override is None else (_maps_override[0][lo:hi], _maps_override[1][lo:hi])
                dh = det.detect_start(pages_dev[lo:hi], mo)
                # reading order + crop descriptors of the group's pages on the device, right behind the box filters: the host
                # then needs only the crop COUNTS to enqueue the recogniser (Page / Word assembly moves to collect_batch)
                ro = rl = qd = sk = rg = None
                if recognize_text and dh.final_boxes is not None and self.device_order:
                    if ratios is not None:  # the same kernel body with the XY-cut ahead of the line walk
                        ro, rl, sk, rg = ops.reading_order_regions(dh.final_boxes, dh.final_counts, (H, W), self.min_text_size, rec.img_h,
                                                                   rec.img_w, lo, 0.6, float("inf"), *ratios, lines=group_lines, deskew=deskew)
                    elif deskew:  # the same kernel body with the skew estimate and the ordering boxes compiled in
                        ro, rl, sk = ops.reading_order_deskew(dh.final_boxes, dh.final_counts, (H, W), self.min_text_size, rec.img_h, rec.img_w,
                                                              page_base=lo, lines=group_lines)
                    elif group_lines:  # the same kernel body with the line outputs compiled in
                        ro, rl = ops.reading_order_lines(dh.final_boxes, dh.final_counts, (H, W), self.min_text_size, rec.img_h, rec.img_w,
                                                         page_base=lo)
                    else:
                        ro = ops.ReadingOrder(*ops.reading_order_crops(dh.final_boxes, dh.final_counts, (H, W), self.min_text_size,
                                                                       rec.img_h, rec.img_w, page_base=lo))
                    if rectify:  # quad descriptors of the same words, right behind, same order
                        qd = ops.quad_crop_descriptors(dh.final_boxes, dh.final_counts, ro, rec.img_h, rec.img_w)
                ev = torch.cuda.Event()
                ev.record(dst)  # detector outputs of this group complete
                groups.append(_Group(lo, hi, st, dst, dh, ev, ro, rl, qd, sk, rg))
        return _Batch(arrays, pages_dev, main, groups, recognize_text, profile, rectify, {} if group_lines else None, n_best, lexicon, lm, lm_weight,
                      ingest_pending,
                      lambda: self.submit_batch(images, recognize_text, profile, None, sub_batches, _maps_override, _device_entropy=False),
                      suggest=suggest, skews={} if deskew else None, region_recs=None if ratios is None else {}, ratios=ratios)

    def advance_batch(self, h):
        """Stage 2 of `predict_batch` for a handle from `submit_batch`: per group — wait for its boxes, run the host
        tail + reading order, then enqueue device crops + the recogniser (asynchronous).  Idempotent; returns `h`.  Calling it
        for batch i+1 BEFORE `collect_batch` of batch i keeps recogniser work queued on the device while the host
        annotates batch i (bench.py does)."""
        if h.pages is not None:
            return h
        if h.ingest_pending is not None:
            # the device Huffman stage's verdict on this batch's files (queued right behind the kernels, long done by now): a corrupt
            # stream gets what the host decoder's verdict gives it — the whole batch is read again through the host path (rare)
            pending, h.ingest_pending = h.ingest_pending, None
            if ingest.check_pending(pending):
                h.replace_with(h.resubmit())
        h.pages = [None] * len(h.arrays)
        h.tm = {"detect_wait+tail": 0.0, "order": 0.0, "crop+enqueue": 0.0, "recognize_wait": 0.0, "assign": 0.0}
        with _gc_paused():
            for grp in h.groups:
                if grp.ro is None or not self._advance_device_ordered(h, grp):
                    self._advance_host_ordered(h, grp)
        return h

    def _advance_device_ordered(self, h, grp):
        """Device route: wait for the group's crop COUNTS only (4 bytes per page), enqueue crops + recogniser.  False: host route."""
        with torch.cuda.stream(grp.det_stream):
            t0 = time.perf_counter()
            counts = grp.ro.ncrop.cpu().numpy()
            h.tm["detect_wait+tail"] += time.perf_counter() - t0
        if not bool((counts >= 0).all()):
            return False
        t0 = time.perf_counter()
        grp.device_ordered, off = True, 0
        for c in counts.tolist():
            grp.spans.append([off, c])
            off += c
        if off:
            self._enqueue_recognizer(h, grp, up=grp.det_stream, counts=counts.tolist())
        h.tm["crop+enqueue"] += time.perf_counter() - t0
        return True

    def _advance_host_ordered(self, h, grp):
        """Host route of a group: the detector's host tail, reading order and crop descriptors on the host, then crops + recogniser."""
        rec, (lo, hi), st = self.recognizer, (grp.lo, grp.hi), grp.stream
        H, W = h.arrays[0].shape[:2]
        with torch.cuda.stream(grp.det_stream):
            t0 = time.perf_counter()
            res = self.detector.detect_finish(grp.det, h.arrays[lo:hi], profile=h.profile)
            h.tm["detect_wait+tail"] += time.perf_counter() - t0
        if st is not h.main:
            st.wait_stream(h.main)  # the page upload
        h.pages[lo:hi] = [self._page_of(r) for r in res]
        if not h.recognize_text:
            return
        with torch.cuda.stream(st):
            t0 = time.perf_counter()
            grp.words, boxes, page_ids = [], [], []
            for pi in range(lo, hi):
                if h.line_recs is not None:
                    h.line_recs[pi] = []
                if h.region_recs is not None:
                    h.region_recs[pi] = []
                cols = () if h.region_recs is None else (h.region_recs[pi], h.ratios)
                if h.skews is None:
                    words, bxs = self._order_boxes(h.pages[pi], None if h.line_recs is None else h.line_recs[pi], None, *cols)
                else:
                    words, bxs, h.skews[pi] = self._order_boxes(h.pages[pi], None if h.line_recs is None else h.line_recs[pi], (H, W), *cols)
                grp.spans.append([len(grp.words), len(words)])
                grp.words += words
                boxes += bxs
                page_ids += [pi] * len(bxs)
            h.tm["order"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            if boxes:
                desc, keep = ops.crop_descriptors(boxes, page_ids, (H, W), rec.img_h, rec.img_w)
                if not keep.all():  # empty clamped crops are skipped by the reference (_pipeline.py:135)
                    grp.words = [w for w, k in zip(grp.words, keep) if k]
                    kept_pages = np.asarray(page_ids)[keep]
                    grp.spans, n0 = [], 0
                    for pi in range(lo, hi):
                        c = int((kept_pages == pi).sum())
                        grp.spans.append([n0, c])
                        n0 += c
                if len(desc):
                    grp.desc_host = desc
                    if h.rectify:  # the host twin's descriptors from the kept words' polygons, in the order of desc
                        grp.qdesc_host = ops.quad_descriptors([w.polygon for w in grp.words], desc, rec.img_h, rec.img_w)
                    self._enqueue_recognizer(h, grp, up=grp.det_stream if self.upload_on_det_stream else st)
            h.tm["crop+enqueue"] += time.perf_counter() - t0

    def _enqueue_recognizer(self, h, grp, up, counts=None):
        """The tail both routes share, for a group with crops: the small blocking uploads on `up` (the high-priority detector stream,
        so that they do not queue behind other groups' recogniser work), the waits of the group's recogniser stream, the crops — AABB
        windows, or cut along the quadrilaterals with `rectify_crops` — and the recogniser, or all of it as one graph replay.
        Device route (`counts` = the pages' crop counts): the descriptors are grp.ro / grp.qd, compacted here on the recogniser stream.
        Host route: grp.desc_host / grp.qdesc_host, uploaded here; the kernel validates the device copy against them."""
        rec, st, pages_dev, rectify, details = self.recognizer, grp.stream, h.pages_dev, h.rectify, bool(self.char_details)
        on_device = counts is not None
        spans = [(first, n) for first, n in grp.spans if n > 0]
        rows = sum(n for _, n in spans)
        use_graph = on_device and rec.use_graphs
        desc_dev = qdesc_dev = prepared = None
        with torch.cuda.stream(up):
            if not on_device:
                dev = torch.from_numpy((grp.qdesc_host if rectify else grp.desc_host).astype("int32", copy=False)).to(self.detector.device)
                desc_dev, qdesc_dev = (None, dev) if rectify else (dev, None)
            if not use_graph:
                prepared = rec.prepare_chunks(rows, spans)
        if on_device and st is not h.main:
            st.wait_stream(h.main)  # the page upload (the host route waited for it before its host stage)
        if on_device or st is not up:
            st.wait_stream(up)
        with torch.cuda.stream(st):
            if on_device:
                def compact(t):
                    t.record_stream(st)
                    return torch.cat([t[pi, :c] for pi, c in enumerate(counts) if c])
                desc_dev, qdesc_dev = compact(grp.ro.desc), (compact(grp.qd) if rectify else None)
                if details:
                    grp.desc_dev, grp.qdesc_dev = desc_dev, qdesc_dev
                if use_graph:  # crop + encode + decode as one hipGraph replay (declines when details or rectified crops are asked for)
                    grp.handle = rec.recognize_start_graph(pages_dev, desc_dev, spans, upload_stream=up, char_details=details, rectified=rectify)
            if grp.handle is None:
                if prepared is None:  # graph path declined (first call of a bucket, ...): plain launches
                    with torch.cuda.stream(up):
                        prepared = rec.prepare_chunks(rows, spans)
                    st.wait_stream(up)
                if rectify:
                    canv = ops.quad_crop(pages_dev, grp.qdesc_host, rec.img_h, rec.img_w, qdesc_dev=qdesc_dev)
                else:
                    canv = ops.crop_resize_pad(pages_dev, grp.desc_host, rec.img_h, rec.img_w, desc_dev=desc_dev)
                grp.handle = rec.recognize_start(canv, spans=spans, prepared=prepared, char_details=details, lexicon=h.lexicon,
                                                 **({} if h.lm is None else {"lm": h.lm, "lm_weight": h.lm_weight}))

    def collect_batch(self, h):
        """Stages 2-3 of `predict_batch` for a handle from `submit_batch` -> list of Pages (stage 2 = `advance_batch`,
        skipped when already done; stage 3 = per group: finish the recogniser (sync) and annotate the words)."""
        self.advance_batch(h)
        rec, main, pages, tm = self.recognizer, h.main, h.pages, h.tm
        with _gc_paused():
            for grp in h.groups:
                lo, hi, st = grp.lo, grp.hi, grp.stream
                if grp.device_ordered:
                    # device-ordered group: Page / Word assembly happens here, off the path that feeds the device.
                    # read the boxes back on a copy stream of their own that only waits for the group's detector outputs: on the
                    # detector stream these copies would queue behind the detector work of the batch after next (it shares that
                    # stream), on the recogniser stream behind this batch's whole recogniser
                    if self._copy_stream is None:
                        self._copy_stream = torch.cuda.Stream(priority=-1)
                    self._copy_stream.wait_event(grp.det_event)
                    with torch.cuda.stream(self._copy_stream):
                        t0 = time.perf_counter()
                        res = self.detector.detect_finish(grp.det, h.arrays[lo:hi], profile=h.profile)
                        order_h, keep_h = grp.ro.order.cpu().numpy(), grp.ro.keep.cpu().numpy()
                        if grp.rl is not None:  # the records carry the spans; the per-position line index stays on the device
                            lines_h, nlines_h = grp.rl.lines.cpu().numpy(), grp.rl.nlines.cpu().numpy()
                        if grp.rg is not None:
                            regions_h, nregions_h = grp.rg.regions.cpu().numpy(), grp.rg.nregions.cpu().numpy()
                        if grp.sk is not None:
                            for pi, (sx, sy, _m, applied) in enumerate(grp.sk.skew.cpu().numpy().tolist()):
                                h.skews[lo + pi] = float(np.degrees(np.arctan2(float(sy), float(sx)))) if applied else 0.0
                        tm["detect_wait+tail"] += time.perf_counter() - t0
                    t0 = time.perf_counter()
                    grp.words = []
                    for pi, r in enumerate(res):
                        page = self._page_of(r)
                        pages[lo + pi] = page
                        k0 = 0
                        if grp.rl is not None:
                            h.line_recs[lo + pi] = []
                        if grp.rg is not None:
                            h.region_recs[lo + pi] = []
                        for block in page.blocks:  # this package's EAST returns one block (infer.py:390)
                            nw = len(block.words)
                            if nw:
                                old = block.words
                                block.words = [old[k] for k in order_h[pi, k0:k0 + nw].tolist()]
                                grp.words += [block.words[pos] for pos in np.flatnonzero(keep_h[pi, k0:k0 + nw]).tolist()]
                            if grp.rl is not None:
                                h.line_recs[lo + pi].append(lines_h[pi, :int(nlines_h[pi])] if nw else _NO_LINES)
                            if grp.rg is not None:
                                h.region_recs[lo + pi].append(regions_h[pi, :int(nregions_h[pi])] if nw else _NO_LINES)
                            k0 += nw
                    tm["order"] += time.perf_counter() - t0
                if grp.handle is not None:
                    details = grp.handle.char_details
                    with torch.cuda.stream(st):
                        t0 = time.perf_counter()
                        fin = rec.recognize_finish(grp.handle, spans=[(first, n) for first, n in grp.spans if n > 0], n_best=h.n_best,
                                                   **({} if h.suggest is None else {"suggest": h.suggest[0], "suggest_k": h.suggest[1],
                                                                                    "suggest_max_distance": h.suggest[2]}),
                                                   **({} if h.suggest is None or h.suggest[3] is None else {"suggest_costs": h.suggest[3]}))
                        if h.suggest is not None:
                            fin, (sug_index, sug_dist) = fin[:-2], fin[-2:]
                        if h.n_best:
                            fin, (alt_ids, _alt_prob, alt_conf, alt_logp) = fin[:-4], fin[-4:]
                        if details:
                            ids, trun, conf, prob, centre, _peak = fin
                            desc = grp.desc_host if grp.desc_host is not None else grp.desc_dev.cpu().numpy()
                            qdesc = grp.qdesc_host if grp.qdesc_dev is None else grp.qdesc_dev.cpu().numpy()
                        else:
                            ids, trun, conf = fin
                        tm["recognize_wait"] += time.perf_counter() - t0
                    t0 = time.perf_counter()
                    texts = rec.texts(ids, trun)
                    for word, text, c in zip(grp.words, texts, conf.tolist()):
                        word.text = text
                        word.recognition_confidence = c
                    chars = alts = None
                    if details and qdesc is not None:  # rectified: x through the quad's patch instead of the AABB window
                        chars = rec.chars(ids, trun, prob, centre, qdesc[:, 9], None, None, qdesc=qdesc)
                    elif details:
                        chars = rec.chars(ids, trun, prob, centre, desc[:, 5], desc[:, 1], desc[:, 3])
                    if h.n_best:
                        alts = (rec.lm_alternatives(alt_ids, trun, alt_conf, alt_logp, h.lm) if h.lm is not None else
                                rec.alternatives(alt_ids, trun, alt_conf, alt_logp) if h.lexicon is None else
                                rec.lexicon_alternatives(alt_ids, trun, alt_conf, alt_logp, h.lexicon))
                    if details or h.n_best or h.lexicon is not None or h.lm is not None or h.suggest is not None:
                        self._attach_details(grp.words, pages[lo:hi], chars, alts,
                                             None if h.lexicon is None else rec.lexicon_indices(ids, h.lexicon),
                                             None if h.lm is None else rec.lm_logps(ids, trun, h.lm),
                                             None if h.suggest is None else h.suggest[0].suggestions(sug_index, sug_dist))
                    tm["assign"] += time.perf_counter() - t0
                if st is not main:
                    main.wait_stream(st)
            for grp in h.groups:
                if grp.det_stream is not main:
                    main.wait_stream(grp.det_stream)
            if h.region_recs:  # after _attach_details, so that the regions and lines hold the CharWords / AltWords
                for pi, rrecs in h.region_recs.items():
                    self._split_regions(pages[pi], rrecs, None if h.line_recs is None else h.line_recs[pi])
            elif h.line_recs:
                for pi, recs in h.line_recs.items():
                    self._split_lines(pages[pi], recs)
            if h.skews:
                for pi, deg in h.skews.items():
                    pages[pi] = self._skew_page(pages[pi], deg)
        self.last_profile = tm
        if h.profile:
            print("Pipeline.predict_batch host stages (s):", {k: round(v, 4) for k, v in tm.items()})
        return pages

    @staticmethod
    def _attach_details(words, pages, chars=None, alts=None, lex_idx=None, lm_logp=None, suggestions=None):
        """Replace every recognised Word of `pages` by a CharWord carrying its symbols (`chars`, char_details), or by an AltWord that
        also carries its readings (`alts`, n_best; its `chars` stay empty without char_details).  chars[k] / alts[k] belong to
        words[k]; x is in page pixels (the recogniser mapped the attention centroid into the word's clamped crop window).  lex_idx
        (lexicon): a LexWord instead, carrying lex_idx[k]; its alternatives are LexAlternatives.  lm_logp (lm): an LmWord instead,
        carrying lm_logp[k]; its alternatives are LmAlternatives.  suggestions (suggest): a SuggestWord (a SuggestLmWord with lm_logp)
        instead, carrying suggestions[k] as Suggestions."""
        from .detectors._types import (Alternative, AltWord, Char, CharWord, LexAlternative, LexWord, LmAlternative, LmWord, Suggestion,
                                       SuggestLmWord, SuggestWord)
        new = {}
        for k, word in enumerate(words):
            extra = {} if chars is None else {"chars": [Char(**d) for d in chars[k]]}
            if alts is not None:
                alt_cls = LexAlternative if lex_idx is not None else LmAlternative if lm_logp is not None else Alternative
                extra["alternatives"] = [alt_cls(**d) for d in alts[k]]
            if lex_idx is not None:
                extra["lexicon_index"] = lex_idx[k]
            if lm_logp is not None:
                extra["lm_logp"] = lm_logp[k]
            if suggestions is not None:
                extra["suggestions"] = [Suggestion(**d) for d in suggestions[k]]
            # the [0, 1] clamp is a no-op guard for CharWord's validation: the confidence is a mean of exp(log-softmax) values, each
            # <= 1 by the kernel's arithmetic (logp <= 0), so the value equals the plain Word's and a default dump does not change
            c = word.recognition_confidence
            new[id(word)] = ((SuggestLmWord if lm_logp is not None else SuggestWord) if suggestions is not None else
                             LexWord if lex_idx is not None else LmWord if lm_logp is not None else CharWord if alts is None else AltWord)(
                polygon=word.polygon, detection_confidence=word.detection_confidence, text=word.text,
                recognition_confidence=None if c is None else min(max(c, 0.0), 1.0), **extra)
        for page in pages:
            for block in page.blocks:
                block.words = [new.get(id(w), w) for w in block.words]

    @staticmethod
    def _skew_page(page, skew_deg):
        """deskew: the page as a SkewPage over the same blocks (and so the same words)."""
        from .detectors._types import SkewPage
        return SkewPage.model_construct(blocks=page.blocks, skew_deg=skew_deg)

    @staticmethod
    def _split_lines(page, line_recs):
        """group_lines: replace every block of `page` by its text lines, block-major.  line_recs[b] = the [L,6] records
        {first, count, x0, y0, x1, y1} of block b over the positions of its reading-ordered words; a block without words has none."""
        from .detectors._types import TextLine
        lines = []
        for block, recs in zip(page.blocks, line_recs):
            for first, count, x0, y0, x1, y1 in np.asarray(recs).tolist():
                lines.append(TextLine(words=block.words[first:first + count], bbox=(x0, y0, x1, y1)))
        page.blocks = lines

    @staticmethod
    def _split_regions(page, region_recs, line_recs=None):
        """columns: replace every block of `page` by its Regions, block-major; with `line_recs` (group_lines) by its RegionLines.
        region_recs[b] / line_recs[b] = the [R,6] / [L,6] records {first, count, x0, y0, x1, y1} of block b over the positions of its
        reading-ordered words; the regions are numbered through the page."""
        from .detectors._types import Region, RegionLine
        out, base = [], 0
        for b, block in enumerate(page.blocks):
            rrecs = np.asarray(region_recs[b]).reshape(-1, 6).tolist()
            if line_recs is None:
                for r, (first, count, x0, y0, x1, y1) in enumerate(rrecs):
                    out.append(Region(words=block.words[first:first + count], bbox=(x0, y0, x1, y1), index=base + r))
            else:
                r = 0
                for first, count, x0, y0, x1, y1 in np.asarray(line_recs[b]).reshape(-1, 6).tolist():
                    while first >= rrecs[r][0] + rrecs[r][1]:  # lines come region-major, and a line never spans two regions
                        r += 1
                    out.append(RegionLine(words=block.words[first:first + count], bbox=(x0, y0, x1, y1), region=base + r))
            base += len(rrecs)
        page.blocks = out

    def score_page(self, image: Union[str, np.ndarray, Image.Image], page, strict: bool = True):
        """Forced decode of a transcribed page (this package's extension; needs this package's TRBA): `page` is a Page whose words
        carry a `text`.  -> (a deep copy of the page, logps).  Every word that has a text (not None) and whose box passes
        min_text_size and has a window on the page comes back as a CharWord: recognition_confidence = the confidence of the GIVEN
        text under the recogniser (TRBA.score's "confidence"), chars = its symbols with their probabilities and x positions in page
        pixels, text = the text as packed (the word's own under strict=True).  Every other word is left as it was.  logps: one entry
        per word in the page's word order (blocks in order, words in order), the summed log-probability of the text and its EOS,
        None for a word that was not scored.  The caller's word order is kept: nothing is reordered and the detector is not run.
        Crops are cut on the device from the words' boxes, along their quadrilaterals with `rectify_crops`, exactly as the
        recognising routes cut them.  strict as for TRBA.score: a character outside the charset or a text longer than max_len
        raises ValueError (False: dropped / truncated).  The positions are attention centroids: estimates, meaningful for trained
        weights only."""
        import copy
        rec = self.recognizer
        if not isinstance(rec, TRBA):
            raise TypeError("score_page needs this package's TRBA as the recogniser")
        from .recognizers._trba.transforms import pack_targets
        page = copy.deepcopy(page)
        all_words = [w for block in page.blocks for w in block.words]
        logps: List[Optional[float]] = [None] * len(all_words)
        arr = np.ascontiguousarray(read_image(image))
        if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
            raise ValueError(f"score_page needs an RGB uint8 image, got shape {arr.shape} {arr.dtype}")
        H, W = arr.shape[:2]
        cand, boxes = [], []
        for k, word in enumerate(all_words):
            if word.text is None:
                continue
            (x0, y0, x1, y1), _poly = _word_aabb(word)
            if (x1 - x0) >= self.min_text_size and (y1 - y0) >= self.min_text_size:
                cand.append(k)
                boxes.append((x0, y0, x1, y1))
        if not cand:
            return page, logps
        desc, keep = ops.crop_descriptors(boxes, [0] * len(boxes), (H, W), rec.img_h, rec.img_w)
        rows = [k for k, kp in zip(cand, keep) if kp]  # a word without a window on the page is left as it was
        if not rows:
            return page, logps
        words = [all_words[k] for k in rows]
        try:
            tok_in, target, trun, packed = pack_targets([w.text for w in words], rec.stoi, rec.max_length, strict=strict)
        except ValueError as e:
            raise ValueError(f"score_page, scored words in page order: {e}") from None
        pages_dev = torch.from_numpy(arr[None]).to(rec.device)
        qdesc = None
        if self.rectify_crops:
            qdesc = ops.quad_descriptors([w.polygon for w in words], desc, rec.img_h, rec.img_w)
            canv = ops.quad_crop(pages_dev, qdesc, rec.img_h, rec.img_w)
        else:
            canv = ops.crop_resize_pad(pages_dev, desc, rec.img_h, rec.img_w)
        logp, conf, _lps, prob, centre, _peak = rec.score_canvases(canv, np.arange(len(rows)), tok_in, target, trun)
        if qdesc is not None:
            chars = rec.chars(target, trun, prob, centre, qdesc[:, 9], None, None, qdesc=qdesc)
        else:
            chars = rec.chars(target, trun, prob, centre, desc[:, 5], desc[:, 1], desc[:, 3])
        for k, word, text, c, lp in zip(rows, words, packed, conf.tolist(), logp.tolist()):
            word.text = text
            word.recognition_confidence = c
            logps[k] = lp
        self._attach_details(words, [page], chars)
        return page, logps

    def evaluate(self, images, gt_pages, iou: float = 0.5) -> Dict[str, Any]:
        """Detection, recognition and end-to-end quality against an annotated set (this package's extension).

        gt_pages[i]: the annotated words of images[i], a list of (quad [4,2], text).  Every image goes through `predict` as this
        pipeline is configured; the words of all blocks, flattened in the order they come back, are the predictions.  They are
        matched to the annotations at the one IoU threshold `iou` by detectors.match_detections (on the detector's device when it
        is this package's EAST, else by the host twin), and for the matched pairs the Levenshtein distances come from
        recognizers.edit_distances (on the recogniser's device when it is this package's TRBA).  A word the pipeline left without a
        text reads as "".  Returns
          "detection":   {precision, recall, f1, tp, fp, fn}
          "recognition": {n, accuracy, cer_micro, cer_mean} over the matched pairs, with TRBA.evaluate's conventions (an empty
                         reference counts inf in cer_mean if the reading is not empty, else 0; no pairs: all 0)
          "end_to_end":  {precision, recall, f1}: a true positive is a matched word whose text is identical to the annotation's
          "matches":     per page a list of (prediction index, ground-truth index, iou, reference text, recognised text)."""
        from .detectors import detection_f1, match_detections
        from .recognizers import edit_distances
        images, gt_pages = list(images), [list(g) for g in gt_pages]
        if len(images) != len(gt_pages):
            raise ValueError(f"{len(images)} images but {len(gt_pages)} annotated pages")
        pred_quads, pred_texts = [], []
        for image in images:
            page = self.predict(image)
            words = [w for block in page.blocks for w in block.words]
            pred_quads.append(np.array([w.polygon for w in words], dtype=np.float32).reshape(-1, 4, 2))
            pred_texts.append([w.text if w.text is not None else "" for w in words])
        gt_quads = [np.array([q for q, _t in g], dtype=np.float32).reshape(-1, 4, 2) for g in gt_pages]
        m = match_detections(pred_quads, gt_quads, [float(iou)], device=self.detector.device if isinstance(self.detector, EAST) else None)
        det = detection_f1(m.counts, m.thresholds)
        matches, refs, hyps = [], [], []
        for p, g in enumerate(gt_pages):
            rows = []
            for i, j in enumerate(m.match[p][0].tolist()):
                if j >= 0:
                    rows.append((i, j, float(m.iou[p][0, i]), g[j][1], pred_texts[p][i]))
                    refs.append(g[j][1])
                    hyps.append(pred_texts[p][i])
            matches.append(rows)
        is_trba = isinstance(self.recognizer, TRBA)
        dist = edit_distances(refs, hyps, stoi=self.recognizer.stoi if is_trba else None,
                              device=self.recognizer.device if is_trba else None).astype(np.float64)
        n = len(refs)
        L = np.array([len(r) for r in refs], dtype=np.float64)
        cer = np.where(L > 0, dist / np.maximum(L, 1), np.where(dist > 0, np.inf, 0.0))
        total = float(L.sum())
        same = sum(1 for r, h in zip(refs, hyps) if r == h)
        n_pred, n_gt = sum(len(q) for q in pred_quads), sum(len(g) for g in gt_pages)
        prec = same / n_pred if n_pred > 0 else 0.0
        rec = same / n_gt if n_gt > 0 else 0.0
        return {
            "detection": {"precision": float(det["precision"][0]), "recall": float(det["recall"][0]), "f1": float(det["f1"][0]),
                          "tp": int(det["tp"][0]), "fp": int(det["fp"][0]), "fn": int(det["fn"][0])},
            "recognition": {"n": n, "accuracy": same / n if n else 0.0,
                            "cer_micro": (float(dist.sum()) / total if total > 0 else (float("inf") if dist.sum() > 0 else 0.0)),
                            "cer_mean": float(cer.mean()) if n else 0.0},
            "end_to_end": {"precision": prec, "recall": rec, "f1": 2 * prec * rec / (prec + rec) if (prec + rec) > 0 else 0.0},
            "matches": matches,
        }

    def evaluate_text(self, images, gt_texts, breakdown: bool = False) -> Dict[str, Any]:
        """Character and word error rate of the pages' running text, in this pipeline's reading order, against plain transcriptions
        (this package's extension).  Unlike `evaluate` it needs no boxes and it sees the order: a page read
        across its gutter scores worse than one read column by column.

        gt_texts[i]: the transcription of images[i], one str.  Every image goes through `predict` as this pipeline is configured;
        the hypothesis is the texts of all blocks' words, flattened in the order they come back (the order `evaluate` uses) and
        joined by one space; a word without text is skipped.  Returns recognizers.text_error_rates' figures, per page and pooled
        (distances on the recogniser's device when it is this package's TRBA, else by the host twin: foreign plugins need no GPU),
        and "hypotheses": the pages' texts as they were compared.
        breakdown=True adds what the distances are made of (text_error_rates' "char_counts", "word_counts", "char_confusions",
        "word_confusions", "word_alignments") and changes no other figure: both levels then come from one
        call of the alignment, on the recogniser's device when it is this package's TRBA (measured end to end on pages of
        characters: 1.09 ms against 7.54 ms for the host twin, profiles/edit_alignment.txt), else by the host twin."""
        from .recognizers import text_error_rates
        images, gt_texts = list(images), list(gt_texts)
        if len(images) != len(gt_texts):
            raise ValueError(f"{len(images)} images but {len(gt_texts)} transcriptions")
        hyps = []
        for image in images:
            page = self.predict(image)
            hyps.append(" ".join(w.text for block in page.blocks for w in block.words if w.text))
        out = text_error_rates(gt_texts, hyps, device=self.recognizer.device if isinstance(self.recognizer, TRBA) else None,
                               breakdown=breakdown)
        out["hypotheses"] = hyps
        return out

    def transfer_text(self, image, gt_text: str, max_cer: Optional[float] = None, device=None):
        """Hand the words of a plain transcription to the boxes of the page (this package's extension):
        archives have transcriptions without boxes, and an alignment of the words read, in reading order, with the transcription's
        words gives every detected quadrilateral its true text.  -> (page, unpaired).

        The image goes through `predict` as this pipeline is configured.  The words that have a text, flattened in the order
        `evaluate_text` flattens them, are aligned at word level with gt_text.split() (recognizers.sequence_alignments: the
        transcription is the reference).  Each of those words comes back as a TransferWord, which keeps the fields of the word it
        was: paired as a hit or a substitution it carries gt_text, gt_index (into gt_text.split()) and char_distance (the
        Levenshtein distance between its text and gt_text, recognizers.sequence_edit_distances); a word the alignment left alone
        has None in all three.  max_cer: a pair with char_distance / len(gt_text) above it is un-paired again; there is no default,
        none can be tuned offline.  unpaired: the indices of the transcription's words left without a box, ascending.  A word
        without text stays as it was.  device: None = the host twin, which is the faster route for a page of words (measured: 0.18 ms
        against 0.27 ms on the device with its transfers, profiles/edit_alignment.txt) and all a foreign plugin needs; a device:
        msocr_edit_alignment there, the same result bit for bit."""
        from .detectors._types import TransferWord
        from .recognizers import sequence_alignments, sequence_edit_distances
        if not isinstance(gt_text, str):
            raise TypeError(f"the transcription is one str, got {type(gt_text).__name__}")
        page = self.predict(image)
        words = [w for block in page.blocks for w in block.words if w.text]
        gt_words = gt_text.split()
        al = sequence_alignments([gt_words], [[w.text for w in words]], device=device)[0]
        pairs = [(k, g) for k, g in enumerate(al.hyp_to_ref.tolist()) if g >= 0]
        dist = sequence_edit_distances([gt_words[g] for _k, g in pairs], [words[k].text for k, _g in pairs], device=device).tolist()
        extra = {}
        for (k, g), d in zip(pairs, dist):
            if max_cer is None or not d / len(gt_words[g]) > max_cer:
                extra[k] = {"gt_text": gt_words[g], "gt_index": g, "char_distance": d}
        new = {}
        for k, word in enumerate(words):
            fields = {name: getattr(word, name) for name in type(word).model_fields}
            new[id(word)] = TransferWord(**fields, **extra.get(k, {}))
        for block in page.blocks:
            block.words = [new.get(id(w), w) for w in block.words]
        taken = {e["gt_index"] for e in extra.values()}
        return page, [g for g in range(len(gt_words)) if g not in taken]

    def search(self, pages_or_images, queries, max_distance=None, max_error_rate=None, overlapping: bool = False, device=None,
               costs=None):
        """Where do the queries occur in these pages, allowing for what the recogniser may have misread (this package's extension;
        DESIGN.md section 4.24)?  -> a list of detectors._types.SearchHit in canonical order (query, page, end).

        pages_or_images: Pages are taken as they are, so searching needs neither the networks nor a GPU; anything else goes
        through `predict` first.  A page's text is the texts of its words that have one, flattened in the order `evaluate_text`
        flattens them and joined by one space; a query is whitespace-normalised the same way and may span words and blocks.  Exactly
        one of max_distance (edits allowed: an int, or one per query) and max_error_rate (k = min(floor(rate * len(query)),
        len(query) - 1)) is given; a query has 1 to 64 characters.  A hit carries the words it touches as (block index, word index).
        overlapping=True reports every end position within the bound instead of the occurrences.  device: None = the host twin; a
        device: msocr_text_search there, the same hits bit for bit.  No automatic switch between the two (Pages must be searchable
        without a GPU): 16 pages x 10 queries take 2.4 ms on one host core and 0.16 ms on the device with the corpus upload and the
        read-back (profiles/text_search.txt), and for many searches of one collection a PageCorpus keeps it on the device.
        costs=EditCosts(...): the search under confusion-weighted costs (msocr_text_search_weighted): the
        bounds and SearchHit.distance are then in cost units, as recognizers.TextCorpus.search says."""
        from ._search import PageCorpus
        from .detectors._types import Page
        pages = [p if isinstance(p, Page) else self.predict(p) for p in pages_or_images]
        return PageCorpus(pages, device=device).search(queries, max_distance=max_distance, max_error_rate=max_error_rate,
                                                       overlapping=overlapping, costs=costs)

    def index_words(self, images, pages=None):
        """A WordIndex of the words of these pages, for word spotting by example (this package's extension; DESIGN.md section 4.25;
        needs this package's TRBA).  pages: the Pages of `images`, one each; None runs `predict` on every image first.  The words
        are cut as `score_page` cuts them, with this pipeline's min_text_size and rectify_crops; the index lives on the
        recogniser's device."""
        from ._spotting import WordIndex
        if not isinstance(self.recognizer, TRBA):
            raise TypeError("index_words needs this package's TRBA as the recogniser")
        images = list(images)
        pages = [self.predict(im) for im in images] if pages is None else list(pages)
        index = WordIndex(self.recognizer)
        index.min_text_size, index.rectify_crops = self.min_text_size, bool(self.rectify_crops)
        index.add_pages(images, pages)
        return index

    def spot(self, index, queries, k: int = 10, max_length_ratio: Optional[float] = 2.0, partial: bool = False):
        """WordIndex.spot with one more kind of query: (image, polygon), a region of a page, which is cut as this pipeline cuts a
        word (min_text_size, rectify_crops) and embedded.  Word images and (page, block, word) references pass through.  -> one list
        of detectors._types.SpotHit per query.  partial=True: "which words contain this", e.g. a boxed stem; the hits are
        PartSpotHit with the matched stretch of frames (WordIndex.spot)."""
        from ._spotting import WordIndex
        resolved = []
        for q in queries:
            if isinstance(q, tuple) and len(q) == 2:
                cutter = WordIndex(self.recognizer)
                cutter.min_text_size, cutter.rectify_crops = self.min_text_size, bool(self.rectify_crops)
                q = cutter.frames_of_polygon(q[0], q[1])
            resolved.append(q)
        return index.spot(resolved, k=k, max_length_ratio=max_length_ratio, partial=partial)

    def process_batch(self, images: List[Union[str, np.ndarray, Image.Image]], recognize_text: bool = True, vis: bool = False,
                      profile: bool = False):
        results = []
        for img in images:
            res = self.predict(img, recognize_text=recognize_text, vis=vis, profile=profile)
            results.append(res[0] if vis else res)
        return results

    def get_text(self, page) -> str:
        lines = []
        for block in page.blocks:
            ordered = sorted(block.words, key=lambda w: min(p[0] for p in w.polygon))
            texts = [w.text for w in ordered if getattr(w, "text", None)]
            if texts:
                lines.append(" ".join(texts))
        return "\n".join(lines)

    def _extract_word_image(self, image: np.ndarray, polygon: np.ndarray, quad=None) -> Optional[np.ndarray]:
        """The word's clamped AABB window of the page (reference _pipeline.py:204-221).  With `rectify_crops` set and the word's
        float corners given as `quad`: the region cut along the quadrilateral at its natural size, (rint(h), rint(w), 3), through
        the host twin msocr_quad_crop_host (same sampling as the device kernel; the recogniser's own resize follows, so these
        pixels are resampled twice) — or, when the recogniser is this package's TRBA and its canvas therefore known, the finished
        (img_h, img_w, 3) canvas of the device route, which TRBA's ResizeAndPadA leaves as it is (a crop of the canvas size is pasted
        unscaled at the origin).  A word without a window has no region either way."""
        try:
            x_min, y_min = np.min(polygon, axis=0)
            x_max, y_max = np.max(polygon, axis=0)
            h, w = image.shape[:2]
            x1, y1 = max(0, int(x_min)), max(0, int(y_min))
            x2, y2 = min(w, int(x_max)), min(h, int(y_max))
            region = image[y1:y2, x1:x2]  # a view of the page, never mutated
            if region.size == 0:
                return None
        except Exception:
            return None
        if quad is not None and self.rectify_crops and image.ndim == 3 and image.shape[2] == 3:
            rec = self.recognizer
            canvas = (rec.img_h, rec.img_w) if isinstance(rec, TRBA) else None
            desc, _ = ops.crop_descriptors([(x_min, y_min, x_max, y_max)], [0], (h, w), *(canvas or (1, 1)))
            if len(desc) and canvas:  # the device route's descriptor and canvas
                return ops.quad_crop_host(image[None], ops.quad_descriptors([quad], desc, *canvas), *canvas)[0]
            if len(desc):  # always: the window above is not empty
                qd = ops.quad_descriptors([quad], desc, natural=True)
                return ops.quad_crop_host(image[None], qd, int(qd[0, 10]), int(qd[0, 9]))[0]
        return region
