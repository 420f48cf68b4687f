"""Word spotting by example (this package's extension): WordIndex keeps the recogniser's encoder frames of
the words of pages, as unit frames with their lengths, and answers "which indexed words look like this one" by the normalised
dynamic-time-warping distance of include/msocr.h ("word spotting").  Matching is done on image features, never on transcriptions,
so it also finds what the recogniser reads badly.

What is built and tested is the arithmetic and the plumbing.  Whether near words are the same word depends on the recogniser's
weights; no trained weights exist here and nothing about retrieval quality is claimed."""
from typing import List, Optional, Sequence

import numpy as np

from . import ops
from .detectors._types import PartSpotHit, SpotHit

_LIMIT = (1 << 31) - 1  # elements of one feature array of a native call (msocr.h: N T H < 2^31)


class _Frames:
    """a query that is already frames: unit [T, H] (a device tensor or an array, as the index stores them) and its length"""

    def __init__(self, unit, length):
        self.unit, self.length = unit, int(length)


def length_bounds(lengths, max_length_ratio, T):
    """The length gate of a query of `lengths` frames: (len_lo, len_hi) int32, ceil(L / r) and floor(L * r) clipped into [1, T];
    max_length_ratio None admits every length."""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if max_length_ratio is None:
        return np.ones(len(L), dtype=np.int32), np.full(len(L), T, dtype=np.int32)
    r = float(max_length_ratio)
    if not (r >= 1.0) or not np.isfinite(r):
        raise ValueError(f"max_length_ratio must be a finite number >= 1 or None, got {max_length_ratio!r}")
    lo = np.ceil(L / r - 1e-9).astype(np.int64)
    hi = np.floor(L * r + 1e-9).astype(np.int64)
    return np.clip(lo, 1, T).astype(np.int32), np.clip(hi, 1, T).astype(np.int32)


class WordIndex:
    """WordIndex(recognizer, device=None): `recognizer` is this package's TRBA (it embeds the words; None for an index of
    pre-computed features, see `from_features`).  device: where the unit frames live and the search runs; None = the recogniser's
    device, or, without a recogniser, host memory (NumPy) and the host twins: the same API without a GPU.

    Storage is f32: T * H * 4 bytes of unit frames and 4 bytes of length per word, about 34 KB at T = 33, H = 256 (`nbytes`)."""

    def __init__(self, recognizer=None, device=None):
        self.recognizer = recognizer
        if device is None and recognizer is not None:
            device = getattr(recognizer, "device", None)
        if device is not None:
            import torch
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError("a WordIndex lives on a HIP device or, with device=None and no recogniser, in host memory")
        self.device = device
        self.min_text_size = 5       # Pipeline.index_words sets both from the pipeline
        self.rectify_crops = False
        self.ids: List[tuple] = []              # (page, block, word) per indexed word, in index order
        self.texts: List[Optional[str]] = []
        self.pages = 0                          # pages added so far: the next page's index
        self.skipped = 0                        # words of added pages that were not indexed (too small, or no window on the page)
        self.T = self.H = None
        self._row = {}
        self._blocks = []                       # [(unit [n, T, H], lengths [n])], each inside one native call's limit
        self._pending = []

    # ------------------------------------------------------------------------------------- storage
    def __len__(self):
        return len(self.ids)

    @property
    def nbytes(self):
        return sum(int(u.shape[0]) for u, _ in self._blocks + self._pending) * ((self.T or 0) * (self.H or 0) * 4 + 4)

    def _cat(self, xs):
        if self.device is None:
            return np.concatenate(xs)
        import torch
        return torch.cat(xs)

    def _append(self, unit, lengths, ids, texts):
        n = int(unit.shape[0])
        if len(ids) != n or len(texts) != n or int(lengths.shape[0]) != n:
            raise ValueError("one id, one text and one length per word")
        if n == 0:
            return
        T, H = int(unit.shape[1]), int(unit.shape[2])
        if self.T is None:
            self.T, self.H = T, H
        elif (T, H) != (self.T, self.H):
            raise ValueError(f"this index holds [{self.T}, {self.H}] frames, got [{T}, {H}]")
        for i in ids:
            i = tuple(int(v) for v in i)
            if len(i) != 3 or i in self._row:
                raise ValueError(f"ids are distinct (page, block, word) triples, got {i}")
            self._row[i] = len(self.ids)
            self.ids.append(i)
        self.texts.extend(texts)
        self._pending.append((unit, lengths))

    def _pack(self):
        """pending pieces join the last block while it stays inside one native call's limit; a new block begins where it would not"""
        per_call = max(1, _LIMIT // (self.T * self.H)) if self.T else 1
        for unit, lengths in self._pending:
            at = 0
            while at < unit.shape[0]:
                room = per_call - int(self._blocks[-1][0].shape[0]) if self._blocks else 0
                if room <= 0:
                    take = min(per_call, int(unit.shape[0]) - at)
                    self._blocks.append((unit[at:at + take], lengths[at:at + take]))
                else:
                    take = min(room, int(unit.shape[0]) - at)
                    u, l = self._blocks[-1]
                    self._blocks[-1] = (self._cat([u, unit[at:at + take]]), self._cat([l, lengths[at:at + take]]))
                at += take
        self._pending = []

    def _normalize(self, feat, lengths):
        """raw frames [n, T, H] and lengths [n] (host) -> (unit frames, lengths) as the index stores them"""
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if self.device is None:
            feat = np.ascontiguousarray(feat, dtype=np.float32)
            if feat.ndim != 3 or feat.shape[0] != len(lengths):
                raise ValueError("features are [n, T, H] with one length per word")
            if len(lengths) and (lengths.min() < 1 or lengths.max() > feat.shape[1]):
                raise ValueError("lengths lie in [1, T]")
            return ops.frame_normalize_host(feat, lengths), lengths
        import torch
        if not isinstance(feat, torch.Tensor):
            feat = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32))
        feat = feat.to(self.device, dtype=torch.float32).contiguous()
        if feat.dim() != 3 or feat.shape[0] != len(lengths):
            raise ValueError("features are [n, T, H] with one length per word")
        if len(lengths) and (lengths.min() < 1 or lengths.max() > feat.shape[1]):
            raise ValueError("lengths lie in [1, T]")
        with torch.cuda.device(self.device):
            len_dev = torch.from_numpy(lengths).to(self.device)
            return ops.frame_normalize(feat, len_dev), len_dev

    @classmethod
    def from_features(cls, features, lengths, ids, texts=None, device=None, normalized=False):
        """An index of pre-computed frames: features [N, T, H] f32 (an array, or a device tensor), lengths [N] in [1, T], ids [N]
        distinct (page, block, word) triples.  They are normalised as `add_page` normalises, unless `normalized` says they are unit
        frames with zeros behind their lengths already (they are then kept as given, not copied).  No recogniser: such an index
        answers reference queries and `spot_features`, on the host with device=None."""
        index = cls(None, device=device)
        index.add_features(features, lengths, ids, texts, normalized=normalized)
        return index

    def add_features(self, features, lengths, ids, texts=None, normalized=False):
        ids = list(ids)
        if normalized:
            lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
            if len(lens) and (lens.min() < 1 or lens.max() > features.shape[1]):
                raise ValueError("lengths lie in [1, T]")
            if self.device is None:
                unit = np.ascontiguousarray(features, dtype=np.float32)
            else:
                import torch
                unit = torch.as_tensor(features, dtype=torch.float32, device=self.device).contiguous()
                lens = torch.from_numpy(lens).to(self.device)
        else:
            unit, lens = self._normalize(features, lengths)
        self._append(unit, lens, ids, list(texts) if texts is not None else [None] * len(ids))
        if ids:
            self.pages = max(self.pages, max(int(i[0]) for i in ids) + 1)

    # ------------------------------------------------------------------------------------- pages
    def _cut(self, arr, polygons):
        """the recogniser's canvases of `polygons` on the page `arr`, cut as Pipeline.score_page cuts them -> (canvases on the
        device, new_w [m], kept: which polygons have a canvas)"""
        import torch
        from ._pipeline import _word_aabb
        rec = self.recognizer
        H, W = arr.shape[:2]
        cand, boxes = [], []
        for k, poly in enumerate(polygons):
            (x0, y0, x1, y1), _ = _word_aabb(poly)
            if (x1 - x0) >= self.min_text_size and (y1 - y0) >= self.min_text_size:
                cand.append(k)
                boxes.append((x0, y0, x1, y1))
        if not cand:
            return None, np.zeros(0, dtype=np.int64), []
        desc, keep = ops.crop_descriptors(boxes, [0] * len(boxes), (H, W), rec.img_h, rec.img_w)
        rows = [k for k, kp in zip(cand, keep) if kp]
        if not rows:
            return None, np.zeros(0, dtype=np.int64), []
        pages_dev = torch.from_numpy(arr[None]).to(rec.device)
        if self.rectify_crops:
            qdesc = ops.quad_descriptors([polygons[k].polygon for k in rows], desc, rec.img_h, rec.img_w)
            return ops.quad_crop(pages_dev, qdesc, rec.img_h, rec.img_w), np.asarray(qdesc[:, 9]), rows
        return ops.crop_resize_pad(pages_dev, desc, rec.img_h, rec.img_w), np.asarray(desc[:, 5]), rows

    def _page_array(self, image):
        from .detectors import read_image
        arr = np.ascontiguousarray(read_image(image))
        if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
            raise ValueError(f"a page is an RGB uint8 image, got shape {arr.shape} {arr.dtype}")
        return arr

    def _need_recognizer(self):
        from .recognizers import TRBA
        if not isinstance(self.recognizer, TRBA):
            raise TypeError("embedding words needs this package's TRBA as the index's recogniser")

    def add_page(self, image, page) -> int:
        """Index every word of `page` (a Page of `image`): the words whose boxes pass min_text_size and have a window on the page
        are cut on the device exactly as Pipeline.score_page cuts them (along their quadrilaterals with rectify_crops), embedded
        (TRBA.embed_canvases), normalised and appended with the ids (page index, block index, word index); the page index counts
        the pages added to this index.  Words that are not cut are counted in `skipped`.  -> the number of words added."""
        self._need_recognizer()
        arr = self._page_array(image)
        where = [(b, w) for b, block in enumerate(page.blocks) for w in range(len(block.words))]
        words = [page.blocks[b].words[w] for b, w in where]
        p = self.pages
        self.pages += 1
        canv, new_w, rows = self._cut(arr, words)
        self.skipped += len(words) - len(rows)
        if not rows:
            return 0
        feat, lengths = self.recognizer.embed_canvases(canv, new_w)
        unit, lens = self._normalize(feat, lengths)
        self._append(unit, lens, [(p,) + where[k] for k in rows], [getattr(words[k], "text", None) for k in rows])
        return len(rows)

    def add_pages(self, images, pages) -> int:
        images, pages = list(images), list(pages)
        if len(images) != len(pages):
            raise ValueError(f"{len(images)} images but {len(pages)} pages")
        return sum(self.add_page(im, pg) for im, pg in zip(images, pages))

    # ------------------------------------------------------------------------------------- queries
    def frames_of(self, ref) -> _Frames:
        """the stored unit frames of the indexed word (page, block, word)"""
        ref = tuple(int(v) for v in ref)
        if ref not in self._row:
            raise KeyError(f"no word {ref} in this index")
        self._pack()
        row = self._row[ref]
        for unit, lengths in self._blocks:
            if row < unit.shape[0]:
                return _Frames(unit[row], int(lengths[row]))
            row -= int(unit.shape[0])
        raise AssertionError("rows and blocks disagree")

    def frames_of_polygon(self, image, polygon) -> _Frames:
        """the unit frames of the region `polygon` of the page `image`, cut as `add_page` cuts a word"""
        self._need_recognizer()
        from .detectors._types import Word
        word = polygon if hasattr(polygon, "polygon") else Word(polygon=[tuple(float(c) for c in pt) for pt in polygon],
                                                                detection_confidence=1.0)
        canv, new_w, rows = self._cut(self._page_array(image), [word])
        if not rows:
            raise ValueError("the query's polygon is smaller than min_text_size or has no window on its page")
        unit, lens = self._normalize(*self.recognizer.embed_canvases(canv, new_w))
        return _Frames(unit[0], int(lens[0]))

    def _resolve(self, queries):
        out, images, slots = [], [], []
        for q in queries:
            if isinstance(q, _Frames):
                out.append(q)
            elif isinstance(q, tuple) and len(q) == 3 and all(isinstance(v, (int, np.integer)) for v in q):
                out.append(self.frames_of(q))
            else:
                slots.append(len(out))
                out.append(None)
                images.append(q)
        if images:
            self._need_recognizer()
            unit, lens = self._normalize(*self.recognizer.embed(images))
            for s, k in zip(slots, range(len(images))):
                out[s] = _Frames(unit[k], int(lens[k]))
        return out

    def spot(self, queries: Sequence, k: int = 10, max_length_ratio: Optional[float] = 2.0, partial: bool = False) -> List[List[SpotHit]]:
        """The k nearest indexed words of every query -> one list of SpotHit per query, nearest first.

        A query is a word image (an array, a path or a PIL image; it is embedded as TRBA.embed embeds it) or a reference
        (page, block, word) to a word of this index, whose stored frames are then the query.  A reference query finds itself: its own
        word comes back at rank 0 with a distance of about 0 (inside the distance's own bound, (3 H + 4 L + 16) 2^-24 for L frames:
        the unit frames' rounding), unless an identical word entered the index before it.  k is 1 .. 256.  max_length_ratio r gates the pairs by length, before any
        arithmetic: a query of L frames is compared with words of ceil(L / r) .. floor(L r) frames only, None compares it with all.
        The default 2.0 is a placeholder, not a tuned value.  Fewer than k hits come back where fewer words pass the gate.

        partial=True asks "which words CONTAIN this" (DESIGN.md section 4.28): the query may start and end anywhere inside a word
        (msocr_dtw_subsequence), the distance is the path's cost divided by the query's length alone, and the hits are PartSpotHit:
        a SpotHit with the stretch of the word's frames that was matched (`frame_start`, `frame_end`, `fraction`).  The gate is then
        ceil(L / r) .. T: a word may be longer than the query by any amount, but not much shorter; r is the same placeholder.
        Nothing constrains the stretch (a query may collapse onto one frame), and the encoder's frames carry context, so a stem cut
        alone and the same stem inside a longer word need not embed alike: nothing about retrieval quality is claimed."""
        frames = self._resolve(list(queries))
        if not frames:
            return []
        if self.device is None:
            unit = np.stack([np.asarray(f.unit, dtype=np.float32) for f in frames])
        else:
            import torch
            unit = torch.stack([f.unit for f in frames])
        return self.spot_features(unit, [f.length for f in frames], k=k, max_length_ratio=max_length_ratio, normalized=True,
                                  partial=partial)

    def spot_features(self, features, lengths, k: int = 10, max_length_ratio: Optional[float] = 2.0, normalized: bool = False,
                      partial: bool = False):
        """`spot` for queries given as frames: features [Q, T, H] f32, lengths [Q] in [1, T]; they are normalised unless
        `normalized` says they are unit frames already.  partial: as for `spot`."""
        k = int(k)
        if not 1 <= k <= ops.SPOT_MAX_K:
            raise ValueError(f"k must lie in 1 .. {ops.SPOT_MAX_K}, got {k}")
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        Q = len(lengths)
        if Q == 0:
            return []
        if len(self) == 0:
            return [[] for _ in range(Q)]
        if tuple(features.shape) != (Q, self.T, self.H):
            raise ValueError(f"queries must be [{Q}, {self.T}, {self.H}] frames, got {tuple(features.shape)}")
        if lengths.min() < 1 or lengths.max() > self.T:
            raise ValueError("lengths lie in [1, T]")
        lo, hi = length_bounds(lengths, max_length_ratio, self.T)
        self._pack()
        per_call = max(1, _LIMIT // (self.T * self.H))
        if partial:
            return self._spot_partial(features, lengths, lo, k, normalized, per_call)
        if self.device is None:
            unit = np.ascontiguousarray(features, dtype=np.float32)
            if not normalized:
                unit = ops.frame_normalize_host(unit, lengths)
            parts = [ops.dtw_distances_host(unit[s:s + per_call], lengths[s:s + per_call], lo[s:s + per_call], hi[s:s + per_call], cu, cl)
                     for s in range(0, Q, per_call) for cu, cl in self._blocks]
            nb = len(self._blocks)
            dist = np.concatenate([np.concatenate(parts[r * nb:(r + 1) * nb], axis=1) for r in range(len(parts) // nb)])
            idx, val = ops.topk_smallest_host(dist, k)
        else:
            import torch
            with torch.cuda.device(self.device):
                if not isinstance(features, torch.Tensor):
                    features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
                unit = features.to(self.device, dtype=torch.float32).contiguous()
                ql, lo_d, hi_d = (torch.from_numpy(a).to(self.device) for a in (lengths, lo, hi))
                if not normalized:
                    unit = ops.frame_normalize(unit, ql)
                if len(self._blocks) == 1 and Q <= per_call:
                    dist = ops.dtw_distances(unit, ql, lo_d, hi_d, *self._blocks[0])
                else:  # an index or a query set beyond one call's N T H < 2^31: block by block into one [Q, N] array
                    dist = torch.empty((Q, len(self)), dtype=torch.float32, device=self.device)
                    for s in range(0, Q, per_call):
                        at = 0
                        for cu, cl in self._blocks:
                            n = int(cu.shape[0])
                            dist[s:s + per_call, at:at + n] = ops.dtw_distances(unit[s:s + per_call], ql[s:s + per_call],
                                                                                lo_d[s:s + per_call], hi_d[s:s + per_call], cu, cl)
                            at += n
                idx, val = ops.topk_smallest(dist, k)
                idx, val = idx.cpu().numpy(), val.cpu().numpy()
        out = []
        for q in range(Q):
            hits = []
            for rank, (i, d) in enumerate(zip(idx[q].tolist(), val[q].tolist())):
                if i < 0:
                    break
                page, block, word = self.ids[i]
                hits.append(SpotHit(query=q, page=page, block=block, word=word, distance=d, rank=rank, text=self.texts[i]))
            out.append(hits)
        return out

    def _spot_partial(self, features, lengths, lo, k, normalized, per_call):
        """spot_features(partial=True) behind its checks: the subsequence distance under the gate [lo, T]; spans are joined over
        blocks and query pieces exactly as the distances are, and the selection is the same one"""
        Q = len(lengths)
        hi = np.full(Q, self.T, dtype=np.int32)
        if self.device is None:
            unit = np.ascontiguousarray(features, dtype=np.float32)
            if not normalized:
                unit = ops.frame_normalize_host(unit, lengths)
            parts = [ops.dtw_subsequence_host(unit[s:s + per_call], lengths[s:s + per_call], lo[s:s + per_call], hi[s:s + per_call], cu, cl)
                     for s in range(0, Q, per_call) for cu, cl in self._blocks]
            nb = len(self._blocks)
            dist = np.concatenate([np.concatenate([d for d, _ in parts[r * nb:(r + 1) * nb]], axis=1) for r in range(len(parts) // nb)])
            span = np.concatenate([np.concatenate([sp for _, sp in parts[r * nb:(r + 1) * nb]], axis=1) for r in range(len(parts) // nb)])
            idx, val = ops.topk_smallest_host(dist, k)
            word_len = np.concatenate([np.asarray(cl) for _, cl in self._blocks])
        else:
            import torch
            with torch.cuda.device(self.device):
                if not isinstance(features, torch.Tensor):
                    features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
                unit = features.to(self.device, dtype=torch.float32).contiguous()
                ql, lo_d, hi_d = (torch.from_numpy(a).to(self.device) for a in (lengths, lo, hi))
                if not normalized:
                    unit = ops.frame_normalize(unit, ql)
                if len(self._blocks) == 1 and Q <= per_call:
                    dist, span = ops.dtw_subsequence(unit, ql, lo_d, hi_d, *self._blocks[0])
                else:
                    dist = torch.empty((Q, len(self)), dtype=torch.float32, device=self.device)
                    span = torch.empty((Q, len(self), 2), dtype=torch.int32, device=self.device)
                    for s in range(0, Q, per_call):
                        at = 0
                        for cu, cl in self._blocks:
                            n = int(cu.shape[0])
                            d, sp = ops.dtw_subsequence(unit[s:s + per_call], ql[s:s + per_call], lo_d[s:s + per_call],
                                                        hi_d[s:s + per_call], cu, cl)
                            dist[s:s + per_call, at:at + n] = d
                            span[s:s + per_call, at:at + n] = sp
                            at += n
                idx, val = ops.topk_smallest(dist, k)
                # the spans and word lengths of the selected words only: [Q, k, 2] and [Q, k] leave the device
                at = idx.clamp(min=0).long()
                span = torch.gather(span, 1, at[:, :, None].expand(-1, -1, 2)).cpu().numpy()
                word_len = torch.cat([cl for _, cl in self._blocks])[at].cpu().numpy()
                idx, val = idx.cpu().numpy(), val.cpu().numpy()
        out = []
        for q in range(Q):
            hits = []
            for rank, (i, d) in enumerate(zip(idx[q].tolist(), val[q].tolist())):
                if i < 0:
                    break
                if self.device is None:
                    (a, b), L = span[q, i].tolist(), int(word_len[i])
                else:
                    (a, b), L = span[q, rank].tolist(), int(word_len[q, rank])
                page, block, word = self.ids[i]
                hits.append(PartSpotHit(query=q, page=page, block=block, word=word, distance=d, rank=rank, text=self.texts[i],
                                        frame_start=a, frame_end=b, fraction=(a / L, b / L)))
            out.append(hits)
        return out
