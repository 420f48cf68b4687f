"""Detection quality against a ground truth: the matching rule and the F1 figures of the reference's
compute_f1 / compute_f1_metrics (detectors/_east/utils.py:435-474, 680-697 of the project this one was modelled on) without its
shapely dependency.  The IoU is the reference's own lanms.polygon_iou on canonically wound, strictly convex quads; the rule is
written out in include/msocr.h ("detection quality").

  match_detections(pred_pages, gt_pages, thresholds, scores=None, device=None)  per-page matches, IoUs and tp / fp / fn
  detection_f1(counts, thresholds)                                              precision / recall / F1 per threshold, F1@0.5, mean F1
  load_coco_quads(path)                                                         COCO ground truth -> image_id -> [n,4,2] f32

The matching runs in msocr_quad_match (device given) or its host twin (device None, no GPU needed); both give the same arrays bit
for bit.
"""
import json
from typing import NamedTuple

import numpy as np

DEFAULT_IOU_THRESHOLDS = np.arange(0.50, 0.95 + 1e-9, 0.05)  # compute_f1_metrics' iou_vals, f64; the first is exactly 0.5
MAX_QUADS_PER_PAGE = 16384  # msocr_quad_match's envelope on either side


class Matches(NamedTuple):
    """match[p] int32 [T, n_p]: per threshold the ground-truth index of prediction i of page p AS GIVEN (-1 false positive, -2 invalid
    quad); iou[p] f64 [T, n_p]: the best IoU among the ground truths still free when the prediction's turn came; counts int32
    [N, T, 3]: tp, fp, fn per page and threshold; thresholds f64 [T]."""
    match: list
    iou: list
    counts: np.ndarray
    thresholds: np.ndarray


def _quads(a, what):
    q = np.asarray(a, dtype=np.float32)
    if q.size == 0:
        return np.zeros((0, 4, 2), dtype=np.float32)
    if q.ndim == 2 and q.shape[1] == 8:
        q = q.reshape(-1, 4, 2)
    if q.ndim != 3 or q.shape[1:] != (4, 2):
        raise ValueError(f"{what}: quads are [n,4,2] (or [n,8]) arrays, got shape {q.shape}")
    return np.ascontiguousarray(q)


def pack_pages(pages, what="quads"):
    """A list of [n_p,4,2] arrays -> ([N,max(n_p),4,2] f32 zero-filled, [N] int32).  A page above 16384 quads raises ValueError."""
    pages = [_quads(q, what) for q in pages]
    n = np.array([len(q) for q in pages], dtype=np.int32)
    if len(n) and int(n.max()) > MAX_QUADS_PER_PAGE:
        raise ValueError(f"{what}: a page holds {int(n.max())} quads, at most {MAX_QUADS_PER_PAGE} per page are matched")
    out = np.zeros((len(pages), int(n.max()) if len(n) else 0, 4, 2), dtype=np.float32)
    for p, q in enumerate(pages):
        out[p, : len(q)] = q
    return out, n


def match_detections(pred_pages, gt_pages, thresholds=DEFAULT_IOU_THRESHOLDS, scores=None, device=None):
    """Match every page's predictions to its ground truth at every threshold -> Matches.

    pred_pages, gt_pages: equally long lists of [n,4,2] arrays (n may be 0).  thresholds: f64 values in (0, 1], at most 16.
    scores: optional list of [n] arrays; each page's predictions then take their turns in descending score (stable: equal scores in
    the given order), as a caller of the reference who sorted its predictions would have it.  Without scores the given order is kept,
    as in the reference.  The result is indexed by the predictions as given either way.
    device None: the host twin (no GPU needed); a device: msocr_quad_match there.
    A page above 16384 quads on either side raises ValueError (the kernel's and the host twin's envelope)."""
    from ... import ops
    pred_pages, gt_pages = list(pred_pages), list(gt_pages)
    if len(pred_pages) != len(gt_pages):
        raise ValueError(f"{len(pred_pages)} pages of predictions but {len(gt_pages)} pages of ground truth")
    pred_pages = [_quads(q, "predictions") for q in pred_pages]
    th = ops._thresholds(thresholds)
    if not 1 <= len(th) <= 16 or not bool(np.all((th > 0) & (th <= 1))):
        raise ValueError("thresholds: 1 to 16 values in (0, 1]")
    order = None
    if scores is not None:
        scores = list(scores)
        if len(scores) != len(pred_pages) or any(len(np.atleast_1d(s)) != len(q) for s, q in zip(scores, pred_pages)):
            raise ValueError("scores: one value per prediction")
        order = [np.argsort(-np.asarray(s, dtype=np.float64).reshape(-1), kind="stable") for s in scores]
        pred_pages = [q[o] for q, o in zip(pred_pages, order)]
    pred, n_pred = pack_pages(pred_pages, "predictions")
    gt, n_gt = pack_pages(gt_pages, "ground truth")
    if len(n_pred) == 0:
        return Matches([], [], np.zeros((0, len(th), 3), dtype=np.int32), th)
    if device is None:
        match, iou, counts = ops.quad_match_host(pred, n_pred, gt, n_gt, th)
    else:
        import torch
        dev = torch.device(device)
        with torch.cuda.device(dev):
            match, iou, counts = (t.cpu().numpy() for t in ops.quad_match(*(torch.from_numpy(a).to(dev) for a in (pred, n_pred, gt, n_gt)), th))
    ms, is_ = [], []
    for p, n in enumerate(n_pred):
        m, i = match[p, :, :n].copy(), iou[p, :, :n].copy()
        if order is not None:  # back to the given order
            m[:, order[p]], i[:, order[p]] = m.copy(), i.copy()
        ms.append(m)
        is_.append(i)
    return Matches(ms, is_, counts, th)


def detection_f1(counts, thresholds=None):
    """counts [..., T, 3] (tp, fp, fn; leading axes, the pages, are summed: micro-averaging as in the reference) ->
    {"thresholds", "tp", "fp", "fn", "precision", "recall", "f1", "f1_at_05", "f1_avg"} with the reference's zero guards
    (utils.py:472-474): an empty denominator gives 0.  f1_avg = np.mean(f1) (compute_f1_metrics); f1_at_05 is the F1 at the threshold
    equal to 0.5, None when there is none.  thresholds None: DEFAULT_IOU_THRESHOLDS (counts must then have its ten rows)."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim < 2 or c.shape[-1] != 3:
        raise ValueError(f"counts are [..., T, 3], got shape {c.shape}")
    c = c.reshape(-1, c.shape[-2], 3).sum(axis=0)
    th = DEFAULT_IOU_THRESHOLDS if thresholds is None else np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    if len(th) != len(c):
        raise ValueError(f"{len(c)} rows of counts for {len(th)} thresholds")
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    prec = np.array([t / (t + f) if t + f > 0 else 0.0 for t, f in zip(tp.tolist(), fp.tolist())], dtype=np.float64)
    rec = np.array([t / (t + f) if t + f > 0 else 0.0 for t, f in zip(tp.tolist(), fn.tolist())], dtype=np.float64)
    f1 = np.array([2 * p * r / (p + r) if (p + r) > 0 else 0.0 for p, r in zip(prec.tolist(), rec.tolist())], dtype=np.float64)
    at05 = np.flatnonzero(th == 0.5)
    return {"thresholds": th, "tp": tp, "fp": fp, "fn": fn, "precision": prec, "recall": rec, "f1": f1,
            "f1_at_05": float(f1[at05[0]]) if len(at05) else None, "f1_avg": float(np.mean(f1))}


def load_coco_quads(path):
    """COCO ground truth as the reference's load_gt reads it (annotations[*].segmentation[0], keyed by image_id; an annotation without
    a segmentation is skipped) -> {image_id: [n,4,2] f32}.  A segmentation that is not 8 numbers raises ValueError."""
    with open(path, "r", encoding="utf-8") as f:
        coco = json.load(f)
    segs = {}
    for ann in coco["annotations"]:
        seg = ann.get("segmentation", [])
        if not seg:
            continue
        s = seg[0]
        if not isinstance(s, (list, tuple)) or len(s) != 8 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in s):
            raise ValueError(f"annotation {ann.get('id')!r} of image {ann.get('image_id')!r}: a quad is 8 numbers, got {s!r}")
        segs.setdefault(ann["image_id"], []).append(s)
    return {iid: np.asarray(v, dtype=np.float32).reshape(-1, 4, 2) for iid, v in segs.items()}
