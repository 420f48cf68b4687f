"""TRBA recogniser plugin — drop-in for the reference class
(/root/reference/src/manuscript/recognizers/_trba/__init__.py:23-434, inference half).

Same constructor (model_path / charset_path / config_path / device / weights_path alias), same
`predict` signature, outputs and exceptions.  SE-ResNet31, the BiLSTM encoder and the attention
decoder (greedy and beam) run on the MI355X through libmsocr.so; there is no CPU execution path.

Extensions (keyword-only): precision="fp32"|"bf16" for the CNN (recurrent/attention stages are
always exact f32), state_dict=... / config=... for in-memory weights (nothing can be downloaded
offline), device_batch=2048 rows per launch sequence, predict(..., return_chars=True) for per-symbol
confidence and position (from the decoder's attention weights), predict(..., n_best=n) for the beam search's n
best final readings with their scores, score(images, texts) for the forced decode of given transcriptions: how
well a text fits a word image and where its symbols sit, predict(..., lexicon=Lexicon(...)) for a beam search
constrained to a closed vocabulary, predict(..., lm=CharLM(...), lm_weight=w) for a beam search fused with a
character n-gram language model, for open-vocabulary text, predict(..., suggest=Lexicon(...)) for the
lexicon words nearest to every reading by edit distance, behind any decode, and evaluate(images, texts) for accuracy and CER over
the same distance.  Confidences reproduce the reference's
dependence on `batch_size` chunks (its decode loop stops per chunk, model.py:215,254).
"""
import json
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
from PIL import Image

from ... import _native as nat
from ... import ops
from ..._graphpool import GraphPool, Lease
from .net import TrbaNet
from .transforms import decode_tokens, frame_to_pixel, frame_to_quad_x, load_charset, pack_targets, resize_and_pad, resized_size


class _Launch(NamedTuple):
    """What the decode of one launch left on the device (AttnDecoder.greedy / beam); the other mode's fields are None."""
    logits: Optional[torch.Tensor] = None  # greedy: [B, steps, V] f32
    ids: Optional[torch.Tensor] = None     # greedy: [B, steps] i32
    ws: Optional[torch.Tensor] = None      # beam: the back-tracking workspace for beam_finalize
    fin: Optional[torch.Tensor] = None     # beam: [B] i32, the step at which each row's beams were all finished
    alpha: Optional[torch.Tensor] = None   # char_details: the attention weights (greedy) / their per-beam trace (beam)


@dataclass(slots=True)
class _Recognition:
    """Handle from recognize_start / recognize_start_graph for recognize_finish."""
    parts: List[Optional[_Launch]]  # one per launch; recognize_finish clears each once it is reduced
    bounds: List[Tuple[int, int]]   # the launches' row ranges
    N: int                          # rows launched
    rows: int                       # rows asked for: a graph replay carries N - rows padding rows behind them
    mode: str
    beam: int
    char_details: bool = False
    graph_inst: Optional[Lease] = None  # the replayed graph instance; None = plain launches
    lexicon: Any = None                 # the Lexicon the beam decode was constrained to; None = the open search
    lm: Any = None                      # the CharLM the beam decode was fused with; None = the model's own scores


def _row_ends(ids, trun, eos_id):
    """ids [N,T], t_run [N] -> per row, where its text ends: the first EOS, at most t_run (what decode_tokens reads)."""
    stop = (ids == eos_id) | (np.arange(ids.shape[1])[None, :] >= np.asarray(trun)[:, None])
    return np.where(stop.any(axis=1), stop.argmax(axis=1), ids.shape[1])


class TRBA:
    _DEFAULT_PRESET_NAME = "exp_1_baseline"
    _DEFAULT_STORAGE_ROOT = Path.home() / ".manuscript" / "trba"
    _DEFAULT_WEIGHTS_FILENAME = "weights.pth"
    _DEFAULT_CONFIG_FILENAME = "config.json"

    def __init__(self, model_path: Optional[str] = None, charset_path: Optional[str] = None, config_path: Optional[str] = None,
                 device: str = "auto", **kwargs: Any):
        weights_path = kwargs.pop("weights_path", None)
        precision = kwargs.pop("precision", "fp32")
        state_dict = kwargs.pop("state_dict", None)
        config = kwargs.pop("config", None)
        self.device_batch = int(kwargs.pop("device_batch", 2048))
        # hipGraph replay of crop + encode + beam decode (recognize_start_graph), for Pipeline's device-ordered route; bench.py --graphs
        self.use_graphs = bool(kwargs.pop("use_graphs", False))
        self.graph_cache_buckets = int(kwargs.pop("graph_cache_buckets", 8))  # captured (stream, pages, row bucket) keys kept
        self._graphs = GraphPool()
        self.last_rows = self.last_run_length_sum = 0  # rows finished and the sum of their chunks' run lengths; bench.py reads and resets
        if kwargs:
            raise TypeError(f"Unexpected keyword argument(s): {', '.join(kwargs.keys())}")
        if weights_path is not None and model_path is not None:
            if os.path.abspath(os.fspath(weights_path)) != os.path.abspath(os.fspath(model_path)):
                raise ValueError("Provide either model_path or weights_path, but not both with different values.")

        if state_dict is None:
            self.model_path, resolved_config = self._resolve_paths(weights_path if weights_path is not None else model_path, config_path)
        else:
            self.model_path, resolved_config = None, (os.fspath(config_path) if config_path is not None else None)
            if resolved_config is not None and not os.path.exists(resolved_config):
                raise FileNotFoundError(f"Config file not found: {resolved_config}")

        if charset_path is None:
            charset_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "charset.txt")
        self.charset_path = os.fspath(charset_path)
        self.config_path = resolved_config
        if not os.path.exists(self.charset_path):
            raise FileNotFoundError(f"Charset file not found: {self.charset_path}")
        if config is None:
            if self.config_path is not None:
                with open(self.config_path, "r", encoding="utf-8") as f:
                    config = json.load(f)
            else:
                config = {}
        self.max_length = config.get("max_len", 25)
        self.hidden_size = config.get("hidden_size", 256)
        self.img_h = config.get("img_h", 64)
        self.img_w = config.get("img_w", 256)

        if device == "auto":
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        else:
            self.device = torch.device(device)
        self.itos, self.stoi = load_charset(self.charset_path)
        self.pad_id = self.stoi["<PAD>"]
        self.sos_id = self.stoi["<SOS>"]
        self.eos_id = self.stoi["<EOS>"]
        self.blank_id = self.stoi.get("<BLANK>", None)

        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(
                f"manuscript_ocr_amd.TRBA runs only on a HIP device (MI355X); device={self.device}, "
                f"torch.cuda.is_available()={torch.cuda.is_available()}. There is no CPU fallback."
            )
        if state_dict is None:
            obj = torch.load(self.model_path, map_location="cpu", weights_only=True)
            state_dict = obj["model_state"] if isinstance(obj, dict) and "model_state" in obj else obj  # training/utils.py:54-59
        self.precision = precision
        if precision not in ("fp32", "fp32-exact", "bf16"):
            raise ValueError(f"precision must be 'fp32', 'fp32-exact' or 'bf16', got {precision!r}")
        self.model = TrbaNet(state_dict, len(self.itos), self.hidden_size, torch.bfloat16 if precision == "bf16" else torch.float32,
                             self.device, split=(False if precision == "fp32-exact" else None))

    # ------------------------------------------------------------------------------------- paths
    def _resolve_paths(self, model_path, config_path) -> Tuple[str, Optional[str]]:
        if model_path is None:
            target = self._DEFAULT_STORAGE_ROOT.expanduser() / self._DEFAULT_PRESET_NAME
            for cand in (Path("weights") / "trba" / self._DEFAULT_WEIGHTS_FILENAME, target / self._DEFAULT_WEIGHTS_FILENAME):
                if cand.exists():
                    model_path = os.fspath(cand)
                    break
            else:  # the reference downloads trba_exp_1_64.pth/.json with gdown (__init__.py:207-243); no network here
                raise FileNotFoundError(
                    "TRBA weights not found: pass model_path=... (or state_dict=...), or place weights.pth (+config.json) under "
                    "./weights/trba/ or ~/.manuscript/trba/exp_1_baseline/ (automatic download is unavailable offline)."
                )
        resolved = os.fspath(model_path)
        if not os.path.exists(resolved):
            raise FileNotFoundError(f"Model checkpoint not found: {resolved}")
        if config_path is not None:
            cfg = os.fspath(config_path)
            if not os.path.exists(cfg):
                raise FileNotFoundError(f"Config file not found: {cfg}")
        else:
            wf = Path(resolved)
            cfg = next((os.fspath(c) for c in (wf.with_suffix(".json"), wf.parent / "config.json") if c.exists()), None)
        return resolved, cfg

    # ------------------------------------------------------------------------------------- preprocessing
    def _load_rgb(self, image) -> np.ndarray:
        if isinstance(image, str):
            if not os.path.exists(image):
                raise FileNotFoundError(f"Image file not found: {image}")
            try:
                with Image.open(image) as im:
                    return np.array(im.convert("RGB"))
            except Exception:
                raise ValueError(f"Cannot read image: {image}")
        if isinstance(image, Image.Image):
            return np.array(image.convert("RGB"))
        if isinstance(image, np.ndarray):
            return image
        raise ValueError(f"Unsupported image type: {type(image)}")

    def _canvases(self, images) -> np.ndarray:
        """ResizeAndPadA on the host (u8), one [img_h, img_w, 3] canvas per crop."""
        return np.stack([resize_and_pad(self._load_rgb(im), self.img_h, self.img_w) for im in images])

    # ------------------------------------------------------------------------------------- device path
    def _device_batches(self, N, spans, batch_size):
        """Reference chunks (slices of `batch_size` rows inside each span = one model call of the reference) packed into
        launches of at most `device_batch` rows that never split a chunk.  -> (bounds [(lo, hi)], per-launch int32 meta
        = chunk ids of the rows followed by the chunk sizes)."""
        chunk_of = np.full(N, -1, dtype=np.int64)
        chunks = []
        for s0, cnt in (spans if spans is not None else [(0, N)]):
            for c0 in range(s0, s0 + cnt, batch_size):
                c1 = min(c0 + batch_size, s0 + cnt)
                chunk_of[c0:c1] = len(chunks)
                chunks.append((c0, c1))
        contiguous = len(chunks) > 0 and chunks[0][0] == 0 and chunks[-1][1] == N and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        if not contiguous:  # rows outside every span, or spans out of order: no chunk information (all steps run)
            return [(s, min(s + self.device_batch, N)) for s in range(0, N, self.device_batch)], None
        bounds, metas, lo, first = [], [], 0, 0
        for k, (c0, c1) in enumerate(chunks + [(N, N)]):
            if k == len(chunks) or (c1 - lo > self.device_batch and c0 > lo):
                ids = chunk_of[lo:c0] - first
                sizes = np.array([b - a for a, b in chunks[first:k]], dtype=np.int64)
                bounds.append((lo, c0))
                metas.append(np.concatenate([ids, sizes]).astype(np.int32))
                lo, first = c0, k
        return bounds, metas

    def prepare_chunks(self, N, spans, batch_size=32):
        """Chunk metadata of `recognize_start` for N rows, uploaded on the CURRENT stream (one small blocking copy).  Callers
        that pipeline several streams do this on a high-priority stream and pass the result as `prepared=` so the copy does
        not queue behind the recogniser work of other groups."""
        bounds, metas = self._device_batches(N, spans, batch_size)
        meta_dev = torch.from_numpy(np.concatenate(metas)).to(self.device) if metas is not None else None
        return bounds, metas, meta_dev

    def recognize_start(self, canvases_dev: torch.Tensor, mode="beam", beam_size=8, temperature=1.7, alpha=0.9, spans=None,
                        batch_size=32, prepared=None, char_details=False, lexicon=None, lm=None, lm_weight=0.5):
        """Phase 1 — encode + decode of [N,img_h,img_w,3] u8 device canvases, enqueued on the CURRENT stream without any
        synchronisation.  Returns a handle for `recognize_finish`.  `spans`/`batch_size` (the same values `recognize_finish`
        will get) tell the beam kernel which rows share a reference chunk, so it can stop a chunk where the reference's
        loop does; without them every row runs all max_length steps (same results).  char_details: the decode also keeps its attention
        weights (on the device) and `recognize_finish` returns per-symbol arrays; every other result is the same either way.
        lexicon (a Lexicon built for this recogniser's charset and max_len; mode "beam"): the beam search is constrained to the
        lexicon's words — every hypothesis carries a node of its prefix tree and may be extended only along it (DESIGN.md section
        4.15).  Every array `recognize_finish` returns keeps its meaning; `Lexicon.find` of a row's ids gives the word's index.
        lm (a CharLM over this recogniser's charset; mode "beam"; not together with a lexicon) and lm_weight (finite, >= 0; the default
        0.5 is a placeholder, not a tuned value): every candidate of a live hypothesis gains lm_weight * log P_lm(token | context)
        (DESIGN.md section 4.16).  Every array `recognize_finish` returns keeps its meaning: log-probabilities and confidences are the
        model's own numbers; `lm_logps` gives the language model's for the returned ids."""
        if mode not in ("greedy", "beam"):
            raise ValueError(f"Unknown mode: {mode}")
        self._check_lexicon(lexicon, mode)
        self._check_lm(lm, lm_weight, mode, lexicon)
        N = canvases_dev.shape[0]
        if mode == "beam" and prepared is not None:
            bounds, metas, meta_dev = prepared
            if meta_dev is not None:
                meta_dev.record_stream(torch.cuda.current_stream())
        elif mode == "beam" and spans is not None:
            bounds, metas, meta_dev = self.prepare_chunks(N, spans, batch_size)  # before any encoder work is queued here
        else:
            bounds, metas, meta_dev = [(s, min(s + self.device_batch, N)) for s in range(0, N, self.device_batch)], None, None
        parts, off = [], 0
        for k, (lo, hi) in enumerate(bounds):
            cv = canvases_dev[lo:hi]
            batch_H, proj_H = self.model.encode(cv)
            if mode == "greedy":
                res = self.model.greedy(batch_H, proj_H, self.max_length, self.sos_id, self.eos_id, self.blank_id, want_alpha=char_details)
                logits, ids, al = res if char_details else (*res, None)
                parts.append(_Launch(logits=logits, ids=ids, alpha=al))
            else:
                chunks = None
                if meta_dev is not None:
                    nrows, nch = hi - lo, len(metas[k]) - (hi - lo)
                    chunks = (meta_dev[off:off + nrows], meta_dev[off + nrows:off + nrows + nch],
                              torch.zeros((2 * nch,), dtype=torch.int32, device=self.device))
                    off += nrows + nch
                res = self.model.beam(batch_H, proj_H, self.max_length, beam_size, alpha, temperature, self.sos_id, self.eos_id,
                                      self.blank_id, chunks, want_alpha=char_details, lexicon=lexicon,
                                      **({} if lm is None else {"lm": lm, "lm_weight": lm_weight}))
                if lexicon is not None or lm is not None:  # these kernels always write the weight trace; it is kept only if asked for
                    ws, fin, _lp, al, _nodes = res
                    al = al if char_details else None
                else:
                    ws, fin, _lp, al = res if char_details else (*res, None)
                parts.append(_Launch(ws=ws, fin=fin, alpha=al))
        return _Recognition(parts, bounds, N, N, mode, beam_size, bool(char_details), lexicon=lexicon, lm=lm)

    def recognize_start_graph(self, pages_dev: torch.Tensor, desc_dev: torch.Tensor, spans, batch_size=32, beam_size=8,
                              temperature=1.7, alpha=0.9, upload_stream=None, char_details=False, rectified=False, lexicon=None, lm=None):
        """`recognize_start` for crops that are still descriptors on the device (ops.reading_order_crops), as ONE hipGraph replay:
        crop + ResizeAndPadA, SE-ResNet31, BiLSTMs and the beam decode of up to `device_batch` rows are captured once per
        (page tensor, row bucket) and replayed (BASELINE configs[3]: "hipGraph-captured").  The row count is rounded up to a
        multiple of 32; the padding rows repeat crop 0 and form a reference chunk of their own, so they can neither change a real
        row's result nor delay a real chunk's early exit.  Falls back to the eager path (returns None) for empty or oversized
        batches, while kernels are being profiled, and for the first call of a bucket (lazy one-time kernel attributes must not
        fall into a capture), and whenever char_details or rectified crops (Pipeline.rectify_crops: the captured graph holds the AABB
        crop kernel, not msocr_quad_crop) are asked for (those paths are not captured).  Results are bit-identical to the eager path
        (tests/test_gpu_pipeline.py).  `recognize_finish(n_best=...)` needs nothing from this route: the captured graph ends at the
        decode, and the beam workspace the alternatives are read from is in the handle it returns.  A lexicon is a ValueError here:
        captured graphs are not provided for the lexicon-constrained decode.  So is a language model (lm)."""
        if lm is not None:
            raise ValueError("captured graphs are not provided for the decode fused with a language model: use recognize_start, or a "
                             "recogniser without use_graphs")
        if lexicon is not None:
            raise ValueError("captured graphs are not provided for the lexicon-constrained decode: use recognize_start, or a "
                             "recogniser without use_graphs")
        M = int(desc_dev.shape[0])
        Mcap = (M + 31) // 32 * 32
        if M == 0 or Mcap > self.device_batch or ops.PROFILE is not None or char_details or rectified:
            return None
        nch_cap = Mcap // batch_size + len(spans) + 2  # chunks of the real rows (<= rows/batch_size + one per page) + the padding chunk
        # one pool per launch stream: the groups of a batch are in flight together, each replays its own instances
        key = (torch.cuda.current_stream().cuda_stream, pages_dev.data_ptr(), tuple(pages_dev.shape), Mcap, nch_cap, batch_size, beam_size,
               float(temperature), float(alpha))
        # bounded cache: the key holds the page tensor's address, so callers whose pages move would otherwise capture
        # without end, each instance pinning a private pool of up to device_batch crops of activations.
        if not self._graphs.warm(key, max_buckets=self.graph_cache_buckets):
            return None
        # chunk metadata of the real rows (as prepare_chunks) + one chunk for the padding rows, into the instance's static buffer
        bounds, metas = self._device_batches(M, spans, batch_size)
        if metas is None or len(bounds) != 1:
            return None
        ids, sizes = metas[0][:M], metas[0][M:]
        if len(sizes) + 1 > nch_cap:
            return None
        meta = np.zeros(Mcap + nch_cap, dtype=np.int32)
        meta[:M] = ids
        meta[M:Mcap] = len(sizes)
        meta[Mcap:Mcap + len(sizes)] = sizes
        meta[Mcap + len(sizes)] = max(Mcap - M, 1)

        def capture():
            dbuf = torch.zeros((Mcap, 8), dtype=torch.int32, device=self.device)
            mbuf = torch.zeros((Mcap + nch_cap,), dtype=torch.int32, device=self.device)
            dbuf[:M].copy_(desc_dev)
            dbuf[M:] = desc_dev[0]
            mbuf.copy_(torch.from_numpy(meta).to(self.device))
            torch.cuda.current_stream().synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                canv = ops.crop_resize_pad(pages_dev, None, self.img_h, self.img_w, desc_dev=dbuf)
                state = torch.zeros((2 * nch_cap,), dtype=torch.int32, device=self.device)
                batch_H, proj_H = self.model.encode(canv)
                ws, fin, _lp = self.model.beam(batch_H, proj_H, self.max_length, beam_size, alpha, temperature, self.sos_id, self.eos_id,
                                               self.blank_id, (mbuf[:Mcap], mbuf[Mcap:], state))
            return graph, (dbuf, mbuf, _Launch(ws=ws, fin=fin))

        inst = self._graphs.acquire(key, capture)
        if inst is None:
            return None
        dbuf, mbuf, part = inst.state
        dbuf[:M].copy_(desc_dev, non_blocking=True)
        if Mcap > M:
            dbuf[M:] = desc_dev[0]
        # the small blocking upload of the chunk metadata must not queue behind the recogniser work already on this stream
        cur = torch.cuda.current_stream()
        up = upload_stream if upload_stream is not None else cur
        with torch.cuda.stream(up):
            meta_dev = torch.from_numpy(meta).to(self.device)
        if up is not cur:
            cur.wait_stream(up)
            meta_dev.record_stream(cur)
        mbuf.copy_(meta_dev, non_blocking=True)
        inst.graph.replay()
        return _Recognition([part], [(0, Mcap)], Mcap, M, "beam", beam_size, graph_inst=Lease(inst))

    def recognize_finish(self, handle, batch_size=32, spans=None, return_logits=False, n_best=0, suggest=None, suggest_k=3,
                         suggest_max_distance=None, targets=None, suggest_costs=None):
        """Phases 2-3 — derive the reference's per-chunk run lengths, back-track (beam) and reduce confidences.

        `spans` = [(start, count), ...] groups of rows that the reference would have passed to ONE predict() call
        (one page each); inside a span rows are chunked by `batch_size` and every chunk stops at its own step
        (greedy: first step where every row emits EOS; beam: once every beam of every row is finished) — that run
        length enters the confidences.  Only ids and one float per row cross PCIe (msocr_seq_confidence).
        A handle started with char_details=True: three more host arrays [N, steps] behind the others — prob (f32: the probability
        of the token of every step, whose mean over t < t_run is the confidence), centre (f32: the attention centroid in encoder
        frames) and peak (i32: the arg-max frame); steps t >= t_run hold 0, 0, -1 (msocr_seq_char_details; the weights stay on the
        device).
        n_best >= 1 (beam handles, n_best <= the handle's beam width): four more host arrays behind everything else — alt_ids
        [N, n_best, steps] i32, alt_prob [N, n_best, steps] f32, alt_conf [N, n_best] f32 and alt_logp [N, n_best] f32, the search's
        n_best best final hypotheses per row in its own order (msocr_attn_beam_nbest; `alternatives` turns them into texts).  Rank 0
        is the row's own ids and confidence.
        suggest (a Lexicon over this recogniser's charset; not for a handle whose decode was constrained to a lexicon): two more host
        arrays behind all others — sug_index [N, suggest_k] i32 and sug_dist [N, suggest_k] i32, per row the suggest_k lexicon words
        nearest to its text by Levenshtein distance, nearest first, -1 / -1 where there are fewer or suggest_max_distance (None = no
        bound) drops them (msocr_lexicon_nearest on the finalised device ids; `Lexicon.suggestions` turns
        them into words).  With n_best they describe rank 0.  Nothing else changes with the switch.
        suggest_costs (an EditCosts over the same charset, only with suggest): the lookup ranks by the confusion-weighted distance
        instead (msocr_lexicon_nearest_weighted); sug_dist and suggest_max_distance are then in cost units.
        targets = (target [N, steps_t] i32, t_run [N] i32), host arrays as transforms.pack_targets packs transcriptions: three more
        host arrays behind all others — distance [N] i32, the Levenshtein distance between every row's text and its target's, and the
        two text lengths hyp_len [N], ref_len [N] (msocr_edit_distance_pairs on the device ids; `evaluate`)."""
        try:
            self._check_suggest(suggest, suggest_k, suggest_max_distance, handle.lexicon, handle.mode, suggest_costs)
            if n_best < 0 or (n_best and (handle.mode != "beam" or n_best > handle.beam)):
                raise ValueError(f"n_best = {n_best} needs a beam decode of at least that width (mode {handle.mode!r}, beam_size {handle.beam})")
            return self._recognize_finish(handle, batch_size, spans, return_logits, int(n_best),
                                          None if suggest is None else (suggest, suggest_k, suggest_max_distance, suggest_costs),
                                          targets)
        finally:
            if handle.graph_inst is not None:  # also on an exception: the instance must not stay leased for ever
                handle.graph_inst.release()

    def _recognize_finish(self, handle, batch_size, spans, return_logits, n_best=0, suggest=None, targets=None):
        parts, N, M_real, mode, beam_size = handle.parts, handle.N, handle.rows, handle.mode, handle.beam
        spans = spans if spans is not None else [(0, M_real)]
        steps = self.max_length + 1 if mode == "greedy" else self.max_length
        trun = np.ones(N, dtype=np.int32)
        host = np.concatenate([(p.ids if mode == "greedy" else p.fin).cpu().numpy() for p in parts])
        for s0, cnt in spans:
            for c0 in range(s0, s0 + cnt, batch_size):
                c1 = min(c0 + batch_size, s0 + cnt)
                if mode == "greedy":
                    hit = np.flatnonzero(np.all(host[c0:c1] == self.eos_id, axis=0))
                    trun[c0:c1] = (hit[0] + 1) if len(hit) else steps
                else:
                    trun[c0:c1] = host[c0:c1].max()
        self.last_run_length_sum += int(trun[:M_real].sum())
        self.last_rows += M_real
        trun_dev = torch.from_numpy(trun).to(self.device)
        details = handle.char_details
        ids_out, conf_out, logit_out, det_out, alt_out, sug_out, pair_out = [], [], [], [], [], [], []
        if targets is not None:
            if steps > 64:
                raise ValueError(f"the edit-distance kernel takes rows of at most 64 steps, this decode has {steps}")
            tgt = np.ascontiguousarray(targets[0], dtype=np.int32)
            if tgt.ndim != 2 or tgt.shape[0] != M_real or not 1 <= tgt.shape[1] <= 64 or np.shape(targets[1]) != (M_real,):
                raise ValueError(f"targets must be ([{M_real}, 1..64], [{M_real}]) arrays")
            tgt_full = np.full((N, tgt.shape[1]), self.eos_id, dtype=np.int32)  # a graph replay's padding rows compare against ""
            tgt_full[:M_real] = tgt
            ttr_full = np.zeros(N, dtype=np.int32)
            ttr_full[:M_real] = targets[1]
            tgt_dev, ttr_dev = torch.from_numpy(tgt_full).to(self.device), torch.from_numpy(ttr_full).to(self.device)
        for k, (s, hi) in enumerate(handle.bounds):
            B = hi - s
            tr = trun_dev[s:s + B]
            part = parts[k]
            if mode == "greedy":
                lg, ids, al = part.logits, part.ids, part.alpha
            elif details:
                lg, ids, al = self.model.beam_finalize(part.ws, B, steps, beam_size, tr, alpha_ws=part.alpha)
            else:
                lg, ids = self.model.beam_finalize(part.ws, B, steps, beam_size, tr)
            conf = torch.empty((B,), dtype=torch.float32, device=self.device)
            nat.check(nat.lib().msocr_seq_confidence(lg.data_ptr(), ids.data_ptr(), tr.data_ptr(), B, self.model.V, steps, conf.data_ptr(),
                                                     ops._stream()), "seq_confidence")
            ids_out.append(ids), conf_out.append(conf)
            if suggest is not None:  # on the device ids, before they cross PCIe
                sug_out.append(suggest[0].nearest_device(ids, tr, suggest[1], suggest[2], suggest[3]))
            if targets is not None:
                po = torch.empty((3, B), dtype=torch.int32, device=self.device)
                ids_c = ids.contiguous()
                nat.check(nat.lib().msocr_edit_distance_pairs(ids_c.data_ptr(), tr.data_ptr(), steps, tgt_dev[s:s + B].data_ptr(),
                                                              ttr_dev[s:s + B].data_ptr(), tgt_dev.shape[1], B, self.model.V, self.eos_id,
                                                              self.pad_id, -1 if self.blank_id is None else self.blank_id,
                                                              po[0].data_ptr(), po[1].data_ptr(), po[2].data_ptr(), ops._stream()),
                          "edit_distance_pairs")
                pair_out.append(po)
            if details:
                prob = torch.empty((B, steps), dtype=torch.float32, device=self.device)
                centre = torch.empty((B, steps), dtype=torch.float32, device=self.device)
                peak = torch.empty((B, steps), dtype=torch.int32, device=self.device)
                nat.check(nat.lib().msocr_seq_char_details(lg.data_ptr(), ids.data_ptr(), al.data_ptr(), tr.data_ptr(), B, self.model.V, steps,
                                                           al.shape[-1], prob.data_ptr(), centre.data_ptr(), peak.data_ptr(), ops._stream()),
                          "seq_char_details")
                det_out.append((prob, centre, peak))
            if return_logits:
                logit_out.append(lg.cpu().numpy())
            if n_best:
                alt_out.append(self.model.beam_nbest(part.ws, B, steps, beam_size, tr, n_best, self.eos_id))
            parts[k] = part = None
        ids_h = torch.cat(ids_out).cpu().numpy()[:M_real]
        conf_h = torch.cat(conf_out).cpu().numpy()[:M_real]
        out = (ids_h, trun[:M_real], conf_h)
        if return_logits:
            out += (np.concatenate(logit_out)[:M_real],)
        if details:
            out += tuple(torch.cat([d[i] for d in det_out]).cpu().numpy()[:M_real] for i in range(3))
        if n_best:
            out += tuple(torch.cat([a[i] for a in alt_out]).cpu().numpy()[:M_real] for i in range(4))
        if suggest is not None:
            out += tuple(torch.cat([g[i] for g in sug_out]).cpu().numpy()[:M_real] for i in range(2))
        if targets is not None:
            out += tuple(torch.cat([g[i] for g in pair_out]).cpu().numpy()[:M_real] for i in range(3))
        return out

    def recognize_canvases(self, canvases_dev: torch.Tensor, batch_size=32, mode="beam", beam_size=8, temperature=1.7, alpha=0.9,
                           spans=None, return_logits=False, char_details=False, n_best=0, lexicon=None, lm=None, lm_weight=0.5,
                           suggest=None, suggest_k=3, suggest_max_distance=None, suggest_costs=None):
        """canvases [N,img_h,img_w,3] u8 on device -> (ids [N,steps] i32, t_run [N] i32, conf [N] f32[, logits][, prob, centre, peak]
        [, alt_ids, alt_prob, alt_conf, alt_logp][, sug_index, sug_dist]) on host.  lexicon, lm, lm_weight: as for `recognize_start`;
        suggest, suggest_k, suggest_max_distance, suggest_costs: as for `recognize_finish`."""
        self._check_n_best(n_best, mode, beam_size)
        self._check_suggest(suggest, suggest_k, suggest_max_distance, lexicon, mode, suggest_costs)
        return self.recognize_finish(self.recognize_start(canvases_dev, mode, beam_size, temperature, alpha,
                                                          spans if spans is not None else [(0, canvases_dev.shape[0])], batch_size,
                                                          char_details=char_details, lexicon=lexicon, lm=lm, lm_weight=lm_weight),
                                     batch_size, spans, return_logits, n_best=n_best, suggest=suggest, suggest_k=suggest_k,
                                     suggest_max_distance=suggest_max_distance, suggest_costs=suggest_costs)

    def texts(self, ids, trun) -> List[str]:
        """decode_tokens (transforms.py:196-206) over the first t_run ids of every row, vectorised: the text ends at the
        first EOS; PAD (and BLANK) ids are skipped."""
        ids = np.asarray(ids)
        T = ids.shape[1] if ids.ndim == 2 else 0
        if not len(ids) or T == 0:
            return ["" for _ in range(len(ids))]
        end = _row_ends(ids, trun, self.eos_id)
        itos, skip = self.itos, {self.pad_id, self.blank_id}
        rows = ids.tolist()
        return ["".join([itos[t] for t in row[:e] if t not in skip]) for row, e in zip(rows, end.tolist())]

    @staticmethod
    def _check_n_best(n_best, mode, beam_size):
        if n_best < 0:
            raise ValueError(f"n_best must not be negative, got {n_best}")
        if n_best and mode == "greedy":
            raise ValueError("n_best needs mode='beam': the greedy decode has one hypothesis")
        if n_best > beam_size:
            raise ValueError(f"n_best = {n_best} exceeds beam_size = {beam_size}: the search keeps beam_size hypotheses")

    def _check_lexicon(self, lexicon, mode):
        if lexicon is None:
            return
        if mode == "greedy":
            raise ValueError("a lexicon needs mode='beam': a constrained arg-max walks into the trie's locally best branch and is not provided")
        if lexicon.max_len != self.max_length:
            raise ValueError(f"the lexicon was built for max_len {lexicon.max_len}, this recogniser's is {self.max_length}")
        if lexicon.num_classes != len(self.itos):
            raise ValueError(f"the lexicon was built for a charset of {lexicon.num_classes} tokens, this recogniser's has {len(self.itos)}")

    def _check_suggest(self, suggest, suggest_k, suggest_max_distance, lexicon=None, mode="beam", suggest_costs=None):
        if suggest is None:
            if suggest_costs is not None:
                raise ValueError("suggest_costs needs suggest: the costs weight a lexicon lookup, they start none")
            return
        if lexicon is not None:
            raise ValueError("suggest together with a lexicon is not provided: a constrained decode's word is in its lexicon, at distance 0")
        if suggest.num_classes != len(self.itos):
            raise ValueError(f"the suggest lexicon was built for a charset of {suggest.num_classes} tokens, this recogniser's has {len(self.itos)}")
        suggest._check_k_bound(suggest_k, suggest_max_distance)
        suggest._check_costs(suggest_costs)
        steps = self.max_length + 1 if mode == "greedy" else self.max_length
        if steps > 64:
            raise ValueError(f"the nearest-word lookup takes rows of at most 64 steps, this decode has {steps}")
        suggest._check_wordlist()

    def _check_lm(self, lm, lm_weight, mode, lexicon=None):
        if lm is None:
            return
        if mode == "greedy":
            raise ValueError("a language model needs mode='beam': greedy decoding under a language model is not provided")
        if lexicon is not None:
            raise ValueError("a language model and a lexicon in one decode are not provided")
        if lm.num_classes != len(self.itos) or lm.sos_id != self.sos_id:
            raise ValueError(f"the language model was built for a charset of {lm.num_classes} tokens with sos_id {lm.sos_id}, this "
                             f"recogniser's has {len(self.itos)} with sos_id {self.sos_id}")
        if lm.eos_id is not None and lm.eos_id != self.eos_id:
            raise ValueError(f"the language model's eos_id is {lm.eos_id}, this recogniser's {self.eos_id}")
        if not (np.isfinite(lm_weight) and lm_weight >= 0):
            raise ValueError(f"lm_weight must be finite and >= 0, got {lm_weight!r}")

    def lm_logps(self, ids, trun, lm) -> List[float]:
        """Per row of ids [N, steps], the unweighted language-model log-probability of its reading: the sum of table[ctx][id] over the
        first t_run ids up to and including the first EOS, in float64 on the host (CharLM.logp; the table is on the host anyway and a
        word has a few tokens, so no device gather)."""
        V, ctx0, n_ctx, tab, eos = lm.num_classes, lm.ctx0, lm.n_ctx, lm.table, self.eos_id
        out = []
        for row, e in zip(np.asarray(ids).tolist(), np.asarray(trun).tolist()):
            ctx, total = ctx0, 0.0
            for t in row[:e]:
                if t < 0:
                    break
                total += float(tab[ctx, t])
                if t == eos:
                    break
                ctx = (ctx * V + t) % n_ctx
            out.append(total)
        return out

    def lexicon_indices(self, ids, lexicon) -> List[int]:
        """Per row of ids [N, steps], `lexicon.find`: the index of the row's word in lexicon.words, -1 if it is none (a constrained
        decode returns such a row only where its logits were not finite)."""
        return [lexicon.find(row) for row in np.asarray(ids).tolist()]

    def alternatives(self, alt_ids, trun, alt_conf, alt_logp) -> List[List[Dict[str, Any]]]:
        """Per row, its readings as {"text", "confidence", "logp"} in rank order, from recognize_finish(n_best=...)'s arrays: text by
        `texts` over the rank's ids, confidence as the word's own is computed, logp the hypothesis's summed log-probability.  Entry 0
        is the word's own text and confidence and is always kept; a later rank whose text equals an earlier one of its row is
        dropped (two hypotheses can differ only in PAD tokens, or behind their EOS)."""
        return self._alternatives(alt_ids, trun, alt_conf, alt_logp, None)

    def lexicon_alternatives(self, alt_ids, trun, alt_conf, alt_logp, lexicon) -> List[List[Dict[str, Any]]]:
        """`alternatives` for a decode constrained to `lexicon`: a later rank is kept only if its ids are a lexicon word (a slot that
        died in the search, or never held a word, is none), and every entry also carries "lexicon_index"."""
        return self._alternatives(alt_ids, trun, alt_conf, alt_logp, lexicon)

    def lm_alternatives(self, alt_ids, trun, alt_conf, alt_logp, lm) -> List[List[Dict[str, Any]]]:
        """`alternatives` for a decode fused with `lm`: every entry also carries "lm_logp", the language model's unweighted
        log-probability of its reading; "logp" and "confidence" stay the model's.  The ranks are in fused-score order."""
        return self._alternatives(alt_ids, trun, alt_conf, alt_logp, None, lm)

    def _alternatives(self, alt_ids, trun, alt_conf, alt_logp, lexicon, lm=None):
        alt_ids = np.asarray(alt_ids)
        N, n = alt_ids.shape[:2]
        if not N or not n:
            return [[] for _ in range(N)]
        lex_idx = self.lexicon_indices(alt_ids.reshape(N * n, -1), lexicon) if lexicon is not None else None
        texts = self.texts(alt_ids.reshape(N * n, -1), np.repeat(np.asarray(trun), n))
        lm_lp = self.lm_logps(alt_ids.reshape(N * n, -1), np.repeat(np.asarray(trun), n), lm) if lm is not None else None
        cs = np.clip(np.asarray(alt_conf, dtype=np.float64), 0.0, 1.0).tolist()  # means of exp(log-softmax): within [0, 1] up to rounding
        ls = np.asarray(alt_logp, dtype=np.float64).tolist()
        out = []
        for b in range(N):
            seen, row = set(), []
            for r in range(n):
                t = texts[b * n + r]
                if lex_idx is not None and r and lex_idx[b * n + r] < 0:
                    continue
                if t not in seen:
                    seen.add(t)
                    row.append({"text": t, "confidence": cs[b][r], "logp": ls[b][r]})
                    if lex_idx is not None:
                        row[-1]["lexicon_index"] = lex_idx[b * n + r]
                    if lm_lp is not None:
                        row[-1]["lm_logp"] = lm_lp[b * n + r]
            out.append(row)
        return out

    def _results(self, ids, trun, conf) -> List[Dict[str, Any]]:
        """__init__.py:415-432: decode_tokens over the t_run generated ids; confidence computed on the device."""
        return [{"text": decode_tokens(ids[j, : int(trun[j])], self.itos, self.pad_id, self.eos_id, self.blank_id),
                 "confidence": float(conf[j])} for j in range(len(ids))]

    def chars(self, ids, trun, prob, centre, new_w, x1, x2, qdesc=None) -> List[List[Dict[str, Any]]]:
        """Per row, one {"char", "confidence", "x"} per token that `texts` / decode_tokens keep (t < t_run, up to the first EOS, PAD
        and BLANK skipped), so "".join(c["char"]) is the row's text.  x = frame_to_pixel(centre, new_w, x1, x2): new_w [N] the resized
        widths ResizeAndPadA pasted at x = 0, [x1, x2) the rows' windows in the image the positions are wanted in.  qdesc [N,12]
        (rows cut along quadrilaterals, ops.quad_crop): x = frame_to_quad_x(centre, qdesc) instead, x1 / x2 unused."""
        ids = np.asarray(ids)
        n, T = (ids.shape[0], ids.shape[1]) if ids.ndim == 2 else (len(ids), 0)
        if not n or T == 0:
            return [[] for _ in range(n)]
        end = _row_ends(ids, trun, self.eos_id)
        if qdesc is not None:
            xs = frame_to_quad_x(centre, qdesc).tolist()
        else:
            new_w, x1, x2 = (np.asarray(v, dtype=np.float64).reshape(n, 1) for v in (new_w, x1, x2))
            xs = frame_to_pixel(centre, new_w, x1, x2).tolist()
        ps = np.clip(np.asarray(prob, dtype=np.float64), 0.0, 1.0).tolist()  # exp of a log-softmax: within [0, 1] up to rounding
        itos, skip = self.itos, {self.pad_id, self.blank_id}
        return [[{"char": itos[t], "confidence": p, "x": x} for t, p, x in zip(row[:e], pr, xr) if t not in skip]
                for row, e, pr, xr in zip(ids.tolist(), end.tolist(), ps, xs)]

    # ------------------------------------------------------------------------------------- forced decode
    def score_canvases(self, canvases_dev: torch.Tensor, row_image, tok_in, target, trun, temperature=1.0):
        """The forced decode of R candidate rows over N encoded canvases: canvases [N,img_h,img_w,3] u8 on the device, row_image [R]
        the canvas each row reads, tok_in / target [R, max_length+1] int32 and trun [R] int32 from transforms.pack_targets (host
        arrays).  The encoder runs once per canvas; a row gathers its canvas's encoder outputs, so candidates of one image share
        them.  Not captured into a hipGraph.  -> host arrays (logp [R] f32, conf [R] f32, logp_steps [R, steps] f32, prob [R, steps]
        f32, centre [R, steps] f32, peak [R, steps] i32): the summed log-probability of target over t < trun (msocr_seq_logp, at
        `temperature`), the confidence as predict computes it (msocr_seq_confidence) and msocr_seq_char_details' per-step arrays."""
        N, R = int(canvases_dev.shape[0]), len(row_image)
        steps = self.max_length + 1
        tok_in, target = (np.ascontiguousarray(v, dtype=np.int32) for v in (tok_in, target))
        trun = np.ascontiguousarray(trun, dtype=np.int32)
        row_image = np.ascontiguousarray(row_image, dtype=np.int64)
        if tok_in.shape != (R, steps) or target.shape != (R, steps) or trun.shape != (R,):
            raise ValueError(f"tok_in / target must be [{R}, {steps}] and trun [{R}]")
        if R and (row_image.min() < 0 or row_image.max() >= N):
            raise ValueError("row_image must index the canvases")
        V = self.model.V
        if R and (min(tok_in.min(), target.min()) < 0 or max(tok_in.max(), target.max()) >= V or trun.min() < 0 or trun.max() > steps):
            raise ValueError("token ids must lie in [0, num_classes) and trun in [0, max_length + 1]")
        if R == 0:
            z = np.zeros((0, steps), dtype=np.float32)
            return np.zeros(0, np.float32), np.zeros(0, np.float32), z, z.copy(), z.copy(), np.zeros((0, steps), np.int32)
        enc = [self.model.encode(canvases_dev[s:s + self.device_batch]) for s in range(0, N, self.device_batch)]
        batch_H, proj_H = (torch.cat([e[i] for e in enc]) for i in (0, 1))
        T = batch_H.shape[1]
        dec = self.model.dec
        ctxg = dec.ctx_gates(batch_H).view(N, -1) if dec._matrix_core(T) else None  # the hoisted context product, once per image
        dev = lambda a: torch.from_numpy(a).to(self.device)
        row_dev, tok_dev, tgt_dev, trun_dev = dev(row_image), dev(tok_in), dev(target), dev(trun)
        outs = []
        for s in range(0, R, self.device_batch):
            idx = row_dev[s:s + self.device_batch]
            B = int(idx.shape[0])
            tgt, tr = tgt_dev[s:s + B], trun_dev[s:s + B]
            logits, al = self.model.forced(batch_H.index_select(0, idx), proj_H.index_select(0, idx), tok_dev[s:s + B], self.sos_id,
                                           self.blank_id, ctx_gates=None if ctxg is None else ctxg.index_select(0, idx))
            lps, lp = dec.seq_logp(logits, tgt, tr, temperature)
            prob = torch.empty((B, steps), dtype=torch.float32, device=self.device)
            centre = torch.empty((B, steps), dtype=torch.float32, device=self.device)
            peak = torch.empty((B, steps), dtype=torch.int32, device=self.device)
            nat.check(nat.lib().msocr_seq_char_details(logits.data_ptr(), tgt.data_ptr(), al.data_ptr(), tr.data_ptr(), B, V, steps, T,
                                                       prob.data_ptr(), centre.data_ptr(), peak.data_ptr(), ops._stream()), "seq_char_details")
            conf = torch.empty((B,), dtype=torch.float32, device=self.device)
            nat.check(nat.lib().msocr_seq_confidence(logits.data_ptr(), tgt.data_ptr(), tr.data_ptr(), B, V, steps, conf.data_ptr(),
                                                     ops._stream()), "seq_confidence")
            outs.append((lp, conf, lps, prob, centre, peak))
        return tuple(torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(6))

    def score(self, images, texts, batch_size: int = 32, temperature: float = 1.0, *, strict: bool = True):
        """Forced decode (this package's extension; the reference has the pass only inside training, model.py:287-320): how well does a
        given transcription fit a word image, and where does each of its symbols sit?  texts[i] is a str, or a list of str (candidate
        readings of image i, e.g. from a lexicon).  The decoder is run along the given symbols instead of its own arg-max.  Per image
        one dict for a str, a list of dicts in the given order for a list:
          {"text": the text as packed, "logp": log P(text, EOS | image), the sum of log_softmax(logits / temperature) over the
           text's symbols and its EOS, "confidence": the mean probability of those tokens, as predict computes a confidence (without
           temperature), "chars": [{"char", "confidence", "x"}] as predict(return_chars=True) gives them}.
        Candidates are comparable by logp; exp(logp / (len(text) + 1)) is a per-token geometric mean.  The encoder runs once per
        image whatever the number of candidates.  strict=True: a character outside the charset or a text longer than the model's
        max_len raises ValueError; strict=False drops such characters and truncates, as the reference's pack_attention_targets does
        ("text" then shows what was scored).  batch_size is accepted for symmetry with predict and does not enter the numbers: a
        forced row runs over its own length + 1 steps, there is no chunk-wide stopping step.  "x" is an attention centroid: an
        estimate that means something for trained weights only."""
        if isinstance(images, list) and isinstance(texts, str):
            raise TypeError("texts must have one entry (a str or a list of str) per image")
        images_list, texts_list = (images, list(texts)) if isinstance(images, list) else ([images], [texts])
        if len(texts_list) != len(images_list):
            raise ValueError(f"{len(images_list)} images but {len(texts_list)} entries of texts")
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if not (temperature > 0):
            raise ValueError(f"temperature must be positive, got {temperature}")
        if not images_list:
            return []
        single = [isinstance(t, str) for t in texts_list]
        cands = [[t] if one else list(t) for t, one in zip(texts_list, single)]
        row_image = np.repeat(np.arange(len(cands)), [len(c) for c in cands])
        R = len(row_image)
        packs = []
        for i, c in enumerate(cands):
            try:
                packs.append(pack_targets(c, self.stoi, self.max_length, strict=strict))
            except ValueError as e:
                raise ValueError(f"image {i}: {e}") from None
        tok_in, target, trun = (np.concatenate([p[k] for p in packs]) for k in range(3))
        packed = [t for p in packs for t in p[3]]
        arrays = [self._load_rgb(im) for im in images_list]
        canv = torch.from_numpy(self._canvases(arrays)).to(self.device, non_blocking=True)
        logp, conf, _lps, prob, centre, _peak = self.score_canvases(canv, row_image, tok_in, target, trun, temperature)
        src_w = np.array([a.shape[1] for a in arrays], dtype=np.float64)[row_image]
        new_w = np.array([resized_size(a.shape[0], a.shape[1], self.img_h, self.img_w)[0] for a in arrays], dtype=np.float64)[row_image]
        chars = self.chars(target, trun, prob, centre, new_w, np.zeros(R), src_w)
        entries = [{"text": t, "logp": float(l), "confidence": float(c), "chars": ch} for t, l, c, ch in zip(packed, logp, conf, chars)]
        out, k = [], 0
        for c, one in zip(cands, single):
            out.append(entries[k] if one else entries[k:k + len(c)])
            k += len(c)
        return out

    # ------------------------------------------------------------------------------------- word spotting
    def embed_canvases(self, canvases_dev: torch.Tensor, new_w):
        """The encoder's frames of crops that are already canvases on the device (this package's extension):
        canvases [N, img_h, img_w, 3] u8, new_w [N] the resized width of each crop on its canvas (desc[:, 5], qdesc[:, 9]).
        -> (features [N, T, H] f32 on the device: batch_H of `model.encode`, run in `device_batch` chunks; lengths [N] int32, host:
        min(T, new_w // FRAME_STRIDE + 1), the frames whose column 8 t lies on the crop and not on the canvas padding, which is
        frame_to_pixel's own mapping).  The decoder is not run and `recognize_start` is not touched."""
        from .transforms import FRAME_STRIDE
        N = int(canvases_dev.shape[0])
        new_w = np.asarray(new_w, dtype=np.int64).reshape(-1)
        if new_w.shape != (N,):
            raise ValueError(f"new_w must be [{N}]")
        if N == 0:
            T = self.img_w // FRAME_STRIDE + 1
            return torch.empty((0, T, self.hidden_size), dtype=torch.float32, device=self.device), np.zeros(0, dtype=np.int32)
        feats = torch.cat([self.model.encode(canvases_dev[s:s + self.device_batch])[0] for s in range(0, N, self.device_batch)])
        T = int(feats.shape[1])
        lengths = np.clip(new_w // FRAME_STRIDE + 1, 1, T).astype(np.int32)
        return feats.contiguous(), lengths

    def embed(self, images, batch_size: int = 32):
        """Word images (arrays, paths or PIL images, or one of them) -> (features [N, T, H] f32 on the device, lengths [N] int32), as
        `embed_canvases` gives them for the canvases `predict` would build.  batch_size is accepted for symmetry with predict and
        does not enter the numbers: the encoder has no chunk-wide state."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        images_list = images if isinstance(images, list) else [images]
        arrays = [self._load_rgb(im) for im in images_list]
        if not arrays:
            return self.embed_canvases(torch.empty((0, self.img_h, self.img_w, 3), dtype=torch.uint8, device=self.device), [])
        canv = torch.from_numpy(self._canvases(arrays)).to(self.device, non_blocking=True)
        new_w = [resized_size(a.shape[0], a.shape[1], self.img_h, self.img_w)[0] for a in arrays]
        return self.embed_canvases(canv, new_w)

    def evaluate(self, images, texts, batch_size: int = 32, *, strict: bool = True, **predict_kwargs) -> Dict[str, Any]:
        """Recognise `images` and compare with their transcriptions `texts` (one str per image) by the reference's evaluation
        measures (its trba_metrics.py: CER = Levenshtein / len(reference) per sample, accuracy = exact matches), with the distances
        computed on the device from the decode's ids (msocr_edit_distance_pairs).  The texts are packed as
        `score` packs them (strict=True: a character outside the charset or a text longer than max_len raises ValueError; False drops
        and truncates).  predict_kwargs: mode, beam_size, temperature, alpha, lm, lm_weight, lexicon, as for `predict`.
        -> {"n", "accuracy", "cer_mean" (the mean of the per-sample CERs; a sample with an empty reference counts inf if its text is
        not empty, else 0), "cer_micro" (sum of distances / sum of reference lengths), "distances" [n] i32, "ref_lengths" [n] i32,
        "texts" (the recognised strings)}.  Word error rate is not provided (single-word crops: 1 - accuracy)."""
        images_list = images if isinstance(images, list) else [images]
        texts_list = [texts] if isinstance(texts, str) else list(texts)
        if len(texts_list) != len(images_list):
            raise ValueError(f"{len(images_list)} images but {len(texts_list)} texts")
        unknown = set(predict_kwargs) - {"mode", "beam_size", "temperature", "alpha", "lm", "lm_weight", "lexicon"}
        if unknown:
            raise TypeError(f"evaluate() got unexpected keyword arguments {sorted(unknown)}")
        if not images_list:
            return {"n": 0, "accuracy": 0.0, "cer_mean": 0.0, "cer_micro": 0.0, "distances": np.zeros(0, np.int32),
                    "ref_lengths": np.zeros(0, np.int32), "texts": []}
        _tok_in, target, ttrun, packed = pack_targets(texts_list, self.stoi, self.max_length, strict=strict)
        mode = predict_kwargs.get("mode", "beam")
        if mode not in ("greedy", "beam"):
            raise ValueError(f"Unknown mode: {mode}")
        arrays = [self._load_rgb(im) for im in images_list]
        canv = torch.from_numpy(self._canvases(arrays)).to(self.device, non_blocking=True)
        kw = {k: predict_kwargs[k] for k in ("beam_size", "temperature", "alpha", "lexicon", "lm", "lm_weight") if k in predict_kwargs}
        n = len(images_list)
        handle = self.recognize_start(canv, mode, spans=[(0, n)], batch_size=batch_size, **kw)
        fin = self.recognize_finish(handle, batch_size, None, targets=(target, ttrun))
        ids, trun = fin[:2]
        dist, _hyp_len, ref_len = fin[-3:]
        hyp = self.texts(ids, trun)
        d, L = dist.astype(np.float64), ref_len.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            cer = np.where(L > 0, d / np.maximum(L, 1), np.where(d > 0, np.inf, 0.0))
        total = float(L.sum())
        micro = float(d.sum()) / total if total > 0 else (float("inf") if d.sum() > 0 else 0.0)
        return {"n": n, "accuracy": float(np.mean(dist == 0)), "cer_mean": float(cer.mean()), "cer_micro": micro, "distances": dist,
                "ref_lengths": ref_len, "texts": hyp}

    # ------------------------------------------------------------------------------------- API
    def predict(self, images, batch_size: int = 32, mode: str = "beam", beam_size: int = 8, temperature: float = 1.7,
                alpha: float = 0.9, *, return_chars: bool = False, n_best: int = 0, lexicon=None, lm=None,
                lm_weight: float = 0.5, suggest=None, suggest_k: int = 3, suggest_max_distance=None,
                suggest_costs=None) -> List[Dict[str, Any]]:
        """Same contract as the reference TRBA.predict (__init__.py:290-434).  return_chars=True (this package's keyword-only extension): every
        result also has "chars", a list of {"char", "confidence", "x"} with one entry per symbol of "text": the probability the
        decoder gave the symbol and the estimated x of its centre in pixels of the input image (the attention centroid mapped
        through transforms.FRAME_STRIDE and the resize; an estimate, not a measured glyph position).
        n_best >= 1 (keyword-only extension, mode="beam", n_best <= beam_size): every result also has "alternatives", a list of
        {"text", "confidence", "logp"}: the beam search's n_best best final hypotheses in its own order, duplicates of an earlier text
        dropped (`alternatives`); entry 0 is the result's own text and confidence.  "chars" describes the best reading only.
        lexicon=Lexicon(words, recognizer.stoi, recognizer.max_length) (keyword-only extension, mode="beam"): the beam search is
        constrained to the lexicon's words.  Every result also has "lexicon_index", the index of its text in
        lexicon.words (-1 only where the decoder's logits were not finite); "alternatives" then keeps only readings that are lexicon
        words, each with its "lexicon_index".  A result's rank-0 "logp" is the number `score` gives that text at the same temperature.
        lm=CharLM.from_texts(texts, recognizer.stoi) with lm_weight (keyword-only extension, mode="beam", not together with a lexicon):
        the beam search is fused with the character n-gram language model: every candidate gains lm_weight *
        log P_lm(token | its last order - 1 tokens), nothing is forbidden.  Every result also has "lm_logp", the language model's
        unweighted log-probability of its reading (CharLM.logp of its ids), and so has every entry of "alternatives"; "logp" and
        "confidence" stay the model's own numbers.  The default lm_weight of 0.5 is a placeholder, not a tuned value.
        suggest=Lexicon(...) with suggest_k (1..16) and suggest_max_distance (None = no bound) (keyword-only extension, any mode, not
        together with `lexicon`): every result also has "suggestions", a list of {"text", "lexicon_index", "distance"}: the
        suggest_k words of the lexicon nearest to "text" by Levenshtein distance, nearest first, ties by ascending index (DESIGN.md
        section 4.17).  Distance 0 means "text" is a lexicon word; an empty list means nothing lies within the bound.  The decode
        itself is untouched: every other field is what the same call without `suggest` returns.
        suggest_costs=EditCosts(...) (only with `suggest`, over the same charset): the suggestions are ranked by the
        confusion-weighted edit distance instead, what it costs to turn "text" into the word under the recogniser's own confusions
        (DESIGN.md section 4.26); "distance" and suggest_max_distance are then in cost units."""
        images_list = images if isinstance(images, list) else [images]
        if mode not in ("greedy", "beam"):
            raise ValueError(f"Unknown mode: {mode}")
        self._check_n_best(n_best, mode, beam_size)
        self._check_lexicon(lexicon, mode)
        self._check_lm(lm, lm_weight, mode, lexicon)
        self._check_suggest(suggest, suggest_k, suggest_max_distance, lexicon, mode, suggest_costs)
        if not images_list:
            return []
        arrays = [self._load_rgb(im) for im in images_list]
        canv = torch.from_numpy(self._canvases(arrays)).to(self.device, non_blocking=True)
        if not return_chars and not n_best and lexicon is None and lm is None and suggest is None:
            return self._results(*self.recognize_canvases(canv, batch_size, mode, beam_size, temperature, alpha))
        fin = self.recognize_canvases(canv, batch_size, mode, beam_size, temperature, alpha, char_details=return_chars, n_best=n_best,
                                      lexicon=lexicon, lm=lm, lm_weight=lm_weight, suggest=suggest, suggest_k=suggest_k,
                                      suggest_max_distance=suggest_max_distance, suggest_costs=suggest_costs)
        if suggest is not None:
            fin, sug = fin[:-2], suggest.suggestions(*fin[-2:])
        ids, trun, conf = fin[:3]
        results = self._results(ids, trun, conf)
        if lm is not None:
            for r, v in zip(results, self.lm_logps(ids, trun, lm)):
                r["lm_logp"] = v
        if lexicon is not None:
            for r, k in zip(results, self.lexicon_indices(ids, lexicon)):
                r["lexicon_index"] = k
        if return_chars:
            prob, centre = fin[3:5]
            src_w = [a.shape[1] for a in arrays]
            new_w = [resized_size(a.shape[0], a.shape[1], self.img_h, self.img_w)[0] for a in arrays]
            for r, ch in zip(results, self.chars(ids, trun, prob, centre, new_w, np.zeros(len(arrays)), src_w)):
                r["chars"] = ch
        if n_best:
            alt_ids, _alt_prob, alt_conf, alt_logp = fin[-4:]
            for r, al in zip(results, self._alternatives(alt_ids, trun, alt_conf, alt_logp, lexicon, lm)):
                r["alternatives"] = al
        if suggest is not None:
            for r, sg in zip(results, sug):
                r["suggestions"] = sg
        return results
