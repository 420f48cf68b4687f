"""CharLM: a character n-gram language model the beam decode is fused with (shallow fusion).

The model is a dense f32 table [V^(order - 1), V] of natural-log probabilities, order 1..3: row ctx is the context made of the last
order - 1 tokens of a hypothesis, the most recent one least significant; positions before the start of the word count as <SOS>.  The
kernels (csrc/attn_general_lm.hip, csrc/attn_lm_mfma.hip) add lm_weight * table[ctx][token] to every candidate of a live hypothesis
and carry ctx per beam slot; `walk` and `logp` are their host twins.  `from_texts` trains the table from transcribed text alone
(interpolated Witten-Bell smoothing, float64); a table from elsewhere goes through the constructor.
"""
import ctypes

import numpy as np

from ... import _native as nat
from .transforms import encode_text

MAX_ELEMS = 1 << 26  # n_ctx * V, the C ABI's cap (256 MiB of f32): every index fits 32 bits


def _n_ctx(num_classes, order):
    if not isinstance(order, (int, np.integer)) or not 1 <= order <= 3:
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    V = int(num_classes)
    if V < 1:
        raise ValueError(f"num_classes must be positive, got {num_classes!r}")
    n = V ** (int(order) - 1)
    if n * V > MAX_ELEMS:
        raise ValueError(f"a table of order {order} over {V} tokens has {n * V} elements, more than the cap of 2^26; use a lower order")
    return n


class CharLM:
    """CharLM(table, num_classes, order, sos_id, eos_id=None)

    table: array-like [num_classes^(order - 1), num_classes] of natural-log probabilities, all finite (put a large negative number,
    not -inf, where a token cannot follow: the decode's arithmetic and its weight-0 identity rely on finite values); kept as a
    C-contiguous float32 array.  order 1..3; num_classes^order <= 2^26.  sos_id: the token that stands for the positions before the
    start of a word.  `eos_id` (None by default; `from_texts` sets it): where `walk` and `logp` stop, as the decode does."""

    def __init__(self, table, num_classes, order, sos_id, eos_id=None):
        n = _n_ctx(num_classes, order)  # before the table is touched: an oversized request is refused without allocating it
        self.num_classes, self.order = int(num_classes), int(order)
        self.n_ctx = n
        if not 0 <= int(sos_id) < self.num_classes:
            raise ValueError(f"sos_id {sos_id} is outside [0, {self.num_classes})")
        self.sos_id = int(sos_id)
        self.eos_id = None if eos_id is None else int(eos_id)
        t = np.asarray(table)
        if t.shape != (n, self.num_classes):
            raise ValueError(f"the table of an order-{order} model over {self.num_classes} tokens has shape ({n}, {self.num_classes}), "
                             f"got {t.shape}")
        if not np.isfinite(t).all():
            raise ValueError("the table holds non-finite values; use a finite floor (such as -30) instead of -inf")
        with np.errstate(over="ignore"):
            self.table = np.ascontiguousarray(t, dtype=np.float32)
        if not np.isfinite(self.table).all():
            raise ValueError("the table holds values outside the float32 range")
        self.ctx0 = 0
        for _ in range(self.order - 1):
            self.ctx0 = self.ctx0 * self.num_classes + self.sos_id
        self._device = {}

    @classmethod
    def from_table(cls, table, stoi, order):
        """The constructor with num_classes, sos_id and eos_id read from the recogniser's token table (TRBA.stoi)."""
        return cls(table, max(stoi.values()) + 1, order, stoi["<SOS>"], stoi["<EOS>"])

    @classmethod
    def from_texts(cls, texts, stoi, order=3, *, strict=True, floor_logp=-30.0):
        """Train from transcribed text: `texts` is an iterable of str (words or lines as the recogniser is to read them), `stoi` the
        recogniser's token table (TRBA.stoi, or its itos list).  Every text is encoded by transforms.encode_text (the character rule
        of pack_targets and Lexicon); strict=True raises ValueError naming the text and the character it cannot encode, strict=False
        drops such characters.  A training sequence is SOS^(order - 1), the ids, EOS.
        Smoothing: interpolated Witten-Bell in float64, backed off level by level down to the uniform distribution over the
        emittable tokens (the charset without <PAD>, <SOS> and <BLANK>):
            P_n(v | h) = (c(h, v) + T(h) * P_{n-1}(v | h')) / (c(h) + T(h)),   T(h) = distinct tokens seen after h,
        and P_n = P_{n-1} where c(h) = 0.  The non-emittable columns hold floor_logp (finite) in every row.  The result also keeps
        `prob64`, the float64 probabilities the table is the logarithm of."""
        stoi = stoi if isinstance(stoi, dict) else {s: i for i, s in enumerate(stoi)}
        for name in ("<PAD>", "<SOS>", "<EOS>"):
            if name not in stoi:
                raise ValueError(f"the charset has no {name} token")
        if not np.isfinite(floor_logp):
            raise ValueError(f"floor_logp must be finite, got {floor_logp!r}")
        V = max(stoi.values()) + 1
        _n_ctx(V, order)
        sos, eos = stoi["<SOS>"], stoi["<EOS>"]
        dead = sorted({stoi["<PAD>"], sos} | ({stoi["<BLANK>"]} if "<BLANK>" in stoi else set()))
        emit = np.ones(V, dtype=bool)
        emit[dead] = False
        # counts[k]: [V^k, V] f64, how often token v followed the context of its k last tokens
        counts = [np.zeros((V ** k, V), dtype=np.float64) for k in range(order)]
        for i, s in enumerate(texts):
            if not isinstance(s, str):
                raise TypeError(f"texts[{i}] must be a str, got {type(s).__name__}")
            ids, _kept, rejected = encode_text(s, stoi)
            if strict and rejected:
                raise ValueError(f"texts[{i}] = {s!r}: character {rejected[0][0]!r} is {rejected[0][1]}")
            seq = [sos] * (order - 1) + ids + [eos]
            for p in range(order - 1, len(seq)):
                ctx = 0
                for k in range(order):  # context of the k last tokens, most recent least significant
                    if k:
                        ctx += seq[p - k] * V ** (k - 1)
                    counts[k][ctx, seq[p]] += 1.0
        prob = np.where(emit, 1.0 / emit.sum(), 0.0)[None, :]  # level -1: uniform over the emittable tokens
        for k in range(order):
            c = counts[k]
            tot = c.sum(axis=1, keepdims=True)
            distinct = (c > 0).sum(axis=1, keepdims=True).astype(np.float64)
            # the back-off row of context h = (t_-k .. t_-1) drops its oldest token t_-k, the most significant digit
            lower = prob if k == 0 else prob[np.arange(V ** k) % prob.shape[0]]
            with np.errstate(invalid="ignore", divide="ignore"):
                p = (c + distinct * lower) / (tot + distinct)
            prob = np.where(tot > 0, p, lower)
        with np.errstate(divide="ignore"):
            table = np.log(prob)
        table[:, ~emit] = floor_logp
        if not np.isfinite(table).all():  # an emittable token the uniform floor gives mass can only be 0 by underflow
            raise ValueError("the smoothed table is not finite")
        lm = cls(table, V, order, sos, eos)
        lm.prob64 = prob  # the float64 probabilities before the logarithm and the cast (rows sum to 1 over the emittable tokens)
        return lm

    def walk(self, ids):
        """The context after every token of `ids` (a list of len(ids) ints), from the all-SOS start: the host twin of the kernels'
        ctx_out along one hypothesis.  With an eos_id, the context stays what it was from the first EOS on (the `ended` rule)."""
        V, ctx, out, ended = self.num_classes, self.ctx0, [], False
        for t in ids:
            t = int(t)
            if not 0 <= t < V:
                raise ValueError(f"token {t} is outside [0, {V})")
            ended = ended or (self.eos_id is not None and t == self.eos_id)
            if not ended:
                ctx = (ctx * V + t) % self.n_ctx
            out.append(ctx)
        return out

    def logp(self, ids):
        """The float64 sum of table[ctx][id] along `ids`, up to and including the first EOS (all of `ids` without an eos_id or an EOS;
        a negative id, the PAD of a finalized row, also ends it): the unweighted LM log-probability of a reading, a Python float."""
        V, ctx, total = self.num_classes, self.ctx0, 0.0
        for t in ids:
            t = int(t)
            if t < 0:
                break
            if t >= V:
                raise ValueError(f"token {t} is outside [0, {V})")
            total += float(self.table[ctx, t])
            if self.eos_id is not None and t == self.eos_id:
                break
            ctx = (ctx * V + t) % self.n_ctx
        return total

    def to(self, device):
        """(table tensor on `device`, the msocr_charlm struct that points at it), cached per device."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            t = torch.from_numpy(self.table).to(dev)
            st = nat.CharLMTable()
            st.table, st.order, st.V, st.n_ctx = t.data_ptr(), self.order, self.num_classes, self.n_ctx
            self._device[dev] = (t, st)
        return self._device[dev]

    def struct(self, device):
        return ctypes.pointer(self.to(device)[1])  # what the field AttnDesc.lm takes
