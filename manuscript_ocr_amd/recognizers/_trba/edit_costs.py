"""EditCosts: per-symbol edit costs for the nearest-word lookup.

The tables price turning a RECOGNISED row into a LEXICON word: sub[a, b] is what it costs to read the recognised symbol a as the lexicon
symbol b (not symmetric), delete[a] to drop a recognised symbol the recogniser added, insert[b] to supply a lexicon symbol it dropped.
A confusion counted by `error_breakdown` is keyed (reference, hypothesis) — true r read as h — and therefore lands in sub[h, r]: the
lookup starts from what was read.  `Lexicon.nearest(..., costs=...)`, `TRBA.predict(..., suggest_costs=...)` and
`pipeline.suggest_costs` take an EditCosts; msocr_lexicon_nearest_weighted and its host twin do the arithmetic, in exact integers.
"""
import ctypes
import math

import numpy as np

from ... import _native as nat

_SPECIAL = ("<PAD>", "<SOS>", "<EOS>", "<BLANK>")


def _stoi(charset):
    return charset if isinstance(charset, dict) else {s: i for i, s in enumerate(charset)}


class EditCosts:
    """EditCosts(sub, delete, insert, charset, unknown=None)

    sub [V, V], delete [V], insert [V]: uint8 arrays over the ids of `charset` (a recogniser's `stoi` dict or `itos` list, V = the largest
    id + 1, at most 512).  The diagonal of sub is 0; every other entry of the three is 1..255, so that distance 0 still means "the row
    is in the lexicon".  unknown (1..255, default the largest cost in the tables): any edit that involves a symbol outside the charset.
    msocr_edit_costs_check_host validates the tables once; a violation is a ValueError."""

    def __init__(self, sub, delete, insert, charset, unknown=None):
        self.stoi = dict(_stoi(charset))  # symbol -> class: TextCorpus.search maps the corpus characters through it
        self.num_classes = max(self.stoi.values()) + 1
        V = self.num_classes
        arrays = []
        for name, a, shape in (("sub", sub, (V, V)), ("delete", delete, (V,)), ("insert", insert, (V,))):
            a = np.asarray(a)
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape} for a charset of {V} tokens, got {a.shape}")
            if a.dtype != np.uint8:
                if not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
                    raise ValueError(f"{name} must hold integers in 0..255")
            arrays.append(np.ascontiguousarray(a, dtype=np.uint8))
        self.sub, self.delete, self.insert = arrays
        self.unknown = int(max(self.sub.max(), self.delete.max(), self.insert.max())) if unknown is None else int(unknown)
        self.min_ins, self.min_del = int(self.insert.min()), int(self.delete.min())
        rc = nat.lib().msocr_edit_costs_check_host(self.sub.ctypes.data, self.delete.ctypes.data, self.insert.ctypes.data, V, self.unknown,
                                                   self.min_ins, self.min_del)
        if rc != 0:
            why = [w for bad, w in ((V > 512, f"the charset has {V} tokens, at most 512 are taken"),
                                    (bool(np.diagonal(self.sub).any()), "the diagonal of sub must be 0"),
                                    (bool((self.sub + np.eye(V, dtype=np.uint8) == 0).any()), "an off-diagonal entry of sub is 0"),
                                    (bool((self.delete == 0).any()), "an entry of delete is 0"),
                                    (bool((self.insert == 0).any()), "an entry of insert is 0"),
                                    (not 1 <= self.unknown <= 255, f"unknown = {self.unknown} is outside 1..255")) if bad]
            raise ValueError("msocr_edit_costs_check_host refused the tables: " + ("; ".join(why) or f"code {rc}"))
        self._device = {}

    def to(self, device):
        """The three tables on `device` and the msocr_edit_costs struct that points at them, cached per device: (sub, delete, insert,
        struct).  device None: the host arrays themselves (for the host twin)."""
        if device is None:
            key = None
        else:
            import torch
            key = torch.device(device)
            if key.type == "cuda" and key.index is None:
                key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._device:
            ec = nat.EditCostsTable()
            if key is None:
                ts = (self.sub, self.delete, self.insert)
                ec.sub, ec.del_, ec.ins = (a.ctypes.data for a in ts)
            else:
                import torch
                ts = tuple(torch.from_numpy(a).to(key) for a in (self.sub, self.delete, self.insert))
                ec.sub, ec.del_, ec.ins = (t.data_ptr() for t in ts)
            ec.V, ec.unknown, ec.min_ins, ec.min_del = self.num_classes, self.unknown, self.min_ins, self.min_del
            self._device[key] = ts + (ec,)
        return self._device[key]

    def struct(self, device):
        return ctypes.pointer(self.to(device)[3])

    @classmethod
    def uniform(cls, charset, cost=1):
        """Every substitution, deletion and insertion at `cost` (1..255), `unknown` too: cost 1 is the unit-cost Levenshtein distance."""
        V = max(_stoi(charset).values()) + 1
        sub = np.full((V, V), int(cost), dtype=np.int64)
        np.fill_diagonal(sub, 0)
        return cls(sub, np.full(V, int(cost), dtype=np.int64), np.full(V, int(cost), dtype=np.int64), charset, unknown=int(cost))

    @classmethod
    def from_confusions(cls, confusions, ref_counts, charset, unit=32, floor=1e-4):
        """Costs from a recogniser's counted errors: `confusions` is the Counter of `error_breakdown` / `evaluate_text(breakdown=True)`,
        {(r, h): c} = true r read as h, c times, with (r, None) a deletion and (None, h) an insertion; `ref_counts` {r: how often r
        occurs in the references}.  Relative frequencies and where they go (recognised -> lexicon, so the key is turned round):
          substitution (r, h): p = c / ref_counts[r]        -> sub[h, r]
          deletion (r, None):  p = c / ref_counts[r]        -> insert[r]   (the lookup has to supply r)
          insertion (None, h): p = c / sum of ref_counts    -> delete[h]   (the lookup has to drop h)
        cost = clamp(round(unit * ln p / ln floor), 1, unit): an edit seen with frequency `floor` or less costs `unit`, one seen every
        time costs 1; nothing observed, or p = 0, costs `unit`; `unknown` = unit.  Tokens outside the charset and the special tokens
        (<PAD>, <SOS>, <EOS>, <BLANK>) are ignored.  unit = 32 and floor = 1e-4 are placeholders, not tuned values: no trained
        checkpoint was at hand to tune them on."""
        stoi = _stoi(charset)
        unit = int(unit)
        if not 1 <= unit <= 255:
            raise ValueError(f"unit must be between 1 and 255, got {unit}")
        if not 0.0 < float(floor) < 1.0:
            raise ValueError(f"floor must lie strictly between 0 and 1, got {floor}")
        V = max(stoi.values()) + 1
        sub = np.full((V, V), unit, dtype=np.int64)
        np.fill_diagonal(sub, 0)
        delete, insert = np.full(V, unit, dtype=np.int64), np.full(V, unit, dtype=np.int64)
        known = lambda t: t in stoi and t not in _SPECIAL
        total = sum(int(n) for t, n in ref_counts.items() if known(t))

        def cost(c, n):
            p = c / n if n > 0 else 0.0
            if p <= 0.0:
                return unit
            return min(max(int(round(unit * math.log(min(p, 1.0)) / math.log(float(floor)))), 1), unit)

        for (r, h), c in confusions.items():
            if r is not None and not known(r) or h is not None and not known(h) or (r is None and h is None):
                continue
            if r is None:
                delete[stoi[h]] = cost(c, total)
            elif h is None:
                insert[stoi[r]] = cost(c, int(ref_counts.get(r, 0)))
            elif r != h:
                sub[stoi[h], stoi[r]] = cost(c, int(ref_counts.get(r, 0)))
        return cls(sub, delete, insert, charset, unknown=unit)

    @classmethod
    def from_pairs(cls, refs, hyps, charset, unit=32, floor=1e-4, device=None):
        """`from_confusions` on the character confusions of `error_breakdown(refs, hyps)` (strings: reference, what was read), the
        reference tokens counted here.  device: where `error_breakdown` aligns the pairs (None = its host twin, no GPU needed)."""
        from collections import Counter

        from .metrics import error_breakdown
        refs, hyps = list(refs), list(hyps)
        counts = Counter(ch for r in refs for ch in r)
        return cls.from_confusions(error_breakdown(refs, hyps, device=device)["confusions"], counts, charset, unit=unit, floor=floor)
