"""Recognition metrics over the package's own edit distance: the reference's definitions
(recognizers/_trba/training/metrics.py:6-33 of the project this one was modelled on) without its Levenshtein dependency.

  edit_distances(refs, hyps, stoi=None, device=None)  Levenshtein distance of every pair, as an int32 array
  character_error_rate(ref, hyp)                      distance / len(ref); an empty reference gives inf for a non-empty hypothesis, else 0
  accuracy(refs, hyps)                                 share of exact matches; 0 for no pairs

The distances come from msocr_edit_distance_pairs (device given) or its host twin (device None, no GPU needed): unit costs, strings
of at most 64 characters.  Word error rate is not provided: the reference takes it from jiwer, whose tokenisation rules cannot be pinned
here; for single-word crops it equals 1 - accuracy.
"""
import numpy as np

from ... import _native as nat

_MAX_LEN, _MAX_V = 64, 512


def _encode(refs, hyps, stoi):
    """Both lists as id rows over one alphabet: the charset's ids where it has the character, fresh ids behind it for every other
    character met (equal characters must compare equal whether the charset knows them or not).  PAD and EOS are two ids no character
    has; rows are EOS-filled."""
    table = {} if stoi is None else {ch: i for ch, i in stoi.items() if len(ch) == 1}
    nxt = (max(stoi.values()) + 1) if stoi else 0
    rows = []
    for s in list(refs) + list(hyps):
        if not isinstance(s, str):
            raise TypeError(f"texts must be str, got {type(s).__name__}")
        if len(s) > _MAX_LEN:
            raise ValueError(f"text {s!r}: {len(s)} characters, at most {_MAX_LEN} are provided")
        row = []
        for ch in s:
            i = table.get(ch)
            if i is None:
                i = table[ch] = nxt
                nxt += 1
            row.append(i)
        rows.append(row)
    pad_id, eos_id = nxt, nxt + 1
    V = nxt + 2
    if V > _MAX_V:
        raise ValueError(f"{V} distinct symbols; the distance kernel takes alphabets of at most {_MAX_V}")
    ids = np.full((len(rows), _MAX_LEN), eos_id, dtype=np.int32)
    for r, row in enumerate(rows):
        ids[r, :len(row)] = row
    return ids, np.array([len(r) for r in rows], dtype=np.int32), V, eos_id, pad_id


def edit_distances(refs, hyps, stoi=None, device=None):
    """Levenshtein distance (unit costs) between refs[i] and hyps[i] -> int32 [N].  stoi: a recogniser's charset (TRBA.stoi), used
    for the ids of the characters it has; characters outside it still compare by equality.  device None: the host twin."""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references but {len(hyps)} hypotheses")
    N = len(refs)
    if N == 0:
        return np.zeros(0, dtype=np.int32)
    ids, lens, V, eos_id, pad_id = _encode(refs, hyps, stoi)
    a, b, la, lb = ids[:N], ids[N:], lens[:N], lens[N:]
    if device is None:
        a, b, la, lb = (np.ascontiguousarray(v) for v in (a, b, la, lb))
        out = [np.empty(N, dtype=np.int32) for _ in range(3)]
        nat.check(nat.lib().msocr_edit_distance_pairs_host(a.ctypes.data, la.ctypes.data, _MAX_LEN, b.ctypes.data, lb.ctypes.data,
                                                           _MAX_LEN, N, V, eos_id, pad_id, -1, *(o.ctypes.data for o in out)),
                  "edit_distance_pairs_host")
        return out[0]
    import torch
    from ... import ops
    dev = torch.device(device)
    with torch.cuda.device(dev):
        a, b, la, lb = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (a, b, la, lb))
        out = [torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(3)]
        nat.check(nat.lib().msocr_edit_distance_pairs(a.data_ptr(), la.data_ptr(), _MAX_LEN, b.data_ptr(), lb.data_ptr(), _MAX_LEN, N, V,
                                                      eos_id, pad_id, -1, *(o.data_ptr() for o in out), ops._stream()),
                  "edit_distance_pairs")
        return out[0].cpu().numpy()


def character_error_rate(reference, hypothesis):
    """CER = Levenshtein(reference, hypothesis) / len(reference); an empty reference: inf if the hypothesis is not empty, else 0."""
    if len(reference) == 0:
        return float("inf") if len(hypothesis) > 0 else 0.0
    return int(edit_distances([reference], [hypothesis])[0]) / len(reference)


def accuracy(references, hypotheses):
    """Share of exact matches (prediction == reference); 0 for no pairs."""
    references = list(references)
    if not references:
        return 0.0
    return sum(1 for r, h in zip(references, hypotheses) if r == h) / len(references)
