"""Recognition metrics over the package's own edit distance: the reference's definitions
(recognizers/_trba/training/metrics.py:6-33 of the project this one was modelled on) without its Levenshtein dependency.

  edit_distances(refs, hyps, stoi=None, device=None)  Levenshtein distance of every pair, as an int32 array
  character_error_rate(ref, hyp)                      distance / len(ref); an empty reference gives inf for a non-empty hypothesis, else 0
  accuracy(refs, hyps)                                 share of exact matches; 0 for no pairs

The distances come from msocr_edit_distance_pairs (device given) or its host twin (device None, no GPU needed): unit costs, strings
of at most 64 characters.

Running text (a page in reading order against its transcription), over msocr_edit_distance_long and its host
twin, sequences of at most 16384 tokens:

  sequence_edit_distances(refs, hyps, device=None)   distance of every pair of strings (characters) or lists (items), int32 array
  word_error_rate(ref, hyp)                           word distance / words of ref, words = str.split(); empty reference as for CER
  text_error_rates(refs, hyps, device=None)           per pair and pooled: character and word distances, CER, WER, bag-of-words errors

The word error rate here is this package's: words are str.split() of the strings as they are.  The reference takes WER from jiwer,
whose transforms cannot be pinned here, so the two need not agree on punctuation or case; for single-word crops WER equals 1 - accuracy.

The alignment behind those rates, over msocr_edit_alignment and its host twin:

  sequence_alignments(refs, hyps, device=None)       per pair an Alignment: counts of hits / substitutions / deletions / insertions
                                                      and the two index maps; the reference is always the pattern
  error_breakdown(refs, hyps, device=None)           pooled counts and a Counter of confusions {(ref token, hyp token): count}
  text_error_rates(..., breakdown=True)               the figures above plus counts, confusions and word alignments of both levels
"""
from collections import Counter
from typing import NamedTuple

import numpy as np

from ... import _native as nat

_MAX_LEN, _MAX_V = 64, 512
MAX_SEQUENCE_LEN = 16384  # msocr.h MSOCR_EDL_MAX_LEN


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


# ------------------------------------------------------------------------------------------------- running text
def _tokens(x):
    if isinstance(x, str):
        return x
    if isinstance(x, (list, tuple)):
        return x
    raise TypeError(f"a sequence is a str (its characters) or a list of hashable items, got {type(x).__name__}")


def _encode_pair(ref, hyp):
    """One pair as (pattern ids, text ids, v): the shorter side is the pattern (the distance is symmetric, and the pattern's side
    sizes the match-mask table); its distinct tokens are numbered 0 .. v - 1 in order of first occurrence, the other side's remaining
    tokens get ids >= v: equal tokens equal ids, none of which can match the pattern."""
    a, b = (hyp, ref) if len(hyp) < len(ref) else (ref, hyp)
    table = {}
    pat = [table.setdefault(t, len(table)) for t in a]
    v = len(table)
    txt = [table.setdefault(t, len(table)) for t in b]
    return pat, txt, v


def sequence_edit_distances(refs, hyps, device=None):
    """Levenshtein distance (unit costs) between refs[i] and hyps[i] -> int32 [N].  An item is a str (tokens = its characters) or a
    list / tuple of hashables (tokens = its items, compared by equality); at most 16384 tokens a side (ValueError above).
    device None: the host twin msocr_edit_distance_long_host (no GPU needed); a device: msocr_edit_distance_long there."""
    refs, hyps = [_tokens(r) for r in refs], [_tokens(h) for h in hyps]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references but {len(hyps)} hypotheses")
    N = len(refs)
    if N == 0:
        return np.zeros(0, dtype=np.int32)
    for s in refs + hyps:
        if len(s) > MAX_SEQUENCE_LEN:
            raise ValueError(f"a sequence of {len(s)} tokens; at most {MAX_SEQUENCE_LEN} are provided")
    from ... import ops
    pats, txts, v = [], [], np.empty(N, dtype=np.int32)
    for p, (r, h) in enumerate(zip(refs, hyps)):
        pat, txt, v[p] = _encode_pair(r, h)
        pats.append(pat)
        txts.append(txt)
    if max(sum(len(x) for x in pats), sum(len(x) for x in txts)) > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31 - 1 tokens in one call: split the batch")
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in pats])]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum([len(x) for x in txts])]).astype(np.int32)
    a_tok = np.fromiter((t for x in pats for t in x), dtype=np.int32, count=int(a_off[-1]))
    b_tok = np.fromiter((t for x in txts for t in x), dtype=np.int32, count=int(b_off[-1]))
    if device is None:
        return ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
    import torch
    dev = torch.device(device)
    with torch.cuda.device(dev):
        return ops.edit_distance_long(torch.from_numpy(a_tok).to(dev), a_off, torch.from_numpy(b_tok).to(dev), b_off, v).cpu().numpy()


def _rate(dist, length):
    """distance / length with the reference's empty-reference convention: inf for a non-empty hypothesis, else 0"""
    if length == 0:
        return float("inf") if dist > 0 else 0.0
    return dist / length


def word_error_rate(reference, hypothesis):
    """WER = Levenshtein distance over words / words of the reference; an empty reference: inf if the hypothesis has a word, else 0.
    Words are str.split() of the strings as they are: this package's tokenisation, not jiwer's (which the reference uses and whose
    transforms cannot be pinned here)."""
    r, h = reference.split(), hypothesis.split()
    return _rate(int(sequence_edit_distances([r], [h])[0]), len(r))


def text_error_rates(refs, hyps, device=None, breakdown=False):
    """Character and word error rates of running text: refs[i] a transcription, hyps[i] the text read, both str.  Both are
    whitespace-normalised first (" ".join(s.split())); words are str.split() (this package's tokenisation, not jiwer's).  Returns
      per pair (arrays [N]):  "char_dist", "ref_chars", "word_dist", "ref_words" (int), "cer", "wer" (float; an empty reference
                              gives inf for a non-empty hypothesis, else 0), and
                              "bag_errors" = max(|R|, |H|) - |R & H| over the word multisets: the word errors left when the order
                              is ignored, computed on the host.  bag_errors <= word_dist; the gap is what the reading order costs.
      pooled:                 "n", "cer_micro", "wer_micro" (summed distances / summed reference lengths, same convention),
                              "cer_mean", "wer_mean" (means of the per-pair rates; 0 for no pairs), "bag_error_rate" (summed
                              bag_errors / summed reference words).
    The 2 N distances are one call of sequence_edit_distances (device None: the host twin).
    breakdown=True adds what the distances are made of, and takes them and everything above from ONE call of the alignment
    (msocr_edit_alignment, reference = pattern; distance = substitutions + deletions + insertions, so no figure above changes):
      "char_counts", "word_counts"  int64 [N, 4]: hits, substitutions, deletions, insertions per pair
      "char_confusions", "word_confusions"  pooled Counters {(ref token, hyp token): count}, None for the missing side
      "word_alignments"  per pair the Alignment of the word lists (which transcription word belongs to which word read)."""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references but {len(hyps)} hypotheses")
    for s in refs + hyps:
        if not isinstance(s, str):
            raise TypeError(f"texts must be str, got {type(s).__name__}")
    N = len(refs)
    rw, hw = [r.split() for r in refs], [h.split() for h in hyps]
    rc, hc = [" ".join(w) for w in rw], [" ".join(w) for w in hw]
    if breakdown and N:
        dist, r2h, h2r, counts = _align(rc + rw, hc + hw, device)
        dist, counts = dist.astype(np.int64), counts.astype(np.int64)
    else:
        dist = sequence_edit_distances(rc + rw, hc + hw, device=device).astype(np.int64)
    char_dist, word_dist = dist[:N], dist[N:]
    ref_chars = np.array([len(s) for s in rc], dtype=np.int64)
    ref_words = np.array([len(w) for w in rw], dtype=np.int64)
    bag = np.array([max(len(r), len(h)) - sum((Counter(r) & Counter(h)).values()) for r, h in zip(rw, hw)], dtype=np.int64)
    cer = np.array([_rate(int(d), int(n)) for d, n in zip(char_dist, ref_chars)], dtype=np.float64)
    wer = np.array([_rate(int(d), int(n)) for d, n in zip(word_dist, ref_words)], dtype=np.float64)
    out = {
        "char_dist": char_dist, "ref_chars": ref_chars, "word_dist": word_dist, "ref_words": ref_words, "cer": cer, "wer": wer,
        "bag_errors": bag, "n": N,
        "cer_micro": _rate(int(char_dist.sum()), int(ref_chars.sum())), "wer_micro": _rate(int(word_dist.sum()), int(ref_words.sum())),
        "cer_mean": float(cer.mean()) if N else 0.0, "wer_mean": float(wer.mean()) if N else 0.0,
        "bag_error_rate": _rate(int(bag.sum()), int(ref_words.sum())),
    }
    if breakdown:
        out["char_counts"] = counts[:N] if N else np.zeros((0, 4), dtype=np.int64)
        out["word_counts"] = counts[N:] if N else np.zeros((0, 4), dtype=np.int64)
        out["char_confusions"], out["word_confusions"], out["word_alignments"] = Counter(), Counter(), []
        for p in range(N):
            out["char_confusions"].update(_confusions(rc[p], hc[p], r2h[p], h2r[p]))
            out["word_confusions"].update(_confusions(rw[p], hw[p], r2h[N + p], h2r[N + p]))
            out["word_alignments"].append(Alignment(int(dist[N + p]), *(int(c) for c in counts[N + p]), r2h[N + p], h2r[N + p]))
    return out


# ------------------------------------------------------------------------------------- the alignment behind the rates
class Alignment(NamedTuple):
    """One optimal alignment of a reference with a hypothesis (msocr_edit_alignment's tie rule, reference = pattern): walking back
    from the ends, a pair of equal tokens is a hit; else a substitution where that is optimal; else a deletion (a reference token
    dropped) where that is optimal; else an insertion (a hypothesis token added)."""
    distance: int
    hits: int
    substitutions: int
    deletions: int
    insertions: int
    ref_to_hyp: np.ndarray   # int32 [len(ref)]: the index of each reference token's partner in the hypothesis, or -1
    hyp_to_ref: np.ndarray   # int32 [len(hyp)]: the index of each hypothesis token's partner in the reference, or -1


def _align(refs, hyps, device):
    """(dist [N], ref maps, hyp maps, counts [N, 4]) of token-checked sequences; the maps as lists of int32 arrays"""
    N = len(refs)
    for s in refs + hyps:
        if len(s) > MAX_SEQUENCE_LEN:
            raise ValueError(f"a sequence of {len(s)} tokens; at most {MAX_SEQUENCE_LEN} are provided")
    if sum(len(x) for x in refs) > np.iinfo(np.int32).max or sum(len(x) for x in hyps) > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31 - 1 tokens in one call: split the batch")
    from ... import ops
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in refs])]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum([len(x) for x in hyps])]).astype(np.int32)
    a_tok, b_tok, v = np.empty(int(a_off[-1]), dtype=np.int32), np.empty(int(b_off[-1]), dtype=np.int32), np.empty(N, dtype=np.int32)
    for p, (r, h) in enumerate(zip(refs, hyps)):
        # the reference is the pattern whatever the lengths (the tie rule is not symmetric): its distinct tokens are 0 .. v - 1 in
        # order of first occurrence, the hypothesis's other tokens get ids >= v, which match nothing
        table = {}
        a_tok[a_off[p]:a_off[p + 1]] = [table.setdefault(t, len(table)) for t in r]
        v[p] = len(table)
        b_tok[b_off[p]:b_off[p + 1]] = [table.setdefault(t, len(table)) for t in h]
    if device is None:
        dist, a_map, b_map, counts = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    else:
        import torch
        dev = torch.device(device)
        with torch.cuda.device(dev):
            out = ops.edit_alignment(torch.from_numpy(a_tok).to(dev), a_off, torch.from_numpy(b_tok).to(dev), b_off, v)
            dist, a_map, b_map, counts = (t.cpu().numpy() for t in out)
    return (dist, [a_map[a_off[p]:a_off[p + 1]] for p in range(N)], [b_map[b_off[p]:b_off[p + 1]] for p in range(N)], counts)


def sequence_alignments(refs, hyps, device=None):
    """One optimal alignment of refs[i] with hyps[i] -> a list of Alignment.  Items as for sequence_edit_distances: a str (tokens =
    its characters) or a list / tuple of hashables, at most 16384 tokens a side (ValueError above).  The reference is always the
    pattern of msocr_edit_alignment, so the tie rule reads the same whatever the lengths.  device None: the host twin
    msocr_edit_alignment_host (no GPU needed); a device: msocr_edit_alignment there, bit for bit the same."""
    refs, hyps = [_tokens(r) for r in refs], [_tokens(h) for h in hyps]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references but {len(hyps)} hypotheses")
    if not refs:
        return []
    dist, r2h, h2r, counts = _align(refs, hyps, device)
    return [Alignment(int(d), *(int(c) for c in cnt), a, b) for d, cnt, a, b in zip(dist, counts, r2h, h2r)]


def _confusions(ref, hyp, ref_to_hyp, hyp_to_ref):
    """the errors of one aligned pair: (ref token, hyp token) of every substitution, (ref token, None) of every deletion,
    (None, hyp token) of every insertion; O(m + n) on the host"""
    c = Counter((r, hyp[k]) for r, k in zip(ref, ref_to_hyp.tolist()) if k >= 0 and r != hyp[k])
    c.update((r, None) for r, k in zip(ref, ref_to_hyp.tolist()) if k < 0)
    c.update((None, h) for h, k in zip(hyp, hyp_to_ref.tolist()) if k < 0)
    return c


def error_breakdown(refs, hyps, device=None):
    """What the distance between refs[i] and hyps[i] is made of, pooled over the pairs: {"hits", "substitutions", "deletions",
    "insertions" (int), "confusions": a Counter {(ref token, hyp token): count} over the errors, the missing side of a deletion or
    an insertion being None; hits are not listed}.  Items and device as for sequence_alignments, whose alignment this reads."""
    refs, hyps = [_tokens(r) for r in refs], [_tokens(h) for h in hyps]
    als = sequence_alignments(refs, hyps, device=device)
    conf = Counter()
    for r, h, al in zip(refs, hyps, als):
        conf.update(_confusions(r, h, al.ref_to_hyp, al.hyp_to_ref))
    return {"hits": sum(a.hits for a in als), "substitutions": sum(a.substitutions for a in als),
            "deletions": sum(a.deletions for a in als), "insertions": sum(a.insertions for a in als), "confusions": conf}
