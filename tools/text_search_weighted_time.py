"""Times the confusion-weighted text search (msocr_text_search_weighted) beside the unit-cost search on the same
arrays and beside its host twin (dev tool).
  python tools/text_search_weighted_time.py [--repeats N] [--patterns N] [--texts N] [--chars N] [--host-texts N] [--out FILE]
Workload: that of tools/text_search_time.py: --patterns (1000) patterns of Poisson-8 length (at least 3) against --texts (1024) texts
of about --chars (3400) characters over a 60-symbol alphabet, every pattern planted in a few texts with 0, 1 or 2 random edits; and the
small case that fixes the crossover for Pipeline.search: 10 patterns against 16 texts.  Costs: random tables over 60 classes, sub 1..8,
delete and insert 2..8, unknown 8, every token with a class; the bound is 8 cost units for every pattern (one dear edit, or several
cheap ones), the unit search beside it runs with k = 1.
Before anything is timed the device's hits in the first --host-texts (64) texts, sorted into canonical order, are compared with the
host twin's on those texts (the small case is compared whole).  Per round the versions take turns; one line each with the median and
the spread (max - min) over --repeats rounds (default 7), after two warm-up rounds:
  (a) the weighted device call on a resident corpus, hits left on the device: device events around 3 calls of
      ops.text_search_weighted_into with room for every hit (the upload of the offsets, which the call waits for, and the two kernels)
  (u) the same for the unit-cost ops.text_search_into on the same arrays with k = 1
  (b) patterns up, ops.text_search_weighted (its two passes where the first 65536 records do not hold the hits), hits read back
  (c) as (b) with the upload of the corpus and of the class map in front
  (d) the host twin on the first --host-texts texts, host clock, and that time scaled to all texts (said to be scaled)
The report goes to --out (default profiles/text_search_weighted.txt)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from manuscript_ocr_amd import ops
from manuscript_ocr_amd.recognizers import EditCosts
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--patterns", type=int, default=1000)
ap.add_argument("--texts", type=int, default=1024)
ap.add_argument("--chars", type=int, default=3400)
ap.add_argument("--host-texts", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_search_weighted.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
V = 60
CALLS = 3
BOUND = 8


def workload(seed, Q, T, chars):
    """(pat_tok, pat_off, m, txt_tok, txt_off): tools/text_search_time.py's"""
    rng = np.random.default_rng(seed)
    m = np.maximum(rng.poisson(8, Q), 3)
    pats = [rng.integers(0, V, int(k)) for k in m]
    texts = [rng.integers(0, V, int(chars * rng.uniform(0.9, 1.1))) for _ in range(T)]
    for q, p in enumerate(pats):
        for edits in range(3):
            c = p.tolist()
            for _ in range(edits):
                op, at = int(rng.integers(0, 3)), int(rng.integers(0, len(c)))
                if op == 0:
                    c[at] = int(rng.integers(0, V))
                elif op == 1:
                    c.insert(at, int(rng.integers(0, V)))
                elif len(c) > 1:
                    del c[at]
            t = int(rng.integers(0, T))
            at = int(rng.integers(0, len(texts[t]) - len(c)))
            texts[t][at:at + len(c)] = c
    off = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)  # noqa: E731
    tok = lambda rows: np.concatenate(rows).astype(np.int32)  # noqa: E731
    return tok(pats), off(pats), m.astype(np.int32), tok(texts), off(texts)


def canonical(h):
    return h[np.lexsort((h[:, 3], h[:, 1], h[:, 0]))] if len(h) else h


rng = np.random.default_rng(7)
sub = rng.integers(1, 9, (V, V))
np.fill_diagonal(sub, 0)
costs = EditCosts(sub, rng.integers(2, 9, V), rng.integers(2, 9, V), [f"<{k}>" for k in range(V)], unknown=8)
cls = np.arange(V, dtype=np.int32)
lines = []
for name, Q, T, host_texts in (("1000 x 1024", a.patterns, a.texts, a.host_texts), ("10 x 16", 10, 16, 16)):
    pat_tok, pat_off, m, txt_tok, txt_off = workload(1 if Q == a.patterns else 2, Q, T, a.chars)
    host_texts = min(host_texts, T)
    ks, ku = np.full(Q, BOUND, dtype=np.int32), np.ones(Q, dtype=np.int32)
    pd, td, cd = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda(), torch.from_numpy(cls).cuda()
    got = ops.text_search_weighted(pd, pat_off, ks, td, txt_off, V, cd, costs)
    part_off = txt_off[:host_texts + 1]
    want, _ = ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, part_off, V, cls, costs)
    assert np.array_equal(canonical(got[got[:, 1] < host_texts]), want), "the two routes differ"
    n, nu = len(got), len(ops.text_search(pd, pat_off, ku, td, txt_off, V))
    ws = torch.empty((max(ops.text_search_weighted_workspace_bytes(pat_off, ks, txt_off, V, costs), 8),), dtype=torch.uint8, device="cuda")
    wsu = torch.empty((max(ops.text_search_workspace_bytes(pat_off, ku, txt_off, V), 8),), dtype=torch.uint8, device="cuda")
    hits = torch.empty((max(n, nu, 1), 5), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    steps = int(len(txt_tok)) * Q
    lines.append(f"msocr_text_search_weighted, {name}: {Q} patterns of {int(m.min())}..{int(m.max())} tokens (mean {float(m.mean()):.1f}), "
                 f"bound {BOUND} cost units, {T} texts, {len(txt_tok)} tokens, alphabet {V}, {steps:.3e} pattern-column steps; {n} hits "
                 f"({len(ops.text_search_select(got))} after selection; the unit search with k = 1: {nu}); hits of the first {host_texts} "
                 f"texts identical on both routes ({len(want)})")
    ms = {"(a) weighted device call, corpus resident, hits left on the device": [],
          "(u) unit-cost device call on the same arrays, k = 1": [],
          "(b) patterns up + ops.text_search_weighted + hits read back, corpus resident": [],
          "(c) corpus and class map up + (b)": [],
          f"(d) host twin, first {host_texts} of {T} texts": []}
    keys = list(ms)
    for rep in range(a.repeats + 2):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for _ in range(CALLS):
            ops.text_search_weighted_into(pd, pat_off, ks, td, txt_off, V, cd, costs, hits, cnt, workspace=ws)
        e1.record()
        for _ in range(CALLS):
            ops.text_search_into(pd, pat_off, ku, td, txt_off, V, hits, cnt, workspace=wsu)
        e2.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = ops.text_search_weighted(torch.from_numpy(pat_tok).cuda(), pat_off, ks, td, txt_off, V, cd, costs)
        t1 = time.perf_counter()
        back = ops.text_search_weighted(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, V,
                                        torch.from_numpy(cls).cuda(), costs)
        t2 = time.perf_counter()
        ops.text_search_weighted_host(pat_tok, pat_off, ks, txt_tok, part_off, V, cls, costs)
        t3 = time.perf_counter()
        assert len(back) == n
        if rep >= 2:  # two warm-up rounds
            for key, t in zip(keys, (e0.elapsed_time(e1) / CALLS, e1.elapsed_time(e2) / CALLS, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)):
                ms[key].append(t)
    for key, t in ms.items():
        lines.append(f"  {key}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
    if host_texts < T:
        frac = int(part_off[-1]) / len(txt_tok)
        lines.append(f"  (d) SCALED to all {T} texts by tokens (x {1 / frac:.2f}; not run): {statistics.median(ms[keys[4]]) / frac:.0f} ms")
    med, medu = statistics.median(ms[keys[0]]), statistics.median(ms[keys[1]])
    lines.append(f"  (a) per pattern-column step: {med * 1e6 / steps * 1e3:.3f} ps; {steps / med / 1e6:.1f} G steps/s; (a) / (u) = {med / medu:.1f}")
lines.append("the host twin runs the patterns and texts one after the other on one core; the device cuts every text into segments of "
             f"{ops.SEARCH_SEGMENT} tokens, one lane per (pattern, segment), its column of up to 64 cells in registers")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
