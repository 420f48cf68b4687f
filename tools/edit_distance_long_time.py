"""Times the long-sequence edit distance (msocr_edit_distance_long) beside its host twin on the same arrays
(dev tool).
  python tools/edit_distance_long_time.py [--repeats N] [--pairs N] [--chars N] [--words N] [--out FILE]
Two batches, the two calls Pipeline.evaluate_text makes of one page each: 16 pairs of about 3 400 characters (an alphabet of 60) and
16 pairs of about 480 words (a vocabulary of 2 000); the hypothesis is the reference with a twentieth of its tokens replaced, a few
runs dropped and two stretches swapped.  Per round the two versions take turns: 20 device calls between two events, then one host
call on the host clock; one line per version with the median and the spread (max - min) over --repeats rounds (default 9), after two
warm-up rounds.  The device time is the whole entry point on tokens already on the device: the upload of the heads, which the call
waits for, and the three kernels.  The upload of the tokens and the read-back are timed separately.  The results of the two are
compared for equality before anything is timed.  The report goes to --out (default profiles/edit_distance_long.txt)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from manuscript_ocr_amd import ops
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--pairs", type=int, default=16)
ap.add_argument("--chars", type=int, default=3400)
ap.add_argument("--words", type=int, default=480)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_long.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"


def batch(seed, length, vocab):
    """(a_tok, a_off, b_tok, b_off, v) as sequence_edit_distances packs them: the shorter side is the pattern, its distinct tokens are
    0 .. v - 1 in order of first occurrence, the other side's remaining tokens lie behind them"""
    rng = np.random.default_rng(seed)
    pats, txts, v = [], [], []
    for _ in range(a.pairs):
        n = int(length * rng.uniform(0.9, 1.1))
        ref = rng.integers(0, vocab, n)
        hyp = ref.copy()
        hit = rng.random(n) < 0.05
        hyp[hit] = rng.integers(0, vocab + 20, int(hit.sum()))
        cut = sorted(int(c) for c in rng.integers(0, n - n // 8, 2))
        hyp = np.concatenate([hyp[:cut[0]], hyp[cut[1]:cut[1] + n // 8], hyp[cut[0]:cut[1]], hyp[cut[1] + n // 8:]])
        hyp = np.delete(hyp, np.arange(n // 3, n // 3 + n // 50))
        pat, txt = (hyp, ref) if len(hyp) < len(ref) else (ref, hyp)
        table = {}
        pats.append([table.setdefault(int(t), len(table)) for t in pat])
        v.append(len(table))
        txts.append([table.setdefault(int(t), len(table)) for t in txt])
    off = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)  # noqa: E731
    tok = lambda rows: np.array([t for r in rows for t in r], dtype=np.int32)  # noqa: E731
    return tok(pats), off(pats), tok(txts), off(txts), np.array(v, dtype=np.int32)


lines = []
CALLS = 20
for name, (a_tok, a_off, b_tok, b_off, v) in (("characters", batch(1, a.chars, 60)), ("words", batch(2, a.words, 2000))):
    need = ops.edit_distance_long_workspace_bytes(a_off, b_off, v)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    out = torch.empty((a.pairs,), dtype=torch.int32, device="cuda")
    ad, bd = torch.from_numpy(a_tok).cuda(), torch.from_numpy(b_tok).cuda()
    host = ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
    got = ops.edit_distance_long(ad, a_off, bd, b_off, v, workspace=ws, out=out).cpu().numpy()
    assert np.array_equal(got, host)
    m, n = np.diff(a_off), np.diff(b_off)
    lines.append(f"msocr_edit_distance_long vs msocr_edit_distance_long_host, {name}: {a.pairs} pairs, pattern {int(m.min())}..{int(m.max())} "
                 f"tokens, text {int(n.min())}..{int(n.max())} tokens, alphabets {int(v.min())}..{int(v.max())}, workspace {need} bytes; "
                 f"distances identical, {int(host.min())}..{int(host.max())}")
    ms = {"device call": [], "host twin": [], "upload + device call + read-back": []}
    for rep in range(a.repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            ops.edit_distance_long(ad, a_off, bd, b_off, v, workspace=ws, out=out)
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
        t1 = time.perf_counter()
        back = ops.edit_distance_long(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v, workspace=ws,
                                      out=out).cpu()
        t2 = time.perf_counter()
        if rep >= 2:  # two warm-up rounds
            ms["device call"].append(e0.elapsed_time(e1) / CALLS)
            ms["host twin"].append((t1 - t0) * 1e3)
            ms["upload + device call + read-back"].append((t2 - t1) * 1e3)
    for k, t in ms.items():
        lines.append(f"  {k}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
lines.append("one wave per pair: 16 pairs occupy 16 of the chip's waves and the time is that of the longest pair's step chain, not of the "
             "chip; the host twin runs the pairs one after the other on one core")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
