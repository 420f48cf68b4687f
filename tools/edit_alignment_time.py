"""Times the alignment behind the error rates (msocr_edit_alignment) beside the distance kernel it extends
and beside its host twin, on the arrays of tools/edit_distance_long_time.py (dev tool).
  python tools/edit_alignment_time.py [--repeats N] [--pairs N] [--chars N] [--words N] [--no-kernels] [--out FILE]
Two batches, one page each as Pipeline.evaluate_text(breakdown=True) sends them: 16 pairs of about 3 400 characters (an alphabet of
60) and 16 pairs of about 480 words (a vocabulary of 2 000); the hypothesis is the reference with a twentieth of its tokens
replaced, a few runs dropped and two stretches swapped.  The reference is the pattern, as recognizers.sequence_alignments packs it.
Per round the versions take turns: 20 calls of msocr_edit_alignment between two events, 20 calls of msocr_edit_distance_long on the
same arrays between two events (the difference is the price of the trace stores and the traceback), then one host-twin call on the
host clock, then upload + call + read-back of all four arrays on the host clock; one line per version with the median and the
spread (max - min) over --repeats rounds (default 9), after two warm-up rounds.  The results of the two routes are compared for
equality before anything is timed.
The sweep and the traceback separately: kernel times of a run of its own under `rocprofv3 --kernel-trace --stats` (this script
starts itself once more as `--child NAME` behind rocprofv3, 23 calls a batch, the mean over all of them; --no-kernels leaves that
out).
The report goes to --out (default profiles/edit_alignment.txt)."""
import argparse, csv, glob, os, statistics, subprocess, sys, tempfile, time
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
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--child", default=None, help="internal: run the calls of one batch and exit (behind rocprofv3)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_alignment.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
CALLS = 20


def batch(seed, length, vocab):
    """(a_tok, a_off, b_tok, b_off, v): the pages of edit_distance_long_time.py with the reference as the pattern, its distinct
    tokens 0 .. v - 1 in order of first occurrence, the hypothesis's remaining tokens behind them"""
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
        table = {}
        pats.append([table.setdefault(int(t), len(table)) for t in ref])
        v.append(len(table))
        txts.append([table.setdefault(int(t), len(table)) for t in hyp])
    off = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)  # noqa: E731
    tok = lambda rows: np.array([t for r in rows for t in r], dtype=np.int32)  # noqa: E731
    return tok(pats), off(pats), tok(txts), off(txts), np.array(v, dtype=np.int32)


BATCHES = {"characters": lambda: batch(1, a.chars, 60), "words": lambda: batch(2, a.words, 2000)}


def buffers(a_tok, a_off, b_tok, b_off, v):
    ws = torch.empty((ops.edit_alignment_workspace_bytes(a_off, b_off, v),), dtype=torch.uint8, device="cuda")
    out = (torch.empty((a.pairs,), dtype=torch.int32, device="cuda"), torch.empty((len(a_tok),), dtype=torch.int32, device="cuda"),
           torch.empty((len(b_tok),), dtype=torch.int32, device="cuda"), torch.empty((a.pairs, 4), dtype=torch.int32, device="cuda"))
    return ws, out


if a.child is not None:
    a_tok, a_off, b_tok, b_off, v = BATCHES[a.child]()
    ws, out = buffers(a_tok, a_off, b_tok, b_off, v)
    ad, bd = torch.from_numpy(a_tok).cuda(), torch.from_numpy(b_tok).cuda()
    for _ in range(3 + CALLS):
        ops.edit_alignment(ad, a_off, bd, b_off, v, workspace=ws, out=out)
    torch.cuda.synchronize()
    sys.exit(0)


def kernel_times(name):
    """{kernel: mean microseconds} of the alignment's kernels for one batch, from a rocprofv3 run of its own; {} if that fails"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--pairs", str(a.pairs), "--chars", str(a.chars), "--words", str(a.words)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.TimeoutExpired) as e:
            print(f"rocprofv3 did not run: {e}")
            return {}
        if r.returncode != 0:
            print(f"rocprofv3 failed ({r.returncode}): {r.stderr[-500:]}")
            return {}
        res = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for key in ("eal_sweep_kernel", "eal_traceback_kernel", "edl_zero_kernel", "edl_masks_kernel"):
                        if key in row.get("Name", ""):
                            res[key] = (float(row["TotalDurationNs"]) / max(int(row["Calls"]), 1) / 1e3, int(row["Calls"]))
        return res


lines = []
for name, make in BATCHES.items():
    a_tok, a_off, b_tok, b_off, v = make()
    ws, out = buffers(a_tok, a_off, b_tok, b_off, v)
    dist_ws = torch.empty((max(ops.edit_distance_long_workspace_bytes(a_off, b_off, v), 8),), dtype=torch.uint8, device="cuda")
    dist_out = torch.empty((a.pairs,), dtype=torch.int32, device="cuda")
    ad, bd = torch.from_numpy(a_tok).cuda(), torch.from_numpy(b_tok).cuda()
    host = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    got = [t.cpu().numpy() for t in ops.edit_alignment(ad, a_off, bd, b_off, v, workspace=ws, out=out)]
    assert all(np.array_equal(g, h) for g, h in zip(got, host))
    assert np.array_equal(ops.edit_distance_long(ad, a_off, bd, b_off, v, workspace=dist_ws, out=dist_out).cpu().numpy(), host[0])
    m, n = np.diff(a_off), np.diff(b_off)
    cnt = host[3].sum(axis=0).tolist()
    lines.append(f"msocr_edit_alignment vs msocr_edit_alignment_host, {name}: {a.pairs} pairs, pattern {int(m.min())}..{int(m.max())} tokens, "
                 f"text {int(n.min())}..{int(n.max())} tokens, alphabets {int(v.min())}..{int(v.max())}, workspace {ws.numel()} bytes "
                 f"(the distance's: {dist_ws.numel()}); all four arrays identical; distances {int(host[0].min())}..{int(host[0].max())}, "
                 f"hits / substitutions / deletions / insertions {cnt}")
    ms = {"(a) msocr_edit_alignment, device call": [], "(b) msocr_edit_distance_long, device call, same arrays": [],
          "(c) msocr_edit_alignment_host": [], "(d) upload + msocr_edit_alignment + read-back of the four arrays": []}
    for rep in range(a.repeats + 2):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for _ in range(CALLS):
            ops.edit_alignment(ad, a_off, bd, b_off, v, workspace=ws, out=out)
        e1.record()
        for _ in range(CALLS):
            ops.edit_distance_long(ad, a_off, bd, b_off, v, workspace=dist_ws, out=dist_out)
        e2.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
        t1 = time.perf_counter()
        back = [t.cpu() for t in ops.edit_alignment(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v,
                                                    workspace=ws, out=out)]
        t2 = time.perf_counter()
        if rep >= 2:  # two warm-up rounds
            for key, t in zip(ms, (e0.elapsed_time(e1) / CALLS, e1.elapsed_time(e2) / CALLS, (t1 - t0) * 1e3, (t2 - t1) * 1e3)):
                ms[key].append(t)
    for k, t in ms.items():
        lines.append(f"  {k}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
    if not a.no_kernels:
        kt = kernel_times(name)
        if kt:
            lines.append("  (a) by kernel, rocprofv3 --kernel-trace --stats in a run of its own, mean over the calls: "
                         + ", ".join(f"{k} {us / 1e3:.3f} ms ({calls} calls)" for k, (us, calls) in sorted(kt.items())))
        else:
            lines.append("  (a) by kernel: not measured (rocprofv3 gave no kernel statistics)")
lines.append("one wave per pair in both kernels: 16 pairs occupy 16 of the chip's waves; the sweep's time is that of the longest pair's "
             "step chain plus its trace stores, the traceback's that of the longest walk; the host twin runs the pairs one after the "
             "other on one core")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
