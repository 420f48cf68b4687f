"""Times the approximate text search (msocr_text_search) beside its host twin on the same arrays (dev tool).
  python tools/text_search_time.py [--repeats N] [--patterns N] [--texts N] [--chars N] [--host-texts N] [--no-kernels] [--out FILE]
Workload: --patterns (1000) patterns of Poisson-8 length (at least 3) against --texts (1024) texts of about --chars (3400) characters
over a 60-symbol alphabet; every pattern is planted in a few texts with 0, 1 or 2 random edits.  Two bounds: k = 1 for every pattern,
and max_error_rate = 0.25 (k = min(floor(m / 4), m - 1)).  A second, small case fixes the crossover for Pipeline.search: 16 texts
against 10 patterns.
Before anything is timed the two routes are compared for equality: the device's hits in the first --host-texts (64) texts, sorted
into canonical order, against the host twin's on those texts (the twin on all of them takes a minute a bound; the small case is
compared whole).  Per round the versions take turns; one line each with the median and the spread (max - min) over --repeats rounds
(default 7), after two warm-up rounds:
  (a) the device call on a resident corpus, hits left on the device: device events around 5 calls of ops.text_search_into with room
      for every hit (the upload of the offsets, which the call waits for, and the four kernels)
  (b) patterns up, ops.text_search (its two passes where the first 65536 records do not hold the hits), hits read back: host clock
  (c) as (b) with the upload of the corpus in front
  (d) the host twin on the first --host-texts texts, host clock, and that time scaled to all texts (said to be scaled)
The scan, start, mask and clear kernels separately: kernel times of a run of its own under `rocprofv3 --kernel-trace --stats` (this
script starts itself once more as `--child NAME` behind rocprofv3; --no-kernels leaves that out).  The report goes to --out (default
profiles/text_search.txt)."""
import argparse, csv, glob, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from manuscript_ocr_amd import ops
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--patterns", type=int, default=1000)
ap.add_argument("--texts", type=int, default=1024)
ap.add_argument("--chars", type=int, default=3400)
ap.add_argument("--host-texts", type=int, default=64)
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--child", default=None, help="internal: run the calls of one case and exit (behind rocprofv3)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_search.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
V = 60
CALLS = 5


def workload(seed, Q, T, chars):
    """(pat_tok, pat_off, m, txt_tok, txt_off)"""
    rng = np.random.default_rng(seed)
    m = np.maximum(rng.poisson(8, Q), 3)
    pats = [rng.integers(0, V, int(k)) for k in m]
    texts = [rng.integers(0, V, int(chars * rng.uniform(0.9, 1.1))) for _ in range(T)]
    for q, p in enumerate(pats):  # planted noisy copies: each pattern in three texts with 0, 1 and 2 edits
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


def cases():
    big = workload(1, a.patterns, a.texts, a.chars)
    small = workload(2, 10, 16, a.chars)
    rate = lambda m: np.minimum(m // 4, m - 1).astype(np.int32)  # noqa: E731
    return {"k=1": (big, np.ones(a.patterns, dtype=np.int32), a.host_texts),
            "rate=0.25": (big, rate(big[2]), a.host_texts),
            "small,k=1": (small, np.ones(10, dtype=np.int32), 16),
            "small,rate=0.25": (small, rate(small[2]), 16)}


def canonical(h):
    return h[np.lexsort((h[:, 3], h[:, 1], h[:, 0]))] if len(h) else h


if a.child is not None:
    (pat_tok, pat_off, _m, txt_tok, txt_off), ks, _ = cases()[a.child]
    pd, td = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda()
    n = len(ops.text_search(pd, pat_off, ks, td, txt_off, V))
    hits = torch.empty((max(n, 1), 5), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ws = torch.empty((ops.text_search_workspace_bytes(pat_off, ks, txt_off, V),), dtype=torch.uint8, device="cuda")
    for _ in range(2 + CALLS):
        ops.text_search_into(pd, pat_off, ks, td, txt_off, V, hits, cnt, workspace=ws)
    torch.cuda.synchronize()
    sys.exit(0)


KERNELS = ("ts_scan_kernel", "ts_start_kernel", "ts_masks_kernel", "ts_zero_kernel")


def kernel_times(name):
    """{kernel: (mean microseconds, calls)} of one case, from a rocprofv3 run of its own; {} if that fails"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--patterns", str(a.patterns), "--texts", str(a.texts), "--chars", str(a.chars)]
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
                    for key in KERNELS:
                        if key in row.get("Name", ""):
                            res[key] = (float(row["TotalDurationNs"]) / max(int(row["Calls"]), 1) / 1e3, int(row["Calls"]))
        return res


lines = []
for name, ((pat_tok, pat_off, m, txt_tok, txt_off), ks, host_texts) in cases().items():
    Q, T = len(ks), len(txt_off) - 1
    host_texts = min(host_texts, T)
    pd, td = torch.from_numpy(pat_tok).cuda(), torch.from_numpy(txt_tok).cuda()
    got = ops.text_search(pd, pat_off, ks, td, txt_off, V)
    part_off = txt_off[:host_texts + 1]
    want, _ = ops.text_search_host(pat_tok, pat_off, ks, txt_tok, part_off, V)
    assert np.array_equal(canonical(got[got[:, 1] < host_texts]), want), "the two routes differ"
    assert np.array_equal(ops.text_search_select(got[got[:, 1] < host_texts]), ops.text_search_select(want))
    n = len(got)
    need = ops.text_search_workspace_bytes(pat_off, ks, txt_off, V)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    hits = torch.empty((max(n, 1), 5), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
    steps = int(len(txt_tok)) * Q
    lines.append(f"msocr_text_search vs msocr_text_search_host, {name}: {Q} patterns of {int(m.min())}..{int(m.max())} tokens (mean "
                 f"{float(m.mean()):.1f}), bounds {int(ks.min())}..{int(ks.max())}, {T} texts, {len(txt_tok)} tokens, alphabet {V}, "
                 f"{steps:.3e} pattern-column steps, workspace {need} bytes; {n} hits ({len(ops.text_search_select(got))} after selection); "
                 f"hits of the first {host_texts} texts identical on both routes ({len(want)})")
    ms = {"(a) device call, corpus resident, hits left on the device": [],
          "(b) patterns up + ops.text_search + hits read back, corpus resident": [],
          "(c) corpus up + (b)": [],
          f"(d) host twin, first {host_texts} of {T} texts": []}
    keys = list(ms)
    for rep in range(a.repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            ops.text_search_into(pd, pat_off, ks, td, txt_off, V, hits, cnt, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = ops.text_search(torch.from_numpy(pat_tok).cuda(), pat_off, ks, td, txt_off, V)
        t1 = time.perf_counter()
        back = ops.text_search(torch.from_numpy(pat_tok).cuda(), pat_off, ks, torch.from_numpy(txt_tok).cuda(), txt_off, V)
        t2 = time.perf_counter()
        ops.text_search_host(pat_tok, pat_off, ks, txt_tok, part_off, V)
        t3 = time.perf_counter()
        assert len(back) == n
        if rep >= 2:  # two warm-up rounds
            for key, t in zip(keys, (e0.elapsed_time(e1) / CALLS, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)):
                ms[key].append(t)
    for key, t in ms.items():
        lines.append(f"  {key}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
    if host_texts < T:
        frac = int(part_off[-1]) / len(txt_tok)
        lines.append(f"  (d) SCALED to all {T} texts by tokens (x {1 / frac:.2f}; not run): {statistics.median(ms[keys[3]]) / frac:.0f} ms")
    med = statistics.median(ms[keys[0]])
    lines.append(f"  (a) per pattern-column step: {med * 1e6 / steps * 1e3:.3f} ps; {steps / med / 1e6:.1f} G steps/s")
    if not a.no_kernels:
        kt = kernel_times(name)
        if kt:
            lines.append("  kernels (rocprofv3 --kernel-trace --stats, a run of its own, mean over the calls): " +
                         ", ".join(f"{k} {kt[k][0]:.1f} us x {kt[k][1]}" for k in KERNELS if k in kt))
        else:
            lines.append("  kernels: not measured (rocprofv3 did not run)")
lines.append("the host twin runs the patterns and texts one after the other on one core; the device cuts every text into segments of "
             f"{ops.SEARCH_SEGMENT} tokens, one lane per (pattern, segment)")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
