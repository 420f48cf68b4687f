"""Times the quad matching (msocr_quad_match) beside its host twin on the same arrays (dev tool).
  python tools/quad_match_time.py [--repeats N] [--pages N] [--words N] [--out FILE]
16 pages x about 480 predictions / 480 ground truths (a grid of words; the ground truth jittered, a tenth dropped, a tenth of the
predictions spurious), T = 10 thresholds 0.50 .. 0.95.  Per round the two versions take turns: 20 device calls between two
events, then one host call on the host clock; one line per version with the median and the spread (max - min) over --repeats rounds
(default 9), after two warm-up rounds.  The device time is the call on arrays already on the device (three kernels); the
upload of the quads and the read-back of the results are timed separately.  The results of the two are compared for equality before
anything is timed.  The report goes to --out (default profiles/quad_match.txt).  The reference's shapely loop was not measured:
shapely is not available offline."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from manuscript_ocr_amd import ops
from test_quad_match_cpu import DEFAULT_T, pack, random_page, same_bits
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--pages", type=int, default=16)
ap.add_argument("--words", type=int, default=480)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_match.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
pages = [random_page(1000 + k, a.words) for k in range(a.pages)]
P, n_pred = pack([p for p, _ in pages])
G, n_gt = pack([g for _, g in pages])
dev_in = [torch.from_numpy(x).cuda() for x in (P, n_pred, G, n_gt)]
ws = torch.empty((ops.quad_match_workspace_bytes(a.pages, P.shape[1], G.shape[1]),), dtype=torch.uint8, device="cuda")
out = (torch.empty((a.pages, len(DEFAULT_T), P.shape[1]), dtype=torch.int32, device="cuda"),
       torch.empty((a.pages, len(DEFAULT_T), P.shape[1]), dtype=torch.float64, device="cuda"),
       torch.empty((a.pages, len(DEFAULT_T), 3), dtype=torch.int32, device="cuda"))
host = ops.quad_match_host(P, n_pred, G, n_gt, DEFAULT_T)
got = [t.cpu().numpy() for t in ops.quad_match(*dev_in, DEFAULT_T, workspace=ws, out=out)]
assert np.array_equal(got[2], host[2])
for p, n in enumerate(n_pred):
    assert np.array_equal(got[0][p, :, :n], host[0][p, :, :n]) and same_bits(got[1][p, :, :n], host[1][p, :, :n])
lines = [f"msocr_quad_match vs msocr_quad_match_host: {a.pages} pages, {int(n_pred.sum())} predictions, {int(n_gt.sum())} ground truths "
         f"(max {P.shape[1]} / {G.shape[1]} per page), T = {len(DEFAULT_T)}; pairs per call {int((n_pred.astype(np.int64) * n_gt).sum())}",
         f"results identical (match, IoU bit for bit, counts); tp / fp / fn at 0.50: {host[2][:, 0].sum(axis=0).tolist()}, "
         f"at 0.95: {host[2][:, -1].sum(axis=0).tolist()}"]
CALLS = 20
ms = {"device call": [], "host twin": [], "upload + device call + read-back": []}
for rep in range(a.repeats + 2):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        ops.quad_match(*dev_in, DEFAULT_T, workspace=ws, out=out)
    e1.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.quad_match_host(P, n_pred, G, n_gt, DEFAULT_T)
    t1 = time.perf_counter()
    up = [torch.from_numpy(x).cuda() for x in (P, n_pred, G, n_gt)]
    back = [t.cpu() for t in ops.quad_match(*up, DEFAULT_T, workspace=ws, out=out)]
    t2 = time.perf_counter()
    if rep >= 2:  # two warm-up rounds
        ms["device call"].append(e0.elapsed_time(e1) / CALLS)
        ms["host twin"].append((t1 - t0) * 1e3)
        ms["upload + device call + read-back"].append((t2 - t1) * 1e3)
for k, v in ms.items():
    lines.append(f"{k}: median {statistics.median(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
lines.append("the host twin computes each page's IoUs once for all thresholds on one core; the reference's shapely loop (every intersection "
             "again per threshold) was not measured: shapely is not available offline")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
