"""Times word spotting (msocr_frame_normalize, msocr_dtw_distances, msocr_topk_smallest) beside the host twins
(dev tool).
  python tools/word_spotting_time.py [--repeats N] [--cases a,b,c] [--host-words N] [--no-kernels] [--out FILE]
Cases, random features at T = 33, H = 256, lengths 4 .. 33, k = 10:
  a  10 queries x 1 048 576 indexed words        b  1 000 x 65 536        c  10 x 7 680 (the words of one bench step)
The corpus is made on the device, in blocks inside one native call's N T H < 2^31 (253 599 words here), as WordIndex keeps it.
Before anything is timed the device's distances of the first --host-words (64) words are held to the host twin's within the f32
bound of the distance, and the device's selection to the host twin's selection of the device's own distances, bit for bit.  Per
round, after two warm-up rounds, median and spread (max - min) over --repeats rounds (default 5), device events around 3 calls:
  (n) ops.frame_normalize over the whole corpus (what entering an index costs once)
  (d) ops.dtw_distances over all blocks, every length admitted (max_length_ratio None)
  (g) the same under the default gate, max_length_ratio 2.0
  (t) ops.topk_smallest on the [Q, N] distances
  (s) WordIndex.spot_features as a whole, host clock: queries normalised, distances block by block into one array, selection, the
      hits read back and turned into SpotHit
  (h) the host twin msocr_dtw_distances_host on the first --host-words words, host clock, and that time SCALED to the whole corpus
The three kernels separately: kernel times of a run of its own under `rocprofv3 --kernel-trace --stats` (this script starts itself
once more as `--child CASE` behind rocprofv3; --no-kernels leaves that out).  The report goes to --out (default
profiles/word_spotting.txt)."""
import argparse, csv, glob, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from manuscript_ocr_amd import WordIndex, ops
from manuscript_ocr_amd._spotting import length_bounds
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cases", default="a,b,c")
ap.add_argument("--host-words", type=int, default=64)
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--child", default=None, help="internal: run the calls of one case and exit (behind rocprofv3)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_spotting.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
T, H, K, CALLS = 33, 256, 10, 3
CASES = {"a": (10, 1 << 20), "b": (1000, 1 << 16), "c": (10, 7680)}
PER_CALL = ((1 << 31) - 1) // (T * H)
EPS = 2.0 ** -24


def make(seed, n):
    """n random words on the device -> [(raw frames, lengths)] in blocks of at most PER_CALL words"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for s in range(0, n, PER_CALL):
        m = min(PER_CALL, n - s)
        out.append((torch.randn((m, T, H), generator=g, device="cuda"),
                    torch.randint(4, T + 1, (m,), generator=g, device="cuda", dtype=torch.int32)))
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def setup(name):
    Q, N = CASES[name]
    corpus = make(1, N)
    (qraw, ql), = make(2, Q)
    qu = ops.frame_normalize(qraw, ql)
    units = [(ops.frame_normalize(f, l), l) for f, l in corpus]
    qlh = ql.cpu().numpy()
    gates = {r: tuple(torch.from_numpy(x).cuda() for x in length_bounds(qlh, r, T)) for r in (None, 2.0)}
    return Q, N, corpus, qu, ql, units, gates


def distances(qu, ql, gate, units):
    return [ops.dtw_distances(qu, ql, gate[0], gate[1], cu, cl) for cu, cl in units]


if a.child is not None:
    Q, N, corpus, qu, ql, units, gates = setup(a.child)
    for _ in range(2 + CALLS):
        for f, l in corpus:
            ops.frame_normalize(f, l, out=f)  # in place: a second copy of case a does not fit beside the first
        dist = torch.cat(distances(qu, ql, gates[None], units), dim=1)
        ops.topk_smallest(dist, K)
    torch.cuda.synchronize()
    sys.exit(0)

KERNELS = ("ws_normalize_kernel", "ws_dtw_kernel", "ws_topk_kernel")


def kernel_times(name):
    """{kernel: (mean microseconds, calls)} of one case, from a rocprofv3 run of its own; {} if that fails"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
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
for name in a.cases.split(","):
    Q, N, corpus, qu, ql, units, gates = setup(name)
    hw = min(a.host_words, N)
    # the two routes agree: distances within the f32 bound of the kernel, the selection bit for bit
    dist = torch.cat(distances(qu, ql, gates[None], units), dim=1)
    idx, val = ops.topk_smallest(dist, K)
    dist_h, qlh, clh = dist.cpu().numpy(), ql.cpu().numpy(), units[0][1][:hw].cpu().numpy()
    quh, cuh = qu.cpu().numpy(), units[0][0][:hw].cpu().numpy()
    lo, hi = length_bounds(qlh, None, T)
    want = ops.dtw_distances_host(quh, qlh, lo, hi, cuh, clh)
    err = np.abs(dist_h[:, :hw] - want)
    lim = (H + 2 * (qlh[:, None] + clh[None, :]) + 16) * EPS
    assert (err <= lim).all(), "the two routes differ"
    hidx, hval = ops.topk_smallest_host(dist_h, K)
    assert np.array_equal(idx.cpu().numpy(), hidx) and idx.cpu().numpy().tobytes() == hidx.tobytes(), "the selections differ"
    assert val.cpu().numpy().tobytes() == hval.tobytes(), "the selections differ"
    gated = torch.cat(distances(qu, ql, gates[2.0], units), dim=1)
    admitted = float(torch.isfinite(gated).float().mean())
    clens = torch.cat([l for _, l in units]).cpu().numpy().astype(np.int64)
    # local costs: Lq x Ln x H multiply-adds per pair; as issued: 32 x 32 blocks by the two lengths, K = H
    useful = float(qlh.astype(np.int64).sum()) * float(clens.sum()) * 2 * H
    issued = float(((qlh.astype(np.int64) + 31) // 32).sum()) * float(((clens + 31) // 32).sum()) * 32 * 32 * 2 * H
    lines.append(f"word spotting, case {name}: {Q} queries x {N} words, T {T}, H {H}, lengths 4..{T}, k {K}; corpus "
                 f"{N * (T * H * 4 + 4) / 1e9:.2f} GB in {len(units)} block(s); {useful / 1e12:.3f} TFLOP of Lq x Ln x H local costs, "
                 f"{issued / 1e12:.3f} TFLOP as issued in 32 x 32 blocks; first {hw} words: device within the bound of the host twin "
                 f"(max err {err.max():.2e}); selection identical to the host twin's; the default gate admits {admitted:.3f} of the pairs")
    index = WordIndex(None, device="cuda")
    at = 0
    for u, l in units:  # the index shares the blocks: no second copy
        index.add_features(u, l.cpu().numpy(), [(0, 0, at + i) for i in range(int(u.shape[0]))], normalized=True)
        at += int(u.shape[0])
    ms = {"(n) frame_normalize, whole corpus": [], "(d) dtw_distances, every length admitted": [],
          "(g) dtw_distances, max_length_ratio 2.0": [], "(t) topk_smallest": [],
          "(s) WordIndex.spot_features, whole call with read-back (host clock)": [], f"(h) host twin, first {hw} of {N} words (host clock)": []}
    keys = list(ms)
    for rep in range(a.repeats + 2):
        tn = timed(lambda: [ops.frame_normalize(f, l, out=u) for (f, l), (u, _) in zip(corpus, units)])
        td = timed(lambda: distances(qu, ql, gates[None], units))
        tg = timed(lambda: distances(qu, ql, gates[2.0], units))
        tt = timed(lambda: ops.topk_smallest(dist, K))
        t0 = time.perf_counter()
        hits = index.spot_features(qu, qlh, k=K, max_length_ratio=None, normalized=True)
        ts = (time.perf_counter() - t0) * 1e3
        assert [h.word for h in hits[0]] == hidx[0].tolist()
        t0 = time.perf_counter()
        ops.dtw_distances_host(quh, qlh, lo, hi, cuh, clh)
        th = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            for key, t in zip(keys, (tn, td, tg, tt, ts, th)):
                ms[key].append(t)
    for key, t in ms.items():
        lines.append(f"  {key}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
    med = statistics.median(ms[keys[1]])
    lines.append(f"  (d) {Q * N / med / 1e3:.2f} M pairs/s; {useful / med / 1e9:.1f} TFLOP/s of local costs, {issued / med / 1e9:.1f} TFLOP/s as issued")
    part = float((qlh[:, None].astype(np.float64) * clh[None, :]).sum()) * 2 * H
    lines.append(f"  (h) SCALED to the whole corpus by local-cost FLOP (x {useful / part:.0f}; not run): {statistics.median(ms[keys[5]]) * useful / part / 1e3:.1f} s")
    if not a.no_kernels:
        kt = kernel_times(name)
        if kt:
            lines.append("  kernels (rocprofv3 --kernel-trace --stats, a run of its own, mean over the launches; a launch covers one block): " +
                         ", ".join(f"{k} {kt[k][0]:.1f} us x {kt[k][1]}" for k in KERNELS if k in kt))
        else:
            lines.append("  kernels: not measured (rocprofv3 did not run)")
    del corpus, units, dist, gated, index
    torch.cuda.empty_cache()
lines.append(f"the host twin runs the pairs one after the other on one core, every product and table entry in f64; the device gives "
             f"every corpus word to one wave, {ops.SPOT_TILE} words per workgroup")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
