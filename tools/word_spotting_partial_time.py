"""Times the subsequence distance (msocr_dtw_subsequence) against the global one (msocr_dtw_distances, section
4.25) on the same arrays in the same job (dev tool): what the second carried value of the table walk costs.
  python tools/word_spotting_partial_time.py [--repeats N] [--cases a,b,c] [--host-words N] [--no-kernels] [--out FILE]
Cases, random features at T = 33, H = 256, lengths 4 .. 33 (those of tools/word_spotting_time.py):
  a  10 queries x 1 048 576 indexed words        b  1 000 x 65 536        c  10 x 7 680 (the words of one bench step)
The corpus is made on the device and normalised in place, in blocks inside one native call's N T H < 2^31 (253 599 words here).
Before anything is timed the device's subsequence distances of the first --host-words (64) words are held to the host twin's within
the f32 bound of the kernel from the same unit frames, (H + 2 (Lq + Ln) + 16) 2^-24 (Lq + Ln) / Lq, and every span to its word.
Then, alternating within every round, after two warm-up rounds, median and spread (max - min) over --repeats rounds (default 5),
device events around 3 calls over all blocks, results into preallocated tensors:
  (D) ops.dtw_distances, every length admitted            (S) ops.dtw_subsequence, every length admitted
  (Dg) ops.dtw_distances under the partial route's gate   (Sg) ops.dtw_subsequence under it: ceil(Lq / 2) .. T
The two kernels separately: kernel times of a run of its own under `rocprofv3 --kernel-trace --stats` (this script starts itself
once more as `--child CASE` behind rocprofv3; --no-kernels leaves that out).  The report goes to --out (default
profiles/word_spotting_partial.txt)."""
import argparse, csv, glob, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from manuscript_ocr_amd import ops
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cases", default="a,b,c")
ap.add_argument("--host-words", type=int, default=64)
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--child", default=None, help="internal: run the calls of one case and exit (behind rocprofv3)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_spotting_partial.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the timing needs the MI355X"
T, H, CALLS = 33, 256, 3
CASES = {"a": (10, 1 << 20), "b": (1000, 1 << 16), "c": (10, 7680)}
PER_CALL = ((1 << 31) - 1) // (T * H)
EPS = 2.0 ** -24


def make(seed, n):
    """n random words on the device, normalised in place -> [(unit frames, lengths)] in blocks of at most PER_CALL words"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for s in range(0, n, PER_CALL):
        m = min(PER_CALL, n - s)
        f = torch.randn((m, T, H), generator=g, device="cuda")
        l = torch.randint(4, T + 1, (m,), generator=g, device="cuda", dtype=torch.int32)
        out.append((ops.frame_normalize(f, l, out=f), l))
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
    units = make(1, N)
    (qu, ql), = make(2, Q)
    qlh = ql.cpu().numpy()
    gates = {"open": (torch.ones_like(ql), torch.full_like(ql, T)),
             "partial": (torch.from_numpy(np.maximum(-(-qlh // 2), 1).astype(np.int32)).cuda(), torch.full_like(ql, T))}
    dist = [torch.empty((Q, int(u.shape[0])), dtype=torch.float32, device="cuda") for u, _ in units]
    span = [torch.empty((Q, int(u.shape[0]), 2), dtype=torch.int32, device="cuda") for u, _ in units]
    return Q, N, qu, ql, qlh, units, gates, dist, span


def run_global(qu, ql, gate, units, dist):
    for (cu, cl), d in zip(units, dist):
        ops.dtw_distances(qu, ql, gate[0], gate[1], cu, cl, out=d)


def run_sub(qu, ql, gate, units, dist, span):
    for (cu, cl), d, s in zip(units, dist, span):
        ops.dtw_subsequence(qu, ql, gate[0], gate[1], cu, cl, out=d, span_out=s)


if a.child is not None:
    Q, N, qu, ql, qlh, units, gates, dist, span = setup(a.child)
    for _ in range(2 + CALLS):
        run_global(qu, ql, gates["open"], units, dist)
        run_sub(qu, ql, gates["open"], units, dist, span)
    torch.cuda.synchronize()
    sys.exit(0)

KERNELS = ("ws_dtw_kernel", "ws_dtw_sub_kernel")


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
                        if key in row.get("Name", ""):  # neither name contains the other
                            res[key] = (float(row["TotalDurationNs"]) / max(int(row["Calls"]), 1) / 1e3, int(row["Calls"]))
        return res


lines = []
for name in a.cases.split(","):
    Q, N, qu, ql, qlh, units, gates, dist, span = setup(name)
    hw = min(a.host_words, N)
    # the two routes agree on the first words: d within the kernel's f32 bound from the same unit frames, every span inside its word
    run_sub(qu, ql, gates["open"], units, dist, span)
    torch.cuda.synchronize()
    clh = units[0][1][:hw].cpu().numpy()
    quh, cuh = qu.cpu().numpy(), units[0][0][:hw].cpu().numpy()
    want, wspan = ops.dtw_subsequence_host(quh, qlh, np.ones(Q, dtype=np.int32), np.full(Q, T, dtype=np.int32), cuh, clh)
    got, gspan = dist[0][:, :hw].cpu().numpy(), span[0][:, :hw].cpu().numpy()
    both = qlh[:, None].astype(np.float64) + clh[None, :]
    lim = (H + 2 * both + 16) * EPS * both / qlh[:, None]
    err = np.abs(got - want)
    assert (err <= lim).all(), "the two routes differ"
    assert ((0 <= gspan[..., 0]) & (gspan[..., 0] < gspan[..., 1]) & (gspan[..., 1] <= clh[None, :])).all(), "a span outside its word"
    same_span = float((gspan == wspan).all(axis=2).mean())
    run_sub(qu, ql, gates["partial"], units, dist, span)
    admitted = sum(int(torch.isfinite(d).sum()) for d in dist) / (Q * N)
    lines.append(f"partial word spotting, case {name}: {Q} queries x {N} words, T {T}, H {H}, lengths 4..{T}; corpus "
                 f"{N * (T * H * 4 + 4) / 1e9:.2f} GB in {len(units)} block(s); first {hw} words: device within the bound of the host twin "
                 f"(max err {err.max():.2e}, worst err/bound {(err / lim).max():.4f}), {same_span:.4f} of the spans equal to the host "
                 f"twin's (near-ties may fall differently); the partial gate admits {admitted:.3f} of the pairs")
    ms = {"(D) dtw_distances, every length admitted": [], "(S) dtw_subsequence, every length admitted": [],
          "(Dg) dtw_distances, gate ceil(Lq / 2) .. T": [], "(Sg) dtw_subsequence, gate ceil(Lq / 2) .. T": []}
    keys = list(ms)
    for rep in range(a.repeats + 2):
        t = (timed(lambda: run_global(qu, ql, gates["open"], units, dist)),
             timed(lambda: run_sub(qu, ql, gates["open"], units, dist, span)),
             timed(lambda: run_global(qu, ql, gates["partial"], units, dist)),
             timed(lambda: run_sub(qu, ql, gates["partial"], units, dist, span)))
        if rep >= 2:
            for key, v in zip(keys, t):
                ms[key].append(v)
    for key, t in ms.items():
        lines.append(f"  {key}: median {statistics.median(t):.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} rounds")
    med = [statistics.median(ms[k]) for k in keys]
    lines.append(f"  subsequence / global: {med[1] / med[0]:.3f} with every length admitted, {med[3] / med[2]:.3f} under the gate; "
                 f"(S) {Q * N / med[1] / 1e3:.2f} M pairs/s")
    if not a.no_kernels:
        kt = kernel_times(name)
        if kt:
            lines.append("  kernels (rocprofv3 --kernel-trace --stats, a run of its own, every length admitted, mean over the launches; a "
                         "launch covers one block): " + ", ".join(f"{k} {kt[k][0]:.1f} us x {kt[k][1]}" for k in KERNELS if k in kt))
        else:
            lines.append("  kernels: not measured (rocprofv3 did not run)")
    del units, dist, span
    torch.cuda.empty_cache()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
