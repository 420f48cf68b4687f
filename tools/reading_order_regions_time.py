"""Times msocr_reading_order_regions against msocr_reading_order_lines on the same boxes on the GPU box (dev tool; DESIGN.md section
4.20): the bench's shape, 16 pages 1536 x 2048 of about 480 synthetic words each, once as they are (one column: the cut finds nothing
and the page ends as one region) and once rearranged as two columns (the lower half of every page moved up beside the upper half,
both squeezed to 0.45 of the width).  Versions alternating inside one process, warm shapes, device events around the launches, median
and spread.  With the path of another build of libmsocr.so (the parent commit's) its msocr_reading_order_lines runs in the same
alternation as the yardstick:

    (p) msocr_reading_order_lines of the other library      the yardstick, when given
    (a) msocr_reading_order_lines                           the same entry point of this tree (Pipeline.group_lines)
    (b) msocr_reading_order_regions                         Pipeline.columns = True with group_lines

    python tools/reading_order_regions_time.py [pages] [output file] [other libmsocr.so]
"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import _native as nat  # noqa: E402
from manuscript_ocr_amd import ops, synth  # noqa: E402


def spread(ts):
    return f"median {statistics.median(ts):.3f} ms, min {min(ts):.3f}, max {max(ts):.3f} (n={len(ts)})"


def two_columns(rects, H, W):
    r = np.asarray(rects, dtype=np.float64).copy()
    low = 0.5 * (r[:, 1] + r[:, 3]) >= 0.5 * H
    r[:, [0, 2]] *= 0.45
    r[low, 0] += 0.55 * W
    r[low, 2] += 0.55 * W
    r[low, 1] -= 0.5 * H
    r[low, 3] -= 0.5 * H
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    other = sys.argv[3] if len(sys.argv) > 3 else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    H, W, img_h, img_w = 1536, 2048, 32, 100
    rects = [np.asarray(synth.synth_layout(100 + k, H, W), dtype=np.float64) for k in range(n)]
    max_cand = max(len(r) for r in rects)
    nbox_dev = torch.tensor([len(r) for r in rects], dtype=torch.int32).cuda()

    def upload(pages):
        boxes = np.zeros((n, max_cand, 9), dtype=np.float32)
        for k, r in enumerate(pages):
            boxes[k, :len(r), :8] = np.stack([r[:, [0, 1]], r[:, [2, 1]], r[:, [2, 3]], r[:, [0, 3]]], axis=1).reshape(-1, 8)
            boxes[k, :len(r), 8] = 0.9
        return torch.from_numpy(boxes).cuda()

    one, two = upload(rects), upload([two_columns(r, H, W) for r in rects])
    ws = torch.empty((nat.lib().msocr_reading_order_regions_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    plain = lambda b: ops.reading_order_lines(b, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws)
    regions = lambda b: ops.reading_order_regions(b, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws)
    versions = {}
    if other:
        lib = ctypes.CDLL(other)
        fn = lib.msocr_reading_order_lines
        fn.restype, fn.argtypes = nat._SIGS["msocr_reading_order_lines"]
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
        outs = [i32(n, max_cand), i32(n, max_cand), i32(n, max_cand, 8), i32(n), i32(n, max_cand), i32(n, min(max_cand, 4096), 6), i32(n)]

        def other_lines(b):
            nat.check(fn(b.data_ptr(), nbox_dev.data_ptr(), n, max_cand, H, W, 5, img_h, img_w, 0.6, float("inf"), 0,
                         *[t.data_ptr() for t in outs], ws.data_ptr(), ops._stream()), "the other library's reading_order_lines")
            return outs

        versions["(p) reading_order_lines of the other library, one column"] = lambda: other_lines(one)
        versions["(p) reading_order_lines of the other library, two columns"] = lambda: other_lines(two)
    # the outputs first: a page of one column is one region and keeps its bits; the rearranged pages are cut in two
    (ro_a, rl_a), (ro_b, rl_b, _sk, rg_b), (ro_c, rl_c), (ro_d, rl_d, _sk, rg_d) = plain(one), regions(one), plain(two), regions(two)
    assert bool((rg_b.nregions == 1).all()) and all(torch.equal(x, y) for x, y in zip(ro_a + rl_a, ro_b + rl_b))
    assert bool((ro_d.ncrop >= 0).all()) and bool((rg_d.nregions >= 2).all()) and not torch.equal(ro_c.order, ro_d.order)
    if other:
        got = [t.clone() for t in other_lines(one)]
        assert all(torch.equal(x, y) for x, y in zip(ro_a + rl_a, got)), "the other library orders the same pages differently"
    say(f"{n} pages {H} x {W}, {int(nbox_dev.sum())} words ({int(nbox_dev.min())}..{int(nbox_dev.max())} per page); device {torch.cuda.get_device_name(0)}")
    say(f"one column: regions per page {rg_b.nregions.float().mean():.1f}, lines {rl_b.nlines.float().mean():.1f}; two columns: regions "
        f"{rg_d.nregions.float().mean():.1f} ({int(rg_d.nregions.min())}..{int(rg_d.nregions.max())}), lines page-wide rule "
        f"{rl_c.nlines.float().mean():.1f}, by region {rl_d.nlines.float().mean():.1f}")
    versions.update({
        "(a) reading_order_lines, one column": lambda: plain(one),
        "(b) reading_order_regions, one column": lambda: regions(one),
        "(a) reading_order_lines, two columns": lambda: plain(two),
        "(b) reading_order_regions, two columns": lambda: regions(two),
    })
    for fn_ in versions.values():
        for _ in range(3):
            fn_()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    inner = 8
    for _ in range(25):
        for name, fn_ in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn_()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    say(f"per step of {n} pages (device events, {inner} launches per sample, versions alternating):")
    for name, ts in times.items():
        say(f"  {name}: {spread(ts)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
