"""Times msocr_reading_order_deskew against msocr_reading_order_lines on the same boxes on the GPU box (dev tool; DESIGN.md section
4.19): the bench's shape, 16 pages 1536 x 2048 of about 480 synthetic words each.  Versions alternating inside one process, warm
shapes, device events around the launches, median and spread:

    (a) msocr_reading_order_lines,  upright words       the yardstick (Pipeline.group_lines)
    (b) msocr_reading_order_deskew, upright words       the two extra passes alone: the rotation is not applied, same boxes ordered
    (c) msocr_reading_order_lines,  pages turned by 3   the page-frame rule on skewed pages (lines fall apart: more lines to walk)
    (d) msocr_reading_order_deskew, pages turned by 3   Pipeline.deskew = True on the same boxes

    python tools/reading_order_deskew_time.py [pages] [output file]
"""
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import ops, synth  # noqa: E402


def spread(ts):
    return f"median {statistics.median(ts):.3f} ms, min {min(ts):.3f}, max {max(ts):.3f} (n={len(ts)})"


def turned(rects, deg, centre):
    r = np.asarray(rects, dtype=np.float64)
    q = np.stack([r[:, [0, 1]], r[:, [2, 1]], r[:, [2, 3]], r[:, [0, 3]]], axis=1) - centre
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.stack([c * q[..., 0] - s * q[..., 1], s * q[..., 0] + c * q[..., 1]], axis=-1) + centre


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    H, W, img_h, img_w = 1536, 2048, 32, 100
    rects = [synth.synth_layout(100 + k, H, W) for k in range(n)]
    max_cand = max(len(r) for r in rects)
    nbox_dev = torch.tensor([len(r) for r in rects], dtype=torch.int32).cuda()

    def upload(deg):
        boxes = np.zeros((n, max_cand, 9), dtype=np.float32)
        for k, r in enumerate(rects):
            boxes[k, :len(r), :8] = turned(r, deg, np.array([0.5 * W, 0.5 * H])).reshape(-1, 8)
            boxes[k, :len(r), 8] = 0.9
        return torch.from_numpy(boxes).cuda()

    upright, skewed = upload(0.0), upload(3.0)
    ws = torch.empty((ops.nat.lib().msocr_reading_order_deskew_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    plain = lambda b: ops.reading_order_lines(b, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws)
    deskew = lambda b: ops.reading_order_deskew(b, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws)
    # the outputs first: upright pages are untouched, skewed pages are estimated at 3 degrees and get their lines back
    (ro_a, rl_a), (ro_b, rl_b, sk_b), (ro_c, rl_c), (ro_d, rl_d, sk_d) = plain(upright), deskew(upright), plain(skewed), deskew(skewed)
    assert all(torch.equal(x, y) for x, y in zip(ro_a + rl_a, ro_b + rl_b)) and not bool(sk_b.skew[:, 3].any())
    assert bool((ro_d.ncrop >= 0).all()) and bool(sk_d.skew[:, 3].all())
    deg = torch.rad2deg(torch.atan2(sk_d.skew[:, 1].double(), sk_d.skew[:, 0].double()))
    say(f"{n} pages {H} x {W}, {int(nbox_dev.sum())} words ({int(nbox_dev.min())}..{int(nbox_dev.max())} per page); device {torch.cuda.get_device_name(0)}")
    say(f"lines per page: upright {rl_a.nlines.float().mean():.1f}; turned by 3 degrees: page frame {rl_c.nlines.float().mean():.1f}, "
        f"deskewed {rl_d.nlines.float().mean():.1f}; estimated skew {float(deg.min()):.3f}..{float(deg.max()):.3f} degrees")
    versions = {
        "(a) reading_order_lines, upright": lambda: plain(upright),
        "(b) reading_order_deskew, upright": lambda: deskew(upright),
        "(c) reading_order_lines, turned by 3 degrees": lambda: plain(skewed),
        "(d) reading_order_deskew, turned by 3 degrees": lambda: deskew(skewed),
    }
    for fn in versions.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    inner = 8
    for _ in range(25):
        for name, fn in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
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
