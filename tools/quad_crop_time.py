"""Times the rectified crop against the AABB crop on the GPU box (dev tool): 16 pages 1536 x 2048 of synthetic words tilted by up to
10 degrees, 32 x 100 canvases (about 7.7 k crops per step).  Versions alternating inside one process, warm shapes, device events
around the launches:

    (a) msocr_crop_resize_pad on the words' AABB windows     the yardstick (what the pipeline runs by default)
    (b) msocr_quad_crop on the same words' quadrilaterals    Pipeline.rectify_crops = True
    (c) msocr_reading_order_crops alone                      the descriptor stage of the default route
    (d) (c) + msocr_quad_crop_descriptors                    the descriptor stage with rectified crops

    python tools/quad_crop_time.py [pages] [output file]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import ops, synth  # noqa: E402


def spread(ts):
    return f"median {statistics.median(ts):.3f} ms, min {min(ts):.3f}, max {max(ts):.3f} (n={len(ts)})"


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
    pages, quads = [], []
    for k in range(n):
        pg, rects = synth.synth_page(100 + k, H, W)
        pages.append(pg)
        quads.append(synth.synth_tilted_quads(rects, 100 + k, max_deg=10.0).astype(np.float32))
    max_cand = max(len(q) for q in quads)
    boxes = np.zeros((n, max_cand, 9), dtype=np.float32)
    for k, q in enumerate(quads):
        boxes[k, :len(q), :8] = q.reshape(-1, 8)
        boxes[k, :len(q), 8] = 0.9
    nbox = np.array([len(q) for q in quads], dtype=np.int32)
    pages_dev = torch.from_numpy(np.stack(pages)).cuda()
    boxes_dev, nbox_dev = torch.from_numpy(boxes).cuda(), torch.from_numpy(nbox).cuda()
    ro = ops.reading_order_crops(boxes_dev, nbox_dev, (H, W), 5, img_h, img_w)
    qd = ops.quad_crop_descriptors(boxes_dev, nbox_dev, ro, img_h, img_w)
    nc = ro[3].cpu().numpy()
    assert (nc >= 0).all()
    desc_dev = torch.cat([ro[2][k, :c] for k, c in enumerate(nc.tolist())]).contiguous()
    qdesc_dev = torch.cat([qd[k, :c] for k, c in enumerate(nc.tolist())]).contiguous()
    M = int(desc_dev.shape[0])
    # the outputs first: the kernel's canvases are the host twin's
    qdesc = qdesc_dev.cpu().numpy()
    probe = np.linspace(0, M - 1, 64).astype(np.int64)
    got = ops.quad_crop(pages_dev, None, img_h, img_w, qdesc_dev=qdesc_dev)[torch.from_numpy(probe).cuda()].cpu().numpy()
    assert np.array_equal(got, ops.quad_crop_host(np.stack(pages), qdesc[probe], img_h, img_w))
    c = qdesc[:, 1:9].copy().view(np.float32).reshape(-1, 4, 2).astype(np.float64)
    w = np.maximum(np.hypot(*(c[:, 1] - c[:, 0]).T), np.hypot(*(c[:, 2] - c[:, 3]).T))
    S = np.clip(np.ceil(w / qdesc[:, 9]), 1, 4)
    say(f"{n} pages {H} x {W}, {M} crops onto {img_h} x {img_w} canvases, tilt up to 10 degrees; sub-samples per axis: "
        + ", ".join(f"{int(s)}: {int((S == s).sum())}" for s in (1, 2, 3, 4)) + f"; device {torch.cuda.get_device_name(0)}")
    ws = torch.empty((ops.nat.lib().msocr_reading_order_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    qout = torch.empty((n, max_cand, 12), dtype=torch.int32, device="cuda")
    versions = {
        "(a) crop_resize_pad, AABB windows": lambda: ops.crop_resize_pad(pages_dev, None, img_h, img_w, desc_dev=desc_dev),
        "(b) quad_crop, quadrilaterals": lambda: ops.quad_crop(pages_dev, None, img_h, img_w, qdesc_dev=qdesc_dev),
        "(c) reading_order_crops": lambda: ops.reading_order_crops(boxes_dev, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws),
        "(d) reading_order_crops + quad_crop_descriptors": lambda: ops.quad_crop_descriptors(
            boxes_dev, nbox_dev, ops.reading_order_crops(boxes_dev, nbox_dev, (H, W), 5, img_h, img_w, workspace=ws), img_h, img_w, out=qout),
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
