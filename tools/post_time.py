"""Times the page post-processing chain stage by stage on the GPU box (dev tool): 16 synthetic pages 1536 x 2048 of words tilted by
up to 10 degrees, their injected score / geometry maps (synth.synth_quad_maps) at 1/4 resolution, the detector's default
parameters.  Warm shapes, device events around each stage, every stage fed with the previous stage's (fixed) output:

    decode            msocr_east_decode
    lanms             msocr_east_lanms            (zero + x0 rank + page kernel + bit matrix + greedy wave)
    box tail          msocr_east_box_tail
    reading order     msocr_reading_order_crops
    quad descriptors  msocr_quad_crop_descriptors

It uses only `ops` functions, so the same file times any tree that has them; a digest of each stage's output is printed so that
two trees can be seen to compute the same bytes.

    python tools/post_time.py [pages] [output file] [label]
"""
import hashlib
import os
import statistics
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import ops, synth  # noqa: E402

REPEATS, INNER = 15, 4
H, W = 1536, 2048


def page_maps(k):
    _, rects = synth.synth_page(100 + k, H, W)
    quads = synth.synth_tilted_quads(rects, 100 + k, max_deg=10.0)
    return synth.synth_quad_maps(quads, (H, W), (H // 4, W // 4), 100 + k)


def digest(rows):
    return hashlib.sha1(b"".join(np.ascontiguousarray(r).tobytes() for r in rows)).hexdigest()[:12]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    img_h, img_w, q = 32, 100, 2
    with ProcessPoolExecutor(max_workers=min(n, 8)) as pool:  # seconds per page on one core; forked before the GPU is touched
        score, geo = zip(*pool.map(page_maps, range(n)))
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    score_d, geo_d = torch.from_numpy(np.stack(score)).cuda(), torch.from_numpy(np.stack(geo)).cuda()
    max_cand = (H // 4 // q) * (W // 4 // q)
    lib = ops.nat.lib()
    ws_l = torch.empty((lib.msocr_lanms_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    ws_t = torch.empty((lib.msocr_east_box_tail_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    ws_r = torch.empty((lib.msocr_reading_order_workspace_bytes(n, max_cand),), dtype=torch.uint8, device="cuda")
    qout = torch.zeros((n, max_cand, 12), dtype=torch.int32, device="cuda")

    cand, counts = ops.east_decode(score_d, geo_d, 0.6, 4.0, q, max_cand)
    boxes, nbox = ops.east_lanms(cand, counts, 0.2, workspace=ws_l)
    fboxes, fn = ops.east_box_tail(boxes, nbox, 0.9, 0.9, 1.0, 1.0, True, True, 5.0, 30, workspace=ws_t)
    ro = ops.reading_order_crops(fboxes, fn, (H, W), 5, img_h, img_w, workspace=ws_r)
    qd = ops.quad_crop_descriptors(fboxes, fn, ro, img_h, img_w, out=qout)
    torch.cuda.synchronize()
    c, nb, nf, nc = (t.cpu().numpy() for t in (counts, nbox, fn, ro.ncrop))
    assert (c > 0).all() and (c < max_cand).all() and (nb > 0).all() and (nf > 0).all() and (nc > 0).all()
    say(f"{label + ': ' if label else ''}{n} pages {H} x {W}, max_cand {max_cand}; per page on average: candidates {c.mean():.0f}, "
        f"boxes after LANMS {nb.mean():.0f}, after the tail {nf.mean():.0f}, crops {nc.mean():.0f}; device {torch.cuda.get_device_name(0)}")
    outs = {"decode": (cand, c), "lanms": (boxes, nb), "box tail": (fboxes, nf), "reading order": (ro.desc, nc), "quad descriptors": (qd, nc)}
    say("output digests: " + ", ".join(f"{k} {digest([t[p, :m].cpu().numpy() for p, m in enumerate(cnt)])}" for k, (t, cnt) in outs.items()))
    stages = {
        "decode": lambda: ops.east_decode(score_d, geo_d, 0.6, 4.0, q, max_cand),
        "lanms": lambda: ops.east_lanms(cand, counts, 0.2, workspace=ws_l),
        "box tail": lambda: ops.east_box_tail(boxes, nbox, 0.9, 0.9, 1.0, 1.0, True, True, 5.0, 30, workspace=ws_t),
        "reading order": lambda: ops.reading_order_crops(fboxes, fn, (H, W), 5, img_h, img_w, workspace=ws_r),
        "quad descriptors": lambda: ops.quad_crop_descriptors(fboxes, fn, ro, img_h, img_w, out=qout),
    }
    for fn_ in stages.values():
        for _ in range(3):
            fn_()
    torch.cuda.synchronize()
    times = {k: [] for k in stages}
    for _ in range(REPEATS):
        for name, fn_ in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                fn_()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / INNER)
    say(f"ms per step of {n} pages (device events, {INNER} launches per sample, stages alternating, {REPEATS} samples):")
    for name, ts in times.items():
        say(f"  {name:17s} median {statistics.median(ts):8.4f}  min {min(ts):8.4f}  max {max(ts):8.4f}")
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
