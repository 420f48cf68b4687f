"""Times the tiled detection against the untiled one on the GPU box (dev tool).  One synthetic page of
1536 x 2048, tile 1024 / overlap 128 = 2 x 3 tiles, 2.0x the page's pixels.  Versions alternating inside one process, warm
shapes, device events around the launches:

    (a) EAST(tile_size=1024, tile_overlap=128).detect_device       gather, network on 6 tiles, stitch, decode, LANMS, box filters
    (b) EAST(target_size=(2048, 1536)).detect_device               the untiled detector on the same page
    (c) EastNet.forward on one batch of 6 tiles 1024 x 1024        the network's share of (a)
    (d) msocr_east_tile_gather alone, 1 page and 16 pages          against bytes / HBM_RATE
    (e) msocr_east_stitch_maps alone, 1 page and 16 pages          against bytes / HBM_RATE

HBM_RATE is the 6.3 TB/s a float4 copy reaches on the MI355X (8 TB/s is the specification).  One page moves 28 MB (gather) and
14 MB (stitch), which the 256 MiB Infinity Cache holds: the 16-page rows are the ones that stream from HBM.

    python tools/east_tiles_time.py [output file]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import ops, synth  # noqa: E402
from manuscript_ocr_amd.detectors import EAST  # noqa: E402
from manuscript_ocr_amd.detectors._east import tiles  # noqa: E402

HBM_RATE = 6.3e12  # bytes / s


def spread(ts):
    return f"median {statistics.median(ts):.3f} ms, min {min(ts):.3f}, max {max(ts):.3f} (n={len(ts)})"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    H, W, T, OV = 1536, 2048, 1024, 128
    sd = synth.east_state_dict()
    tiled = EAST(state_dict=sd, device="cuda", tile_size=T, tile_overlap=OV)
    plain = EAST(state_dict=sd, device="cuda", target_size=(W, H))
    tab = ops.east_tile_tables(tiles.page_grid(H, W, (T, T), OV), "cuda")
    g = tab.grid
    page = torch.from_numpy(synth.synth_page(7, H, W)[0][None]).cuda()
    pages16 = page.expand(16, H, W, 3).contiguous()
    tile_px = ops.east_tile_gather(page, tab)
    ratio = g.ntiles * T * T / (H * W)
    say(f"page {H} x {W}, tile {T}, overlap {OV}: {g.ny} x {g.nx} tiles, {ratio:.2f}x the page's pixels; device {torch.cuda.get_device_name(0)}")
    maps = {n: (torch.rand((n, g.ntiles, T // 4, T // 4), device="cuda"), torch.randn((n, g.ntiles, T // 4, T // 4, 8), device="cuda"))
            for n in (1, 16)}
    gather_bytes = {n: n * (H * W * 3 + g.ntiles * T * T * 3) for n in (1, 16)}
    stitch_bytes = {n: n * 2 * 9 * 4 * (H // 4) * (W // 4) for n in (1, 16)}
    versions = {
        "(a) tiled detector": (lambda: tiled.detect_device(page), 1),
        "(b) untiled detector": (lambda: plain.detect_device(page), 1),
        "(c) network, 6 tiles": (lambda: tiled.model.forward(tile_px.view(g.ntiles, T, T, 3)), 1),
        "(d) gather, 1 page": (lambda: ops.east_tile_gather(page, tab), 20),
        "(d) gather, 16 pages": (lambda: ops.east_tile_gather(pages16, tab), 20),
        "(e) stitch, 1 page": (lambda: ops.east_stitch_maps(*maps[1], tab), 20),
        "(e) stitch, 16 pages": (lambda: ops.east_stitch_maps(*maps[16], tab), 20),
    }
    for fn, _ in versions.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(15):
        for name, (fn, inner) in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    say("per call (device events, detector and network 1 call per sample, kernels 20; versions alternating):")
    for name, ts in times.items():
        say(f"  {name}: {spread(ts)}")
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"tiled / untiled = {med['(a) tiled detector'] / med['(b) untiled detector']:.2f} (pixel ratio {ratio:.2f}); "
        f"the network on the tiles is {med['(c) network, 6 tiles'] / med['(a) tiled detector']:.2f} of the tiled detector")
    for n in (1, 16):
        for kind, nbytes in (("gather", gather_bytes[n]), ("stitch", stitch_bytes[n])):
            key = f"({'d' if kind == 'gather' else 'e'}) {kind}, {n} page{'s' if n > 1 else ''}"
            floor_ms = nbytes / HBM_RATE * 1e3
            say(f"  {kind}, {n} page(s): {nbytes / 1e6:.1f} MB, floor {floor_ms:.4f} ms at {HBM_RATE / 1e12:.1f} TB/s, measured {med[key]:.4f} ms = "
                f"{floor_ms / med[key]:.2f} of the HBM rate")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
