"""Times the oriented last stage of the JPEG reconstruction on the GPU box (dev tool): 16 pages 2048 x 1536, quality 90, 4:2:0, from
files.  Per batch, versions alternating inside one process, warm shapes, device events around the launches of a batch:

    (a) msocr_jpeg_reconstruct, upright                      the yardstick
    (b) msocr_jpeg_reconstruct_oriented, orientation 3       mirrored destinations, rows stay rows
    (c) msocr_jpeg_reconstruct_oriented, orientation 6       the tiled transposing colour kernel
    (d) (a) + torch.rot90(page, -1).contiguous()             orientation 6 without a fused kernel
    (e) read_images_device + stack on orientation-6 files    end to end, host clock around a synchronise
    (f) read_image of every file + stack + upload            the route such files took before

    python tools/jpeg_orientation_time.py [pages] [output file]
"""
import ctypes
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import _native as nat, ingest, ops, synth  # noqa: E402
from manuscript_ocr_amd.detectors import read_image  # noqa: E402


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
    lib = nat.lib()
    H, W = 2048, 1536
    say(f"{n} pages {H} x {W}, quality 90, 4:2:0, no restart markers; device {torch.cuda.get_device_name(0)}; "
        f"CPUs of this process: {len(os.sched_getaffinity(0))}")
    pages = [synth.synth_page(100 + k, H, W)[0] for k in range(n)]
    ex = Image.Exif()
    ex[0x0112] = 6
    with tempfile.TemporaryDirectory(prefix="msocr_jo_", dir="/tmp") as td:
        up, turned = [], []
        for k, pg in enumerate(pages):
            up.append(os.path.join(td, f"up_{k}.jpg"))
            Image.fromarray(pg).save(up[-1], quality=90)
            turned.append(os.path.join(td, f"o6_{k}.jpg"))
            Image.fromarray(pg).save(turned[-1], quality=90, exif=ex.tobytes())
        # resident coefficients of the batch: the stage under test starts from them
        parsed = [ingest._read_and_parse(p) for p in up]
        batch = ingest.SyncBatch(parsed)
        coef, status, _ = ingest.entropy_sync_batch_device(batch)
        assert not status.cpu().numpy().any()
        infos = [batch.infos[batch.pages[i]] for i in range(n)]
        ws = [torch.empty(int(lib.msocr_jpeg_workspace_bytes(ctypes.byref(f))), dtype=torch.uint8, device="cuda") for f, _ in infos]
        out = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
        out_t = [torch.empty((W, H, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]

        def stage(orientation, dst):
            s = ops._stream()
            for (f, base), w, o in zip(infos, ws, dst):
                if orientation == 0:
                    nat.check(lib.msocr_jpeg_reconstruct(ctypes.byref(f), coef[base:].data_ptr(), w.data_ptr(), o.data_ptr(), s), "reconstruct")
                else:
                    nat.check(lib.msocr_jpeg_reconstruct_oriented(ctypes.byref(f), orientation, coef[base:].data_ptr(), w.data_ptr(), o.data_ptr(), s),
                              "reconstruct_oriented")

        versions = {
            "(a) upright msocr_jpeg_reconstruct": lambda: stage(0, out),
            "(b) oriented, orientation 3": lambda: stage(3, out),
            "(c) oriented, orientation 6": lambda: stage(6, out_t),
            "(d) upright + torch.rot90(-1).contiguous()": lambda: (stage(0, out), [torch.rot90(o, -1, (0, 1)).contiguous() for o in out]),
        }
        # the outputs first: (b) and (c) are the transposes of (a)
        stage(0, out)
        ref = [o.clone() for o in out]
        stage(3, out)
        assert all(torch.equal(o, torch.rot90(r, 2, (0, 1))) for o, r in zip(out, ref))
        stage(6, out_t)
        assert all(torch.equal(o, torch.rot90(r, -1, (0, 1))) for o, r in zip(out_t, ref))
        for fn in versions.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in versions}
        inner = 4
        for _ in range(25):
            for name, fn in versions.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / inner)
        say(f"reconstruction stage per batch of {n} pages (IDCT + colour stage, device events, {inner} batches per sample, versions alternating):")
        for name, ts in times.items():
            say(f"  {name}: {spread(ts)}")

        def dev_route():
            return torch.stack(ingest.read_images_device(turned))

        def host_route():
            return torch.from_numpy(np.ascontiguousarray(np.stack([read_image(p) for p in turned]))).to("cuda")

        a, b = dev_route(), host_route()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and tuple(a.shape) == (n, W, H, 3)
        del a, b
        e2e = {"(e) read_images_device + stack, orientation-6 files": dev_route, "(f) read_image per file + stack + upload": host_route}
        times = {k: [] for k in e2e}
        for _ in range(6):
            for name, fn in e2e.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
        say(f"end to end per batch of {n} orientation-6 files (host clock around a synchronise, versions alternating, after one warm call each):")
        for name, ts in times.items():
            say(f"  {name}: {spread(ts)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
