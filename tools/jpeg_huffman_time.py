"""Times the stages of the JPEG ingest of one bench batch (16 pages 2048 x 1536, quality 90, 4:2:0) on the GPU box (dev tool):
host marker walk, upload, device Huffman kernel (one thread per restart interval) for several interval lengths, reconstruction;
the self-synchronising stage (kernel sequence by device events, rounds taken, read_images_device end to end) for the files
without restart markers and for rows=1 / rows=4 — and the host thread-pool entropy decode of the same files.

    python tools/jpeg_huffman_time.py [pages]
"""
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manuscript_ocr_amd import ingest, synth  # noqa: E402


def end_to_end(paths, reps=3, **kw):
    """read_images_device per batch, ms: (mean, min, max) of `reps` calls after one warm-up call."""
    ingest.read_images_device(paths, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ingest.read_images_device(paths, **kw)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sum(ts) / len(ts), min(ts), max(ts)


def sync_stage(label, paths, n):
    """The self-synchronising stage on `paths`: kernel sequence by device events, rounds, end to end against the host pool."""
    parsed = [ingest._read_and_parse(p) for p in paths]
    t0 = time.perf_counter()
    batch = ingest.SyncBatch(parsed)
    t1 = time.perf_counter()
    bytes_dev = torch.from_numpy(batch.bytes).to("cuda")
    for _ in range(2):
        coef, status, rounds = ingest.entropy_sync_batch_device(batch, bytes_dev=bytes_dev)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        coef, status, rounds = ingest.entropy_sync_batch_device(batch, bytes_dev=bytes_dev)
    e1.record()
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    rounds = rounds.cpu().numpy()
    dev = end_to_end(paths, device_entropy=None)   # the default route: long intervals and plain files take the stage
    host = end_to_end(paths, device_entropy=False)
    print(f"{label}, self-synchronising stage: {batch.max_subseq} subsequences of {batch.subseq_bytes} B per page, rounds {rounds.min()}..{rounds.max()} "
          f"of {ingest.SYNC_MAX_ROUNDS}; marker walk + layout {1e3 * (t1 - t0):.1f} ms (serial, one thread), tables + bounds upload + memset + "
          f"kernel sequence {e0.elapsed_time(e1) / 5:.2f} ms per batch of {n}; read_images_device end to end {dev[0]:.1f} ms per batch "
          f"(min {dev[1]:.1f}, max {dev[2]:.1f}) against the host pool's {host[0]:.1f} ms (min {host[1]:.1f}, max {host[2]:.1f})", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    print(f"CPUs of this process: {len(os.sched_getaffinity(0))} (os.cpu_count() {os.cpu_count()})", flush=True)
    pages = [synth.synth_page(100 + k, 2048, 1536)[0] for k in range(n)]
    with tempfile.TemporaryDirectory(prefix="msocr_jt_", dir="/tmp") as td:
        for label, kw in (("rows=1", {"restart_marker_rows": 1}), ("rows=4", {"restart_marker_rows": 4}), ("blocks=32", {"restart_marker_blocks": 32}),
                          ("blocks=16", {"restart_marker_blocks": 16}), ("blocks=4", {"restart_marker_blocks": 4})):
            paths = []
            for k, pg in enumerate(pages):
                paths.append(os.path.join(td, f"{label}_{k}.jpg"))
                Image.fromarray(pg).save(paths[-1], quality=90, **kw)
            size = sum(os.path.getsize(p) for p in paths) / n
            t0 = time.perf_counter()
            parsed = [ingest._read_and_parse(p) for p in paths]
            t1 = time.perf_counter()
            batch = ingest.ScanBatch(parsed)
            t2 = time.perf_counter()
            bytes_dev = torch.from_numpy(batch.bytes).to("cuda")
            for _ in range(2):
                coef, status = ingest.entropy_batch_device(batch, bytes_dev=bytes_dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                coef, status = ingest.entropy_batch_device(batch, bytes_dev=bytes_dev)
            e1.record()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any()
            t3 = time.perf_counter()
            ingest.read_images_device(paths, device_entropy=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for _ in range(3):
                out = ingest.read_images_device(paths, device_entropy=True)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            print(f"{label}: {size / 1e3:.0f} kB/page, {batch.max_intervals} intervals/page; read+parse {1e3 * (t1 - t0):.1f} ms, marker walk + layout "
                  f"{1e3 * (t2 - t1):.1f} ms (serial, one thread), tables + bounds upload + memset + Huffman kernel {e0.elapsed_time(e1) / 5:.2f} ms per batch of {n}; "
                  f"read_images_device end to end {1e3 * (t4 - t3) / 3:.1f} ms per batch", flush=True)
            if label in ("rows=1", "rows=4"):
                sync_stage(label, paths, n)
        paths = []
        for k, pg in enumerate(pages):
            paths.append(os.path.join(td, f"plain_{k}.jpg"))
            Image.fromarray(pg).save(paths[-1], quality=90)
        sync_stage("no restart markers", paths, n)
        host = end_to_end(paths)
        print(f"no restart markers, default route (self-synchronising stage): "
              f"read_images_device {host[0]:.1f} ms per batch of {n} (min {host[1]:.1f}, max {host[2]:.1f})", flush=True)


if __name__ == "__main__":
    main()
