"""Image ingest on the device: JPEG file -> RGB u8 tensor in HBM (msocr_jpeg_* of libmsocr.so, csrc/jpeg.hip).

Replaces the file branch of the reference's read_image (detectors/_east/utils.py:477-497: cv2.imread + BGR->RGB, PIL
fallback — both libjpeg-turbo with default settings).  The file's bytes are uploaded as they are and the Huffman stage runs on
the MI355X: one thread per restart interval for files written with short restart intervals (`entropy_batch_device`), the
self-synchronising decode of a serial segment for files without restart markers and for long intervals
(`entropy_sync_batch_device`); the serial host decoder on a thread pool is the other route (`read_images_device` has the table of
which file takes which by default).  Dequantisation, inverse DCT, chroma upsampling and colour conversion always run on the
device, so the decoded page (9.4 MB at 2048x1536, 69 MB for the reference's 5390x4250 example page) is produced in HBM instead of
crossing PCIe.
A file with an Exif orientation (tag 0x0112 = 2..8: a page photographed in portrait) takes the same routes: the entropy stages do
not care, `_parse_oriented` reports the orientation beside the frame geometry and the reconstruction applies it in its last write
(msocr_jpeg_reconstruct_oriented), so the tensor that comes back is what read_image returns (ImageOps.exif_transpose): [W, H, 3]
for orientations 5..8.
Formats outside the kernel's scope (progressive, CMYK, 12-bit, two Exif segments, PNG, ...) return None: callers fall back to
read_image.
"""
import ctypes
import os

import numpy as np

from . import _native as nat


def _parse(data: bytes):
    info = nat.JpegInfo()
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    rc = nat.lib().msocr_jpeg_parse_host(ctypes.addressof(buf), len(data), ctypes.byref(info))
    if rc != 0 or not info.supported:
        return None, buf
    return info, buf


def _parse_oriented(data: bytes):
    """`_parse` for the product paths: streams with an Exif orientation are taken too -> (info or None, buffer, orientation 1..8)."""
    info = nat.JpegInfo()
    orient = ctypes.c_int32(1)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    rc = nat.lib().msocr_jpeg_parse_oriented_host(ctypes.addressof(buf), len(data), ctypes.byref(info), ctypes.byref(orient))
    if rc != 0 or not info.supported:
        return None, buf, 1
    return info, buf, int(orient.value)


def _oriented_shape(info, orientation):
    return (info.width, info.height, 3) if orientation >= 5 else (info.height, info.width, 3)


def jpeg_coefficients(data: bytes):
    """Host stage: (info, int16 coefficient array) of a supported JPEG, or None."""
    info, buf = _parse(data)
    if info is None:
        return None
    coef = np.empty(int(info.coef_total), dtype=np.int16)
    rc = nat.lib().msocr_jpeg_entropy_decode_host(ctypes.addressof(buf), len(data), ctypes.byref(info), coef.ctypes.data)
    if rc != 0:
        return None
    return info, coef


def decode_jpeg_host(data: bytes):
    """The whole decode on the CPU through the host twin of the device stage (tests; not a product path)."""
    r = jpeg_coefficients(data)
    if r is None:
        return None
    info, coef = r
    out = np.empty((info.height, info.width, 3), dtype=np.uint8)
    nat.check(nat.lib().msocr_jpeg_reconstruct_host(ctypes.byref(info), coef.ctypes.data, out.ctypes.data), "jpeg_reconstruct_host")
    return out


def decode_jpeg_oriented_host(data: bytes):
    """`decode_jpeg_host` with the Exif orientation applied: oriented parse, host entropy decoder, host twin of the oriented
    reconstruction (tests; not a product path) -> what read_image returns for the file, or None."""
    info, buf, orient = _parse_oriented(data)
    if info is None:
        return None
    coef = np.empty(int(info.coef_total), dtype=np.int16)
    if nat.lib().msocr_jpeg_entropy_decode_host(ctypes.addressof(buf), len(data), ctypes.byref(info), coef.ctypes.data) != 0:
        return None
    out = np.empty(_oriented_shape(info, orient), dtype=np.uint8)
    nat.check(nat.lib().msocr_jpeg_reconstruct_oriented_host(ctypes.byref(info), orient, coef.ctypes.data, out.ctypes.data),
              "jpeg_reconstruct_oriented_host")
    return out


def decode_jpeg_device(data: bytes, device="cuda", device_entropy=True):
    """JPEG bytes -> u8 tensor on the device (current stream), [H, W, 3] or, for Exif orientations 5..8, [W, H, 3] — the page as
    read_image returns it — or None when the stream is not supported.  A stream with
    a restart interval takes the per-interval Huffman kernel, one without the self-synchronising stage (a stream that stage
    declines, status 2, goes on to the host decoder); `device_entropy=False`: the host decoder for every stream."""
    import torch

    from . import ops
    info, buf, orient = _parse_oriented(data)
    if info is None:
        return None
    if device_entropy:
        batch = ScanBatch([(info, buf, len(data))])
        if batch.n_pages:
            coef, status = entropy_batch_device(batch, device)
            img = _reconstruct(info, coef, device, torch, ops, orient)
            return img if int(status.cpu()[0]) == 0 else None
        batch = SyncBatch([(info, buf, len(data))])
        if batch.n_pages:
            coef, status, _ = entropy_sync_batch_device(batch, device)
            st = int(status.cpu()[0])
            if st != 2:
                return _reconstruct(info, coef, device, torch, ops, orient) if st == 0 else None
    coef = np.empty(int(info.coef_total), dtype=np.int16)
    if nat.lib().msocr_jpeg_entropy_decode_host(ctypes.addressof(buf), len(data), ctypes.byref(info), coef.ctypes.data) != 0:
        return None
    return _reconstruct(info, torch.from_numpy(coef).to(device, non_blocking=True), device, torch, ops, orient)


def _prepare(ptr, n, info, bytes_base):
    """Marker walk of one parsed stream -> (descriptor bytes, interval bounds) or None (no restart interval / host decoder's case)."""
    lib = nat.lib()
    mcus = (int(info.blocks_w[0]) // int(info.hs[0])) * (int(info.blocks_h[0]) // int(info.vs[0]))
    d = np.zeros(int(lib.msocr_jpeg_scan_desc_bytes()), dtype=np.uint8)
    b = np.empty(2 * mcus, dtype=np.uint32)   # at most one interval per MCU
    niv = int(lib.msocr_jpeg_scan_prepare_host(ptr, n, ctypes.byref(info), bytes_base, d.ctypes.data, b.ctypes.data, mcus))
    return None if niv <= 0 else (d, b[: 2 * niv])


class ScanBatch:
    """Host side of the device entropy decode for a batch of parsed streams: descriptors, interval bounds, per-page bases and the
    files' bytes laid out as msocr_jpeg_entropy_decode_device takes them.  `pages[i]` = index into `descs` of stream i, or -1 (no
    restart interval, or a marker sequence the host decoder must judge).  `parsed[i]` = (info, ctypes buffer, length) or None;
    `prepared[i]` (optional) = what `_prepare` returned for stream i with `bytes_base[i]` as its base inside `bytes`."""

    def __init__(self, parsed, prepared=None, bytes_=None):
        self.pages, self.infos = [], []
        descs, bounds, chunks, base = [], [], [], []
        pos = coef_base = first = 0
        self.max_intervals = 0
        for i, pr in enumerate(parsed):
            if pr is None:
                self.pages.append(-1)
                continue
            info, buf, n = pr
            r = prepared[i] if prepared is not None else _prepare(ctypes.addressof(buf), n, info, pos)
            if r is None:
                self.pages.append(-1)
                continue
            self.pages.append(len(descs))
            self.infos.append((info, coef_base))
            descs.append(r[0])
            bounds.append(r[1])
            base.append((coef_base, first))
            if prepared is None:
                chunks.append(np.frombuffer(buf, dtype=np.uint8, count=n))
                pad = (-n) % 16
                if pad:
                    chunks.append(np.zeros(pad, dtype=np.uint8))
                pos += n + pad
            coef_base += int(info.coef_total)
            first += len(r[1]) // 2
            self.max_intervals = max(self.max_intervals, len(r[1]) // 2)
        self.n_pages = len(descs)
        self.coef_total = coef_base
        if self.n_pages:
            self.descs = np.stack(descs)
            self.bounds = np.concatenate(bounds)
            self.page_base = np.array(base, dtype=np.int64)
            self.bytes = bytes_ if prepared is not None else np.concatenate(chunks)


def entropy_batch_host_twin(batch: ScanBatch):
    """The kernel's per-interval decoder on the CPU (tests; not a product path) -> (int16 coefficients of the batch, status)."""
    coef = np.empty(batch.coef_total, dtype=np.int16)
    status = np.empty(batch.n_pages, dtype=np.int32)
    nat.check(nat.lib().msocr_jpeg_entropy_decode_intervals_host(batch.bytes.ctypes.data, batch.descs.ctypes.data, batch.n_pages,
                                                                  batch.bounds.ctypes.data, batch.page_base.ctypes.data, coef.ctypes.data,
                                                                  batch.coef_total, status.ctypes.data), "jpeg_entropy_decode_intervals_host")
    return coef, status


def entropy_batch_device(batch: ScanBatch, device="cuda", bytes_dev=None):
    """Uploads the batch's file bytes (unless `bytes_dev` already holds them), descriptors and interval bounds and runs the Huffman
    stage on the device (current stream) -> (int16 coefficient tensor of the batch, int32 status tensor [n_pages]); nothing is
    waited for."""
    import torch

    from . import ops
    up = lambda a: torch.from_numpy(a).to(device)
    if bytes_dev is None:
        bytes_dev = torch.from_numpy(batch.bytes).pin_memory().to(device, non_blocking=True)
    descs_dev, bounds_dev, base_dev = up(batch.descs), up(batch.bounds), up(batch.page_base)
    coef = torch.empty(batch.coef_total, dtype=torch.int16, device=device)
    status = torch.empty(batch.n_pages, dtype=torch.int32, device=device)
    nat.check(nat.lib().msocr_jpeg_entropy_decode_device(bytes_dev.data_ptr(), descs_dev.data_ptr(), batch.n_pages, batch.max_intervals,
                                                          bounds_dev.data_ptr(), base_dev.data_ptr(), coef.data_ptr(), batch.coef_total,
                                                          status.data_ptr(), ops._stream()), "jpeg_entropy_decode_device")
    return coef, status


SYNC_SUBSEQ_BYTES = 256    # a few times the distance page-like streams need to fall into step
SYNC_MAX_ROUNDS = 16
SYNC_MAX_FILE = 0x1ff00000  # the stage keeps bit positions in 32 bits
# Default route (device_entropy=None) of streams without a restart interval and of intervals longer than
# MSOCR_JPEG_DEVICE_MAX_INTERVAL: the self-synchronising stage when True, the host pool when False.  True by the measurement in
# profiles/jpeg_sync_huffman.txt: 6.4-7.0 ms per batch of 16 pages against 14.9-18.1 ms for the host pool.
SYNC_BY_DEFAULT = True


def _prepare_sync(ptr, n, info, bytes_base):
    """`_prepare` for the self-synchronising stage: a stream without a restart interval is one interval of all its MCUs."""
    lib = nat.lib()
    mcus = (int(info.blocks_w[0]) // int(info.hs[0])) * (int(info.blocks_h[0]) // int(info.vs[0]))
    d = np.zeros(int(lib.msocr_jpeg_scan_desc_bytes()), dtype=np.uint8)
    b = np.empty(2 * mcus, dtype=np.uint32)
    niv = int(lib.msocr_jpeg_sync_prepare_host(ptr, n, ctypes.byref(info), bytes_base, d.ctypes.data, b.ctypes.data, mcus))
    return None if niv <= 0 else (d, b[: 2 * niv])


class SyncBatch:
    """`ScanBatch` for the self-synchronising Huffman stage (msocr_jpeg_entropy_decode_sync_device): takes streams with and without
    a restart interval and lays out, beside descriptors / interval bounds / bytes, the subsequences of `subseq_bytes` bytes every
    interval is cut into (`sub_first`, `page_base` [n_pages][4], `max_subseq`, `total_subseq`).  `pages[i]` = index into `descs` of
    stream i, or -1 (a marker sequence the host decoder must judge, a file too large for 32-bit bit positions)."""

    def __init__(self, parsed, prepared=None, bytes_=None, subseq_bytes=SYNC_SUBSEQ_BYTES):
        self.pages, self.infos = [], []
        self.subseq_bytes = int(subseq_bytes)
        descs, bounds, sub_first, chunks, base = [], [], [], [], []
        pos = coef_base = first = sub_base = 0
        self.max_subseq = 0
        for i, pr in enumerate(parsed):
            r = None
            if pr is not None and pr[2] <= SYNC_MAX_FILE:
                info, buf, n = pr
                r = prepared[i] if prepared is not None else _prepare_sync(ctypes.addressof(buf), n, info, pos)
            if r is None:
                self.pages.append(-1)
                continue
            self.pages.append(len(descs))
            self.infos.append((info, coef_base))
            descs.append(r[0])
            bounds.append(r[1])
            length = r[1][1::2].astype(np.int64) - r[1][0::2].astype(np.int64)
            nsub = np.maximum(1, -(-length // self.subseq_bytes))
            sub_first.append((np.cumsum(nsub) - nsub).astype(np.uint32))
            nsub = int(nsub.sum())
            base.append((coef_base, first, sub_base, nsub))
            if prepared is None:
                chunks.append(np.frombuffer(buf, dtype=np.uint8, count=n))
                pad = (-n) % 16
                if pad:
                    chunks.append(np.zeros(pad, dtype=np.uint8))
                pos += n + pad
            coef_base += int(info.coef_total)
            first += len(r[1]) // 2
            sub_base += nsub
            self.max_subseq = max(self.max_subseq, nsub)
        self.n_pages = len(descs)
        self.coef_total = coef_base
        self.total_subseq = sub_base
        if self.n_pages:
            self.descs = np.stack(descs)
            self.bounds = np.concatenate(bounds)
            self.sub_first = np.concatenate(sub_first)
            self.page_base = np.array(base, dtype=np.int64)
            self.bytes = bytes_ if prepared is not None else np.concatenate(chunks)


def entropy_sync_batch_host_twin(batch: SyncBatch, max_rounds=SYNC_MAX_ROUNDS):
    """The self-synchronising stage on the CPU, same rounds and passes as the kernels (tests; not a product path)
    -> (int16 coefficients of the batch, status [n_pages] 0 / 1 / 2, rounds taken [n_pages])."""
    coef = np.empty(batch.coef_total, dtype=np.int16)
    status = np.empty(batch.n_pages, dtype=np.int32)
    rounds = np.empty(batch.n_pages, dtype=np.int32)
    nat.check(nat.lib().msocr_jpeg_entropy_decode_sync_host(batch.bytes.ctypes.data, batch.descs.ctypes.data, batch.n_pages,
                                                             batch.bounds.ctypes.data, batch.sub_first.ctypes.data,
                                                             batch.page_base.ctypes.data, batch.subseq_bytes, int(max_rounds),
                                                             coef.ctypes.data, batch.coef_total, status.ctypes.data, rounds.ctypes.data),
              "jpeg_entropy_decode_sync_host")
    return coef, status, rounds


def entropy_sync_batch_device(batch: SyncBatch, device="cuda", bytes_dev=None, max_rounds=SYNC_MAX_ROUNDS):
    """`entropy_batch_device` for a SyncBatch: uploads and queues the kernel sequence of the self-synchronising stage on the current
    stream -> (int16 coefficient tensor, int32 status tensor [n_pages]: 0 / 1 = bad stream / 2 = declined, take the host decoder,
    int32 tensor of the rounds taken [n_pages]); nothing is waited for."""
    import torch

    from . import ops
    up = lambda a: torch.from_numpy(a).to(device)
    if bytes_dev is None:
        bytes_dev = torch.from_numpy(batch.bytes).pin_memory().to(device, non_blocking=True)
    descs_dev, bounds_dev, sub_dev, base_dev = up(batch.descs), up(batch.bounds), up(batch.sub_first), up(batch.page_base)
    coef = torch.empty(batch.coef_total, dtype=torch.int16, device=device)
    status = torch.empty(batch.n_pages, dtype=torch.int32, device=device)
    rounds = torch.empty(batch.n_pages, dtype=torch.int32, device=device)
    lib = nat.lib()
    ws = torch.empty(int(lib.msocr_jpeg_sync_workspace_bytes(batch.total_subseq, batch.n_pages, int(max_rounds))), dtype=torch.uint8,
                     device=device)
    nat.check(lib.msocr_jpeg_entropy_decode_sync_device(bytes_dev.data_ptr(), descs_dev.data_ptr(), batch.n_pages, bounds_dev.data_ptr(),
                                                        sub_dev.data_ptr(), base_dev.data_ptr(), batch.max_subseq, batch.total_subseq,
                                                        batch.subseq_bytes, int(max_rounds), coef.data_ptr(), batch.coef_total,
                                                        status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), ops._stream()),
              "jpeg_entropy_decode_sync_device")
    return coef, status, rounds


def _reconstruct(info, coef_dev, device, torch, ops, orientation=1):
    """IDCT + upsampling + colour conversion of one page, the Exif orientation applied in the last write (1 = upright, the same
    kernels as msocr_jpeg_reconstruct) -> [H, W, 3] u8, [W, H, 3] for orientations 5..8."""
    ws = torch.empty((nat.lib().msocr_jpeg_workspace_bytes(ctypes.byref(info)),), dtype=torch.uint8, device=device)
    img = torch.empty(_oriented_shape(info, orientation), dtype=torch.uint8, device=device)
    nat.check(nat.lib().msocr_jpeg_reconstruct_oriented(ctypes.byref(info), int(orientation), coef_dev.data_ptr(), ws.data_ptr(),
                                                        img.data_ptr(), ops._stream()), "jpeg_reconstruct_oriented")
    return img


def _read_and_parse(path):
    """File -> (info, ctypes byte buffer, length), or None (not a file / not a supported JPEG).  Streams with an Exif orientation
    are taken (the entropy stages are orientation-blind); a caller that reconstructs asks `_parse_oriented` for the orientation."""
    if not isinstance(path, (str, os.PathLike)) or not os.path.isfile(path):
        return None
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"\xff\xd8":
        return None
    info, buf, _ = _parse_oriented(data)
    return None if info is None else (info, buf, len(data))


_POOL = None
_SLOTS = {}   # slot -> [pinned tensor, event of the last upload from it]; reused across batches (one reader thread at a time)


def _slot_buffer(slot, n, torch, dtype=None):
    ent = _SLOTS.get(slot)
    if ent is None or ent[0].numel() < n:
        ent = _SLOTS[slot] = [torch.empty(n + n // 4, dtype=dtype or torch.int16).pin_memory(), None]
    elif ent[1] is not None:
        ent[1].synchronize()   # the previous batch's upload from this buffer has left the host
    return ent


def _load(path, arr, off, n, want_device):
    """Worker: file -> its slice of the pinned batch buffer, header parse, marker walk.
    -> (info, `_prepare` result or None, `_prepare_sync` result of a stream without restart interval or None, Exif orientation)
    or None."""
    try:
        with open(path, "rb") as f:
            if f.readinto(memoryview(arr[off: off + n])) != n:
                return None
    except OSError:
        return None
    if n < 4 or arr[off] != 0xFF or arr[off + 1] != 0xD8:
        return None
    info = nat.JpegInfo()
    orient = ctypes.c_int32(1)
    ptr = arr.ctypes.data + off
    if nat.lib().msocr_jpeg_parse_oriented_host(ptr, n, ctypes.byref(info), ctypes.byref(orient)) != 0 or not info.supported:
        return None
    if not want_device:
        return info, None, None, int(orient.value)
    pr = _prepare(ptr, n, info, off)
    # no restart interval (or a marker sequence both walks refuse): the self-synchronising stage's view of the stream
    return info, pr, (_prepare_sync(ptr, n, info, off) if pr is None and n <= SYNC_MAX_FILE else None), int(orient.value)


def check_pending(pending):
    """Deferred verdict of the device Huffman stages (`read_images_device(..., defer_status=True)`): waits for the status words of
    that batch (a copy that was queued right behind the kernels; by the time a caller asks, long done) -> indices of the pages whose
    stream a kernel flagged as bad or declined (they must be read again through the host path)."""
    if pending is None:
        return []
    st_host, ev, idx = pending
    ev.synchronize()
    return [i for i, s in zip(idx, st_host.tolist()) if s != 0]


def read_images_device(paths, device="cuda", device_entropy=None, defer_status=False):
    """A batch of files -> list of device RGB tensors (None where read_image must take over).
    A thread pool reads every file into its slice of ONE pinned batch buffer (reused across batches), parses its headers and walks
    its markers (the ctypes calls release the GIL).  The buffer is uploaded as it is and the Huffman stage of the batch is at most
    two launch sequences.  Routes (`device_entropy=True` / False or MSOCR_JPEG_DEVICE_ENTROPY=1 / 0 force the device / the host):

        file                                          False   True                  None (default)
        no restart interval                           host    self-synchronising    self-synchronising if SYNC_BY_DEFAULT, else host
        intervals <= MSOCR_JPEG_DEVICE_MAX_INTERVAL   host    per-interval kernel   per-interval kernel
        longer intervals                              host    per-interval kernel   self-synchronising if SYNC_BY_DEFAULT, else host

    Per-interval kernel (`entropy_batch_device`): one thread per restart interval; its serial chain loses to a host core when an
    interval is long (MSOCR_JPEG_DEVICE_MAX_INTERVAL bytes, default 8192: 1.8 ms per KB of interval on the device against ~15 ms per
    1.6 MB file on a host core).  Self-synchronising stage (`entropy_sync_batch_device`): one thread per SYNC_SUBSEQ_BYTES bytes of
    a serial segment; a page it declines (status 2: no fixed point within SYNC_MAX_ROUNDS rounds, or a truncated stream) is decoded
    by the host pool inside this call, as every page of the "host" column is: the pool decodes one page per core into per-slot
    PINNED coefficient buffers that live across batches (fresh 9 MB arrays per page made the threads serialise on page faults),
    this thread uploads and launches the reconstruction page by page as the decodes finish.  The pixels are the same on every route.
    A file with an Exif orientation 2..8 takes the row of the table its restart intervals put it in, like an upright one: the
    orientation only changes the last write of its reconstruction (and the shape of its tensor: [W, H, 3] for 5..8).
    defer_status=True -> (list, pending): the device path's one host wait — the kernels' per-page verdict — is NOT taken here; the
    caller asks `check_pending(pending)` later (the pipeline does, when it waits for the detector anyway), so that submitting a
    batch never waits for the device; bad and declined pages are both reported there."""
    global _POOL
    import torch
    from concurrent.futures import ThreadPoolExecutor

    from . import ops
    env = os.environ.get("MSOCR_JPEG_DEVICE_ENTROPY")
    if device_entropy is None and env is not None:
        device_entropy = env != "0"
    max_iv = int(os.environ.get("MSOCR_JPEG_DEVICE_MAX_INTERVAL", "8192"))
    if _POOL is None:
        # one process per GPU: the ranks of a node share its cores (LOCAL_WORLD_SIZE is set by torch.distributed.run)
        share = (os.cpu_count() or 2) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(32, share - 1)), thread_name_prefix="msocr-jpeg")
    sizes = [os.path.getsize(p) if isinstance(p, (str, os.PathLike)) and os.path.isfile(p) else -1 for p in paths]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (max(n, 0) + 15) // 16 * 16
    pending = None
    if total == 0:
        return ([None] * len(paths), None) if defer_status else [None] * len(paths)
    ent = _slot_buffer("bytes", total, torch, torch.uint8)
    arr = ent[0].numpy()
    want = device_entropy is not False
    jobs = [(_POOL.submit(_load, p, arr, o, n, want) if n >= 0 else None) for p, o, n in zip(paths, offs, sizes)]
    loaded = [j.result() if j is not None else None for j in jobs]
    on_dev = {}
    if want:
        per_iv = [None if r is None else r[1] for r in loaded]          # the per-interval kernel's pages ...
        sync = [None if r is None else r[2] for r in loaded]            # ... and the self-synchronising stage's
        if device_entropy is None:   # the policy: no interval of the page longer than max_iv bytes
            long_iv = [p is not None and int((p[1][1::2] - p[1][0::2]).max()) > max_iv for p in per_iv]
            if SYNC_BY_DEFAULT:
                sync = [p if lg and n <= SYNC_MAX_FILE else q for p, q, lg, n in zip(per_iv, sync, long_iv, sizes)]
            else:
                sync = [None] * len(loaded)
            per_iv = [None if lg else p for p, lg in zip(per_iv, long_iv)]
        parsed = [None if r is None else (r[0], None, n) for r, n in zip(loaded, sizes)]
        runs = []                    # (batch, coefficient tensor, status tensor)
        bytes_dev = None
        for cls, prepared, run in ((ScanBatch, per_iv, entropy_batch_device), (SyncBatch, sync, entropy_sync_batch_device)):
            batch = cls(parsed, prepared, arr) if any(p is not None for p in prepared) else None
            if batch is None or not batch.n_pages:
                continue
            if bytes_dev is None:
                bytes_dev = ent[0][:total].to(device, non_blocking=True)
                ent[1] = torch.cuda.Event()
                ent[1].record()
            runs.append((batch,) + tuple(run(batch, device, bytes_dev)[:2]))
        if runs:
            imgs, idx = {}, []
            for batch, coef, _ in runs:
                for i, k in enumerate(batch.pages):
                    if k >= 0:
                        info, base = batch.infos[k]
                        imgs[i] = _reconstruct(info, coef[base:], device, torch, ops, loaded[i][3])
                        idx.append(i)
            status = runs[0][2] if len(runs) == 1 else torch.cat([r[2] for r in runs])
            if defer_status:
                st_host = torch.empty(len(idx), dtype=torch.int32).pin_memory()
                st_host.copy_(status, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending = (st_host, ev, idx)
                on_dev = imgs
            else:
                # the one wait of this path.  1: a bad stream goes to the host reader, as the host decoder's verdict would send it;
                # 2: declined, not judged: the host pool below decodes it
                on_dev = {i: (imgs[i] if st == 0 else None) for i, st in zip(idx, status.cpu().tolist()) if st != 2}
    lib = nat.lib()
    futs = []
    for i, r in enumerate(loaded):
        if r is None or i in on_dev:
            futs.append(None)
            continue
        slot = _slot_buffer(i, int(r[0].coef_total), torch)   # main thread: allocation / pinning is not done from the workers
        futs.append((_POOL.submit(lib.msocr_jpeg_entropy_decode_host, arr.ctypes.data + offs[i], sizes[i], ctypes.byref(r[0]), slot[0].data_ptr()), slot))
    out = []
    for i, (r, f) in enumerate(zip(loaded, futs)):
        if i in on_dev:
            out.append(on_dev[i])
            continue
        if f is None or f[0].result() != 0:
            out.append(None)
            continue
        info, slot = r[0], f[1]
        coef_dev = slot[0][: int(info.coef_total)].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        out.append(_reconstruct(info, coef_dev, device, torch, ops, r[3]))
    return (out, pending) if defer_status else out


def read_image_device(path, device="cuda"):
    """File -> device RGB tensor through the JPEG path, or None (not a file / not a supported JPEG: use read_image)."""
    return read_images_device([path], device)[0]
