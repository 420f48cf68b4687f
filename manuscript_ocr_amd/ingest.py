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


def _parse_at(ptr, n, strict):
    """Header parse of the n bytes at `ptr` -> (info or None, Exif orientation 1..8).  strict: msocr_jpeg_parse_host, which refuses a
    stream with orientation 2..8 (the upright reconstruction is not its); else msocr_jpeg_parse_oriented_host, which reports it."""
    info = nat.JpegInfo()
    orient = ctypes.c_int32(1)
    if strict:
        rc = nat.lib().msocr_jpeg_parse_host(ptr, n, ctypes.byref(info))
    else:
        rc = nat.lib().msocr_jpeg_parse_oriented_host(ptr, n, ctypes.byref(info), ctypes.byref(orient))
    if rc != 0 or not info.supported:
        return None, 1
    return info, int(orient.value)


def _parse(data: bytes):
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    return _parse_at(ctypes.addressof(buf), len(data), True)[0], buf


def _parse_oriented(data: bytes):
    """`_parse` for the product paths: streams with an Exif orientation are taken too -> (info or None, buffer, orientation 1..8)."""
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    info, orient = _parse_at(ctypes.addressof(buf), len(data), False)
    return info, buf, orient


def _oriented_shape(info, orientation):
    return (info.width, info.height, 3) if orientation >= 5 else (info.height, info.width, 3)


def _serial_decode(ptr, n, info, coef=None):
    """The serial host decoder — the judge of every stream — on the n bytes at `ptr`, into `coef` (a fresh array when None)
    -> the int16 coefficient array, or None for a bad stream."""
    if coef is None:
        coef = np.empty(int(info.coef_total), dtype=np.int16)
    rc = nat.lib().msocr_jpeg_entropy_decode_host(ptr, n, ctypes.byref(info), coef.ctypes.data)
    return coef if rc == 0 else None


def jpeg_coefficients(data: bytes):
    """Host stage: (info, int16 coefficient array) of a supported JPEG, or None."""
    info, buf = _parse(data)
    coef = None if info is None else _serial_decode(ctypes.addressof(buf), len(data), info)
    return None if coef is None else (info, coef)


def _decode_host(data, strict):
    """The whole decode on the CPU: parse (`strict`: see `_parse_at`), host entropy decoder, host twin of the oriented
    reconstruction -> what read_image returns for the file, or None."""
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    info, orient = _parse_at(ctypes.addressof(buf), len(data), strict)
    coef = None if info is None else _serial_decode(ctypes.addressof(buf), len(data), info)
    if coef is None:
        return None
    out = np.empty(_oriented_shape(info, orient), dtype=np.uint8)
    nat.check(nat.lib().msocr_jpeg_reconstruct_oriented_host(ctypes.byref(info), orient, coef.ctypes.data, out.ctypes.data),
              "jpeg_reconstruct_oriented_host")
    return out


def decode_jpeg_oriented_host(data: bytes):
    """The whole decode on the CPU through the host twin of the device stage, the Exif orientation applied (tests; not a product
    path)."""
    return _decode_host(data, strict=False)


def decode_jpeg_host(data: bytes):
    """`decode_jpeg_oriented_host` with the strict parse: a stream with an Exif orientation 2..8 gives None."""
    return _decode_host(data, strict=True)


def _prepare(ptr, n, info, bytes_base, sync):
    """Marker walk of one parsed stream -> (descriptor bytes, interval bounds) or None (the host decoder's case).  sync=False: the
    per-interval kernel's walk, which also refuses a stream without a restart interval; True: the self-synchronising stage's,
    which takes such a stream as one interval of all its MCUs."""
    lib = nat.lib()
    walk = lib.msocr_jpeg_sync_prepare_host if sync else lib.msocr_jpeg_scan_prepare_host
    mcus = (int(info.blocks_w[0]) // int(info.hs[0])) * (int(info.blocks_h[0]) // int(info.vs[0]))
    d = np.zeros(int(lib.msocr_jpeg_scan_desc_bytes()), dtype=np.uint8)
    b = np.empty(2 * mcus, dtype=np.uint32)   # at most one interval per MCU
    niv = int(walk(ptr, n, ctypes.byref(info), bytes_base, d.ctypes.data, b.ctypes.data, mcus))
    return None if niv <= 0 else (d, b[: 2 * niv])


class _Batch:
    """Host side of a device entropy stage for a batch of parsed streams: descriptors, interval bounds, per-page bases and the
    files' bytes laid out as the stage's entry takes them.  `parsed[i]` = (info, ctypes buffer, length) or None; `prepared[i]`
    (optional) = what `_prepare` returned for stream i with `bytes_base[i]` as its base inside `bytes_`.  `pages[i]` = index into
    `descs` of stream i, or -1.  A subclass names its walk (`_sync`), its file-size cap (`_max_file`) and, in `_page`, the columns
    it adds to a page's row of `page_base` behind (coefficient base, first interval)."""
    _max_file = None

    def __init__(self, parsed, prepared=None, bytes_=None):
        self.pages, self.infos = [], []
        descs, bounds, chunks, rows = [], [], [], []
        pos = coef_base = first = 0
        for i, pr in enumerate(parsed):
            r = None
            if pr is not None and (self._max_file is None or pr[2] <= self._max_file):
                info, buf, n = pr
                r = prepared[i] if prepared is not None else _prepare(ctypes.addressof(buf), n, info, pos, self._sync)
            if r is None:
                self.pages.append(-1)
                continue
            self.pages.append(len(descs))
            self.infos.append((info, coef_base))
            descs.append(r[0])
            bounds.append(r[1])
            rows.append((coef_base, first) + self._page(r[1]))
            if prepared is None:
                chunks.append(np.frombuffer(buf, dtype=np.uint8, count=n))
                pad = (-n) % 16
                if pad:
                    chunks.append(np.zeros(pad, dtype=np.uint8))
                pos += n + pad
            coef_base += int(info.coef_total)
            first += len(r[1]) // 2
        self.n_pages = len(descs)
        self.coef_total = coef_base
        if self.n_pages:
            self.descs = np.stack(descs)
            self.bounds = np.concatenate(bounds)
            self.page_base = np.array(rows, dtype=np.int64)
            self.bytes = bytes_ if prepared is not None else np.concatenate(chunks)


class ScanBatch(_Batch):
    """The batch of the per-interval kernel (msocr_jpeg_entropy_decode_device).  `pages[i]` = -1: no restart interval, or a marker
    sequence the host decoder must judge.  `page_base` is [n_pages][2]."""
    _sync = False

    def __init__(self, parsed, prepared=None, bytes_=None):
        self.max_intervals = 0
        super().__init__(parsed, prepared, bytes_)

    def _page(self, bounds):
        self.max_intervals = max(self.max_intervals, len(bounds) // 2)
        return ()


def _upload(batch, device, bytes_dev, *more):
    """What the two device stages share: the batch's file bytes on the device (uploaded unless `bytes_dev` already holds them),
    its descriptors, interval bounds, page bases and the arrays in `more`, and fresh coefficient and status tensors
    -> (bytes, [descs, bounds, page_base, *more], coef, status)."""
    import torch
    if bytes_dev is None:
        bytes_dev = torch.from_numpy(batch.bytes).pin_memory().to(device, non_blocking=True)
    tables = [torch.from_numpy(a).to(device) for a in (batch.descs, batch.bounds, batch.page_base) + more]
    coef = torch.empty(batch.coef_total, dtype=torch.int16, device=device)
    status = torch.empty(batch.n_pages, dtype=torch.int32, device=device)
    return bytes_dev, tables, coef, status


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
    from . import ops
    bytes_dev, (descs, bounds, base), coef, status = _upload(batch, device, bytes_dev)
    nat.check(nat.lib().msocr_jpeg_entropy_decode_device(bytes_dev.data_ptr(), descs.data_ptr(), batch.n_pages, batch.max_intervals,
                                                          bounds.data_ptr(), base.data_ptr(), coef.data_ptr(), batch.coef_total,
                                                          status.data_ptr(), ops._stream()), "jpeg_entropy_decode_device")
    return coef, status


SYNC_SUBSEQ_BYTES = 256    # a few times the distance page-like streams need to fall into step
SYNC_MAX_ROUNDS = 16
SYNC_MAX_FILE = 0x1ff00000  # the stage keeps bit positions in 32 bits
# The longest restart interval (bytes) the per-interval kernel takes by default: one thread decodes an interval, and its serial
# chain loses to a host core when the interval is long (1.8 ms per KB of interval on the device against ~15 ms per 1.6 MB file on
# a host core).  Longer intervals, like streams without a restart interval, take the self-synchronising stage by default:
# profiles/jpeg_sync_huffman.txt measured it at 6.4-7.0 ms per batch of 16 pages against 14.9-18.1 ms for the
# host pool.
DEVICE_MAX_INTERVAL = 8192


class SyncBatch(_Batch):
    """`ScanBatch` for the self-synchronising Huffman stage (msocr_jpeg_entropy_decode_sync_device): takes streams with and without
    a restart interval and lays out, beside descriptors / interval bounds / bytes, the subsequences of `subseq_bytes` bytes every
    interval is cut into (`sub_first`, `page_base` [n_pages][4], `max_subseq`, `total_subseq`).  `pages[i]` = -1: a marker sequence
    the host decoder must judge, a file too large for 32-bit bit positions."""
    _sync = True
    _max_file = SYNC_MAX_FILE

    def __init__(self, parsed, prepared=None, bytes_=None, subseq_bytes=SYNC_SUBSEQ_BYTES):
        self.subseq_bytes = int(subseq_bytes)
        self.max_subseq = self.total_subseq = 0
        self._sub_first = []
        super().__init__(parsed, prepared, bytes_)
        if self.n_pages:
            self.sub_first = np.concatenate(self._sub_first)
        del self._sub_first

    def _page(self, bounds):
        length = bounds[1::2].astype(np.int64) - bounds[0::2].astype(np.int64)
        nsub = np.maximum(1, -(-length // self.subseq_bytes))
        self._sub_first.append((np.cumsum(nsub) - nsub).astype(np.uint32))
        nsub = int(nsub.sum())
        row = (self.total_subseq, nsub)
        self.total_subseq += nsub
        self.max_subseq = max(self.max_subseq, nsub)
        return row


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
    bytes_dev, (descs, bounds, base, sub), coef, status = _upload(batch, device, bytes_dev, batch.sub_first)
    rounds = torch.empty(batch.n_pages, dtype=torch.int32, device=device)
    lib = nat.lib()
    ws = torch.empty(int(lib.msocr_jpeg_sync_workspace_bytes(batch.total_subseq, batch.n_pages, int(max_rounds))), dtype=torch.uint8,
                     device=device)
    nat.check(lib.msocr_jpeg_entropy_decode_sync_device(bytes_dev.data_ptr(), descs.data_ptr(), batch.n_pages, bounds.data_ptr(),
                                                        sub.data_ptr(), base.data_ptr(), batch.max_subseq, batch.total_subseq,
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


def route(restart, longest_interval, size, interval_ok, sync_ok, device_entropy):
    """Which Huffman decoder a file takes: "interval" (the per-interval kernel), "sync" (the self-synchronising stage) or "host"
    (the serial decoder on the host pool).  The one place that knows the table in `read_images_device`'s docstring.
    restart: the stream has a restart interval; longest_interval: its longest interval in bytes; size: the file's bytes;
    interval_ok / sync_ok: the marker walk of that stage accepted the stream; device_entropy: False / True / None (default)."""
    if device_entropy is False:
        return "host"
    sync = "sync" if sync_ok and size <= SYNC_MAX_FILE else "host"
    if not (restart and interval_ok):
        return sync
    if device_entropy is None and longest_interval > DEVICE_MAX_INTERVAL:
        return sync
    return "interval"


_POOL = None
_SLOTS = {}   # slot -> [pinned tensor, event of the last upload from it]; reused across batches (one reader thread at a time)


def _pool():
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor

        # one process per GPU: the ranks of a node share its cores (LOCAL_WORLD_SIZE is set by torch.distributed.run)
        share = (os.cpu_count() or 2) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(32, share - 1)), thread_name_prefix="msocr-jpeg")
    return _POOL


def _slot_buffer(slot, n, torch, dtype=None):
    """The pinned buffer of `slot` with room for n elements; slot None: a fresh pageable one that nobody shares."""
    if slot is None:
        return [torch.empty(n, dtype=dtype or torch.int16), None]
    ent = _SLOTS.get(slot)
    if ent is None or ent[0].numel() < n:
        ent = _SLOTS[slot] = [torch.empty(n + n // 4, dtype=dtype or torch.int16).pin_memory(), None]
    elif ent[1] is not None:
        ent[1].synchronize()   # the previous batch's upload from this buffer has left the host
    return ent


def _stream(ptr, n, base, walks):
    """Header parse and marker walks of the stream of n bytes at `ptr`, `base` bytes into its batch buffer
    -> (info, per-interval `_prepare` result or None, self-synchronising one or None, Exif orientation) or None."""
    info, orient = _parse_at(ptr, n, strict=False)
    if info is None:
        return None
    if not walks:
        return info, None, None, orient
    iv = _prepare(ptr, n, info, base, sync=False)
    if iv is not None or n > SYNC_MAX_FILE:
        # with a restart interval the two walks are one walk and give one descriptor
        return info, iv, (iv if n <= SYNC_MAX_FILE else None), orient
    # no restart interval (or a marker sequence both walks refuse): the self-synchronising stage's view of the stream
    return info, None, _prepare(ptr, n, info, base, sync=True), orient


def _load(path, arr, off, n, walks):
    """Worker: file -> its slice of the pinned batch buffer, then `_stream`; None for a file that cannot be read / is no JPEG."""
    try:
        with open(path, "rb") as f:
            if f.readinto(memoryview(arr[off: off + n])) != n:
                return None
    except OSError:
        return None
    if n < 4 or arr[off] != 0xFF or arr[off + 1] != 0xD8:
        return None
    return _stream(arr.ctypes.data + off, n, off, walks)


def _load_batch(paths, walks, torch):
    """Lays the files out in ONE pinned batch buffer (16-byte aligned slices, reused across batches) and reads + parses + walks
    them on the pool -> (buffer entry, offsets, sizes, total bytes, `_stream` result per file) or None for a batch without files."""
    sizes = [os.path.getsize(p) if isinstance(p, (str, os.PathLike)) and os.path.isfile(p) else -1 for p in paths]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (max(n, 0) + 15) // 16 * 16
    if total == 0:
        return None
    ent = _slot_buffer("bytes", total, torch, torch.uint8)
    arr = ent[0].numpy()
    jobs = [(_pool().submit(_load, p, arr, o, n, walks) if n >= 0 else None) for p, o, n in zip(paths, offs, sizes)]
    return ent, offs, sizes, total, [j.result() if j is not None else None for j in jobs]


def _routes(streams, sizes, device_entropy):
    out = []
    for s, n in zip(streams, sizes):
        if s is None:
            out.append(None)
            continue
        iv = s[1]
        longest = int((iv[1][1::2] - iv[1][0::2]).max()) if iv is not None else 0
        # the per-interval walk refuses a stream without a restart interval: what it took has one
        out.append(route(iv is not None, longest, n, iv is not None, s[2] is not None, device_entropy))
    return out


def _device_stages(streams, routes, sizes, arr, upload, device, torch, ops):
    """Runs the Huffman stage of every file routed to the device — at most two launch sequences per batch — and its reconstruction
    -> ({file index: image tensor}, those indices in status order, status tensor or None).  `upload()` puts `arr` on the device."""
    parsed = [None if s is None else (s[0], None, n) for s, n in zip(streams, sizes)]
    runs = []                    # (batch, coefficient tensor, status tensor): both Huffman stages are queued before any reconstruction
    bytes_dev = None
    for cls, name, col, run in ((ScanBatch, "interval", 1, entropy_batch_device), (SyncBatch, "sync", 2, entropy_sync_batch_device)):
        prepared = [s[col] if r == name else None for s, r in zip(streams, routes)]
        batch = cls(parsed, prepared, arr) if any(p is not None for p in prepared) else None
        if batch is None or not batch.n_pages:
            continue
        if bytes_dev is None:
            bytes_dev = upload()
        runs.append((batch,) + tuple(run(batch, device, bytes_dev)[:2]))
    imgs, idx = {}, []
    for batch, coef, _ in runs:
        for i, k in enumerate(batch.pages):
            if k >= 0:
                info, base = batch.infos[k]
                imgs[i] = _reconstruct(info, coef[base:], device, torch, ops, streams[i][3])
                idx.append(i)
    return imgs, idx, (None if not runs else runs[0][2] if len(runs) == 1 else torch.cat([r[2] for r in runs]))


def _verdict(imgs, idx, status, defer, torch):
    """The kernels' per-page verdict, taken (the device path's one host wait) or deferred -> ({file index: tensor or None} of the
    files that are done with, `check_pending`'s argument or None)."""
    if status is None:
        return {}, None
    if defer:
        st_host = torch.empty(len(idx), dtype=torch.int32).pin_memory()
        st_host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return imgs, (st_host, ev, idx)
    # 1: a bad stream goes to the host reader, as the host decoder's verdict would send it; 2: declined, not judged: the host
    # stage decodes it
    return {i: (imgs[i] if st == 0 else None) for i, st in zip(idx, status.cpu().tolist()) if st != 2}, None


def _host_stage(streams, todo, offs, sizes, arr, pinned, device, torch, ops):
    """The serial decoder on the pool for the files in `todo`, one page per core, then their reconstruction -> {file index: tensor
    or None}.  pinned: decode into the per-slot PINNED coefficient buffers that live across batches (fresh 9 MB arrays per page made
    the threads serialise on page faults); else into fresh arrays (a caller that may not be the one reader thread).  This thread
    uploads and launches the reconstruction page by page as the decodes finish."""
    jobs = []
    for i in todo:
        info = streams[i][0]
        total = int(info.coef_total)
        slot = _slot_buffer(i if pinned else None, total, torch)   # main thread: allocation / pinning is not done from the workers
        jobs.append((i, info, total, slot, _pool().submit(_serial_decode, arr.ctypes.data + offs[i], sizes[i], info, slot[0].numpy()[:total])))
    out = {}
    for i, info, total, slot, job in jobs:
        if job.result() is None:
            out[i] = None
            continue
        coef_dev = slot[0][:total].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        out[i] = _reconstruct(info, coef_dev, device, torch, ops, streams[i][3])
    return out


def _decode_streams(streams, offs, sizes, arr, upload, pinned, device, device_entropy, defer_status):
    """Route, device stages + reconstruction, verdict, host stage for the rest: `streams[i]` = `_stream`'s result for the sizes[i]
    bytes at arr[offs[i]] -> (tensor or None per stream, pending verdict or None)."""
    import torch

    from . import ops
    routes = _routes(streams, sizes, device_entropy)
    imgs, idx, status = _device_stages(streams, routes, sizes, arr, upload, device, torch, ops)
    done, pending = _verdict(imgs, idx, status, defer_status, torch)
    todo = [i for i, s in enumerate(streams) if s is not None and i not in done]
    done.update(_host_stage(streams, todo, offs, sizes, arr, pinned, device, torch, ops))
    return [done.get(i) for i in range(len(streams))], pending


def decode_jpeg_device(data: bytes, device="cuda", device_entropy=True):
    """JPEG bytes -> u8 tensor on the device (current stream), [H, W, 3] or, for Exif orientations 5..8, [W, H, 3] — the page as
    read_image returns it — or None when the stream is not supported.  The one-stream case of `read_images_device`, with the
    "True" column of its table as the default: a stream with a restart interval takes the per-interval Huffman kernel, one
    without the self-synchronising stage (a stream that stage declines, status 2, goes on to the host decoder);
    `device_entropy=False`: the host decoder for every stream."""
    import torch
    arr = np.frombuffer(bytearray(data), dtype=np.uint8)
    upload = lambda: torch.from_numpy(arr).pin_memory().to(device, non_blocking=True)
    stream = _stream(arr.ctypes.data, len(data), 0, device_entropy is not False)
    return _decode_streams([stream], [0], [len(data)], arr, upload, False, device, device_entropy, False)[0][0]


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
    two launch sequences.  Routes (`route`; `device_entropy=True` / False force the device / the host):

        file                               False   True                  None (default)
        no restart interval                host    self-synchronising    self-synchronising
        intervals <= DEVICE_MAX_INTERVAL   host    per-interval kernel   per-interval kernel
        longer intervals                   host    per-interval kernel   self-synchronising

    Per-interval kernel (`entropy_batch_device`): one thread per restart interval.  Self-synchronising stage
    (`entropy_sync_batch_device`): one thread per SYNC_SUBSEQ_BYTES bytes of a serial segment; a file it cannot take (a marker
    sequence its walk refuses, more than SYNC_MAX_FILE bytes) goes to the host, and a page it declines (status 2: no fixed point
    within SYNC_MAX_ROUNDS rounds, or a truncated stream) is decoded by the host pool inside this call, as every page of the "host"
    column is (`_host_stage`).  The pixels are the same on every route.
    A file with an Exif orientation 2..8 takes the row of the table its restart intervals put it in, like an upright one: the
    orientation only changes the last write of its reconstruction (and the shape of its tensor: [W, H, 3] for 5..8).
    defer_status=True -> (list, pending): the device path's one host wait — the kernels' per-page verdict — is NOT taken here; the
    caller asks `check_pending(pending)` later (the pipeline does, when it waits for the detector anyway), so that submitting a
    batch never waits for the device; bad and declined pages are both reported there."""
    import torch
    batch = _load_batch(paths, device_entropy is not False, torch)
    if batch is None:
        return ([None] * len(paths), None) if defer_status else [None] * len(paths)
    ent, offs, sizes, total, streams = batch

    def upload():
        bytes_dev = ent[0][:total].to(device, non_blocking=True)
        ent[1] = torch.cuda.Event()
        ent[1].record()
        return bytes_dev
    out, pending = _decode_streams(streams, offs, sizes, ent[0].numpy(), upload, True, device, device_entropy, defer_status)
    return (out, pending) if defer_status else out


def read_image_device(path, device="cuda"):
    """File -> device RGB tensor through the JPEG path, or None (not a file / not a supported JPEG: use read_image)."""
    return read_images_device([path], device)[0]
