"""The self-synchronising Huffman stage (csrc/jpeg.hip: sync_round / sync_write, the functions jpeg_sync_*_kernel run) through its
HOST twin msocr_jpeg_entropy_decode_sync_host: one serial entropy-coded segment cut into subsequences that are decoded
independently, brought to the fixed point of their entry states in rounds, placed by a prefix sum and written with DC differences.
The checker is the serial host decoder (ingest.jpeg_coefficients), bit for bit, and PIL."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd import ingest, synth


def _pil_decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def _encode(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", **kw)
    return b.getvalue()


def _test_images():
    """The five images of test_jpeg_cpu._test_images."""
    rng = np.random.default_rng(5)
    page = synth.synth_page(3, 203, 317)[0]                      # odd sizes: partial MCUs on both axes
    noise = rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:97, 0:131]
    smooth = np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], axis=2).astype(np.uint8)
    tiny = rng.integers(0, 256, size=(3, 5, 3), dtype=np.uint8)
    narrow = rng.integers(0, 256, size=(40, 3, 3), dtype=np.uint8)
    return {"page": page, "noise": noise, "smooth": smooth, "tiny": tiny, "narrow": narrow}


def _parsed(data):
    info, buf = ingest._parse(data)
    return None if info is None else (info, buf, len(data))


def _streams():
    imgs = _test_images()
    datas = [_encode(arr, quality=q, subsampling=sub) for arr in imgs.values() for sub in (0, 1, 2) for q in (30, 75, 95)]
    datas.append(_encode(np.array(Image.fromarray(imgs["page"]).convert("L")), quality=85))      # grayscale
    datas.append(_encode(imgs["page"], quality=80, subsampling=2, optimize=True))
    datas.append(_encode(imgs["noise"], quality=90, subsampling=0, optimize=True))
    for rows in (1, 3):
        for name, sub in (("page", 2), ("smooth", 1), ("noise", 0)):
            datas.append(_encode(imgs[name], quality=85, subsampling=sub, restart_marker_rows=rows))
    return datas


@pytest.mark.parametrize("subseq_bytes", [16, 64, 256])
def test_sync_decode_equals_the_serial_decoder(subseq_bytes):
    """Every stream kind at subsequences so short that blocks straddle many boundaries.  Round cap = the number of subsequences of
    the longest page: subsequence r is final after round r, so that cap always reaches the fixed point."""
    datas = _streams()
    batch = ingest.SyncBatch([_parsed(d) for d in datas], subseq_bytes=subseq_bytes)
    assert batch.n_pages == len(datas) and all(k >= 0 for k in batch.pages)    # with and without a restart interval
    coef, status, rounds = ingest.entropy_sync_batch_host_twin(batch, max_rounds=max(2, batch.max_subseq))
    assert not status.any(), status
    for i, d in enumerate(datas):
        info, ref = ingest.jpeg_coefficients(d)
        base = batch.infos[i][1]
        assert np.array_equal(coef[base: base + int(info.coef_total)], ref), (i, subseq_bytes)
    if subseq_bytes < 256:
        assert int(rounds.max()) >= 3        # several rounds did happen
    # ... and through the reconstruction twin against PIL, for one of them
    info, base = batch.infos[4]
    out = np.empty((info.height, info.width, 3), dtype=np.uint8)
    page = np.ascontiguousarray(coef[base: base + int(info.coef_total)])
    nat.check(nat.lib().msocr_jpeg_reconstruct_host(ctypes.byref(info), page.ctypes.data, out.ctypes.data), "reconstruct")
    assert np.array_equal(out, _pil_decode(datas[4]))


def test_sync_decode_noise_needs_its_rounds_and_is_declined_without_them():
    """Noise at quality 100, 4:4:4, optimised tables: every block is full, no EOB realigns k, streams fall into step late.  With as
    many rounds as subsequences the result is the serial decoder's; with two rounds the page is declined (status 2), never wrong."""
    rng = np.random.default_rng(17)
    data = _encode(rng.integers(0, 256, size=(128, 160, 3), dtype=np.uint8), quality=100, subsampling=0, optimize=True)
    info, ref = ingest.jpeg_coefficients(data)
    batch = ingest.SyncBatch([_parsed(data)])
    assert batch.n_pages == 1 and batch.subseq_bytes == ingest.SYNC_SUBSEQ_BYTES and batch.max_subseq > 100
    coef, status, rounds = ingest.entropy_sync_batch_host_twin(batch, max_rounds=batch.max_subseq)
    assert status[0] == 0 and np.array_equal(coef, ref)
    coef, status, rounds = ingest.entropy_sync_batch_host_twin(batch, max_rounds=2)
    assert status[0] == 2


def _first_marker(data, start):
    """Offset of the first 0xFF behind `start` that is not followed by a stuffed 0x00 (len(data) when there is none)."""
    i = start
    while True:
        i = data.find(b"\xff", i)
        if i < 0:
            return len(data)
        if i + 1 < len(data) and data[i + 1] == 0:
            i += 2
            continue
        return i


def damaged_streams(n_random=70, seed=23):
    """One page stream without DRI and its damaged versions: (data, ends_early).  `ends_early`: truncated, or the damage put a marker
    into the entropy-coded data, so that the data ends before the stream's blocks do."""
    rng = np.random.default_rng(seed)
    base = _encode(_test_images()["page"], quality=80, subsampling=2)
    sos = base.index(b"\xff\xda")
    eoi = _first_marker(base, sos + 14)
    cases = [(base, False)]
    for _ in range(n_random):
        b = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(sos + 14, len(b) - 2))] = int(rng.integers(0, 256))
        b = bytes(b)
        cases.append((b, _first_marker(b, sos + 14) != eoi))
    cases.append((base[: sos + (len(base) - sos) // 2], True))                                  # truncated at half the scan
    mid = sos + (len(base) - sos) // 3
    cases.append((base[:mid] + b"\xff\xd9" + base[mid:], True))                                 # a marker in the data
    cases.append((base[:mid] + b"\xff\xd3" + base[mid:], True))
    return cases


def test_sync_decode_damaged_streams_get_the_host_decoders_verdict():
    """The page is bad exactly when the serial decoder refuses the stream; what a speculative decode meets never flags it.  A stream
    the serial decoder takes is decoded to the same bits, or declined — but only when its data ends early."""
    agree = refused = 0
    for data, ends_early in damaged_streams():
        pr = _parsed(data)
        if pr is None:
            continue
        ref = ingest.jpeg_coefficients(data)
        batch = ingest.SyncBatch([pr])
        assert batch.n_pages == 1
        coef, status, _ = ingest.entropy_sync_batch_host_twin(batch)
        if ref is None:
            assert status[0] != 0
            refused += 1
            continue
        assert status[0] in ((0, 2) if ends_early else (0,)), (status[0], ends_early)
        if status[0] == 0:
            assert np.array_equal(coef, ref[1])
            agree += 1
    assert agree >= 10 and refused >= 1, (agree, refused)


def test_sync_decode_host_twin_under_sanitizers(tmp_path):
    """Mutation fuzz of the twin (prepare step, rounds, write pass, DC sums) with AddressSanitizer + UBSan on the CPU build of
    csrc/jpeg.hip (tests/native/jpeg_sync_fuzz.cpp): damaged input must not make the decoder read outside the byte buffer or write
    outside the page's coefficient array.  GPU sanitizers are not available on the pool; the functions are the kernels' own."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "manuscript_ocr_amd", "csrc", "jpeg.hip")
    inc = os.path.join(root, "include")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, drv, exe = tmp_path / "jpeg_asan.o", tmp_path / "fuzz.o", tmp_path / "jpeg_sync_fuzz"
    host_san = [f for s in san for f in ("-Xarch_host", s)]
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", inc,
                           "-c", src, "-o", str(obj)])
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "--offload-arch=gfx950", "-I", inc, "-x", "hip",
                           "-c", os.path.join(root, "tests", "native", "jpeg_sync_fuzz.cpp"), "-o", str(drv)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", san[0], str(obj), str(drv), "-o", str(exe)])
    arr = _test_images()["page"][:96, :128]
    seeds = []
    for k, (q, sub, kw) in enumerate(((80, 2, {}), (90, 0, {"optimize": True}), (60, 1, {}), (85, 2, {"restart_marker_rows": 1}))):
        (tmp_path / f"s{k}.jpg").write_bytes(_encode(arr, quality=q, subsampling=sub, **kw))
        seeds.append(str(tmp_path / f"s{k}.jpg"))
    r = subprocess.run([str(exe), "600", *seeds], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert int(r.stdout.split("jpeg_sync_fuzz:")[1].split()[0]) > 100, r.stdout      # the twin did see damaged streams
    shutil.rmtree(tmp_path, ignore_errors=True)
