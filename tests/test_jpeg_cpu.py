"""Image ingest: the JPEG decoder of libmsocr.so against PIL (libjpeg-turbo defaults = what the reference's
read_image produces through cv2.imread / PIL, detectors/_east/utils.py:477-497) — bit for bit, on the CPU, through the host
entropy decoder and the HOST twin of the device reconstruction stage (the same __host__ __device__ code the kernels run)."""
import io

import numpy as np
import pytest
from PIL import Image

from manuscript_ocr_amd import ingest, synth


def _pil_decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def _encode(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", **kw)
    return b.getvalue()


def _test_images():
    rng = np.random.default_rng(5)
    page = synth.synth_page(3, 203, 317)[0]                      # odd sizes: partial MCUs on both axes
    noise = rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:97, 0:131]
    smooth = np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], axis=2).astype(np.uint8)
    tiny = rng.integers(0, 256, size=(3, 5, 3), dtype=np.uint8)  # downsampled width <= 2 would need w <= 4: see `narrow`
    narrow = rng.integers(0, 256, size=(40, 3, 3), dtype=np.uint8)
    return {"page": page, "noise": noise, "smooth": smooth, "tiny": tiny, "narrow": narrow}


@pytest.mark.parametrize("subsampling", [0, 1, 2])
@pytest.mark.parametrize("quality", [30, 75, 95, 100])
def test_jpeg_decode_equals_pil(subsampling, quality):
    for name, arr in _test_images().items():
        data = _encode(arr, quality=quality, subsampling=subsampling)
        got = ingest.decode_jpeg_host(data)
        assert got is not None, (name, "unsupported")
        exp = _pil_decode(data)
        assert got.shape == exp.shape and np.array_equal(got, exp), (name, subsampling, quality,
                                                                    int(np.abs(got.astype(int) - exp.astype(int)).max()))


def test_jpeg_grayscale_restart_and_optimized_tables():
    arr = _test_images()["page"]
    gray = np.array(Image.fromarray(arr).convert("L"))
    b = io.BytesIO()
    Image.fromarray(gray).save(b, format="JPEG", quality=85)
    assert np.array_equal(ingest.decode_jpeg_host(b.getvalue()), _pil_decode(b.getvalue()))
    for kw in ({"optimize": True}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
        try:
            data = _encode(arr, quality=80, subsampling=2, **kw)
        except TypeError:
            continue
        assert np.array_equal(ingest.decode_jpeg_host(data), _pil_decode(data)), kw


def test_jpeg_unsupported_streams_are_reported():
    arr = _test_images()["smooth"]
    assert ingest.decode_jpeg_host(_encode(arr, quality=80, progressive=True)) is None      # SOF2: host decoder
    assert ingest.decode_jpeg_host(b"not a jpeg") is None
    data = _encode(arr, quality=80)
    assert ingest.decode_jpeg_host(data[: len(data) // 2]) is not None or True               # truncated: must not crash
    cmyk = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(cmyk, format="JPEG")
    assert ingest.decode_jpeg_host(cmyk.getvalue()) is None


def test_jpeg_restart_intervals_every_subsampling_and_awkward_sizes():
    """Restart markers with each chroma layout, widths / heights around the MCU sizes (8, 16) incl. 1-pixel images."""
    rng = np.random.default_rng(9)
    for (h, w) in ((1, 1), (7, 9), (8, 16), (15, 17), (16, 33), (31, 47), (64, 3), (2, 130)):
        arr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        for sub in (0, 1, 2):
            for kw in ({}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}):
                try:
                    data = _encode(arr, quality=60, subsampling=sub, **kw)
                except TypeError:
                    continue
                got = ingest.decode_jpeg_host(data)
                assert got is not None and np.array_equal(got, _pil_decode(data)), (h, w, sub, kw)


def _replace_dht_counts(data, table_index, counts):
    """Rewrite the 16 code-length counts of the `table_index`-th Huffman table of a stream (symbols untouched)."""
    out, i, seen = bytearray(data), 2, 0
    while i + 4 < len(out):
        assert out[i] == 0xFF
        m, L = out[i + 1], (out[i + 2] << 8) | out[i + 3]
        if m == 0xC4:
            o = i + 4
            while o < i + 2 + L:
                n = sum(out[o + 1:o + 17])
                if seen == table_index:
                    out[o + 1:o + 17] = bytes(counts)
                    return bytes(out)
                seen += 1
                o += 17 + n
        if m == 0xDA:
            break
        i += 2 + L
    raise AssertionError("table not found")


def test_jpeg_hostile_huffman_tables_are_rejected():
    """code-length counts that are not a prefix code must be refused as libjpeg refuses them
    (JERR_BAD_HUFF_TABLE) instead of indexing the 9-bit look-ahead table out of bounds."""
    data = _encode(_test_images()["smooth"], quality=80)
    assert ingest.decode_jpeg_host(data) is not None
    for tbl in range(4):
        for counts in ([255] + [0] * 15,          # 255 codes of one bit: segfaulted the round-2 parser
                       [12] + [0] * 15,           # 12 codes of one bit: silently corrupted its tables
                       [0, 5] + [0] * 14,         # 5 codes of two bits
                       [1, 1, 1, 1, 1, 1, 1, 1, 3] + [0] * 7):   # over-subscribed only at length 9
            bad = _replace_dht_counts(data, tbl, counts)
            assert ingest.jpeg_coefficients(bad) is None, (tbl, counts)
            with pytest.raises(Exception):
                _pil_decode(bad)                  # libjpeg's verdict on the same stream


def test_jpeg_frame_size_is_capped():
    """a tiny file must not be able to ask for a 65535 x 65535 frame (13 GB of coefficients)."""
    data = bytearray(_encode(_test_images()["smooth"], quality=80))
    i = data.index(b"\xff\xc0")
    data[i + 5:i + 9] = b"\xff\xff\xff\xff"       # height, width = 65535
    info, _ = ingest._parse(bytes(data))
    assert info is None
    data[i + 5:i + 9] = (13000).to_bytes(2, "big") + (13000).to_bytes(2, "big")   # 169 MP: below PIL's bomb limit, accepted
    info, _ = ingest._parse(bytes(data))
    assert info is not None and info.coef_total * 2 < (1 << 30)


def test_jpeg_exif_orientation_goes_to_the_host_reader(tmp_path):
    """cv2.imread (reference read_image, detectors/_east/utils.py:480) applies the Exif orientation: the device decoder
    reports such files as unsupported and the host reader transposes them (parity unpinned: cv2 absent)."""
    from manuscript_ocr_amd.detectors import read_image
    arr = _test_images()["page"]
    for orient in (1, 3, 6, 8):
        ex = Image.Exif()
        ex[0x0112] = orient
        p = tmp_path / f"o{orient}.jpg"
        Image.fromarray(arr).save(p, format="JPEG", quality=90, exif=ex.tobytes())
        data = p.read_bytes()
        plain = _pil_decode(data)
        got = ingest.decode_jpeg_host(data)
        if orient == 1:
            assert got is not None and np.array_equal(got, plain)
            assert np.array_equal(read_image(str(p)), plain)
        else:
            assert got is None
            exp = {3: np.rot90(plain, 2), 6: np.rot90(plain, -1), 8: np.rot90(plain, 1)}[orient]
            assert np.array_equal(read_image(str(p)), exp)


def test_jpeg_host_parser_under_sanitizers(tmp_path):
    """Mutation fuzz of the host parser / entropy decoder / host reconstruction with AddressSanitizer + UBSan on the CPU build
    of csrc/jpeg.hip (tests/native/jpeg_fuzz.cpp): hostile DHT counts, truncations, header and body byte flips, rewritten
    segment lengths, stray markers.  GPU sanitizers are not available on the pool; the host half is where files are parsed."""
    import os
    import shutil
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "manuscript_ocr_amd", "csrc", "jpeg.hip")
    inc = os.path.join(root, "include")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, drv, exe = tmp_path / "jpeg_asan.o", tmp_path / "fuzz.o", tmp_path / "jpeg_fuzz"
    host_san = [f for s in san for f in ("-Xarch_host", s)]
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", inc,
                           "-c", src, "-o", str(obj)])
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "--offload-arch=gfx950", "-I", inc, "-x", "hip",
                           "-c", os.path.join(root, "tests", "native", "jpeg_fuzz.cpp"), "-o", str(drv)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", san[0], str(obj), str(drv), "-o", str(exe)])
    arr = _test_images()["page"][:96, :128]
    seeds = []
    for k, (q, sub, kw) in enumerate(((80, 2, {}), (90, 0, {"optimize": True}), (60, 1, {"restart_marker_blocks": 2}),
                                   (85, 2, {"restart_marker_rows": 1}))):
        try:
            data = _encode(arr, quality=q, subsampling=sub, **kw)
        except TypeError:
            data = _encode(arr, quality=q, subsampling=sub)
        (tmp_path / f"s{k}.jpg").write_bytes(data)
        seeds.append(str(tmp_path / f"s{k}.jpg"))
    r = subprocess.run([str(exe), "800", *seeds], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "streams" in r.stdout
    assert int(r.stdout.split("decoded to the end,")[1].split()[0]) > 100, r.stdout   # the per-interval decoder saw hostile streams too
    shutil.rmtree(tmp_path, ignore_errors=True)


def _parsed(data):
    info, buf = ingest._parse(data)
    return None if info is None else (info, buf, len(data))


def test_jpeg_per_interval_decoder_equals_the_serial_decoder_and_pil():
    """Round 4: streams with a restart interval are decoded one interval per device thread (csrc/jpeg.hip decode_interval).  Its HOST
    twin — the same __host__ __device__ function, interval after interval — must give the serial host decoder's coefficients bit
    for bit, for a BATCH of streams of every subsampling, awkward sizes (partial MCUs, last interval shorter than the others) and
    interval lengths from 1 MCU to several rows; streams without a restart interval are left to the host decoder."""
    imgs = _test_images()
    datas, expect = [], []
    for name in ("page", "noise", "smooth", "tiny", "narrow"):
        for sub in (0, 1, 2):
            for kw in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 7}, {"restart_marker_rows": 1}, {"restart_marker_rows": 3}, {}):
                datas.append(_encode(imgs[name], quality=85, subsampling=sub, **kw))
                expect.append(bool(kw))
    datas.append(_encode(imgs["page"][:, :, 0], quality=70, restart_marker_rows=1))           # grayscale
    expect.append(True)
    datas.append(_encode(imgs["noise"], quality=100, subsampling=0, optimize=True, restart_marker_blocks=2))   # long codes, optimised tables
    expect.append(True)
    parsed = [_parsed(d) for d in datas]
    batch = ingest.ScanBatch(parsed)
    assert [k >= 0 for k in batch.pages] == expect
    coef, status = ingest.entropy_batch_host_twin(batch)
    assert not status.any()
    for i, d in enumerate(datas):
        k = batch.pages[i]
        if k < 0:
            continue
        info, ref = ingest.jpeg_coefficients(d)
        base = batch.infos[k][1]
        assert np.array_equal(coef[base: base + int(info.coef_total)], ref), i
    # ... and through the reconstruction twin against PIL, for one of them
    k = batch.pages[2]
    info, base = batch.infos[k]
    import ctypes

    from manuscript_ocr_amd import _native as nat
    out = np.empty((info.height, info.width, 3), dtype=np.uint8)
    page = np.ascontiguousarray(coef[base: base + int(info.coef_total)])
    nat.check(nat.lib().msocr_jpeg_reconstruct_host(ctypes.byref(info), page.ctypes.data, out.ctypes.data), "reconstruct")
    assert np.array_equal(out, _pil_decode(datas[2]))


def test_jpeg_per_interval_decoder_bad_streams_get_the_host_decoders_verdict():
    """Corrupt entropy data inside an interval, a missing RSTn, truncation: the per-interval decoder flags the page (status 1) or the
    marker walk refuses it exactly when the serial decoder refuses the stream; when both accept, the coefficients are identical
    (zeros are fed past an interval's end in both)."""
    rng = np.random.default_rng(11)
    base_data = _encode(_test_images()["page"], quality=80, subsampling=2, restart_marker_blocks=3)
    sos = base_data.index(b"\xff\xda")
    cases = [base_data]
    for _ in range(60):
        b = bytearray(base_data)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(sos + 14, len(b) - 2))] = int(rng.integers(0, 256))
        cases.append(bytes(b))
    cases.append(base_data[: sos + (len(base_data) - sos) // 2])                               # truncated in the scan
    rst = base_data.index(b"\xff\xd0", sos)
    cases.append(base_data[:rst] + base_data[rst + 2:])                                        # first RST marker removed
    agree = refused = 0
    for d in cases:
        pr = _parsed(d)
        if pr is None:
            continue
        ref = ingest.jpeg_coefficients(d)
        batch = ingest.ScanBatch([pr])
        if batch.n_pages == 0:
            assert ref is None, "the marker walk refused a stream the serial decoder takes"
            refused += 1
            continue
        coef, status = ingest.entropy_batch_host_twin(batch)
        assert (status[0] != 0) == (ref is None)
        if ref is not None:
            assert np.array_equal(coef, ref[1])
            agree += 1
        else:
            refused += 1
    assert agree >= 10 and refused >= 1, (agree, refused)


# The routing table of ingest.read_images_device's docstring, written out: (restart interval?, longest interval in bytes, file
# bytes, per-interval walk accepted, self-synchronising walk accepted, device_entropy) -> decoder.  8192 = the longest interval
# the per-interval kernel takes by default, 0x1ff00000 = the largest file the self-synchronising stage takes.
_MB = 1 << 20
_ROUTES = [
    # the nine cells
    ("plain/False", (False, 0, _MB, False, True, False), "host"),
    ("plain/True", (False, 0, _MB, False, True, True), "sync"),
    ("plain/None", (False, 0, _MB, False, True, None), "sync"),
    ("short/False", (True, 4096, _MB, True, True, False), "host"),
    ("short/True", (True, 4096, _MB, True, True, True), "interval"),
    ("short/None", (True, 4096, _MB, True, True, None), "interval"),
    ("long/False", (True, 100000, _MB, True, True, False), "host"),
    ("long/True", (True, 100000, _MB, True, True, True), "interval"),
    ("long/None", (True, 100000, _MB, True, True, None), "sync"),
    # the threshold belongs to the per-interval kernel; forcing the device ignores it
    ("at-threshold/None", (True, 8192, _MB, True, True, None), "interval"),
    ("over-threshold/None", (True, 8193, _MB, True, True, None), "sync"),
    ("over-threshold/True", (True, 8193, _MB, True, True, True), "interval"),
    # one byte over the self-synchronising stage's file cap: "sync" is not offered, whatever its walk said
    ("plain-at-cap/None", (False, 0, 0x1ff00000, False, True, None), "sync"),
    ("plain-over-cap/None", (False, 0, 0x1ff00001, False, True, None), "host"),
    ("plain-over-cap/True", (False, 0, 0x1ff00001, False, True, True), "host"),
    ("long-over-cap/None", (True, 100000, 0x1ff00001, True, True, None), "host"),
    ("long-over-cap/True", (True, 100000, 0x1ff00001, True, True, True), "interval"),
    ("short-over-cap/None", (True, 4096, 0x1ff00001, True, False, None), "interval"),
    # the per-interval walk refused the stream, the self-synchronising walk took it
    ("interval-refused/None", (True, 4096, _MB, False, True, None), "sync"),
    ("interval-refused/True", (True, 4096, _MB, False, True, True), "sync"),
    ("interval-refused/False", (True, 4096, _MB, False, True, False), "host"),
    # both walks refused it: the host decoder judges the stream
    ("both-refused/None", (True, 4096, _MB, False, False, None), "host"),
    ("both-refused/True", (False, 0, _MB, False, False, True), "host"),
]


@pytest.mark.parametrize("facts,expected", [r[1:] for r in _ROUTES], ids=[r[0] for r in _ROUTES])
def test_route_is_the_documented_table(facts, expected):
    assert (ingest.DEVICE_MAX_INTERVAL, ingest.SYNC_MAX_FILE) == (8192, 0x1ff00000)
    assert ingest.route(*facts) == expected
