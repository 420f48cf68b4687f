"""Exif orientation on the device JPEG path, CPU half: the oriented parse entry (msocr_jpeg_parse_oriented_host), the permissive
re-parse of the entropy entries and the HOST twin of the oriented reconstruction (msocr_jpeg_reconstruct_oriented_host: the same
__host__ __device__ mapping and pixel arithmetic the kernels run).  The expected pixels are always this package's read_image
(PIL decode + ImageOps.exif_transpose); every comparison is exact equality of u8 arrays."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from manuscript_ocr_amd import ingest, synth
from manuscript_ocr_amd.detectors import read_image

TILE = 64   # edge of the transposing kernel's source tile (kOrientTile, csrc/jpeg.hip)


def _encode(arr, orientation=None, **kw):
    b = io.BytesIO()
    if orientation is not None:
        ex = Image.Exif()
        ex[0x0112] = orientation
        kw["exif"] = ex.tobytes()
    Image.fromarray(arr).save(b, format="JPEG", **kw)
    return b.getvalue()


def _pil_plain(data):
    """PIL's decode as stored: no transpose."""
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def _by_the_table(a, o):
    """The issue's destination table applied with numpy: source pixel (X, Y) of the stored W x H frame -> out[row, col]."""
    if o == 1:
        return a
    H, W = a.shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    row = {2: Y, 3: H - 1 - Y, 4: H - 1 - Y, 5: X, 6: X, 7: W - 1 - X, 8: W - 1 - X}[o]
    col = {2: W - 1 - X, 3: W - 1 - X, 4: X, 5: Y, 6: H - 1 - Y, 7: H - 1 - Y, 8: Y}[o]
    out = np.empty((W, H, 3) if o >= 5 else (H, W, 3), dtype=a.dtype)
    out[row, col] = a
    return out


def _hand_exif(order, orientation, typ=3, count=1):
    """An APP1 segment with a one-entry IFD0 written by hand in byte order `order` ('II' / 'MM')."""
    e = "little" if order == "II" else "big"
    u16, u32 = (lambda v: int(v).to_bytes(2, e)), (lambda v: int(v).to_bytes(4, e))
    tiff = order.encode() + u16(42) + u32(8) + u16(1) + u16(0x0112) + u16(typ) + u32(count) + u16(orientation) + u16(0) + u32(0)
    body = b"Exif\0\0" + tiff
    return b"\xff\xe1" + (len(body) + 2).to_bytes(2, "big") + body


def _with_segments(data, *segments):
    """`data` (a JPEG without Exif) with APP1 segments spliced in right behind SOI."""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segments) + data[2:]


def _images():
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:97, 0:131]
    return {
        "page": synth.synth_page(3, 203, 317)[0],                                     # partial MCUs and partial tiles on both axes
        "noise": rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8),             # exactly one tile high
        "smooth": np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], axis=2).astype(np.uint8),
        "narrow": rng.integers(0, 256, size=(40, 3, 3), dtype=np.uint8),
        "tiny": rng.integers(0, 256, size=(3, 5, 3), dtype=np.uint8),
        "one": rng.integers(0, 256, size=(1, 1, 3), dtype=np.uint8),
        "past_tile": rng.integers(0, 256, size=(TILE + 1, 2 * TILE + 1, 3), dtype=np.uint8),   # one row / column past whole tiles
    }


@pytest.mark.parametrize("sampling", [0, 1, 2, "gray"])
@pytest.mark.parametrize("orientation", [1, 2, 3, 4, 5, 6, 7, 8])
def test_oriented_host_decode_equals_read_image(tmp_path, orientation, sampling):
    for name, arr in _images().items():
        if sampling == "gray":
            data = _encode(np.array(Image.fromarray(arr).convert("L")), orientation, quality=85)
        else:
            data = _encode(arr, orientation, quality=90, subsampling=sampling)
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        exp = read_image(str(p))
        got = ingest.decode_jpeg_oriented_host(data)
        assert got is not None, (name, "refused")
        assert got.shape == exp.shape and np.array_equal(got, exp), (name, orientation, sampling)
        # independently of exif_transpose: the destination table applied to PIL's plain decode
        assert np.array_equal(got, _by_the_table(_pil_plain(data), orientation)), (name, orientation, sampling)
        H, W = arr.shape[:2]
        assert got.shape == ((W, H, 3) if orientation >= 5 else (H, W, 3))


def test_exif_in_both_byte_orders(tmp_path):
    """PIL writes one byte order; the other is built by hand (and the first one too, so that both hand-built forms are pinned)."""
    arr = _images()["page"]
    plain = _encode(arr, quality=88, subsampling=2)
    seen = set()
    pil_written = _encode(arr, 6, quality=88, subsampling=2)
    at = pil_written.index(b"Exif\0\0")
    seen.add(pil_written[at + 6: at + 8])
    for order in ("II", "MM"):
        for o in range(1, 9):
            data = _with_segments(plain, _hand_exif(order, o))
            seen.add(data[data.index(b"Exif\0\0") + 6:][:2])
            info, _, got_o = ingest._parse_oriented(data)
            assert info is not None and got_o == o, (order, o, got_o)
            p = tmp_path / f"{order}{o}.jpg"
            p.write_bytes(data)
            exp = read_image(str(p))
            assert exp.shape == ((317, 203, 3) if o >= 5 else (203, 317, 3))     # PIL honours the hand-built block
            assert np.array_equal(ingest.decode_jpeg_oriented_host(data), exp), (order, o)
    assert seen == {b"II", b"MM"}


def test_values_outside_2_to_8_and_no_exif_are_upright(tmp_path):
    arr = _images()["smooth"]
    plain = _encode(arr, quality=80, subsampling=1)
    cases = {"none": plain}
    for v in (0, 1, 9):
        cases[f"pil{v}"] = _encode(arr, v, quality=80, subsampling=1)
        cases[f"mm{v}"] = _with_segments(plain, _hand_exif("MM", v))
    cases["unreadable"] = _with_segments(plain, b"\xff\xe1\x00\x10Exif\0\0MM\x00\x2a\xff\xff\xff\xff")   # IFD offset past the end
    for name, data in cases.items():
        info, _, o = ingest._parse_oriented(data)
        assert info is not None and o == 1, (name, o)
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        got = ingest.decode_jpeg_oriented_host(data)
        assert np.array_equal(got, _pil_plain(data)) and np.array_equal(got, read_image(str(p))), name
        assert np.array_equal(got, ingest.decode_jpeg_host(data)), name       # orientation 1 is the upright reconstruction itself


def test_oriented_parse_reports_the_tag_and_refuses_two_exif_segments():
    import ctypes

    from manuscript_ocr_amd import _native as nat
    arr = _images()["noise"]
    plain = _encode(arr, quality=85)
    strict, _ = ingest._parse(plain)
    for o in range(1, 9):
        data = _encode(arr, o, quality=85)
        info, _, got = ingest._parse_oriented(data)
        assert info is not None and got == o
        # the geometry is the frame header's, whatever the orientation: same layout as the strict entry gives for the bare stream
        assert (info.width, info.height, info.coef_total) == (strict.width, strict.height, strict.coef_total) == (80, 64, strict.coef_total)
    for a, b in ((1, 1), (1, 6), (6, 1), (6, 6)):
        data = _with_segments(plain, _hand_exif("MM", a), _hand_exif("II", b))
        assert ingest._parse_oriented(data)[0] is None, (a, b)
        assert ingest.decode_jpeg_oriented_host(data) is None
    # an APP1 segment that is not Exif (XMP) beside one Exif segment is not a second one
    xmp = b"http://ns.adobe.com/xap/1.0/\0<x/>"
    data = _with_segments(plain, b"\xff\xe1" + (len(xmp) + 2).to_bytes(2, "big") + xmp, _hand_exif("II", 8))
    assert ingest._parse_oriented(data)[2] == 8
    # argument checks of the new entries
    info, buf, _ = ingest._parse_oriented(plain)
    lib = nat.lib()
    assert lib.msocr_jpeg_parse_oriented_host(ctypes.addressof(buf), len(plain), ctypes.byref(info), None) != 0
    coef = ingest.jpeg_coefficients(plain)[1]
    out = np.empty((64, 80, 3), dtype=np.uint8)
    for bad in (0, 9, -1):
        assert lib.msocr_jpeg_reconstruct_oriented_host(ctypes.byref(info), bad, coef.ctypes.data, out.ctypes.data) == -1


def test_entropy_stages_take_oriented_streams():
    """The entropy entries re-parse the stream: they must accept the `info` of the oriented parse.  Per-interval and
    self-synchronising host twins against the serial decoder, on oriented files with and without a restart interval."""
    import ctypes

    from manuscript_ocr_amd import _native as nat
    imgs = _images()
    datas = []
    for o in (3, 6, 8, 5):
        for name, sub in (("page", 2), ("smooth", 1), ("noise", 0)):
            datas.append(_encode(imgs[name], o, quality=85, subsampling=sub))
            datas.append(_encode(imgs[name], o, quality=85, subsampling=sub, restart_marker_rows=1))
            datas.append(_encode(imgs[name], o, quality=85, subsampling=sub, restart_marker_blocks=3))
    parsed, serial = [], []
    for d in datas:
        info, buf, o = ingest._parse_oriented(d)
        assert info is not None and o in (3, 5, 6, 8)
        coef = np.empty(int(info.coef_total), dtype=np.int16)
        assert nat.lib().msocr_jpeg_entropy_decode_host(ctypes.addressof(buf), len(d), ctypes.byref(info), coef.ctypes.data) == 0
        parsed.append((info, buf, len(d)))
        serial.append(coef)
    scan = ingest.ScanBatch(parsed)
    assert [k >= 0 for k in scan.pages] == [i % 3 != 0 for i in range(len(datas))]
    coef, status = ingest.entropy_batch_host_twin(scan)
    assert not status.any()
    for i, k in enumerate(scan.pages):
        if k >= 0:
            info, base = scan.infos[k]
            assert np.array_equal(coef[base: base + int(info.coef_total)], serial[i]), i
    sync = ingest.SyncBatch(parsed)
    assert sync.n_pages == len(datas)
    coef, status, _ = ingest.entropy_sync_batch_host_twin(sync)
    assert not status.any()
    for i, k in enumerate(sync.pages):
        info, base = sync.infos[k]
        assert np.array_equal(coef[base: base + int(info.coef_total)], serial[i]), i


def test_read_and_parse_takes_oriented_files(tmp_path):
    p = tmp_path / "o6.jpg"
    p.write_bytes(_encode(_images()["page"], 6, quality=90))
    r = ingest._read_and_parse(str(p))
    assert r is not None and (r[0].height, r[0].width) == (203, 317) and r[2] == p.stat().st_size


def test_pipeline_shape_of_is_the_oriented_shape(tmp_path):
    from manuscript_ocr_amd import Pipeline
    arr = _images()["page"]
    for o in range(0, 10):
        p = tmp_path / f"o{o}.jpg"
        p.write_bytes(_encode(arr, o, quality=90))
        want = (317, 203) if o in (5, 6, 7, 8) else (203, 317)
        assert Pipeline._shape_of(str(p)) == want, o
        assert Pipeline._shape_of(str(p)) == read_image(str(p)).shape[:2], o
    p = tmp_path / "bare.jpg"
    p.write_bytes(_encode(arr, quality=90))
    assert Pipeline._shape_of(str(p)) == (203, 317)
    p = tmp_path / "o6.png"                                       # read_image transposes every format PIL finds the tag in
    ex = Image.Exif()
    ex[0x0112] = 6
    Image.fromarray(arr).save(p, exif=ex.tobytes())
    assert Pipeline._shape_of(str(p)) == read_image(str(p)).shape[:2]
    assert Pipeline._shape_of(arr) == (203, 317)


def test_oriented_host_path_under_sanitizers(tmp_path):
    """ASan + UBSan on the host side of csrc/jpeg.hip (tests/native/jpeg_orient_fuzz.cpp): oriented parse -> host entropy decode ->
    oriented host reconstruction into buffers of exactly 3 * W * H bytes, on all eight orientations at odd sizes and on mutated
    Exif segments (flipped bytes, rewritten lengths, IFD offsets and entry counts past the end, doubled segments)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "manuscript_ocr_amd", "csrc", "jpeg.hip")
    inc = os.path.join(root, "include")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, drv, exe = tmp_path / "jpeg_asan.o", tmp_path / "fuzz.o", tmp_path / "jpeg_orient_fuzz"
    host_san = [f for s in san for f in ("-Xarch_host", s)]
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", inc,
                           "-c", src, "-o", str(obj)])
    subprocess.check_call([hipcc, "-O1", "-g", *host_san, "-std=c++17", "--offload-arch=gfx950", "-I", inc, "-x", "hip",
                           "-c", os.path.join(root, "tests", "native", "jpeg_orient_fuzz.cpp"), "-o", str(drv)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", san[0], str(obj), str(drv), "-o", str(exe)])
    rng = np.random.default_rng(29)
    seeds = []
    for o in range(1, 9):
        h, w = [(67, 131), (131, 67), (9, 71), (65, 65)][o % 4]
        arr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        kw = [{}, {"restart_marker_blocks": 2}, {"optimize": True}][o % 3]
        plain = _encode(arr, quality=80, subsampling=o % 3, **kw)
        data = _encode(arr, o, quality=80, subsampling=o % 3, **kw) if o % 2 else _with_segments(plain, _hand_exif("MM", o))
        (tmp_path / f"s{o}.jpg").write_bytes(data)
        seeds.append(str(tmp_path / f"s{o}.jpg"))
    r = subprocess.run([str(exe), "300", *seeds], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "orientations of the seeds: 12345678" in r.stdout, r.stdout
    assert int(r.stdout.split("reconstructed,")[0].split()[-1]) > 300, r.stdout      # mutated streams reached the remap too
    shutil.rmtree(tmp_path, ignore_errors=True)
