"""The envelope of the JPEG ingest kernels (csrc/jpeg.hip), CPU half: the case builders test_gpu_jpeg_envelope.py imports, and the
proof that every case is what it claims to be.  A case is chosen for device-only structure of a kernel — the lane packing of
jpeg_huffman_kernel, the 2048-element scan steps and carries of jpeg_sync_place_kernel / jpeg_sync_dc_kernel, the 256-subsequence
grid split of the round and write kernels, the grid-stride loop of jpeg_color_kernel, the 64 x 64 tiles of
jpeg_color_transpose_kernel, the edge branches of chroma_at, the ends of idct_range_limit — so this file asserts the numbers that
put it there (interval counts, `lanes`, nsub, L, seg, pixel counts), that the serial decoder accepts the stream, and, for the
self-synchronising stage, that the host twin reaches status 0 with the serial decoder's coefficients: a case the twin declines
tests nothing of the place, write or DC kernels.  Every stream comes out of PIL's encoder; every comparison is exact.

Sync cases as measured on the host twin (S = subseq_bytes, rounds taken of the round cap, nsub = subsequences of the page):

    place frames (4:4:4, restart_marker_blocks=1, S 65536, cap 16): 120x136, 128x128, 8x2056, 184x712, 256x512, 24x5464
        -> nsub 255, 256, 257, 2047, 2048, 2049, 1 round each
    nonuniform "noise_plain" (512x640 noise, 4:4:4, quality 92, no restart interval, S 256, cap 16): nsub 2594, 10 rounds
    nonuniform "noise_plain_3steps" (640x1024 noise, else the same, cap 32): nsub 5188, 14 rounds
    nonuniform "noise_s16" (128x128 noise, 4:4:4, quality 92, restart_marker_blocks=1, S 16, cap 16): nsub 2232, 9 rounds
    DC cases (S 256, cap 16), name: nsub / rounds
        444_b1 5120 / 1, 420_b3 1278 / 3, 420_b512 973 / 10, 444_b2048 1873 / 6, 422_b700 1241 / 8, 422_b1100 1240 / 8,
        444_plain_L2047 891 / 7, 444_plain_L2048 890 / 7, 444_plain_L2049 882 / 7, 444_plain_L5120 1872 / 6, 420_plain 971 / 10,
        grey_plain 785 / 7, grey_b5 1024 / 1
    range ends (S 256, cap 64): the 16 streams with restart_marker_blocks=4 take 1 .. 10 rounds (nsub 5 .. 1040); the forms
        without a restart interval are sync cases only with the standard tables, and at quality 100 only at 64 x 80 (2 .. 46
        rounds, nsub 5 .. 106): the 203 x 317 ones take 50 .. 63 of the 64 rounds, and an optimised 4:4:4 quality-100 noise
        stream has no fixed point within 64 and is declined, as test_jpeg_sync_cpu.py shows for its like
    big frames (4099x4111, S 256, cap 16; the product route of the colour-stage test): grey nsub 10234, 3 rounds; 4:2:0 8847, 7
"""
import ctypes
import functools
import io

import numpy as np
import pytest
from PIL import Image, ImageFile

from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd import ingest, synth
from manuscript_ocr_amd.detectors import read_image


def encode(arr, orientation=None, **kw):
    """PIL's encoder -> bytes.  PIL sizes its output buffer from the frame; an optimised quality-100 noise stream is larger than
    that, so the buffer floor is raised for the call."""
    if orientation is not None:
        ex = Image.Exif()
        ex[0x0112] = orientation
        kw["exif"] = ex.tobytes()
    b = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 1 << 23)
    try:
        Image.fromarray(arr).save(b, format="JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return b.getvalue()


def pil_rgb(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def parsed(data):
    info, buf, _ = ingest._parse_oriented(data)
    assert info is not None
    return info, buf, len(data)


@functools.lru_cache(maxsize=None)
def reference(data):
    """(info, coefficients) of the serial decoder — the judge; computed once per stream and never written to."""
    info, buf, _ = ingest._parse_oriented(data)
    coef = ingest._serial_decode(ctypes.addressof(buf), len(data), info)
    assert coef is not None
    coef.setflags(write=False)
    return info, coef


def mixed_page(seed, h, w, frac=0.3):
    """A synthetic page with a fraction of its pixels replaced by noise: page-like statistics, no two alike."""
    rng = np.random.default_rng(seed)
    page = synth.synth_page(seed, h, w)[0].copy()
    m = rng.random((h, w)) < frac
    page[m] = rng.integers(0, 256, size=(int(m.sum()), 3), dtype=np.uint8)
    return page


def grey(arr):
    return np.array(Image.fromarray(arr).convert("L"))


def desc_scan(batch, k):
    """(restart_interval, mcus_x, mcus_y, n_intervals) as page k's descriptor holds them (ScanDesc of csrc/jpeg.hip: the info, an
    int64, then these four int32)."""
    off = ctypes.sizeof(nat.JpegInfo) + 8
    return tuple(int(v) for v in np.frombuffer(batch.descs[k][off: off + 16].tobytes(), dtype=np.int32))


def dc_scan(batch, k):
    """[(L, seg)] per component of page k: sync_dc_scan of csrc/jpeg.hip restated (L = the component's blocks in scan order, seg =
    those of one restart interval)."""
    info = batch.infos[k][0]
    ri, mx, my, _ = desc_scan(batch, k)
    out = []
    for c in range(info.ncomp):
        bpm = int(info.hs[c]) * int(info.vs[c])
        L = mx * my * bpm
        out.append((L, ri * bpm if ri > 0 else L))
    return out


# ------------------------------------------------------------------------------------------------ 1. lane packing
LANE_INTERVALS = 4096         # a 512 x 512 page at 4:4:4 with one MCU per restart interval
LANE_SET = (2, 4, 8, 16, 32)


def launch_lanes(n_cu, n_pages, max_intervals):
    """The launcher's rule (msocr_jpeg_entropy_decode_device): two wave slots per SIMD; lanes doubles while the batch has more
    intervals than slots x lanes."""
    lanes = 1
    while lanes < 64 and n_pages * max_intervals > 8 * n_cu * lanes:
        lanes *= 2
    return lanes


def pages_for_lanes(n_cu, lanes, intervals=LANE_INTERVALS):
    """The largest number of `intervals`-interval pages whose batch is launched with `lanes`, or None."""
    n = 8 * n_cu * lanes // intervals
    return n if n >= 1 and launch_lanes(n_cu, n, intervals) == lanes else None


@functools.lru_cache(maxsize=None)
def lane_page(k):
    return encode(mixed_page(100 + k, 512, 512, 0.05 * (k % 5)), quality=85, subsampling=0, restart_marker_blocks=1)


@functools.lru_cache(maxsize=None)
def ragged_pages():
    """The ragged batch: the three samplings plus grey, 4096 intervals beside 9."""
    return [
        ("444_4096", lane_page(0)),
        ("420_b1", encode(mixed_page(131, 512, 512, 0.2), quality=85, subsampling=2, restart_marker_blocks=1)),
        ("444_24x24", encode(mixed_page(132, 24, 24, 0.5), quality=85, subsampling=0, restart_marker_blocks=1)),
        ("422_rows1", encode(mixed_page(133, 203, 317, 0.2), quality=85, subsampling=1, restart_marker_rows=1)),
        ("grey_b1", encode(grey(mixed_page(134, 512, 512, 0.2)), quality=85, restart_marker_blocks=1)),
        ("420_rows1", encode(mixed_page(135, 333, 222, 0.2), quality=85, subsampling=2, restart_marker_rows=1)),
    ]


RAGGED_INTERVALS = [4096, 1024, 9, 26, 4096, 21]


def ragged_batch_datas(n_cu):
    """The ragged pages, then as many 4096-interval pages as the rule needs for lanes >= 8."""
    datas = [d for _, d in ragged_pages()]
    k = 1
    while launch_lanes(n_cu, len(datas), LANE_INTERVALS) < 8:
        datas.append(lane_page(k))
        k += 1
    return datas


def test_lane_pages_have_4096_intervals_and_the_batches_give_every_lanes():
    for lanes in LANE_SET:
        n = pages_for_lanes(256, lanes)
        assert n == lanes // 2
        batch = ingest.ScanBatch([parsed(lane_page(k)) for k in range(n)])
        assert batch.n_pages == n and batch.max_intervals == LANE_INTERVALS
        assert [desc_scan(batch, k)[3] for k in range(n)] == [LANE_INTERVALS] * n
        assert launch_lanes(256, batch.n_pages, batch.max_intervals) == lanes
    assert len({lane_page(k) for k in range(16)}) == 16
    # other CU counts: page counts follow from the rule (a chip so small that one page already packs 4 lanes has none for 2)
    for n_cu in (304, 512):
        assert all(pages_for_lanes(n_cu, lanes) for lanes in LANE_SET), n_cu
    # the serial decoder takes them, and the per-interval host twin agrees with it
    batch = ingest.ScanBatch([parsed(lane_page(k)) for k in range(2)])
    coef, status = ingest.entropy_batch_host_twin(batch)
    assert not status.any()
    for k in range(2):
        info, ref = reference(lane_page(k))
        assert np.array_equal(coef[batch.infos[k][1]: batch.infos[k][1] + int(info.coef_total)], ref)


def test_ragged_batch_is_ragged():
    datas = ragged_batch_datas(256)
    batch = ingest.ScanBatch([parsed(d) for d in datas])
    assert batch.n_pages == len(datas) and batch.max_intervals == LANE_INTERVALS
    n = len(RAGGED_INTERVALS)
    assert [desc_scan(batch, k)[3] for k in range(n)] == RAGGED_INTERVALS
    assert launch_lanes(256, batch.n_pages, batch.max_intervals) >= 8
    infos = [batch.infos[k][0] for k in range(n)]
    assert [(f.ncomp, f.hs[0], f.vs[0]) for f in infos] == [(3, 1, 1), (3, 2, 2), (3, 1, 1), (3, 2, 1), (1, 1, 1), (3, 2, 2)]
    coef, status = ingest.entropy_batch_host_twin(batch)
    assert not status.any()
    for k, d in enumerate(datas):
        info, ref = reference(d)
        assert np.array_equal(coef[batch.infos[k][1]: batch.infos[k][1] + int(info.coef_total)], ref), k


# ------------------------------------------------------------------------------------------------ 2. place kernel edges
PLACE_FRAMES = [(120, 136), (128, 128), (8, 2056), (184, 712), (256, 512), (24, 5464)]
PLACE_NSUB = [255, 256, 257, 2047, 2048, 2049]
PLACE_SUBSEQ = 65536          # longer than any one-MCU interval: every MCU is its own subsequence


@functools.lru_cache(maxsize=None)
def place_streams(restart=True):
    kw = {"restart_marker_blocks": 1} if restart else {}
    return [encode(mixed_page(10 + k, h, w), quality=92, subsampling=0, **kw) for k, (h, w) in enumerate(PLACE_FRAMES)]


@functools.lru_cache(maxsize=None)
def nonuniform_cases():
    """(name, stream, subseq_bytes, round cap): more than 2048 subsequences with block counts that differ."""
    rng = np.random.default_rng(1)
    big = rng.integers(0, 256, size=(512, 640, 3), dtype=np.uint8)
    small = rng.integers(0, 256, size=(128, 128, 3), dtype=np.uint8)
    wide = rng.integers(0, 256, size=(640, 1024, 3), dtype=np.uint8)
    return [("noise_plain", encode(big, quality=92, subsampling=0), 256, 16),
            ("noise_plain_3steps", encode(wide, quality=92, subsampling=0), 256, 32),    # > 4096: a carry made of two steps' sums
            ("noise_s16", encode(small, quality=92, subsampling=0, restart_marker_blocks=1), 16, 16)]


def sync_batch(datas, subseq_bytes=ingest.SYNC_SUBSEQ_BYTES):
    batch = ingest.SyncBatch([parsed(d) for d in datas], subseq_bytes=subseq_bytes)
    assert batch.n_pages == len(datas)
    return batch


def assert_twin_accepts(datas, subseq_bytes, max_rounds, what):
    """Status 0 on the host twin and the serial decoder's coefficients, for every page -> (batch, status, rounds)."""
    batch = sync_batch(datas, subseq_bytes)
    coef, status, rounds = ingest.entropy_sync_batch_host_twin(batch, max_rounds=max_rounds)
    print(what, "S", subseq_bytes, "nsub", batch.page_base[:, 3].tolist(), "rounds", rounds.tolist(), "status", status.tolist())
    assert not status.any(), (what, status)
    for k, d in enumerate(datas):
        info, ref = reference(d)
        assert np.array_equal(coef[batch.infos[k][1]: batch.infos[k][1] + int(info.coef_total)], ref), (what, k)
    return batch, status, rounds


def test_place_frames_have_the_stated_subsequence_counts():
    batch, _, rounds = assert_twin_accepts(place_streams(), PLACE_SUBSEQ, ingest.SYNC_MAX_ROUNDS, "place")
    assert batch.page_base[:, 3].tolist() == PLACE_NSUB
    assert batch.max_subseq == 2049 and batch.total_subseq == sum(PLACE_NSUB)
    assert [dc_scan(batch, k)[0] for k in range(6)] == [(n, 1) for n in PLACE_NSUB]       # one MCU per interval: seg 1
    alone = assert_twin_accepts(place_streams()[5:], PLACE_SUBSEQ, ingest.SYNC_MAX_ROUNDS, "place 2049 alone")[0]
    assert alone.page_base[:, 3].tolist() == [2049]


def test_nonuniform_cases_pass_2048_subsequences():
    for name, data, S, cap in nonuniform_cases():
        batch, _, rounds = assert_twin_accepts([data], S, cap, name)
        assert int(batch.page_base[0, 3]) > 2048, name
        assert int(rounds[0]) >= 3, name        # guessed entry states had to be corrected


# ------------------------------------------------------------------------------------------------ 3. DC kernel segments
@functools.lru_cache(maxsize=None)
def dc_cases():
    """(name, stream, [(L, seg)] per component)."""
    page = mixed_page(7, 512, 640, 0.1)
    plain = place_streams(False)
    return [
        ("444_b1", encode(page, quality=92, subsampling=0, restart_marker_blocks=1), [(5120, 1)] * 3),
        ("420_b3", encode(page, quality=92, subsampling=2, restart_marker_blocks=3), [(5120, 12), (1280, 3), (1280, 3)]),
        ("420_b512", encode(page, quality=92, subsampling=2, restart_marker_blocks=512), [(5120, 2048), (1280, 512), (1280, 512)]),
        ("444_b2048", encode(page, quality=92, subsampling=0, restart_marker_blocks=2048), [(5120, 2048)] * 3),
        ("422_b700", encode(page, quality=92, subsampling=1, restart_marker_blocks=700), [(5120, 1400), (2560, 700), (2560, 700)]),
        ("422_b1100", encode(page, quality=92, subsampling=1, restart_marker_blocks=1100), [(5120, 2200), (2560, 1100), (2560, 1100)]),
        ("444_plain_L2047", plain[3], [(2047, 2047)] * 3),
        ("444_plain_L2048", plain[4], [(2048, 2048)] * 3),
        ("444_plain_L2049", plain[5], [(2049, 2049)] * 3),
        ("444_plain_L5120", encode(page, quality=92, subsampling=0), [(5120, 5120)] * 3),
        ("420_plain", encode(page, quality=92, subsampling=2), [(5120, 5120), (1280, 1280), (1280, 1280)]),
        ("grey_plain", encode(grey(page), quality=92), [(5120, 5120)]),
        ("grey_b5", encode(grey(page), quality=92, restart_marker_blocks=5), [(5120, 5)]),
    ]


def test_dc_cases_have_the_stated_segments():
    cases = dc_cases()
    batch, _, _ = assert_twin_accepts([d for _, d, _ in cases], ingest.SYNC_SUBSEQ_BYTES, ingest.SYNC_MAX_ROUNDS, "dc")
    for k, (name, _, scan) in enumerate(cases):
        print(name, "L, seg per component:", dc_scan(batch, k))
        assert dc_scan(batch, k) == scan, name
    segs = {s for _, _, scan in cases for _, s in scan}
    assert 1 in segs and 2048 in segs and any(s % 8 for s in segs if s > 1)
    assert any(s > 2048 and s % 2048 and s < L for _, _, scan in cases for L, s in scan)   # a reset inside a later step
    assert {2047, 2048, 2049} <= {L for _, _, scan in cases for L, s in scan if s == L}
    assert any(L == s and L > 4096 for _, _, scan in cases for L, s in scan)


# ------------------------------------------------------------------------------------------------ 5. colour-stage grid stride
BIG = (4099, 4111)            # rows, columns: 16.85 M pixels
COLOR_GRID_PIXELS = 65535 * 256


@functools.lru_cache(maxsize=None)
def big_frames():
    """{name: {orientation: stream}}: a grey and a 4:2:0 frame above the colour kernels' grid, a gradient with flipped pixels.
    The frame is encoded once; the Exif segment PIL writes for the orientation is put behind SOI."""
    h, w = BIG
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int32)
    rgb = np.stack([(xx + yy) >> 4, (2 * xx + h - yy) >> 5, (xx + 3 * yy) >> 6], axis=2).astype(np.uint8)
    flip = rng.random((h, w)) < 0.01
    rgb[flip] = 255 - rgb[flip]
    out = {}
    for name, data in (("grey", encode(np.ascontiguousarray(rgb[:, :, 0]), quality=80)), ("420", encode(rgb, quality=80, subsampling=2))):
        ex = Image.Exif()
        ex[0x0112] = 3
        app1 = ex.tobytes()
        out[name] = {1: data, 3: data[:2] + b"\xff\xe1" + (len(app1) + 2).to_bytes(2, "big") + app1 + data[2:]}
    return out


def expected_image(tmp_path, data, name="e.jpg"):
    """read_image of the stream: PIL's pixels with the Exif orientation applied."""
    p = tmp_path / name
    p.write_bytes(data)
    return read_image(str(p))


def test_big_frames_exceed_the_colour_grid(tmp_path):
    assert BIG[0] * BIG[1] > COLOR_GRID_PIXELS
    for name, by_o in big_frames().items():
        info, coef = reference(by_o[1])
        assert (info.height, info.width) == BIG and info.ncomp == (1 if name == "grey" else 3)
        assert ingest._parse_oriented(by_o[3])[2] == 3 and ingest._parse_oriented(by_o[1])[2] == 1
        exp = expected_image(tmp_path, by_o[3])
        assert np.array_equal(exp, pil_rgb(by_o[1])[::-1, ::-1])
        assert np.array_equal(ingest.decode_jpeg_oriented_host(by_o[3]), exp), name


# ------------------------------------------------------------------------------------------------ 6. tile and chroma edges
EDGE_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
SAMPLINGS = (0, 1, 2, "gray")


@functools.lru_cache(maxsize=None)
def edge_case(h, w, sampling, orientation, restart):
    """Noise of h x w (chroma noise too: every upsampling branch shows in the pixels); restart: two MCUs per restart interval
    (the per-interval kernel's file), else none (the self-synchronising stage's)."""
    rng = np.random.default_rng(h * 1000 + w)
    arr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    kw = {"restart_marker_blocks": 2} if restart else {}
    if sampling == "gray":
        return encode(np.ascontiguousarray(arr[:, :, 1]), orientation, quality=90, **kw)
    return encode(arr, orientation, quality=90, subsampling=sampling, **kw)


def edge_sweep():
    """All 121 size pairs, upright, 4:2:0: (h, w, sampling, orientation)."""
    return [(h, w, 2, 1) for h in EDGE_SIZES for w in EDGE_SIZES]


def edge_cover(orientation):
    """Per sampling 11 pairs that hold every size once on each axis; the pairing shifts with orientation and sampling."""
    n = len(EDGE_SIZES)
    out = []
    for si, sampling in enumerate(SAMPLINGS):
        shift = ((orientation - 1) * len(SAMPLINGS) + si) % n
        out += [(EDGE_SIZES[i], EDGE_SIZES[(i + shift) % n], sampling, orientation) for i in range(n)]
    return out


def check_edge_cases(cases, decode, tmp_path):
    """`decode(stream)` == read_image of the stream's file, for both files of every case."""
    for h, w, sampling, o in cases:
        for restart in (False, True):
            data = edge_case(h, w, sampling, o, restart)
            exp = expected_image(tmp_path, data)
            assert exp.shape == ((w, h, 3) if o >= 5 else (h, w, 3))
            got = decode(data)
            assert got is not None and got.shape == exp.shape and np.array_equal(got, exp), (h, w, sampling, o, restart)


def test_edge_lists_cover_every_size_and_both_routes():
    assert len(set(edge_sweep())) == 121
    for o in range(1, 9):
        cover = edge_cover(o)
        for sampling in SAMPLINGS:
            mine = [c for c in cover if c[2] == sampling]
            assert sorted(c[0] for c in mine) == sorted(c[1] for c in mine) == list(EDGE_SIZES), (o, sampling)
    # the file with a restart interval is the per-interval kernel's, the one without the self-synchronising stage's
    for h, w in ((1, 1), (5, 129), (64, 64)):
        for restart, name in ((False, "sync"), (True, "interval")):
            data = edge_case(h, w, 2, 6, restart)
            arr = np.frombuffer(bytearray(data), dtype=np.uint8)
            stream = ingest._stream(arr.ctypes.data, len(data), 0, True)
            assert ingest._routes([stream], [len(data)], True) == [name] and stream[3] == 6


def test_edge_sweep_on_the_host_path(tmp_path):
    check_edge_cases(edge_sweep(), ingest.decode_jpeg_oriented_host, tmp_path)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_edge_cover_on_the_host_path(tmp_path, orientation):
    check_edge_cases(edge_cover(orientation), ingest.decode_jpeg_oriented_host, tmp_path)


# ------------------------------------------------------------------------------------------------ 7. range ends
RANGE_ROUNDS = 64


@functools.lru_cache(maxsize=None)
def range_cases():
    """(name, stream, takes the per-interval kernel, is a sync case): 0 / 255 noise at quality 100 and 1.  Every combination with
    four MCUs per restart interval (both device stages); the ones with the standard tables also without a restart interval."""
    rng = np.random.default_rng(2)
    out = []
    for zi, (h, w) in enumerate(((64, 80), (203, 317))):
        bw = (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
        for qi, q in enumerate((100, 1)):
            for si, sampling in enumerate(SAMPLINGS):
                arr, kw = (np.ascontiguousarray(bw[:, :, 0]), {}) if sampling == "gray" else (bw, {"subsampling": sampling})
                opt = bool((zi + qi + si) % 2)            # half of them; every sampling and quality gets both settings
                name = f"{h}x{w}_q{q}_{sampling}{'_opt' if opt else ''}"
                out.append((name + "_b4", encode(arr, quality=q, optimize=opt, restart_marker_blocks=4, **kw), True, True))
                if not opt and (zi == 0 or q == 1):     # (the 203 x 317 quality-100 streams take 50 .. 63 of the 64 rounds)
                    out.append((name + "_plain", encode(arr, quality=q, **kw), False, True))
    return out


def test_range_cases_reach_both_ends_of_the_sample_range():
    cases = range_cases()
    assert sum(1 for c in cases if c[2]) == 16 and sum(1 for c in cases if "_opt" in c[0]) == 8
    for name, data, interval, sync in cases:
        exp = pil_rgb(data)
        zero, full = float((exp == 0).mean()), float((exp == 255).mean())
        print(name, len(data), "bytes; pixels at 0: %.3f, at 255: %.3f" % (zero, full))
        if "_q100_" in name:
            assert zero >= 0.05 and full >= 0.05, name
        assert np.array_equal(ingest.decode_jpeg_host(data), exp), name
        assert (ingest.ScanBatch([parsed(data)]).n_pages == 1) == interval, name
    for name, data, _, _ in cases:        # one page per batch: each stream's own rounds
        assert_twin_accepts([data], ingest.SYNC_SUBSEQ_BYTES, RANGE_ROUNDS, name)


# ------------------------------------------------------------------------------------------------ info_ok: the sampling forms
def bad_sampling_infos():
    """(name, info, coefficients): infos no parse produces — h1v2 luma, 2 x 2 chroma — consistent in every other field."""
    out = []
    for name, hs, vs in (("h1v2", (1, 1, 1), (2, 1, 1)), ("chroma_2x2", (2, 2, 2), (2, 2, 2)), ("chroma_h2", (2, 2, 1), (1, 1, 1))):
        info = nat.JpegInfo()
        info.width, info.height, info.ncomp, info.supported = 32, 32, 3, 1
        off = 0
        for c in range(3):
            info.hs[c], info.vs[c] = hs[c], vs[c]
            info.blocks_w[c] = 32 // 8 * hs[c] // hs[0]
            info.blocks_h[c] = 32 // 8 * vs[c] // vs[0]
            info.coef_off[c] = off
            off += info.blocks_w[c] * info.blocks_h[c] * 64
            for k in range(64):
                info.quant[c][k] = 1
        info.coef_total = off
        out.append((name, info, np.zeros(off, dtype=np.int16)))
    return out


def test_reconstruct_host_refuses_sampling_forms_no_parse_produces():
    lib = nat.lib()
    E_ARG = -1                # MSOCR_E_ARG of include/msocr.h
    for name, info, coef in bad_sampling_infos():
        out = np.full((32, 32, 3), 0xA5, dtype=np.uint8)
        assert lib.msocr_jpeg_reconstruct_host(ctypes.byref(info), coef.ctypes.data, out.ctypes.data) == E_ARG, name
        for o in (1, 6):
            assert lib.msocr_jpeg_reconstruct_oriented_host(ctypes.byref(info), o, coef.ctypes.data, out.ctypes.data) == E_ARG, (name, o)
        assert lib.msocr_jpeg_workspace_bytes(ctypes.byref(info)) == -1, name
        assert (out == 0xA5).all(), name
    # the three forms a parse produces, written the same way, are taken
    for hs0, vs0 in ((1, 1), (2, 1), (2, 2)):
        info = bad_sampling_infos()[0][1]
        info.hs[0], info.vs[0] = hs0, vs0
        off = 0
        for c in range(3):
            info.blocks_w[c] = 4 * hs0 if c == 0 else 4
            info.blocks_h[c] = 4 * vs0 if c == 0 else 4
            info.coef_off[c] = off
            off += info.blocks_w[c] * info.blocks_h[c] * 64
        info.coef_total = off
        info.width, info.height = 32 * hs0, 32 * vs0
        out = np.empty((32 * vs0, 32 * hs0, 3), dtype=np.uint8)
        coef = np.zeros(off, dtype=np.int16)
        assert lib.msocr_jpeg_reconstruct_host(ctypes.byref(info), coef.ctypes.data, out.ctypes.data) == 0, (hs0, vs0)
        assert (out == 128).all()
