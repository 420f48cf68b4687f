"""Rectified word crops on the device (Pipeline.rectify_crops): msocr_quad_crop and
msocr_quad_crop_descriptors against their host twins, byte for byte, over the quad set of tests/test_quad_crop_cpu.py (which holds
the twins to a NumPy restatement of the definition); what the kernels refuse; and the Pipeline with the attribute set."""
import ctypes

import numpy as np
import pytest
import torch

from test_quad_crop_cpu import CANVASES, H, W, fallback_cases, lib_descriptors, make_pages, quad_cases, rect, tilt, window_of

pytestmark = pytest.mark.gpu

CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def pages():
    p = make_pages()
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def pages_dev(gpu, pages):
    return torch.from_numpy(pages.copy()).cuda()


def all_cases(img_h, img_w):
    """The quad set, the fallback cases and the eight stored orders of one tilted quad: about 40 crops over the two pages."""
    cases = quad_cases(img_h, img_w) + fallback_cases()
    q = tilt(rect(40, 36, 80, 24), 17).astype(np.float32)
    for k, v in enumerate([np.roll(q, -r, axis=0) for r in range(4)] + [np.roll(q[::-1], -r, axis=0) for r in range(4)]):
        cases.append((f"order_{k}", v, window_of(v, k % 2)))
    return cases


# ------------------------------------------------------------------------------------------- kernel against twin
@pytest.mark.parametrize("img_h,img_w", CANVASES)
def test_kernel_equals_host_twin(gpu, pages, pages_dev, img_h, img_w):
    from manuscript_ocr_amd import ops
    cases = all_cases(img_h, img_w)
    qdesc = lib_descriptors(cases, img_h, img_w)
    assert 35 <= len(qdesc) <= 48 and set(qdesc[:, 0].tolist()) == {0, 1}
    exp = ops.quad_crop_host(pages, qdesc, img_h, img_w)
    got = ops.quad_crop(pages_dev, qdesc, img_h, img_w).cpu().numpy()                                   # validated on the host
    resident = ops.quad_crop(pages_dev, None, img_h, img_w, qdesc_dev=torch.from_numpy(qdesc).cuda()).cpu().numpy()  # by the kernel
    for k, (name, _, _) in enumerate(cases):
        assert np.array_equal(got[k], exp[k]), (name, int(np.abs(got[k].astype(int) - exp[k]).max()))
        assert np.array_equal(resident[k], exp[k]), name
    assert len({c.tobytes() for c in exp}) > 25, "the cases draw different canvases"


def _broken(qdesc, img_h, img_w, n_pages):
    """Copies of descriptor 0 broken one field at a time -> [(what, descriptor)]."""
    out = []
    def put(what, idx, val):
        d = qdesc[0].copy()
        d[idx] = val
        out.append((what, d))
    put("page -1", 0, -1)
    put("page N", 0, n_pages)
    put("new_w 0", 9, 0)
    put("new_w > img_w", 9, img_w + 1)
    d = qdesc[0].copy()
    d[11] = img_h - d[10] + 1
    out.append(("y0 + new_h > img_h", d))
    put("y0 < 0", 11, -1)
    put("new_h 0", 10, 0)
    put("infinite corner", 3, np.array([np.inf], dtype=np.float32).view(np.int32)[0])
    put("nan corner", 8, np.array([np.nan], dtype=np.float32).view(np.int32)[0])
    return out


def test_device_validation(gpu, pages, pages_dev):
    """Every case here is one the kernel checks before it computes an address: refused by the wrapper when the host copy is given,
    a white canvas from the kernel otherwise, with the valid neighbours of the same launch exact."""
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    img_h, img_w = 32, 128
    cases = quad_cases(img_h, img_w)[:6]
    good = lib_descriptors(cases, img_h, img_w)
    exp = ops.quad_crop_host(pages, good, img_h, img_w)
    broken = _broken(good, img_h, img_w, len(pages))
    for what, d in broken:
        mixed = np.concatenate([good[:3], d[None], good[3:]])
        with pytest.raises(nat.NativeError):
            ops.quad_crop(pages_dev, mixed, img_h, img_w)
    mixed = np.concatenate([good[:3]] + [d[None] for _, d in broken] + [good[3:]])
    got = ops.quad_crop(pages_dev, None, img_h, img_w, qdesc_dev=torch.from_numpy(mixed).cuda()).cpu().numpy()
    nb = len(broken)
    assert np.array_equal(got[:3], exp[:3]) and np.array_equal(got[3 + nb:], exp[3:])
    for k, (what, _) in enumerate(broken):
        assert (got[3 + k] == 255).all(), what
    assert np.array_equal(ops.quad_crop_host(pages, mixed, img_h, img_w), got), "the host twin draws the same white canvases"


def test_c_abi_refuses_bad_arguments(gpu, pages_dev):
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    qd = torch.zeros((4, 12), dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 32, 128, 3), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, Q, O = pages_dev.data_ptr(), qd.data_ptr(), out.data_ptr()
    crop = lambda pages=P, N=2, qdesc=Q, M=4, img_h=32, img_w=128, canv=O: L.msocr_quad_crop(pages, N, H, W, qdesc, None, M, img_h, img_w, canv, st)
    assert crop(pages=None) == crop(qdesc=None) == crop(canv=None) == crop(M=0) == crop(img_w=0) == crop(N=0) == crop(img_h=0) == -1
    host = np.zeros((4, 12), dtype=np.int32)
    canv = np.zeros((4, 32, 128, 3), dtype=np.uint8)
    pg = np.zeros((2, H, W, 3), dtype=np.uint8)
    hcrop = lambda pages=pg.ctypes.data, N=2, qdesc=host.ctypes.data, M=4, img_w=128, c=canv.ctypes.data: \
        L.msocr_quad_crop_host(pages, N, H, W, qdesc, M, 32, img_w, c)
    assert hcrop(pages=None) == hcrop(qdesc=None) == hcrop(c=None) == hcrop(M=0) == hcrop(img_w=0) == hcrop(N=0) == -1
    i32 = torch.zeros((64,), dtype=torch.int32, device="cuda")
    f32 = torch.zeros((64 * 9,), dtype=torch.float32, device="cuda")
    I, F = i32.data_ptr(), f32.data_ptr()
    dk = lambda boxes=F, nbox=I, N=1, mc=4, img_w=128, order=I, keep=I, desc=I, ncrop=I, o=I: \
        L.msocr_quad_crop_descriptors(boxes, nbox, N, mc, 32, img_w, order, keep, desc, ncrop, o, st)
    assert dk(boxes=None) == dk(nbox=None) == dk(order=None) == dk(keep=None) == dk(desc=None) == dk(ncrop=None) == dk(o=None) == -1
    assert dk(N=0) == dk(mc=0) == dk(img_w=0) == -1
    assert L.msocr_quad_crop_descriptors_host(None, None, 1, 32, 128, 0, None) == -1
    assert L.msocr_quad_crop_descriptors_host(None, None, 0, 32, 128, 0, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- descriptor kernel
def _tilted_boxes(n, seed, page_hw):
    """n words as boxes [n,9] f32: tilted quads on a grid, every stored order and winding, a few duplicates, a few words under
    min_text_size."""
    rng = np.random.default_rng(seed)
    ph, pw = page_hw
    cols = 6
    out = []
    for k in range(n):
        cx, cy = 50 + (k % cols) * (pw - 100) / (cols - 1), 30 + (k // cols) * 42.0
        w, h = rng.uniform(40, 85), rng.uniform(12, 30)
        if k % 11 == 7:
            w, h = 2.5, 3.0  # under min_text_size = 5: ordered, but no crop
        q = tilt(rect(cx - w / 2, cy - h / 2, w, h), rng.uniform(-30, 30))
        if k % 3 == 1:
            q = q[::-1]
        q = np.roll(q, -(k % 4), axis=0)
        out.append(np.concatenate([q.reshape(8), [0.5 + 0.4 * rng.random()]]))
    out = np.asarray(out, dtype=np.float32)
    out[5] = out[2]    # duplicates: equal boxes re-match to the first word
    out[n - 1] = out[9]
    return out


@pytest.mark.parametrize("page_base", [0, 5])
def test_descriptor_kernel_equals_host_form(gpu, page_base):
    from manuscript_ocr_amd import ops
    page_hw, img_h, img_w, max_cand = (440, 640), 32, 128, 64
    counts = [47, 0, 58, 33]
    boxes = np.zeros((4, max_cand, 9), dtype=np.float32)
    for pg, n in enumerate(counts):
        if n:
            boxes[pg, :n] = _tilted_boxes(n, 100 + pg, page_hw)
    nbox = np.array(counts, dtype=np.int32)
    nbox[3] = -1  # a page the detector left to the host: ncrop = -1, nothing written
    boxes_d, nbox_d = torch.from_numpy(boxes).cuda(), torch.from_numpy(nbox).cuda()
    ro = ops.reading_order_crops(boxes_d, nbox_d, page_hw, 5, img_h, img_w, page_base=page_base)
    SENT = 0x5A5A5A5A
    out = torch.full((4, max_cand, 12), SENT, dtype=torch.int32, device="cuda")
    qd = ops.quad_crop_descriptors(boxes_d, nbox_d, ro, img_h, img_w, out=out).cpu().numpy()
    order, keep, desc, ncrop = (t.cpu().numpy() for t in ro)
    assert ncrop.tolist()[1] == 0 and ncrop.tolist()[3] == -1 and 30 <= ncrop[0] < 47 and 30 <= ncrop[2] < 58
    for pg, n in enumerate(counts):
        nc = int(ncrop[pg])
        if nc <= 0:
            assert (qd[pg] == SENT).all(), pg
            continue
        kept = [int(order[pg, pos]) for pos in range(n) if keep[pg, pos]]
        assert len(kept) == nc
        exp = ops.quad_descriptors(boxes[pg, kept, :8].reshape(-1, 4, 2), desc[pg, :nc], img_h, img_w)
        assert np.array_equal(qd[pg, :nc], exp), pg
        assert (qd[pg, :nc, 0] == page_base + pg).all() and (qd[pg, nc:] == SENT).all()
        # canonical order: the first edge points right, the polygon runs clockwise on screen
        c = qd[pg, :nc, 1:9].copy().view(np.float32).reshape(nc, 4, 2)
        assert (c[:, 1, 0] > c[:, 0, 0]).all() and (c[:, 2, 1] > c[:, 1, 1]).all()


def test_descriptor_kernel_across_scan_boundaries(gpu):
    """The kept words' ranks come from a workgroup scan: 63 / 64 / 65 words are the first prefix that crosses a wave, at 1023 /
    1024 / 1025 the chunk per thread goes 1 -> 2 (QDESC_T = 1024).  The expected words, windows and count come from the host
    side (msocr_reading_order_host + ops.crop_descriptors), not from the kernels' outputs.  The word ORDER comes from the host twin,
    which shares box_hit / box_shrink with reading_order_kernel through word_boxes.h: tests/test_host_cpu.py pins that twin to the
    reference's goldens; the windows, the filter and ncrop come from the NumPy restatement, which shares nothing."""
    from manuscript_ocr_amd import ops
    from manuscript_ocr_amd._pipeline import _reading_order
    page_hw, img_h, img_w, max_cand, min_text = (7300, 640), 32, 128, 1030, 5
    counts = [63, 64, 65, 1023, 1024, 1025, 0]  # the last page stays all sentinel
    N = len(counts)
    boxes = np.zeros((N, max_cand, 9), dtype=np.float32)
    for pg, n in enumerate(counts):
        if n:
            boxes[pg, :n] = _tilted_boxes(n, 200 + pg, page_hw)
    boxes_d, nbox_d = torch.from_numpy(boxes).cuda(), torch.from_numpy(np.array(counts, dtype=np.int32)).cuda()
    ro = ops.reading_order_crops(boxes_d, nbox_d, page_hw, min_text, img_h, img_w)
    SENT = 0x5A5A5A5A
    out = torch.full((N, max_cand, 12), SENT, dtype=torch.int32, device="cuda")
    qd = ops.quad_crop_descriptors(boxes_d, nbox_d, ro, img_h, img_w, out=out).cpu().numpy()
    ncrop = ro[3].cpu().numpy()
    for pg, n in enumerate(counts):
        if n == 0:
            assert ncrop[pg] == 0 and (qd[pg] == SENT).all()
            continue
        pts = boxes[pg, :n, :8].astype(np.int32).reshape(n, 4, 2)  # truncation toward zero
        aabb = np.concatenate([pts.min(axis=1), pts.max(axis=1)], axis=1)
        order = _reading_order(aabb)
        sized = [pos for pos, w in enumerate(order) if min(aabb[w, 2] - aabb[w, 0], aabb[w, 3] - aabb[w, 1]) >= min_text]
        desc, keep = ops.crop_descriptors(aabb[[order[pos] for pos in sized]], [pg] * len(sized), page_hw, img_h, img_w)
        kept_pos = [pos for pos, k in zip(sized, keep) if k]
        kept = [order[pos] for pos in kept_pos]
        nc = len(kept)
        assert 0 <= nc < n and kept_pos != list(range(nc)), "regime: some words filtered, so a kept word's rank != its position"
        assert int(ncrop[pg]) == nc
        exp = ops.quad_descriptors(boxes[pg, kept, :8].reshape(-1, 4, 2), desc, img_h, img_w)
        assert np.array_equal(qd[pg, :nc], exp), pg
        assert (qd[pg, nc:] == SENT).all(), pg


# ------------------------------------------------------------------------------------------- Pipeline
@pytest.fixture(scope="module")
def rec(gpu):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


PH, PW = 224, 320


def _pages_and_maps():
    from manuscript_ocr_amd import synth
    pgs, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, PH, PW, line_pitch=44, word_h=22, margin=14)
        quads = synth.synth_tilted_quads(rects, seed, max_deg=6.0)
        pgs.append(pg)
        maps.append(synth.synth_quad_maps(quads, (PH, PW), (PH // 4, PW // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pgs, mo


def _key(p):
    return [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words]


def _geometry(p):
    return [(w.polygon, w.detection_confidence, w.text is None) for w in p.blocks[0].words]


def _spy_quad_crop(monkeypatch, ops):
    seen = []
    real = ops.quad_crop

    def spy(pages_u8, qdesc_host, img_h, img_w, qdesc_dev=None):
        canv = real(pages_u8, qdesc_host, img_h, img_w, qdesc_dev=qdesc_dev)
        seen.append((qdesc_dev.cpu().numpy() if qdesc_dev is not None else np.array(qdesc_host), canv.cpu().numpy()))
        return canv

    monkeypatch.setattr(ops, "quad_crop", spy)
    return seen


def test_pipeline_rectify_crops(gpu, rec, monkeypatch):
    from manuscript_ocr_amd import Pipeline, ops, synth
    from manuscript_ocr_amd.detectors import EAST
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(PW, PH), device="cuda", axis_aligned_output=False), rec)
    pgs, mo = _pages_and_maps()
    assert not getattr(pipe, "rectify_crops", False)
    off = pipe.predict_batch(pgs, _maps_override=mo)
    n_text = sum(w.text is not None for p in off for w in p.blocks[0].words)
    assert n_text >= 8, n_text
    tilted = [w for p in off for w in p.blocks[0].words if abs(w.polygon[1][1] - w.polygon[0][1]) > 2.0]
    assert len(tilted) >= 4, "the injected maps decode to tilted quads"
    seen = _spy_quad_crop(monkeypatch, ops)
    pipe.rectify_crops = True
    on = pipe.predict_batch(pgs, _maps_override=mo)
    assert [_geometry(p) for p in on] == [_geometry(p) for p in off], "polygons, order, confidences and which words got a text"
    assert [_key(p) for p in on] != [_key(p) for p in off], "the recogniser saw other pixels"
    # the canvases handed to the recogniser are the host twin's bytes for the words' polygons, in reading order
    assert len(seen) == 1
    qdesc, canv = seen[0]
    words = [(pi, w) for pi, p in enumerate(on) for w in p.blocks[0].words if w.text is not None]
    boxes = []
    for _, w in words:
        pts = np.array(w.polygon, dtype=np.int32)
        boxes.append((pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()))
    aabb, keep = ops.crop_descriptors(boxes, [pi for pi, _ in words], (PH, PW), CFG["img_h"], CFG["img_w"])
    assert keep.all()
    exp_desc = ops.quad_descriptors([w.polygon for _, w in words], aabb, CFG["img_h"], CFG["img_w"])
    assert np.array_equal(qdesc, exp_desc)
    assert np.array_equal(canv, ops.quad_crop_host(np.stack(pgs), exp_desc, CFG["img_h"], CFG["img_w"]))
    # host-ordered route: identical pages, identical canvases
    pipe.device_order = False
    host_order = pipe.predict_batch(pgs, _maps_override=mo)
    assert [_key(p) for p in host_order] == [_key(p) for p in on]
    assert len(seen) == 2 and np.array_equal(seen[1][0], qdesc) and np.array_equal(seen[1][1], canv)
    pipe.device_order = True
    # a page the reading-order kernel flags (ncrop = -1) takes the host route, with the same result
    real_ro = ops.reading_order_crops

    def flagged(*args, **kw):
        order, keep_, desc, ncrop = real_ro(*args, **kw)
        return order, keep_, desc, torch.full_like(ncrop, -1)

    monkeypatch.setattr(ops, "reading_order_crops", flagged)
    assert [_key(p) for p in pipe.predict_batch(pgs, _maps_override=mo)] == [_key(p) for p in on]
    monkeypatch.setattr(ops, "reading_order_crops", real_ro)
    # a batch of two pages equals two calls of one page
    single = [pipe.predict_batch([pgs[k]], _maps_override=(mo[0][k:k + 1], mo[1][k:k + 1]))[0] for k in range(2)]
    assert [_key(p) for p in single] == [_key(p) for p in on]
    # off again: the first run, exactly
    pipe.rectify_crops = False
    n_seen = len(seen)
    again = pipe.predict_batch(pgs, _maps_override=mo)
    assert [_key(p) for p in again] == [_key(p) for p in off] and len(seen) == n_seen


def test_pipeline_rectify_crops_with_char_details(gpu, rec):
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import CharWord
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(PW, PH), device="cuda", axis_aligned_output=False), rec)
    pgs, mo = _pages_and_maps()
    pipe.rectify_crops = True
    plain = pipe.predict_batch(pgs, _maps_override=mo)
    pipe.char_details = True
    for device_order in (True, False):
        pipe.device_order = device_order
        on = pipe.predict_batch(pgs, _maps_override=mo)
        assert [_key(p) for p in on] == [_key(p) for p in plain]
        n_chars = 0
        for p in on:
            for w in p.blocks[0].words:
                if w.text is None:
                    continue
                assert isinstance(w, CharWord) and "".join(c.char for c in w.chars) == w.text
                xs = [pt[0] for pt in w.polygon]
                assert all(min(xs) - 1e-6 <= c.x <= max(xs) + 1e-6 for c in w.chars), (xs, [c.x for c in w.chars])
                n_chars += len(w.chars)
        assert n_chars > 20


def test_graph_path_declines_rectified_crops(gpu, monkeypatch):
    """use_graphs=True: recognize_start_graph declines while rectify_crops is set (plain launches, same result as the recogniser
    without graphs) and replays again once it is off."""
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA
    sd = synth.trba_state_dict_confident(194, 256, seed=3)
    grec = TRBA(state_dict=sd, config=CFG, device="cuda", use_graphs=True)
    det = EAST(state_dict=synth.east_state_dict(), target_size=(PW, PH), device="cuda", axis_aligned_output=False)
    pipe = Pipeline(det, grec)
    pipe.stream_sets = 1
    pgs, mo = _pages_and_maps()
    pages_dev = torch.from_numpy(np.stack(pgs)).cuda()
    seen = []
    finish = grec.recognize_finish

    def spy(handle, *a, **kw):
        seen.append(handle.graph_inst is not None)
        return finish(handle, *a, **kw)

    monkeypatch.setattr(grec, "recognize_finish", spy)
    pipe.rectify_crops = True
    first = pipe.predict_batch(pgs, pages_dev=pages_dev, _maps_override=mo)
    second = pipe.predict_batch(pgs, pages_dev=pages_dev, _maps_override=mo)
    assert seen == [False, False], seen
    plain_pipe = Pipeline(det, TRBA(state_dict=sd, config=CFG, device="cuda"))
    plain_pipe.rectify_crops = True
    plain = plain_pipe.predict_batch(pgs, pages_dev=pages_dev, _maps_override=mo)
    assert [_key(p) for p in first] == [_key(p) for p in second] == [_key(p) for p in plain]
    pipe.rectify_crops = False
    pipe.predict_batch(pgs, pages_dev=pages_dev, _maps_override=mo)
    pipe.predict_batch(pgs, pages_dev=pages_dev, _maps_override=mo)
    assert seen[2:] == [False, True], seen
