"""Rectified word crops (Pipeline.rectify_crops) without a device: the host twins
msocr_quad_crop_descriptors_host and msocr_quad_crop_host against a NumPy f64 restatement of the definition, written from its text
(include/msocr.h) and calling nothing of the library; what the definition means geometrically; and the Pipeline's host route.
tests/test_gpu_quad_crop.py runs the same quads through the device kernels."""
import copy

import numpy as np
import pytest

from manuscript_ocr_amd import Pipeline, ops
from manuscript_ocr_amd.detectors._types import Block, Page, Word

H, W = 96, 160
CANVASES = [(32, 128), (64, 256)]


# ------------------------------------------------------------------------------------------- the restatement (NumPy f64)
def ref_canonical(quad):
    """quad [4,2] f32 as stored -> [4,2] f32 in canonical order, or None when unusable."""
    q = np.asarray(quad, dtype=np.float32)
    if not np.isfinite(q).all():
        return None
    p = q.astype(np.float64)
    cross = []
    for i in range(4):
        a = p[(i + 1) % 4] - p[i]
        b = p[(i + 2) % 4] - p[(i + 1) % 4]
        cross.append(a[0] * b[1] - a[1] * b[0])
    if all(c > 0 for c in cross):
        idx = [0, 1, 2, 3]
    elif all(c < 0 for c in cross):
        idx = [3, 2, 1, 0]  # counter-clockwise on screen: walked backwards
    else:
        return None
    best = None
    for r in range(4):
        dx = p[idx[(r + 1) % 4], 0] - p[idx[r], 0]
        if best is None or dx > best[0] or (dx == best[0] and idx[r] < best[1]):
            best = (dx, idx[r], r)
    return q[[idx[(best[2] + k) % 4] for k in range(4)]]


def ref_size(c):
    p = np.asarray(c, dtype=np.float32).astype(np.float64)
    side = lambda a, b: np.sqrt((p[a, 0] - p[b, 0]) * (p[a, 0] - p[b, 0]) + (p[a, 1] - p[b, 1]) * (p[a, 1] - p[b, 1]))
    return max(side(1, 0), side(2, 3)), max(side(3, 0), side(2, 1))


def ref_descriptor(quad, aabb, img_h, img_w, natural=False):
    """-> (int32 [12] descriptor, fell_back)."""
    c = ref_canonical(quad)
    fell_back = c is None
    if not fell_back:
        w, h = ref_size(c)
        fell_back = not (w >= 1.0 and h >= 1.0)
    if fell_back:
        x1, y1, x2, y2 = (np.float32(v) for v in aabb[1:5])
        c = np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]], dtype=np.float32)
        w, h = ref_size(c)
    if natural:
        nw, nh, y0 = max(1, int(np.rint(w))), max(1, int(np.rint(h))), 0
    else:
        scale = min(img_h / h, img_w / w)
        nw = min(max(1, int(np.rint(w * scale))), img_w)
        nh = min(max(1, int(np.rint(h * scale))), img_h)
        y0 = max(0, min((img_h - nh) // 2, img_h - nh))
    d = np.zeros(12, dtype=np.int32)
    d[0] = aabb[0]
    d[1:9] = np.ascontiguousarray(c, dtype=np.float32).reshape(8).view(np.int32)
    d[9:] = nw, nh, y0
    return d, fell_back


def ref_sub_samples(d):
    c = d[1:9].copy().view(np.float32).reshape(4, 2)
    w, h = ref_size(c)
    return int(np.clip(np.ceil(w / d[9]), 1, 4)), int(np.clip(np.ceil(h / d[10]), 1, 4))


def ref_positions(d, i=0, j=0, S=(1, 1)):
    """Page positions p of sub-sample (i, j) of every pixel of the resized region -> (x [nh,nw], y [nh,nw])."""
    P = d[1:9].copy().view(np.float32).reshape(4, 2).astype(np.float64)
    nw, nh = int(d[9]), int(d[10])
    u = ((np.arange(nw, dtype=np.float64) + (i + 0.5) / S[0]) / nw)[None, :]
    v = ((np.arange(nh, dtype=np.float64) + (j + 0.5) / S[1]) / nh)[:, None]
    w0, w1, w2, w3 = (1 - u) * (1 - v), u * (1 - v), u * v, (1 - u) * v
    return w0 * P[0, 0] + w1 * P[1, 0] + w2 * P[2, 0] + w3 * P[3, 0], w0 * P[0, 1] + w1 * P[1, 1] + w2 * P[2, 1] + w3 * P[3, 1]


def ref_canvas(pages, d, img_h, img_w):
    page = pages[d[0]].astype(np.float64)
    ph, pw = page.shape[:2]
    nw, nh, y0 = int(d[9]), int(d[10]), int(d[11])
    S = ref_sub_samples(d)
    total = np.zeros((nh, nw, 3), dtype=np.float64)
    for j in range(S[1]):
        for i in range(S[0]):
            x, y = ref_positions(d, i, j, S)
            x, y = x - 0.5, y - 0.5
            xf, yf = np.floor(x), np.floor(y)
            fx, fy = (x - xf)[..., None], (y - yf)[..., None]
            xa, xb = np.clip(xf, 0, pw - 1).astype(np.int64), np.clip(xf + 1, 0, pw - 1).astype(np.int64)
            ya, yb = np.clip(yf, 0, ph - 1).astype(np.int64), np.clip(yf + 1, 0, ph - 1).astype(np.int64)
            a, b, c, e = page[ya, xa], page[ya, xb], page[yb, xa], page[yb, xb]
            total = total + ((1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * e))
    canvas = np.full((img_h, img_w, 3), 255, dtype=np.uint8)
    canvas[y0:y0 + nh, :nw] = np.clip(np.rint(total / (S[0] * S[1])), 0, 255).astype(np.uint8)
    return canvas


# ------------------------------------------------------------------------------------------- pages and quads
def make_pages():
    rng = np.random.default_rng(20260315)
    noise = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    grad = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (H + W - 2)], axis=2).astype(np.uint8)
    return np.stack([noise, grad])


def rect(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float64)


def tilt(quad, deg):
    """The quad turned by `deg` about its centre (building test INPUTS may use trigonometry; the library does not)."""
    q = np.asarray(quad, dtype=np.float64)
    c, t = q.mean(axis=0), np.deg2rad(deg)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return (q - c) @ R.T + c


def window_of(quad, page):
    """The word's AABB descriptor as the Pipeline forms it (int32 truncation, clamped window); a word without a window (it never
    reaches the recogniser) gets a 1 x 1 one, which a usable quad does not read."""
    p = np.asarray(quad, dtype=np.float32).astype(np.int32)
    box = (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max())
    desc, keep = ops.crop_descriptors([box], [page], (H, W), 32, 128)
    if not keep[0]:
        desc, _ = ops.crop_descriptors([(0, 0, 1, 1)], [page], (H, W), 32, 128)
    return desc[0]


def quad_cases(img_h, img_w):
    """(name, quad [4,2] f32, AABB descriptor [8] i32) for one canvas size: the quad set of the kernel tests."""
    base = rect(40, 36, 80, 24)
    cases = [
        ("anchor", rect(8, 20, 100, img_h)),                       # integer, axis-aligned, new_w == w: the page window itself
        ("anchor_full_width", rect(0, 0, min(img_w, W), img_h)),
        ("sheared", [(30, 20), (110, 20), (122, 50), (42, 50)]),
        ("trapezoid", [(30, 20), (120, 26), (116, 48), (34, 54)]),
        ("two_corners_outside", [(120, 60), (190, 50), (195, 80), (125, 90)]),
        ("fully_outside", rect(200, 120, 80, 30)),
        ("S1_small", rect(50, 40, 30, 12)),
        ("S2", rect(2, 30, 150, 40)),
        ("S3", rect(2, 2, 150, 90)),
        ("S_mixed_3_2", rect(70.25, 10.5, 9, 64)),
        ("S_mixed_4_3", rect(0, 0, 160, 96)),
        ("S_clamped", rect(-100, -50, 600, 200)),                    # ratio above 4 on both axes
        ("S_clamped_tilted", tilt(rect(-100, -50, 600, 200), 12)),
        ("enlarged_6x20", rect(50, 40, 20, 6)),
        ("min_text_size_5px", rect(60, 60, 5, 5)),
        ("tall_y0_0", rect(70, 5, 20, 80)),
        ("tall_tilted", tilt(rect(70, 5, 20, 80), -8)),
        ("wide_y0_positive", rect(5, 40, 150, 10)),
        ("wide_tilted", tilt(rect(5, 40, 150, 10), 3)),
        ("fractional_corners", rect(33.3, 21.7, 77.1, 19.9)),
    ]
    for deg in (5, -5, 30, -30, 44, -44):
        cases.append((f"tilt_{deg}", tilt(base, deg)))
    out = []
    for k, (name, q) in enumerate(cases):
        q = np.asarray(q, dtype=np.float32).reshape(4, 2)
        out.append((name, q, window_of(q, k % 2)))
    return out


NAN = float("nan")
FALLBACKS = [  # (name, quad, window x1 y1 x2 y2)
    ("collinear", [(20, 20), (60, 20), (100, 20), (140, 20)], (20, 18, 140, 30)),
    ("bow_tie", [(30, 20), (110, 50), (110, 20), (30, 50)], (30, 20, 110, 50)),
    ("repeated_corner", [(30, 20), (110, 20), (110, 20), (30, 50)], (30, 20, 110, 50)),
    ("nan_corner", [(30, 20), (110, NAN), (110, 50), (30, 50)], (30, 20, 110, 50)),
    ("sliver_half_px", rect(30, 40, 80, 0.5), (30, 40, 110, 41)),
]


def fallback_cases():
    out = []
    for k, (name, q, win) in enumerate(FALLBACKS):
        desc, keep = ops.crop_descriptors([win], [k % 2], (H, W), 32, 128)
        assert keep[0]
        out.append((name, np.asarray(q, dtype=np.float32).reshape(4, 2), desc[0]))
    return out


def lib_descriptors(cases, img_h, img_w, natural=False):
    return ops.quad_descriptors([q for _, q, _ in cases], np.stack([a for _, _, a in cases]), img_h, img_w, natural=natural)


@pytest.fixture(scope="module")
def pages():
    p = make_pages()
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------------------------------- host twin against the restatement
@pytest.mark.parametrize("img_h,img_w", CANVASES)
def test_descriptors_equal_the_restatement(img_h, img_w):
    cases = quad_cases(img_h, img_w) + fallback_cases()
    got = lib_descriptors(cases, img_h, img_w)
    nat_got = lib_descriptors(cases, 0, 0, natural=True)
    for k, (name, q, aabb) in enumerate(cases):
        exp, fell = ref_descriptor(q, aabb, img_h, img_w)
        assert np.array_equal(got[k], exp), (name, got[k], exp)
        assert fell == (k >= len(cases) - len(FALLBACKS)), name
        assert np.array_equal(nat_got[k], ref_descriptor(q, aabb, 0, 0, natural=True)[0]), name
    by_name = {name: got[k] for k, (name, _, _) in enumerate(cases)}
    assert by_name["tall_y0_0"][9] < img_w and by_name["tall_y0_0"][11] == 0
    assert by_name["wide_y0_positive"][11] > 0
    assert by_name["enlarged_6x20"][9] > 20 * 2


def test_quad_set_reaches_every_sub_sample_count():
    """Sx and Sy of 1, 2, 3 and 4, a pair mixed per axis and a ratio above 4 (clamped), over the two canvas sizes."""
    seen, ratios = set(), []
    for img_h, img_w in CANVASES:
        for name, q, aabb in quad_cases(img_h, img_w):
            d, _ = ref_descriptor(q, aabb, img_h, img_w)
            seen.add(ref_sub_samples(d))
            ratios.append(ref_size(d[1:9].copy().view(np.float32).reshape(4, 2))[0] / d[9])
    assert {s[0] for s in seen} == {1, 2, 3, 4} and {s[1] for s in seen} == {1, 2, 3, 4}, seen
    assert any(s[0] != s[1] for s in seen) and max(ratios) > 4.0, (seen, max(ratios))


@pytest.mark.parametrize("img_h,img_w", CANVASES)
def test_canvases_equal_the_restatement(pages, img_h, img_w):
    cases = quad_cases(img_h, img_w)
    desc = lib_descriptors(cases, img_h, img_w)
    got = ops.quad_crop_host(pages, desc, img_h, img_w)
    for k, (name, q, aabb) in enumerate(cases):
        exp = ref_canvas(pages, ref_descriptor(q, aabb, img_h, img_w)[0], img_h, img_w)
        assert np.array_equal(got[k], exp), (name, int(np.abs(got[k].astype(int) - exp).max()))
    # the anchors: an axis-aligned integer quad at scale 1 IS the page window
    for k in (0, 1):
        name, q, aabb = cases[k]
        x1, y1, x2, y2 = (int(v) for v in (q[0, 0], q[0, 1], q[2, 0], q[2, 1]))
        assert tuple(desc[k, 9:]) == (x2 - x1, y2 - y1, 0), name
        assert np.array_equal(got[k][:, :x2 - x1], pages[desc[k, 0], y1:y2, x1:x2]), name
        assert (got[k][:, x2 - x1:] == 255).all()


@pytest.mark.parametrize("img_h,img_w", CANVASES)
def test_corner_order_does_not_matter(pages, img_h, img_w):
    q = tilt(rect(40, 36, 80, 24), 17).astype(np.float32)
    aabb = window_of(q, 0)
    variants = [np.roll(q, -r, axis=0) for r in range(4)] + [np.roll(q[::-1], -r, axis=0) for r in range(4)]
    cases = [(f"v{k}", v, aabb) for k, v in enumerate(variants)]
    desc = lib_descriptors(cases, img_h, img_w)
    assert all(np.array_equal(d, desc[0]) for d in desc)
    corners = desc[0, 1:9].copy().view(np.float32).reshape(4, 2)
    assert np.array_equal(corners, q), "already (tl, tr, br, bl)"
    canv = ops.quad_crop_host(pages, desc, img_h, img_w)
    assert all(np.array_equal(c, canv[0]) for c in canv)
    assert np.array_equal(canv[0], ref_canvas(pages, ref_descriptor(q, aabb, img_h, img_w)[0], img_h, img_w))


def test_tie_on_the_first_edge_takes_the_smallest_stored_index(pages):
    """A square standing on a corner: two edges have the same x1 - x0; the start corner with the smallest index in the stored
    order wins, whichever way the stored polygon winds."""
    top, right, bottom, left = (80, 28), (100, 48), (80, 68), (60, 48)
    stored_and_expected = [
        ([top, right, bottom, left], [top, right, bottom, left]),    # clockwise: starts 0 (top) and 3 (left) tie -> 0
        ([left, top, right, bottom], [left, top, right, bottom]),    # starts 0 (left) and 1 (top) tie -> 0
        ([right, bottom, left, top], [left, top, right, bottom]),    # starts 2 (left) and 3 (top) tie -> 2
        ([top, left, bottom, right], [top, right, bottom, left]),    # counter-clockwise: starts 1 (left) and 0 (top) tie -> 0
        ([bottom, right, top, left], [top, right, bottom, left]),    # counter-clockwise: starts 3 (left) and 2 (top) tie -> 2
    ]
    cases = [(str(k), np.array(s, dtype=np.float32), window_of(np.array(s, dtype=np.float32), 0)) for k, (s, _) in enumerate(stored_and_expected)]
    desc = lib_descriptors(cases, 32, 128)
    for d, (name, q, aabb), (_, exp) in zip(desc, cases, stored_and_expected):
        assert np.array_equal(d[1:9].copy().view(np.float32).reshape(4, 2), np.array(exp, dtype=np.float32)), name
        assert np.array_equal(d, ref_descriptor(q, aabb, 32, 128)[0]), name
    canv = ops.quad_crop_host(pages, desc, 32, 128)
    for k, (name, q, aabb) in enumerate(cases):
        assert np.array_equal(canv[k], ref_canvas(pages, desc[k], 32, 128)), name


@pytest.mark.parametrize("img_h,img_w", CANVASES)
def test_fallback_takes_the_aabb_window(pages, img_h, img_w):
    cases = fallback_cases()
    desc = lib_descriptors(cases, img_h, img_w)
    canv = ops.quad_crop_host(pages, desc, img_h, img_w)
    for k, (name, q, aabb) in enumerate(cases):
        x1, y1, x2, y2 = (int(v) for v in aabb[1:5])
        win = rect(x1, y1, x2 - x1, y2 - y1).astype(np.float32)
        exp_d, fell = ref_descriptor(win, aabb, img_h, img_w)
        assert not fell and np.array_equal(desc[k], exp_d), name
        assert np.array_equal(canv[k], ref_canvas(pages, exp_d, img_h, img_w)), name


def test_invalid_descriptors_give_white_canvases_on_the_host(pages):
    cases = quad_cases(32, 128)[:3]
    desc = lib_descriptors(cases, 32, 128)
    bad = desc.copy()
    bad[0, 0] = 2        # page out of range
    bad[1, 9] = 129      # wider than the canvas
    good = ops.quad_crop_host(pages, desc, 32, 128)
    got = ops.quad_crop_host(pages, bad, 32, 128)
    assert (got[0] == 255).all() and (got[1] == 255).all() and np.array_equal(got[2], good[2])


# ------------------------------------------------------------------------------------------- what it is for
def test_rectified_canvas_follows_the_tilted_pattern():
    """Page = 128 + 100 sin(2 pi s / 32), s the coordinate along a direction tilted by 20 degrees, sampled at pixel centres and
    rounded.  The rectified canvas of a quad tilted by the same 20 degrees (99.6 x 31.7 onto the 32 x 128 canvas: a scale just above
    1, so one sub-sample per pixel whatever the corners' rounding to f32) must equal the pattern evaluated at the canvas's own sample positions up to
        2 * (1/8) * (2 pi / 32)^2 * 100   bilinear interpolation error (second derivative bound per axis, 4 taps one pixel apart)
      + 0.5                               the page's rounding to integers (the taps are a convex combination of rounded values)
      + 0.5                               the canvas's rounding
    (the sub-sample mean adds nothing at S = 1).  The AABB canvas of the same word misses that by far: this is what the feature
    is for."""
    t = np.deg2rad(20.0)
    k = 2 * np.pi / 32
    pattern = lambda x, y: 128 + 100 * np.sin(k * (x * np.cos(t) + y * np.sin(t)))
    yy, xx = np.mgrid[0:H, 0:W]
    page = np.rint(pattern(xx + 0.5, yy + 0.5)).astype(np.uint8)
    pages = np.repeat(page[None, :, :, None], 3, axis=3)
    q = tilt(rect(30, 32, 99.6, 31.7), 20).astype(np.float32)
    aabb = window_of(q, 0)
    d = ops.quad_descriptors([q], aabb[None], 32, 128)[0]
    cw = int(d[9])
    assert tuple(d[9:]) == (101, 32, 0) and ref_sub_samples(d) == (1, 1)
    canvas = ops.quad_crop_host(pages, d[None], 32, 128)[0]
    x, y = ref_positions(d)
    expected = pattern(x, y)
    bound = 2 * (1 / 8) * k ** 2 * 100 + 0.5 + 0.5
    err = float(np.abs(canvas[:, :cw, 0].astype(np.float64) - expected).max())
    print(f"rectified: max error {err:.3f} levels, bound {bound:.3f}")
    assert err <= bound, (err, bound)
    assert (canvas[:, :cw, 0] == canvas[:, :cw, 1]).all() and (canvas[:, cw:] == 255).all()
    # the AABB crop of the same word (its window resampled axis-aligned), compared where both canvases hold the word
    win = rect(aabb[1], aabb[2], aabb[3] - aabb[1], aabb[4] - aabb[2]).astype(np.float32)
    da, _ = ref_descriptor(win, aabb, 32, 128)
    ca = ref_canvas(pages, da, 32, 128)
    assert tuple(da[9:]) == tuple(aabb[5:]), "the restated window has ops.crop_descriptors' size"
    nw, r0, r1 = min(int(da[9]), cw), int(da[11]), int(da[11] + da[10])
    err_aabb = float(np.abs(ca[r0:r1, :nw, 0].astype(np.float64) - expected[r0:r1, :nw]).max())
    print(f"AABB: max error {err_aabb:.3f} levels")
    assert err_aabb > bound, (err_aabb, bound)


# ------------------------------------------------------------------------------------------- Pipeline, host route
class _StubRecognizer:
    def predict(self, images):
        self.seen = images
        return [{"text": f"w{k}", "confidence": 0.5} for k in range(len(images))]


class _StubDetector:
    def __init__(self, page):
        self.page = page

    def predict(self, image, vis=False, profile=False):
        return {"page": copy.deepcopy(self.page)}


def _tilted_page():
    quads = [tilt(rect(100, 12, 40, 14), 9), tilt(rect(10, 10, 70, 16), 12), tilt(rect(20, 50, 90, 20), -10),
             rect(130, 60, 3, 3), tilt(rect(120, 70, 30, 12), 30)]  # the fourth is under min_text_size
    words = [Word(polygon=[tuple(float(v) for v in pt) for pt in np.asarray(q, dtype=np.float32)], detection_confidence=0.9) for q in quads]
    return Page(blocks=[Block(words=words)])


def test_pipeline_host_route_hands_out_upright_words(pages):
    image = np.ascontiguousarray(pages[0])
    page = _tilted_page()
    pipe = Pipeline(detector=_StubDetector(page), recognizer=_StubRecognizer())
    assert not getattr(pipe, "rectify_crops", False)
    off_words, off_crops = pipe._order_and_crop(copy.deepcopy(page), image)
    pipe.rectify_crops = True
    on_words, on_crops = pipe._order_and_crop(copy.deepcopy(page), image)
    assert [w.polygon for w in on_words] == [w.polygon for w in off_words] and len(on_words) == 4
    for word, crop, plain in zip(on_words, on_crops, off_crops):
        q = np.array(word.polygon, dtype=np.float32)
        w, h = ref_size(ref_canonical(q))
        assert crop.shape == (int(np.rint(h)), int(np.rint(w)), 3) and crop.dtype == np.uint8, (crop.shape, w, h)
        assert crop.shape != plain.shape
        d, _ = ref_descriptor(q, window_of(q, 0), 0, 0, natural=True)
        assert np.array_equal(crop, ref_canvas(image[None], d, crop.shape[0], crop.shape[1]))
    # through predict (foreign plugins): same words, same order, same texts as with the attribute off
    on = pipe.predict(image)
    assert [c.shape for c in pipe.recognizer.seen] == [c.shape for c in on_crops]
    pipe.rectify_crops = False
    off = pipe.predict(image)
    assert [(w.polygon, w.text) for w in on.blocks[0].words] == [(w.polygon, w.text) for w in off.blocks[0].words]
    assert [c.shape for c in pipe.recognizer.seen] == [c.shape for c in off_crops]
