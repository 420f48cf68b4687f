"""Tiled detection of large pages (EAST(tile_size=...), csrc/east_tiles.hip): the gather and stitch kernels against NumPy
restatements, the detector on injected tile maps against the untiled detector and the oracle, the real network's plumbing, the
pipeline, and the refusals.  Stitching only moves data, so every comparison here is bit-exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from manuscript_ocr_amd import synth
from manuscript_ocr_amd.detectors._east import tiles

pytestmark = pytest.mark.gpu

TILE, OVERLAP = 256, 64
MARGIN = 3  # map pixels around a tile's owned region that still hold the page map in the poisoned tile maps


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.east_state_dict()


@functools.lru_cache(maxsize=None)
def _det(**kw):
    from manuscript_ocr_amd.detectors import EAST
    return EAST(state_dict=_sd(), device="cuda", **kw)


def _boxes(res):
    return np.array([[c for pt in w.polygon for c in pt] + [w.detection_confidence] for w in res["page"].blocks[0].words],
                    dtype=np.float32).reshape(-1, 9)


# ------------------------------------------------------------------------------------------- NumPy restatements
def np_gather(pages, g):
    """pages [N,H,W,3] -> tiles [N,T,th,tw,3]: np.pad(mode="edge") up to the grid's extent, then windows."""
    N, H, W, _ = pages.shape
    He, We = max(tiles.round_up(H, 32), g.tile_h), max(tiles.round_up(W, 32), g.tile_w)
    pad = np.pad(pages, ((0, 0), (0, He - H), (0, We - W), (0, 0)), mode="edge")
    return np.stack([np.stack([pad[n, oy:oy + g.tile_h, ox:ox + g.tile_w] for oy in g.oy for ox in g.ox]) for n in range(N)])


def np_stitch(tscore, tgeo, g):
    """Tile maps [N,T,tmh,tmw(,8)] -> page maps [N,Hm,Wm(,8)]: every pixel from its owner at the tile-local position, zeros where
    the page position (4 y, 4 x) lies outside the page."""
    Hm, Wm = g.map_hw
    ys, xs = np.arange(Hm), np.arange(Wm)
    ly, lx = ys - g.oy[g.row_tile] // 4, xs - g.ox[g.col_tile] // 4
    t = g.row_tile[:, None] * g.nx + g.col_tile[None, :]
    score = tscore[:, t, ly[:, None], lx[None, :]].copy()
    geo = tgeo[:, t, ly[:, None], lx[None, :]].copy()
    out = (4 * ys[:, None] >= g.H) | (4 * xs[None, :] >= g.W)
    score[:, out] = 0.0
    geo[:, out] = 0.0
    return score, geo


def _tables(H, W, tile=TILE, overlap=OVERLAP):
    from manuscript_ocr_amd import ops
    tile_wh = (tile, tile) if np.isscalar(tile) else tile
    return ops.east_tile_tables(tiles.page_grid(H, W, tile_wh, overlap), "cuda")


# ------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("N,H,W,tile,overlap", [(2, 443, 570, 256, 64), (1, 70, 100, 128, 32), (1, 256, 256, 256, 64),
                                                 (1, 130, 97, (96, 128), 32)])
def test_gather_bit_identical_to_numpy(gpu, N, H, W, tile, overlap):
    """Two pages that need 2 x 3 tiles with padding on both axes, a page smaller than the tile, a page that is exactly one tile,
    and an odd page width (page rows at every byte alignment) with a non-square tile and a page narrower than it."""
    from manuscript_ocr_amd import ops
    pages = np.random.default_rng(H * W).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    tab = _tables(H, W, tile, overlap)
    got = ops.east_tile_gather(torch.from_numpy(pages).cuda(), tab).cpu().numpy()
    exp = np_gather(pages, tab.grid)
    assert got.shape == exp.shape and got.dtype == np.uint8
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:4]


@pytest.mark.parametrize("H,W", [(443, 569), (129, 97), (70, 101)])
def test_gather_from_a_slice_of_an_odd_sized_batch(gpu, H, W):
    """pages[k:] of a batch of pages with odd H and W starts at k * H * W * 3 bytes, for the first two sizes at every residue mod 4 (the
    pipeline hands the detector such slices, one per sub-batch): the tiles are still NumPy's, whatever the pointer's alignment."""
    from manuscript_ocr_amd import ops
    pages = np.random.default_rng(H + W).integers(0, 256, size=(5, H, W, 3), dtype=np.uint8)
    dev = torch.from_numpy(pages).cuda()
    tab = _tables(H, W, 128, 32)
    seen = set()
    for k in (1, 2, 3, 4):
        sl = dev[k:]
        assert sl.is_contiguous()
        seen.add(sl.data_ptr() % 4)
        got = ops.east_tile_gather(sl, tab).cpu().numpy()
        assert np.array_equal(got, np_gather(pages[k:], tab.grid)), (k, sl.data_ptr() % 4)
    assert len(seen) >= 2 and seen != {0}, seen  # misaligned starts were among them


def _identifying_tile_maps(N, g, seed):
    """Values that name page, tile and position: a wrong owner or offset changes them."""
    tmh, tmw = g.tile_h // 4, g.tile_w // 4
    n, t, y, x = np.meshgrid(np.arange(N), np.arange(g.ntiles), np.arange(tmh), np.arange(tmw), indexing="ij")
    tscore = (((n * g.ntiles + t) * tmh + y) * tmw + x + 1).astype(np.float32)  # < 2^24: exact
    tgeo = tscore[..., None] * 8 + np.arange(8, dtype=np.float32)
    assert tgeo.max() < 2 ** 24
    return tscore, tgeo.astype(np.float32)


@pytest.mark.parametrize("H,W,tile,overlap", [(443, 570, 256, 64), (70, 100, 128, 32), (300, 200, 128, 0)])
def test_stitch_bit_identical_to_numpy(gpu, H, W, tile, overlap):
    from manuscript_ocr_amd import ops
    tab = _tables(H, W, tile, overlap)
    g = tab.grid
    tscore, tgeo = _identifying_tile_maps(2, g, 0)
    score, geo = ops.east_stitch_maps(torch.from_numpy(tscore).cuda(), torch.from_numpy(tgeo).cuda(), tab)
    score, geo = score.cpu().numpy(), geo.cpu().numpy()
    es, eg = np_stitch(tscore, tgeo, g)
    assert score.shape == es.shape == (2,) + g.map_hw and geo.shape == eg.shape
    assert np.array_equal(score, es), np.argwhere(score != es)[:4]
    assert np.array_equal(geo, eg), np.argwhere(geo != eg)[:4]
    Hm, Wm = g.map_hw
    out = (4 * np.arange(Hm)[:, None] >= H) | (4 * np.arange(Wm)[None, :] >= W)
    assert out.any() and np.all(score[:, out] == 0.0) and np.all(geo[:, out] == 0.0)
    assert np.all(score[:, ~out] > 0.0)  # every in-page pixel was written from a tile


# ------------------------------------------------------------------------------------------- injected maps, end to end
def _page_and_map(seed, H, W):
    """A synthetic page of H x W with its injected page map M at round_up(H, 32) / 4 x round_up(W, 32) / 4 (scale exactly 4)."""
    page, rects = synth.synth_page(seed, H, W)
    H32, W32 = tiles.round_up(H, 32), tiles.round_up(W, 32)
    score, geo = synth.synth_maps(rects, (H32, W32), (H32 // 4, W32 // 4), seed)
    return page, score, geo


def _poisoned_tile_maps(score, geo, g, seed):
    """Cut the page map into tile maps: inside a tile's owned region plus MARGIN map pixels the tile map equals the page map,
    everywhere else it is poisoned (score 0.99, random finite geometry below 1e7): a stitch that reads an unowned pixel changes
    the boxes."""
    rng = np.random.default_rng(seed)
    Hm, Wm = g.map_hw
    tmh, tmw = g.tile_h // 4, g.tile_w // 4
    ts = np.full((g.ntiles, tmh, tmw), 0.99, dtype=np.float32)
    tg = rng.uniform(-9e6, 9e6, size=(g.ntiles, tmh, tmw, 8)).astype(np.float32)
    cy, cx = [0] + [c // 4 for c in g.cuts_y] + [Hm], [0] + [c // 4 for c in g.cuts_x] + [Wm]
    for ty in range(g.ny):
        for tx in range(g.nx):
            oy, ox = g.oy[ty] // 4, g.ox[tx] // 4
            y0, y1 = max(cy[ty] - MARGIN, oy, 0), min(cy[ty + 1] + MARGIN, oy + tmh, Hm)
            x0, x1 = max(cx[tx] - MARGIN, ox, 0), min(cx[tx + 1] + MARGIN, ox + tmw, Wm)
            t = ty * g.nx + tx
            ts[t, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = score[y0:y1, x0:x1]
            tg[t, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = geo[y0:y1, x0:x1]
    assert np.isfinite(tg).all() and np.abs(tg).max() < 1e7 and (ts == np.float32(0.99)).mean() > 0.05
    return ts, tg


def _crosses(boxes, axis, cut):
    c = boxes[:, axis:8:2]
    return int(np.sum((c.min(axis=1) < cut) & (c.max(axis=1) > cut)))


@pytest.mark.parametrize("H,W", [(448, 576), (443, 570)])
@pytest.mark.parametrize("q", [1, 2])
def test_injected_tile_maps_equal_untiled_and_oracle(gpu, H, W, q):
    """EAST(tile_size=256, tile_overlap=64) on poisoned tile maps == the untiled detector on the page map M == the oracle on M,
    polygons and scores bit for bit; final boxes cross each of the cuts x = 224, x = 384 and y = 224.  For the 443 x 570 page the
    expected result is the oracle on M with the scores of the out-of-page map pixels (row 111, column 143) set to 0."""
    from oracle import east_post as P
    from oracle import lanms as L
    H32, W32 = tiles.round_up(H, 32), tiles.round_up(W, 32)
    g = tiles.page_grid(H, W, (TILE, TILE), OVERLAP)
    assert g.cuts_x == [224, 384] and g.cuts_y == [224] and g.map_hw == (112, 144)
    pages, ms, mg, tss, tgs = [], [], [], [], []
    for k, seed in enumerate((61, 62)):
        page, score, geo = _page_and_map(seed, H, W)
        ts, tg = _poisoned_tile_maps(score, geo, g, seed)
        pages.append(page), ms.append(score), mg.append(geo), tss.append(ts), tgs.append(tg)
    dev = lambda arrs: torch.from_numpy(np.stack(arrs)).cuda()
    tiled = _det(tile_size=TILE, tile_overlap=OVERLAP, quantization=q)
    got = tiled.predict_batch(pages, _maps_override=(dev(tss), dev(tgs)), return_maps=True)
    untiled = None
    if (H, W) == (H32, W32):
        untiled = _det(target_size=(W32, H32), quantization=q).predict_batch(pages, _maps_override=(dev(ms), dev(mg)))
    out = (4 * np.arange(H32 // 4)[:, None] >= H) | (4 * np.arange(W32 // 4)[None, :] >= W)  # map pixels outside the page
    assert out.any() == ((H, W) != (H32, W32))
    for k in range(2):
        score, geo = ms[k].copy(), mg[k].copy()
        score[out] = 0.0
        exp = P.east_postprocess(score, mg[k], (H32, W32), (W32, H32), L.locality_aware_nms, quantization=q)
        assert len(exp) >= 20
        # the condition on the input: words straddle every cut, so an unowned (poisoned) read would move their boxes
        assert _crosses(exp, 0, 224) >= 1 and _crosses(exp, 0, 384) >= 1 and _crosses(exp, 1, 224) >= 1, (k, q)
        b = _boxes(got[k])
        assert b.shape == exp.shape and np.array_equal(b, exp), (k, q, b.shape, exp.shape)
        if untiled is not None:
            assert np.array_equal(b, _boxes(untiled[k]))
        geo[out] = 0.0  # return_maps returns the stitched page maps: M inside the page, zeros outside
        assert np.array_equal(got[k]["score_map"], score) and np.array_equal(got[k]["geo_map"], geo.transpose(2, 0, 1))


def test_host_tail_on_the_tiled_route(gpu):
    """device_tail = False (the route a page above the device tail's capacity takes): the host box filters scale by 1 on the tiled
    route, whatever `target_size` says, and give the device tail's boxes."""
    from manuscript_ocr_amd.detectors import EAST
    H, W = 448, 576
    g = tiles.page_grid(H, W, (TILE, TILE), OVERLAP)
    page, score, geo = _page_and_map(61, H, W)
    ts, tg = _poisoned_tile_maps(score, geo, g, 61)
    mo = (torch.from_numpy(ts[None]).cuda(), torch.from_numpy(tg[None]).cuda())
    dev_boxes = _boxes(_det(tile_size=TILE, tile_overlap=OVERLAP).predict_batch([page], _maps_override=mo)[0])
    host = EAST(state_dict=_sd(), device="cuda", tile_size=TILE, tile_overlap=OVERLAP)
    host.device_tail = False
    assert len(dev_boxes) >= 20 and np.array_equal(_boxes(host.predict_batch([page], _maps_override=mo)[0]), dev_boxes)


# ------------------------------------------------------------------------------------------- the real network
def test_real_network_maps_are_the_tiles_maps(gpu):
    """return_maps=True on a 448 x 576 page: every pixel of the stitched maps equals the map EastNet.forward gives for the gathered
    tile that owns it, at the tile-local position.  Bit-identical: same kernels, same tile batch (all 6 tiles in one)."""
    from manuscript_ocr_amd import ops
    H, W = 448, 576
    page = synth.synth_page(71, H, W)[0]
    det = _det(tile_size=TILE, tile_overlap=OVERLAP, score_thresh=0.5)
    res = det.predict_batch([page], return_maps=True)[0]
    tab = _tables(H, W)
    g = tab.grid
    tl = ops.east_tile_gather(torch.from_numpy(page[None]).cuda(), tab)
    ts, tg = det.model.forward(tl.view(g.ntiles, TILE, TILE, 3))
    es, eg = np_stitch(ts.cpu().numpy()[None], tg.cpu().numpy()[None], g)
    assert es.std() > 0.01, "degenerate score map: weights do not exercise the network"
    assert np.array_equal(res["score_map"], es[0]) and np.array_equal(res["geo_map"], eg[0].transpose(2, 0, 1))


def test_one_tile_page_equals_the_untiled_detector(gpu):
    page = synth.synth_page(72, 256, 256)[0]
    a = _det(tile_size=256, tile_overlap=64, score_thresh=0.5).predict_batch([page], return_maps=True)[0]
    b = _det(target_size=256, score_thresh=0.5).predict_batch([page], return_maps=True)[0]
    assert np.array_equal(a["score_map"], b["score_map"]) and np.array_equal(a["geo_map"], b["geo_map"])
    assert np.array_equal(_boxes(a), _boxes(b))


def test_tile_batch_and_ragged_input(gpu):
    """tile_batch 1, 4 and 16 give the same boxes (and maps); a ragged list of two page sizes equals the per-page calls."""
    big, small = synth.synth_page(73, 448, 576)[0], synth.synth_page(74, 256, 320)[0]
    res = {tb: _det(tile_size=TILE, tile_overlap=OVERLAP, score_thresh=0.5, tile_batch=tb).predict_batch([big, big[::-1].copy()],
                                                                                                         return_maps=True)
           for tb in (1, 4, 16)}
    for tb in (1, 4):
        for a, b in zip(res[tb], res[16]):
            assert len(_boxes(a)) >= 20 and np.array_equal(_boxes(a), _boxes(b))
            # every tile goes through the same kernels whatever the chunk it is in: the maps are the same bits too
            assert np.array_equal(a["score_map"], b["score_map"]) and np.array_equal(a["geo_map"], b["geo_map"])
    det = _det(tile_size=TILE, tile_overlap=OVERLAP, score_thresh=0.5, tile_batch=16)
    ragged = det.predict_batch([big, small, big], return_maps=True)
    for r, pg in zip(ragged, (big, small, big)):
        one = det.predict_batch([pg], return_maps=True)[0]
        assert r["score_map"].shape == one["score_map"].shape == (pg.shape[0] // 4, pg.shape[1] // 4)
        assert np.array_equal(r["score_map"], one["score_map"]) and np.array_equal(r["geo_map"], one["geo_map"])
        assert np.array_equal(_boxes(r), _boxes(one))


# ------------------------------------------------------------------------------------------- pipeline
def test_pipeline_words_equal_the_untiled_pipeline(gpu):
    """Two 448 x 576 pages with injected tile maps through Pipeline(EAST(tile_size=256, tile_overlap=64), TRBA) give the same
    words as the pipeline with the untiled EAST(target_size=(576, 448)) and the page maps: polygons, reading order, texts and
    confidences identical (planted decoder of synth.trba_state_dict_confident)."""
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 448, 576
    g = tiles.page_grid(H, W, (TILE, TILE), OVERLAP)
    pages, ms, mg, tss, tgs = [], [], [], [], []
    for seed in (81, 82):
        page, score, geo = _page_and_map(seed, H, W)
        ts, tg = _poisoned_tile_maps(score, geo, g, seed)
        pages.append(page), ms.append(score), mg.append(geo), tss.append(ts), tgs.append(tg)
    dev = lambda arrs: torch.from_numpy(np.stack(arrs)).cuda()
    rec = TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=20260128),
               config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}, device="cuda")
    tiled = Pipeline(_det(tile_size=TILE, tile_overlap=OVERLAP), rec).predict_batch(pages, _maps_override=(dev(tss), dev(tgs)))
    plain = Pipeline(_det(target_size=(W, H)), rec).predict_batch(pages, _maps_override=(dev(ms), dev(mg)))
    key = lambda p: [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for b in p.blocks for w in b.words]
    for a, b in zip(tiled, plain):
        assert len(key(a)) >= 20 and sum(1 for w in key(a) if w[2]) >= 10
        assert key(a) == key(b)


def test_pipeline_sub_batches_on_odd_sized_pages(gpu):
    """Pipeline.predict_batch(sub_batches=2) hands the detector pages_dev[lo:hi]; on 443 x 570 pages the second slice starts
    2 bytes off a dword.  Three pages with injected tile maps, in sub-batches of (1, 2): the same words as one page at a time."""
    from manuscript_ocr_amd import Pipeline
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 443, 570
    assert (H * W * 3) % 4 == 2
    g = tiles.page_grid(H, W, (TILE, TILE), OVERLAP)
    pages, tss, tgs = [], [], []
    for seed in (81, 82, 61):
        page, score, geo = _page_and_map(seed, H, W)
        ts, tg = _poisoned_tile_maps(score, geo, g, seed)
        pages.append(page), tss.append(ts), tgs.append(tg)
    mo = (torch.from_numpy(np.stack(tss)).cuda(), torch.from_numpy(np.stack(tgs)).cuda())
    rec = TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=20260128),
               config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}, device="cuda")
    pipe = Pipeline(_det(tile_size=TILE, tile_overlap=OVERLAP), rec)
    key = lambda p: [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for b in p.blocks for w in b.words]
    both = pipe.predict_batch(pages, sub_batches=2, _maps_override=mo)
    for k in range(3):
        one = pipe.predict_batch([pages[k]], _maps_override=(mo[0][k:k + 1], mo[1][k:k + 1]))[0]
        assert len(key(one)) >= 20 and key(both[k]) == key(one), k


# ------------------------------------------------------------------------------------------- refusals
def test_constructor_refuses_bad_tilings(gpu):
    from manuscript_ocr_amd.detectors import EAST
    for kw in ({"tile_size": 250}, {"tile_size": (256, 100)}, {"tile_size": 256, "tile_overlap": 160}, {"tile_size": 256, "tile_overlap": 48},
               {"tile_size": (512, 256), "tile_overlap": 160}, {"tile_size": 256, "tile_overlap": 64, "use_graphs": True},
               {"tile_size": 256, "tile_overlap": 64, "tile_batch": 0}):
        with pytest.raises(ValueError):
            EAST(state_dict=_sd(), device="cuda", **kw)
    det = _det(tile_size=TILE, tile_overlap=OVERLAP, quantization=3)  # 3 does not divide the 112 x 144 map
    with pytest.raises(ValueError):
        det.predict_batch([synth.synth_page(1, 448, 576)[0]])


def test_c_abi_refuses_bad_arguments(gpu):
    """Every refused call gets buffers that are valid for the shape it names, so a broken check cannot fault."""
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, T = 443, 570, 256
    tab = _tables(H, W)
    g = tab.grid
    big = 4 * 2 * 4 * 4 * 288 * 288 * 3  # room for N = 2 and every grid named below
    pages = torch.zeros((2, H + 64, W + 64, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((big,), dtype=torch.uint8, device="cuda")
    i32 = torch.zeros((4096,), dtype=torch.int32, device="cuda")
    P, O, I = pages.data_ptr(), out.data_ptr(), i32.data_ptr()
    hy, hx = g.oy.ctypes.data, g.ox.ctypes.data

    def gather(pages=P, N=2, H=H, W=W, oyd=I, oxd=I, oyh=hy, oxh=hx, ny=g.ny, nx=g.nx, th=T, tw=T, tiles_=O):
        return L.msocr_east_tile_gather(pages, N, H, W, oyd, oxd, oyh, oxh, ny, nx, th, tw, tiles_, st)

    assert gather(pages=None) == gather(oyd=None) == gather(oxd=None) == gather(oyh=None) == gather(oxh=None) == gather(tiles_=None) == -1
    assert gather(N=0) == gather(H=0) == gather(W=-1) == gather(ny=0) == gather(nx=0) == gather(th=0) == gather(tw=-32) == -1
    assert gather(th=250) == gather(tw=48) == gather(th=288) == -1  # not multiples of 32; 288 is one, but the origins are not its grid
    assert gather(ny=1) == gather(nx=2) == -1                       # the tiles no longer reach the end of the axis
    assert gather(H=H + 64) == gather(W=W - 200) == -1              # another page size: the last tile does not end at its L32
    assert gather(tiles_=O + 4) == -1                               # alignment of the output (`pages` may start at any byte)
    for bad in ([32, 192, 320], [0, 200, 320], [0, 320, 192], [0, 0, 320], [0, 32, 320], [0, 192, 352]):
        b = np.asarray(bad, dtype=np.int32)  # not from 0, not a multiple of 32, not ascending, repeated, a gap, past the end
        assert gather(oxh=b.ctypes.data) == -1, bad

    f32 = torch.zeros((big // 4,), dtype=torch.float32, device="cuda")
    F = f32.data_ptr()
    G = F + 4 * (big // 8)         # the page maps: score at G, geometry behind it
    G8 = G + 4 * 2 * 128 * 160
    rows = np.concatenate([g.row_tile, np.full(64, g.row_tile[-1], dtype=np.int32)])  # long enough for every page size named below
    cols = np.concatenate([g.col_tile, np.full(64, g.col_tile[-1], dtype=np.int32)])
    hr, hc = rows.ctypes.data, cols.ctypes.data

    def stitch(ts=F, tg=F, N=2, H=H, W=W, ny=g.ny, nx=g.nx, th=T, tw=T, oyd=I, oxd=I, rd=I, cd=I, oyh=hy, oxh=hx, rh=hr, ch=hc, so=G, go=G8):
        return L.msocr_east_stitch_maps(ts, tg, N, H, W, ny, nx, th, tw, oyd, oxd, rd, cd, oyh, oxh, rh, ch, so, go, st)

    assert stitch(ts=None) == stitch(tg=None) == stitch(oyd=None) == stitch(oxd=None) == stitch(rd=None) == stitch(cd=None) == -1
    assert stitch(oyh=None) == stitch(oxh=None) == stitch(rh=None) == stitch(ch=None) == stitch(so=None) == stitch(go=None) == -1
    assert stitch(N=0) == stitch(H=0) == stitch(W=0) == stitch(ny=0) == stitch(nx=-1) == stitch(th=0) == stitch(tw=250) == -1
    assert stitch(ny=1) == stitch(nx=2) == stitch(H=H + 64) == -1
    assert stitch(ts=F + 4) == stitch(tg=F + 8) == stitch(so=G + 4) == stitch(go=G8 + 12) == -1
    for tab_bad in ((0, 3), (0, -1), (5, 1), (143, 0), (0, 2)):  # out of range twice, changes inside a group of 4, outside the owner's tile twice
        c = cols.copy()
        c[tab_bad[0]] = tab_bad[1]
        assert stitch(ch=c.ctypes.data) == -1, tab_bad
    r = rows.copy()
    r[:] = 0  # map rows 64 .. 111 lie outside tile row 0
    assert stitch(rh=r.ctypes.data) == -1
    torch.cuda.synchronize()
    # and the same arguments unchanged are accepted (the refusals above are not a side effect of the buffers)
    assert gather(oyd=tab.oy.data_ptr(), oxd=tab.ox.data_ptr()) == 0
    assert stitch(oyd=tab.oy.data_ptr(), oxd=tab.ox.data_ptr(), rd=tab.row_tile.data_ptr(), cd=tab.col_tile.data_ptr()) == 0
    torch.cuda.synchronize()
