"""Tile grids of the tiled detection (detectors/_east/tiles.py) and the binding of its two kernels: host arithmetic only."""
import os

import numpy as np
import pytest

from manuscript_ocr_amd.detectors._east import tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(256, 64), (128, 0), (128, 32), (256, 128)]


def test_worked_examples():
    assert tiles.tile_grid(576, 256, 64) == ([0, 192, 320], [224, 384])
    assert tiles.tile_grid(448, 256, 64) == ([0, 192], [224])
    assert tiles.tile_grid(256, 256, 64) == ([0], [])
    assert tiles.tile_grid(100, 128, 32) == ([0], [])


@pytest.mark.parametrize("tile,overlap", CONFIGS)
def test_grid_sweep(tile, overlap):
    for length in range(1, 701):
        origins, cuts = tiles.tile_grid(length, tile, overlap)
        L32 = tiles.round_up(length, 32)
        n = len(origins)
        what = (length, tile, overlap, origins, cuts)
        assert origins[0] == 0 and all(o % 32 == 0 for o in origins), what
        assert all(b > a for a, b in zip(origins, origins[1:])), what
        assert len(cuts) == n - 1, what
        if L32 > tile:
            assert origins[-1] + tile == L32, what
        else:
            assert n == 1, what
        # ownership: tile i owns [cuts[i-1], cuts[i]), the first from 0, the last up to L32
        lo = [0] + cuts
        hi = cuts + [L32]
        owners = np.zeros(L32, dtype=np.int64)
        for i in range(n):
            assert lo[i] < hi[i], what
            owners[lo[i]:hi[i]] += 1
            assert origins[i] <= lo[i] and hi[i] <= origins[i] + tile, what  # every owned pixel lies inside its tile
        assert np.all(owners == 1), what
        for i in range(n - 1):
            a_end, b_start = origins[i] + tile, origins[i + 1]
            assert a_end - b_start >= overlap, what  # consecutive tiles overlap by at least `overlap`
            assert cuts[i] % 16 == 0 and b_start <= cuts[i] <= a_end, what
            assert cuts[i] - b_start == a_end - cuts[i], what  # the middle of the actual overlap
        # away from the page borders an owned pixel keeps overlap / 2 pixels of its own tile on either side
        for i in range(n):
            if i > 0:
                assert lo[i] - origins[i] >= overlap // 2, what
            if i < n - 1:
                assert origins[i] + tile - hi[i] >= overlap // 2, what


@pytest.mark.parametrize("tile,overlap", CONFIGS)
def test_owner_tables_agree_with_the_cuts(tile, overlap):
    for length in (1, 31, 32, 33, 127, 128, 129, 255, 257, 443, 448, 570, 576, 700):
        origins, cuts = tiles.tile_grid(length, tile, overlap)
        tab = tiles.owner_table(length, cuts)
        L32 = tiles.round_up(length, 32)
        assert tab.dtype == np.int32 and tab.shape == (L32 // 4,)
        lo, hi = [0] + cuts, cuts + [L32]
        for m, t in enumerate(tab):
            assert lo[t] <= 4 * m < hi[t], (length, tile, overlap, m, t)
            assert 0 <= m - origins[t] // 4 < tile // 4
        assert np.array_equal(tab, np.repeat(tab[::4], 4))  # constant over every 4 map pixels: one owner per 16-byte score vector


def test_page_grid():
    g = tiles.page_grid(443, 570, (256, 256), 64)
    assert (g.ny, g.nx, g.ntiles, g.map_hw) == (2, 3, 6, (112, 144))
    assert g.oy.tolist() == [0, 192] and g.ox.tolist() == [0, 192, 320] and g.cuts_y == [224] and g.cuts_x == [224, 384]
    assert np.array_equal(g.row_tile, tiles.owner_table(443, [224])) and np.array_equal(g.col_tile, tiles.owner_table(570, [224, 384]))
    g = tiles.page_grid(70, 100, (128, 96), 32)  # tile_wh is (W, H)
    assert (g.tile_h, g.tile_w, g.ny, g.nx, g.map_hw) == (96, 128, 1, 1, (24, 32))


def test_bad_tilings_are_refused():
    for tile, overlap in ((250, 64), (0, 0), (-32, 0), (256, 48), (256, 160), (256, -32)):
        with pytest.raises(ValueError):
            tiles.tile_grid(500, tile, overlap)
    with pytest.raises(ValueError):
        tiles.tile_grid(0, 256, 64)


def test_new_symbols_are_bound():
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "msocr.h"), encoding="utf-8").read()
    for name in ("msocr_east_tile_gather", "msocr_east_stitch_maps"):
        assert name in nat.exported_symbols() and hasattr(L, name)
        assert name + "(" in hdr, name
    assert len(nat._SIGS["msocr_east_tile_gather"][1]) == 14 and len(nat._SIGS["msocr_east_stitch_maps"][1]) == 20
    # nothing is launched for a refused call, so the refusals that need no device memory can be seen here
    assert L.msocr_east_tile_gather(None, 1, 64, 64, None, None, None, None, 1, 1, 64, 64, None, None) == -1
    assert L.msocr_east_stitch_maps(None, None, 1, 64, 64, 1, 1, 64, 64, None, None, None, None, None, None, None, None, None, None, None) == -1
