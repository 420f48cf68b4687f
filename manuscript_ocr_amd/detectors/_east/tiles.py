"""Tile grids for the tiled detection of large pages (EAST(tile_size=...)).

A page is cut into overlapping tiles at its own resolution, the network runs on the tiles as a batch, and the tiles' maps are
stitched into one page-sized map (msocr_east_tile_gather / msocr_east_stitch_maps, csrc/east_tiles.hip).  Everything here is host
arithmetic on one axis at a time, in page pixels; the map is at 1/4 of that.
"""
from typing import List, NamedTuple, Tuple

import numpy as np


def round_up(v: int, m: int) -> int:
    return (int(v) + m - 1) // m * m


def check_tiling(tile: int, overlap: int) -> None:
    """The constraints of one axis: multiples of 32, 0 <= overlap <= tile / 2 (a pixel is covered by at most two tiles)."""
    if tile <= 0 or tile % 32:
        raise ValueError(f"tile size must be a positive multiple of 32, got {tile}")
    if overlap < 0 or overlap % 32 or 2 * overlap > tile:
        raise ValueError(f"tile overlap must be a multiple of 32 with 0 <= overlap <= tile / 2, got overlap {overlap} for tile {tile}")


def tile_grid(length: int, tile: int, overlap: int) -> Tuple[List[int], List[int]]:
    """One axis of `length` pixels -> (origins, cuts).  The axis is covered up to L32 = round_up(length, 32).  L32 <= tile: one
    tile at 0.  Otherwise n = ceil((L32 - overlap) / (tile - overlap)) tiles at min(i * (tile - overlap), L32 - tile): the last one
    is pulled back to end at L32.  cuts[i] is the middle of the overlap of tiles i and i + 1; tile i owns [cuts[i-1], cuts[i])."""
    length, tile, overlap = int(length), int(tile), int(overlap)
    if length <= 0:
        raise ValueError(f"length must be positive, got {length}")
    check_tiling(tile, overlap)
    L32, s = round_up(length, 32), tile - overlap
    if L32 <= tile:
        return [0], []
    n = -(-(L32 - overlap) // s)
    origins = [min(i * s, L32 - tile) for i in range(n)]
    cuts = [(origins[i] + tile + origins[i + 1]) // 2 for i in range(n - 1)]
    return origins, cuts


def owner_table(length: int, cuts: List[int]) -> np.ndarray:
    """Owning tile of every MAP pixel of the axis: int32 [round_up(length, 32) / 4]; map pixel m stands for page pixel 4 m."""
    pos = 4 * np.arange(round_up(length, 32) // 4)
    return np.searchsorted(np.asarray(cuts, dtype=np.int64), pos, side="right").astype(np.int32)


class PageGrid(NamedTuple):
    """Both axes of one page size: what the gather and stitch kernels read."""
    H: int
    W: int
    tile_h: int
    tile_w: int
    oy: np.ndarray        # int32 [ny] tile origins along y, page pixels
    ox: np.ndarray        # int32 [nx]
    cuts_y: List[int]
    cuts_x: List[int]
    row_tile: np.ndarray  # int32 [Hm] owning tile row of every map row
    col_tile: np.ndarray  # int32 [Wm] owning tile column of every map column

    @property
    def ny(self) -> int:
        return len(self.oy)

    @property
    def nx(self) -> int:
        return len(self.ox)

    @property
    def ntiles(self) -> int:
        return len(self.oy) * len(self.ox)

    @property
    def map_hw(self) -> Tuple[int, int]:
        return len(self.row_tile), len(self.col_tile)


def page_grid(H: int, W: int, tile_wh: Tuple[int, int], overlap: int) -> PageGrid:
    """The grid of an H x W page for tiles of tile_wh = (W, H) pixels."""
    tw, th = int(tile_wh[0]), int(tile_wh[1])
    oy, cy = tile_grid(H, th, overlap)
    ox, cx = tile_grid(W, tw, overlap)
    return PageGrid(int(H), int(W), th, tw, np.asarray(oy, dtype=np.int32), np.asarray(ox, dtype=np.int32), cy, cx,
                    owner_table(H, cy), owner_table(W, cx))
