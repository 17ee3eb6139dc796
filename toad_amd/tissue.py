"""Tissue selection on the device: from the pixels of one decoded uint8 region to the ``origins`` the region calls read
(``ResNet_Baseline.forward_u8_region``, ``eval.region_attention_scores``).

The reference tree has no patching script; its bags come from CLAM's, which thresholds HSV saturation and keeps the tiles that hold tissue.
Here the region is already resident when the extractor is called, so the decision is one streaming pass over its bytes (csrc/tissue.hip):
tissue pixels per ``cell x cell`` cell, then per tile of a lattice whose origin, tile shape and strides are multiples of the cell.

The pixel predicate is exact integer arithmetic: with ``mx = max(r, g, b)`` and ``mn = min(r, g, b)`` a pixel is tissue iff
``mx >= val_min and 255 * (mx - mn) > sat_thresh * mx`` - HSV saturation above ``sat_thresh`` on the 8-bit scale, written without the division.
It is not OpenCV's rounded ``S`` channel. ``val_min`` removes black scanner margins, whose JPEG noise is fully saturated; ``mx == 0`` is never tissue.

Conventions: ``tile`` = int or (H, W) as in ``ops.tile_shape``; ``stride`` = int or (sy, sx), the same order, default the tile shape;
``origin`` = (x, y) of the lattice's first tile, x first as in ``origins``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops


def _lattice_args(tile, stride, origin):
    h, w = ops.tile_shape(tile)
    sy, sx = (h, w) if stride is None else ops.tile_shape(stride)
    x0, y0 = origin
    if not (isinstance(x0, int) and isinstance(y0, int)) or x0 < 0 or y0 < 0:
        raise ValueError(f"origin must be (x, y), two non-negative ints, got {origin!r}")
    return h, w, sy, sx, x0, y0


def lattice(hr: int, wr: int, tile, stride=None, origin=(0, 0)):
    """(nx, ny): how many tiles of the lattice lie inside an hr x wr region - tile (j, i) at (x0 + i sx, y0 + j sy), i < nx, j < ny. Host arithmetic.
    Either is 0 where not even the first tile fits."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    nx = (wr - x0 - w) // sx + 1 if wr - x0 >= w else 0
    ny = (hr - y0 - h) // sy + 1 if hr - y0 >= h else 0
    return nx, ny


def lattice_cell(tile, stride=None, origin=(0, 0)) -> int:
    """The largest cell of 64, 32, 16, 8, 4 that divides the tile shape, the strides and the origin: every tile is then an exact union of whole cells."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    vals = (("tile height", h), ("tile width", w), ("stride y", sy), ("stride x", sx), ("origin x", x0), ("origin y", y0))
    for cell in ops.TISSUE_CELLS:
        if all(v % cell == 0 for _, v in vals):
            return cell
    name, v = next((k, v) for k, v in vals if v % 4)
    raise ValueError(f"{name} = {v} is not a multiple of 4: the tile shape, the strides and the origin of a tissue lattice must all be multiples of 4 "
                     "(tiles are summed from 4 x 4 pixel cells at the finest)")


def tissue_tile_fraction(region: torch.Tensor, tile=256, stride=None, origin=(0, 0), sat_thresh: int = 8, val_min: int = 0):
    """(counts, nx, ny): counts int32 [ny,nx] ON THE DEVICE = tissue pixels of every lattice tile inside the region (divide by H W for the fraction).
    Two launches, no synchronisation; an empty lattice (a region smaller than one tile) launches nothing. Defaults as in tissue_origins."""
    _, hr, wr = ops._region_pitch(region, "tissue_tile_fraction")
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    nx, ny = lattice(hr, wr, (h, w), (sy, sx), (x0, y0))
    if nx == 0 or ny == 0:
        return torch.empty((ny, nx), dtype=torch.int32, device=region.device), nx, ny
    cells = ops.region_tissue_cells(region, cell, sat_thresh, val_min)
    return ops.tissue_tile_counts(cells, cell, (x0, y0), (h, w), (sy, sx), (nx, ny)), nx, ny


def tissue_origins(region: torch.Tensor, tile=256, stride=None, min_fraction: float = 0.25, sat_thresh: int = 8, val_min: int = 0, origin=(0, 0),
                   return_counts: bool = False):
    """The origins of the lattice tiles that hold tissue: np.ndarray int64 [B,2] of (x, y) ON THE HOST (``ops.check_origins`` wants them there), in
    row-major order over the lattice, y outer and x inner. A tile is kept iff its tissue-pixel count >= ceil(min_fraction H W); min_fraction in [0, 1],
    0 keeps every tile, 1 only tiles that are tissue throughout. With ``return_counts`` also the kept tiles' counts, int64 [B].

    The call runs two launches and ONE device-to-host copy of ny nx int32 - its one synchronisation. A region smaller than one tile gives an empty
    [0,2] result, not an error.

    The defaults are API defaults in CLAM's units (its ``sthresh = 8``; min_fraction and val_min have no CLAM counterpart), not tuned values: CLAM
    thresholds a median-blurred, OpenCV-rounded saturation channel of a downsampled level, this is the exact per-pixel predicate at the region's level."""
    if not isinstance(min_fraction, (int, float)) or isinstance(min_fraction, bool) or not 0.0 <= min_fraction <= 1.0:
        raise ValueError(f"min_fraction must lie in [0, 1], got {min_fraction!r}")
    counts, nx, ny = tissue_tile_fraction(region, tile, stride, origin, sat_thresh, val_min)
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    if nx == 0 or ny == 0:
        empty = np.zeros((0, 2), dtype=np.int64)
        return (empty, np.zeros((0,), dtype=np.int64)) if return_counts else empty
    c = counts.cpu().numpy().astype(np.int64)                       # the one copy, the one synchronisation
    j, i = np.nonzero(c >= math.ceil(min_fraction * h * w))         # row-major: j (y) outer, i (x) inner
    origins = np.stack([x0 + i * sx, y0 + j * sy], axis=1).astype(np.int64)
    return (origins, c[j, i]) if return_counts else origins
