"""Attention heat maps on the device: from the scores of the tiles of one decoded uint8 region to the canvas a pathologist looks at, rendered where the
region lies (csrc/heatmap.hip). The stage behind ``eval.region_tissue_attention_scores``; the mirror image of ``toad_amd.tissue``.

CLAM draws its heat maps on the host: ``overlay[y:y+h, x:x+w] += score; counter[...] += 1``, divide, colour-map, ``addWeighted``. The same here, defined in
integers so that the canvas has one right answer:

* a score becomes ``q = round(clamp((s - lo) / (hi - lo), 0, 1) * 65535)``, and a NaN score makes its tile absent;
* a ``cell x cell`` cell (``tissue.lattice_cell``) covered by ``n`` present tiles whose ``q`` sum to ``S`` gets the colour index
  ``(2 S + 257 n) // (514 n)``, which is ``255 mean(q) / 65535`` rounded half up; a cell no present tile covers gets none;
* the canvas is the region box-filtered by ``down`` in 1, 2, 4 (mean rounded half up, partial boxes at the right and the bottom edge dropped), and on the
  cells with a colour ``(alpha lut[idx][c] + (256 - alpha) m + 128) >> 8`` with an integer ``alpha`` in [0, 256].

With ``smooth`` or a ``mask`` the colour index and the alpha are decided per canvas pixel (``ops.region_heat_blend_px``), still in integers. For canvas
pixel (ox, oy), ``own`` being the value of the cell that holds it:

* ``smooth``: ``idx_px`` is the bilinear tent between cell centres, in doubled coordinates. Along x ``p = 2 down ox + down - cell``,
  ``g0 = floor(p / (2 cell))`` (may be -1), ``f = p - 2 cell g0`` in [0, 2 cell), weights ``2 cell - f`` for cell g0 and ``f`` for g0 + 1; the same
  along y. A neighbour outside the table or without a value contributes ``own``; ``idx_px = (sum wy wx v + 2 cell^2) >> (2 log2(cell) + 2)``. The
  weights sum to ``4 cell^2``: a constant field is reproduced, and where a canvas pixel is a whole cell (``down = cell = 4``) nothing changes.
* ``mask`` = (plane, t, mask_down), a uint8 [Hr // mask_down, Wr // mask_down] plane with ``mask_down`` in 1, 2, 4, 8, 16, 32 and a multiple of ``down``:
  the pixel is tissue iff ``mx = (down ox) // mask_down`` and ``my = (down oy) // mask_down`` lie inside the plane and ``plane[my, mx] > t`` - the
  (plane, t) of ``tissue.segment_tissue`` read as it lies; the partial boxes the plane dropped are not tissue. Without a mask every pixel is tissue.
* the byte is ``(alpha lut[idx_px][c] + (256 - alpha) m + 128) >> 8`` where ``own >= 0`` and the pixel is tissue, ``m`` elsewhere: coverage edges and
  mask edges stay sharp, only the colour inside them is interpolated.

At overview scale - CLAM renders at a ``vis_level`` whose downsample is typically 16 to 64 - the same per-pixel definition holds with ``down`` in 8, 16,
32 (``ops.region_heat_thumb``): one pass over the region, no full-size canvas in between and no second rounding. There ``down`` must not exceed the
lattice's cell, so that a canvas box still lies in one cell, and ``mask_down`` is a multiple of ``down`` as before.

This is CLAM's ``segment=True``; ``smooth`` alone is one cell wide and removes the staircase inside a cell, not tile-to-tile score noise. ``thresh`` and
``binarize`` (CLAM's ``thresh``, ``binarize``) act on the tiles' scores before the table is built.

``blur`` (CLAM's ``blur``) smooths the cell table itself, before any of the above renders it (``ops.heat_cells_blur``, one launch over the small
``[Gy,Gx]`` table). CLAM blurs the overlay with ``cv2.GaussianBlur(overlay, (4 tile + 1, 4 tile + 1), 0)``, sigma = ``0.6 tile + 0.5`` pixels - about 2.4
cells on the usual 256 / 64 lattice, a field band-limited far below the cell pitch, which the tent then renders. In integers, with a half-kernel
``w[0 .. r]`` of ints, ``1 <= r <= 16``, ``w[0] >= 1``, ``w[d] >= 0``, ``w[0] + 2 sum w[1:] <= 1024`` (``gaussian_taps``):

* a cell without a value keeps none; otherwise, over ``dy, dx`` in ``-r .. r`` such that cell ``(gy + dy, gx + dx)`` lies inside the table and holds a
  value ``v``: ``N = sum w[|dy|] w[|dx|] min(v, 255)``, ``D = sum w[|dy|] w[|dx|]``, and the cell becomes ``(2 N + D) // (2 D)``;
* a normalised convolution: absent cells and cells outside the table carry no weight, so the colour does not fade towards the edge of the tissue
  (CLAM's zero-filled overlay does; this does not claim to be OpenCV bit for bit), a constant field is reproduced exactly, ``(k, 0, ..)`` is the
  identity, and nothing rounds before the one division: the result does not depend on summation order.

Conventions as in ``toad_amd.tissue``: ``tile`` = int or (H, W), ``stride`` = int or (sy, sx), ``origin`` = (x, y) of the lattice's first tile.
Not done here: a sigma per axis for tiles that are not square, radii above 16 cells (``blur=True`` on lattices whose cell is 16 or less), CLAM's second
blur of the coloured image and saving images. Several levels of the vis-level pyramid come from one read of the region: ``window_pyramid`` and
``attention_pyramid`` (``ops.region_heat_pyramid``), ``windows_pyramid`` for a list of windows in one call (``ops.region_heat_pyramid_windows``), and
``down`` as a sequence in the two ``eval`` heat-map calls.

A slide that arrives from the decoder in strips or blocks is rendered window by window with no seams: ``slide_cells`` builds the cell table of the whole
slide - only the lattice and the extent matter to it -, ``window_canvas`` renders one decoded window against that table (``ops.region_heat_window``: a
tent neighbour inside the table contributes its value also where it lies outside the window, and the mask is the slide's), and ``strip_plan`` says which
full-width strip owns which lattice rows and renders which canvas rows. ``attention_canvas`` is ``slide_cells`` plus the blend of one region that is the
whole image. ``eval.slide_attention_heatmap`` is the whole walk, with ONE percentile ranking over the slide."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .tissue import _lattice_args, lattice, lattice_cell


_JET = {}


def jet_lut(device) -> torch.Tensor:
    """The default colours, uint8 [256,3] on ``device``: an integer "jet" - channel k of entry i is ``clamp(765 - |8 i - 510 k|, 0, 510) // 2`` with
    k = 3, 2, 1 for r, g, b - from (0, 0, 127) over blue, cyan, green, yellow and red to (127, 0, 0). No matplotlib. Built and uploaded once per
    device; the tensor is shared between calls and must not be written to."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    lut = _JET.get(device)
    if lut is None:
        i = np.arange(256, dtype=np.int64)[:, None]
        k = np.array([3, 2, 1], dtype=np.int64)[None, :]
        lut = _JET[device] = torch.from_numpy((np.clip(765 - np.abs(8 * i - 510 * k), 0, 510) // 2).astype(np.uint8)).to(device)
    return lut


def quantise_scores(scores: torch.Tensor, score_range=(0, 1)) -> torch.Tensor:
    """int32 [B] on the scores' device: ``round(clamp((s - lo) / (hi - lo), 0, 1) * 65535)``, and -1 (absent) for a NaN score. The default range skips
    the subtraction and the division: exactly ``torch.round(s.clamp(0, 1) * 65535)``, what the percentile scores of ``eval`` need. Torch ops only."""
    lo, hi = score_range
    if not hi > lo:
        raise ValueError(f"score_range must be (lo, hi) with lo < hi, got {score_range!r}")
    s = scores.reshape(-1).to(torch.float32)
    if (lo, hi) != (0, 1):
        s = (s - lo) / (hi - lo)
    q = torch.round(s.clamp(0, 1) * 65535)
    return torch.where(torch.isnan(q), torch.full_like(q, -1), q).to(torch.int32)


def tile_table(origins, scores_q: torch.Tensor, tile, stride, origin, n) -> torch.Tensor:
    """The tile table of the heat-map kernels, int32 [ny,nx] on the device of ``scores_q``: -1 everywhere except at the tiles of ``origins`` ([B,2] of
    (x, y) on the host, as ``tissue.tissue_origins`` returns them), which take their ``scores_q``. Host arithmetic maps each (x, y) to its lattice index
    j nx + i and raises ValueError for an origin off the lattice, outside it or given twice; then one index upload and one scatter, deterministic
    because no index repeats. n = (nx, ny)."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    nx, ny = n
    o = np.asarray(origins)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError(f"origins must be [B,2] integers (x, y), got shape {o.shape} dtype {o.dtype}")
    o = o.astype(np.int64)
    if scores_q.dim() != 1 or scores_q.shape[0] != o.shape[0] or scores_q.dtype != torch.int32:
        raise ValueError(f"scores_q must be int32 [{o.shape[0]}], one per origin, got {scores_q.dtype} {tuple(scores_q.shape)}")
    dx, dy = o[:, 0] - x0, o[:, 1] - y0
    i, j = dx // sx, dy // sy
    for name, bad in (("off the lattice", (dx % sx != 0) | (dy % sy != 0)), ("outside the lattice", (i < 0) | (i >= nx) | (j < 0) | (j >= ny))):
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise ValueError(f"origins[{b}] = (x={int(o[b, 0])}, y={int(o[b, 1])}) is {name}: origin ({x0}, {y0}), stride (sy, sx) = ({sy}, {sx}), "
                             f"{nx} x {ny} tiles (nx x ny)")
    idx = j * nx + i
    uniq, first = np.unique(idx, return_index=True)
    if uniq.size != idx.size:
        b = int(np.setdiff1d(np.arange(idx.size), first)[0])
        raise ValueError(f"origins[{b}] = (x={int(o[b, 0])}, y={int(o[b, 1])}) is given twice: a tile has one score")
    table = torch.full((ny * nx,), -1, dtype=torch.int32, device=scores_q.device)
    if idx.size:
        table[torch.from_numpy(idx).to(scores_q.device)] = scores_q
    return table.view(ny, nx)


def _alpha_arg(alpha) -> int:
    if isinstance(alpha, float) and 0.0 <= alpha <= 1.0:
        return int(round(256 * alpha))
    if isinstance(alpha, int) and not isinstance(alpha, bool) and 0 <= alpha <= 256:
        return alpha
    raise ValueError(f"alpha must be an int in [0, 256] or a float in [0, 1] (meaning round(256 alpha)), got {alpha!r}")


def select_scores(scores: torch.Tensor, scores_q: torch.Tensor, thresh=None, binarize: bool = False) -> torch.Tensor:
    """CLAM's ``thresh`` and ``binarize`` on quantised scores, int32 [B]: a tile whose raw score is below ``thresh`` becomes absent (-1; CLAM keeps
    ``score >= threshold``, and a NaN score, which is >= nothing, stays absent), and with ``binarize`` every present tile gets q = 65535. Torch ops only,
    no synchronisation."""
    q = scores_q
    if thresh is not None:
        q = torch.where(scores.reshape(-1) >= thresh, q, torch.full_like(q, -1))
    if binarize:
        q = torch.where(q >= 0, torch.full_like(q, 65535), q)
    return q


def _mask_arg(mask):
    if mask is None:
        return None, None, 0
    if not isinstance(mask, (tuple, list)) or len(mask) != 3:
        raise ValueError("mask must be None or a (plane, t, mask_down) triple: the plane and the threshold of tissue.segment_tissue and its down")
    return mask


def gaussian_taps(sigma_cells, radius=None) -> tuple:
    """The half-kernel ``w[0 .. r]`` of ``ops.heat_cells_blur`` for a Gaussian of ``sigma_cells`` cells, a tuple of Python ints: ``g[d] = exp(-d^2 / (2
    sigma^2))`` in float64, ``G = g[0] + 2 sum g[1:]``, ``w[d] = floor((1023 - 2 r) g[d] / G + 0.5)``. ``radius`` defaults to ``ceil(3 sigma)``. Each of
    the ``2 r + 1`` taps of the full kernel rounds by at most a half, so the scale ``1023 - 2 r`` keeps the full sum in ``[1024 - 2 (2 r + 1), 1024]``
    with no fix-up step; the taps are symmetric by construction, non-increasing, and ``w[0] >= 1``. ValueError for a sigma that is not a positive finite
    number and for a radius outside 1 .. ``ops.HEAT_BLUR_RADIUS`` = 16 cells."""
    if isinstance(sigma_cells, bool) or not isinstance(sigma_cells, (int, float, np.integer, np.floating)) or not 0 < float(sigma_cells) < math.inf:
        raise ValueError(f"gaussian_taps: sigma must be a positive finite number of cells, got {sigma_cells!r}")
    sigma = float(sigma_cells)
    if radius is None:
        radius = max(1, math.ceil(3 * sigma))
        if radius > ops.HEAT_BLUR_RADIUS:
            raise ValueError(f"gaussian_taps: sigma = {sigma:g} cells needs a radius of ceil(3 sigma) = {radius} cells, above the limit of "
                             f"{ops.HEAT_BLUR_RADIUS} cells (a coarser lattice cell, a smaller sigma or an explicit radius)")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= ops.HEAT_BLUR_RADIUS:
        raise ValueError(f"gaussian_taps: radius must be an int in 1 .. {ops.HEAT_BLUR_RADIUS} cells (sigma = {sigma:g} cells), got {radius!r}")
    r = int(radius)
    g = [math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(r + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    return tuple(int(math.floor((1023 - 2 * r) * gd / total + 0.5)) for gd in g)


def blur_taps(blur, tile, cell):
    """The ``blur`` keyword of ``attention_canvas`` -> None (no blur) or the taps of ``ops.heat_cells_blur``; ``tile`` = (h, w) and ``cell`` are the
    lattice's. False / None: None. True: CLAM's width, ``cv2.GaussianBlur(overlay, (4 tile + 1, 4 tile + 1), 0)``, whose sigma is ``0.3 ((k - 1) / 2
    - 1) + 0.8 = 0.6 tile + 0.5`` pixels - a square tile only. A positive number: sigma in region pixels. A sequence of ints: the taps themselves.
    ValueError otherwise, and where the Gaussian needs more than ``ops.HEAT_BLUR_RADIUS`` cells."""
    if blur is None or blur is False:
        return None
    h, w = tile
    if blur is True:
        if h != w:
            raise ValueError(f"attention_canvas: blur=True is CLAM's width 0.6 tile + 0.5 and needs a square tile, got (H, W) = {(h, w)}; give sigma in "
                             "pixels or the taps (per-axis sigma is not done)")
        return gaussian_taps((0.6 * h + 0.5) / cell)
    if isinstance(blur, (int, float, np.integer, np.floating)):
        if not 0 < float(blur) < math.inf:
            raise ValueError(f"attention_canvas: blur as a number is sigma in region pixels and must be positive and finite, got {blur!r}")
        return gaussian_taps(float(blur) / cell)
    return ops.heat_blur_taps("attention_canvas: blur", blur)


def slide_cells(slide_hw, origins, scores: torch.Tensor, tile=256, stride=None, origin=(0, 0), score_range=(0, 1), thresh=None, binarize: bool = False,
                blur=False, name: str = "slide_cells"):
    """``(cells, cell)``: the cell table of a whole image of ``slide_hw`` = (Hs, Ws) pixels - int32 [ceil(Hs / cell), ceil(Ws / cell)] on the device of
    ``scores`` - and the lattice's cell (``tissue.lattice_cell``). The first half of ``attention_canvas``: the scores are quantised
    (``quantise_scores``), ``thresh`` and ``binarize`` applied (``select_scores``), the tile table built (``tile_table``), the cells summed
    (``ops.heat_cells``) and, with ``blur``, smoothed (``ops.heat_cells_blur``; ``blur_taps``). Only the lattice and the extent matter: no pixel is
    involved, so the table of a slide that arrives strip by strip is built once and rendered window by window (``window_canvas``). Empty ``origins``
    give a table of -1 and launch nothing. ``name`` is the caller's, for messages."""
    hs, ws = slide_hw
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    if not isinstance(scores, torch.Tensor):
        raise ValueError(f"{name}: scores must be a tensor on the device, got {type(scores).__name__}")
    if not isinstance(binarize, bool):
        raise ValueError(f"{name}: binarize must be a bool, got {binarize!r}")
    if thresh is not None and (isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or thresh != thresh):
        raise ValueError(f"{name}: thresh must be None or a number (a raw score), got {thresh!r}")
    taps = blur_taps(blur, (h, w), cell)
    nx, ny = lattice(hs, ws, (h, w), (sy, sx), (x0, y0))
    table = tile_table(origins, select_scores(scores, quantise_scores(scores, score_range), thresh, binarize), (h, w), (sy, sx), (x0, y0), (nx, ny))
    if table.numel() and len(origins):
        cells = ops.heat_cells(table, cell, (x0, y0), (h, w), (sy, sx), (nx, ny), (hs, ws))
        if taps is not None:
            cells = ops.heat_cells_blur(cells, taps)
    else:
        cells = torch.full((-(-hs // cell), -(-ws // cell)), -1, dtype=torch.int32, device=scores.device)
    return cells, cell


def window_canvas(region: torch.Tensor, window, cells: torch.Tensor, cell: int, alpha=102, down: int = 1, lut=None, out=None, smooth: bool = False,
                  mask=None) -> torch.Tensor:
    """The heat map of one window of a slide: uint8 [Hr // down, Wr // down, 3] on the device, byte for byte the rows from ``wy // down`` and the columns
    from ``wx // down`` of the canvas ``attention_canvas`` gives for the whole slide. ``region`` [Hr,Wr,3] is the decoded window, ``window`` = (wx, wy)
    its place in the slide - multiples of max(4, ``down``) - ``cells`` and ``cell`` the slide's table from ``slide_cells``, ``mask`` the SLIDE-wide
    (plane, t, mask_down) triple. ``alpha``, ``down`` (any of 1 .. 32), ``lut``, ``smooth``: ``attention_canvas``; ``out`` may be the window's rows and
    columns of the slide's canvas. The second half of ``attention_canvas``, through ``ops.region_heat_window``: one launch."""
    a = _alpha_arg(alpha)
    if not isinstance(smooth, bool):
        raise ValueError(f"window_canvas: smooth must be a bool, got {smooth!r}")
    plane, t, mask_down = _mask_arg(mask)
    lut = jet_lut(region.device) if lut is None else lut
    return ops.region_heat_window(region, window, cells, cell, lut, a, down, smooth=smooth, mask=plane, mask_down=mask_down if plane is not None else None,
                                  mask_thresh=t if plane is not None else 0, out=out)


def windows_canvas(regions, windows, cells: torch.Tensor, cell: int, alpha=102, down: int = 1, lut=None, outs=None, smooth: bool = False, mask=None) -> tuple:
    """``window_canvas`` for a list of windows of one slide: a tuple of uint8 [Hr_k // down, Wr_k // down, 3] canvases, canvas k byte for byte
    ``window_canvas(regions[k], windows[k], ...)``. ``regions`` are the decoded windows - blocks, strips, of any extents - ``windows`` their places
    (wx, wy) in the slide, ``outs`` None or one view per window, for example each window's rows and columns of the slide's canvas; everything else is
    the slide's and shared. Through ``ops.region_heat_windows``: one library call, one launch per ``ops.HEAT_LIST_MAX`` windows."""
    a = _alpha_arg(alpha)
    if not isinstance(smooth, bool):
        raise ValueError(f"windows_canvas: smooth must be a bool, got {smooth!r}")
    plane, t, mask_down = _mask_arg(mask)
    if lut is None:
        first = regions[0] if not isinstance(regions, torch.Tensor) and hasattr(regions, "__len__") and len(regions) else cells
        lut = jet_lut(first.device if isinstance(first, torch.Tensor) else cells.device)
    return ops.region_heat_windows(regions, windows, cells, cell, lut, a, down, smooth=smooth, mask=plane, mask_down=mask_down if plane is not None else None,
                                   mask_thresh=t if plane is not None else 0, outs=outs)


def window_pyramid(region: torch.Tensor, window, cells: torch.Tensor, cell: int, alpha=102, downs=(1, 4, 16), lut=None, outs=None, smooth: bool = False,
                   mask=None) -> tuple:
    """``window_canvas`` at several levels from ONE read of the window: a tuple of uint8 [Hr // down, Wr // down, 3] canvases in the order of ``downs``,
    each byte for byte ``window_canvas`` at that ``down``. ``downs``: distinct values from 1 .. 32; ``window`` = (wx, wy) in multiples of
    max(4, max(downs)), and the lattice's cell and the mask's ``mask_down`` must suit max(downs) as they must suit ``down`` there. ``outs``: None or one
    view per level, for example the window's rows and columns of per-level slide canvases. Through ``ops.region_heat_pyramid``: one launch."""
    a = _alpha_arg(alpha)
    if not isinstance(smooth, bool):
        raise ValueError(f"window_pyramid: smooth must be a bool, got {smooth!r}")
    plane, t, mask_down = _mask_arg(mask)
    lut = jet_lut(region.device) if lut is None else lut
    return ops.region_heat_pyramid(region, window, cells, cell, lut, a, downs, smooth=smooth, mask=plane, mask_down=mask_down if plane is not None else None,
                                   mask_thresh=t if plane is not None else 0, outs=outs)


def windows_pyramid(regions, windows, cells: torch.Tensor, cell: int, alpha=102, downs=(1, 4, 16), lut=None, outs=None, smooth: bool = False,
                    mask=None) -> tuple:
    """``window_pyramid`` for a list of windows of one slide: a tuple with one tuple of canvases per window, in the order of ``downs``, window k's
    byte for byte ``window_pyramid(regions[k], windows[k], ...)``. ``regions`` are the decoded windows - blocks, strips, of any extents -
    ``windows`` their places (wx, wy) in the slide, multiples of max(4, max(downs)); ``outs`` None or per window one view per level, for example each
    window's rows and columns of per-level slide canvases; everything else is the slide's and shared. Through ``ops.region_heat_pyramid_windows``: one
    library call, one launch per ``ops.HEAT_PYR_LIST_MAX`` windows, one read of every window."""
    a = _alpha_arg(alpha)
    if not isinstance(smooth, bool):
        raise ValueError(f"windows_pyramid: smooth must be a bool, got {smooth!r}")
    plane, t, mask_down = _mask_arg(mask)
    if lut is None:
        first = regions[0] if not isinstance(regions, torch.Tensor) and hasattr(regions, "__len__") and len(regions) else cells
        lut = jet_lut(first.device if isinstance(first, torch.Tensor) else cells.device)
    return ops.region_heat_pyramid_windows(regions, windows, cells, cell, lut, a, downs, smooth=smooth, mask=plane,
                                           mask_down=mask_down if plane is not None else None, mask_thresh=t if plane is not None else 0, outs=outs)


def strip_plan(slide_hw, strips, tile=256, stride=None, origin=(0, 0), down: int = 1):
    """How a slide of ``slide_hw`` = (Hs, Ws) pixels that arrives as full-width row strips is scored and rendered strip by strip. Host arithmetic only.
    ``strips`` = [(y_k, H_k)]: strip k holds the slide's rows y_k .. y_k + H_k, sorted, each abutting or overlapping the one before. One dict per strip:

    * ``rows`` = (j0, j1): the lattice rows j0 <= j < j1 the strip owns - a tile row (y0 + j sy .. + h) belongs to the FIRST strip that holds it whole;
    * ``origin`` = (x, y): the lattice origin of row j0 inside the strip, for ``tissue.tissue_origins`` / ``forward_u8_region`` on the strip (every
      lattice tile of the strip from there on is one it owns; add (0, y_k) for slide coordinates). None where the strip owns no row;
    * ``render`` = (r0, r1): the slide rows it renders, from max(y_k, the end of the previous strip) to its own end.

    ValueError for strips that are not sorted or leave a gap, that do not cover 0 .. Hs, for a lattice tile row that lies whole in no strip (the strips
    must overlap by at least tile - stride rows), and for a render start that is not a multiple of max(4, ``down``) (``ops.region_heat_window``).
    ``down`` may be a sequence of levels (``window_pyramid``): the alignment is then that of its largest."""
    hs, ws = slide_hw
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    _, ny = lattice(hs, ws, (h, w), (sy, sx), (x0, y0))
    if isinstance(down, (tuple, list)):
        down = max(ops.heat_downs_arg("strip_plan", down))
    if down not in ops.HEAT_DOWNS + ops.HEAT_THUMB_DOWNS:
        raise ValueError(f"strip_plan: down must be one of {ops.HEAT_DOWNS + ops.HEAT_THUMB_DOWNS}, got {down!r}")
    strips = [(int(y), int(n)) for y, n in strips]
    if not strips or strips[0][0] != 0 or strips[-1][0] + strips[-1][1] != hs:
        raise ValueError(f"strip_plan: the strips must cover rows 0 .. Hs = {hs}, got {strips!r}")
    align, plan, end, j = max(4, down), [], 0, 0
    for k, (y, n) in enumerate(strips):
        if n < 1 or y + n <= end or (k and y <= strips[k - 1][0]):
            raise ValueError(f"strip_plan: strip {k} = (y, H) = {(y, n)} is empty or not sorted after the strips before it (rows up to {end})")
        if y > end:
            raise ValueError(f"strip_plan: a gap between strip {k - 1}, which ends at row {end}, and strip {k}, which starts at row {y}")
        r0 = max(y, end)
        if r0 % align:
            raise ValueError(f"strip_plan: strip {k} renders from row {r0}, not a multiple of max(4, down) = {align}")
        if j < ny and y0 + j * sy < y:
            raise ValueError(f"strip_plan: lattice tile row {j} (rows {y0 + j * sy} .. {y0 + j * sy + h}) lies whole in no strip: strips {k - 1} and {k} "
                             f"overlap by {end - y} rows, less than tile - stride = {h - sy}")
        j0 = j
        while j < ny and y0 + j * sy + h <= y + n:
            j += 1
        plan.append(dict(rows=(j0, j), origin=(x0, y0 + j0 * sy - y) if j > j0 else None, render=(r0, y + n)))
        end = y + n
    return plan


def attention_canvas(region: torch.Tensor, origins, scores: torch.Tensor, tile=256, stride=None, origin=(0, 0), alpha=102, down: int = 1, lut=None,
                     score_range=(0, 1), out=None, smooth: bool = False, mask=None, thresh=None, binarize: bool = False, blur=False) -> torch.Tensor:
    """The heat map of one decoded uint8 region [Hr,Wr,3]: uint8 [Hr // down, Wr // down, 3] ON THE DEVICE. ``origins`` [B,2] of (x, y) on the host are
    tiles of the lattice (tile, stride, origin) inside the region - ``tissue.tissue_origins`` with the same arguments gives such - and ``scores`` their B
    scores on the device, in that order. The definition is the module's. ``alpha`` an int in [0, 256] or a float in [0, 1] (the default 102 is CLAM's
    0.4), ``lut`` uint8 [256,3] on the device (default ``jet_lut``), ``out`` as in ``ops.region_heat_blend``.

    ``smooth`` interpolates the colour index between cell centres and ``mask`` = (plane, t, mask_down) blends only tissue pixels (the module's per-pixel
    definition; without either ``ops.region_heat_blend_px`` is ``ops.region_heat_blend``, the same kernel). ``thresh`` makes a tile absent whose raw score is below
    it, ``binarize`` gives every present tile the top colour (``select_scores``).

    ``down`` in 8, 16, 32 renders the overview canvas through ``ops.region_heat_thumb`` with the same keywords and the same meaning; the lattice's cell
    (``tissue.lattice_cell``) must be at least ``down`` (ValueError otherwise, before anything is launched).

    ``blur`` smooths the cell table between ``ops.heat_cells`` and the blend (``ops.heat_cells_blur``, the module's normalised convolution; ``blur_taps``):
    False / None - today's launches and today's bytes; True - CLAM's width, sigma = ``0.6 tile + 0.5`` pixels (a square tile); a positive number - sigma
    in region pixels; a sequence of ints - the taps. ``thresh`` and ``binarize`` act before it, ``smooth``, ``mask`` and every ``down`` after it, unchanged.
    ValueError before anything is launched for any other value and for a Gaussian wider than 16 cells (``blur=True`` on a lattice whose cell is 16 or less).

    Two launches (three with ``blur``) and a few small torch ops, no synchronisation. Empty ``origins`` give the box-filtered region and launch no blur."""
    _, hr, wr = ops._region_pitch(region, "attention_canvas")
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    thumb = down in ops.HEAT_THUMB_DOWNS
    if thumb and cell < down:
        raise ValueError(f"attention_canvas: down = {down} exceeds the lattice's cell = {cell} (tile {(h, w)}, stride {(sy, sx)}, origin {(x0, y0)}): a canvas "
                         "box must lie in one cell")
    a = _alpha_arg(alpha)
    if not isinstance(scores, torch.Tensor) or scores.device != region.device:
        raise ValueError(f"attention_canvas: scores must be a tensor on the region's device ({region.device}), got "
                         f"{scores.device if isinstance(scores, torch.Tensor) else type(scores).__name__}")
    if not isinstance(smooth, bool) or not isinstance(binarize, bool):
        raise ValueError(f"attention_canvas: smooth and binarize must be bools, got {smooth!r} and {binarize!r}")
    if thresh is not None and (isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or thresh != thresh):
        raise ValueError(f"attention_canvas: thresh must be None or a number (a raw score), got {thresh!r}")
    plane, t, mask_down = _mask_arg(mask)
    cells, cell = slide_cells((hr, wr), origins, scores, (h, w), (sy, sx), (x0, y0), score_range, thresh, binarize, blur, name="attention_canvas")
    lut = jet_lut(region.device) if lut is None else lut
    blend = ops.region_heat_thumb if thumb else ops.region_heat_blend_px
    return blend(region, cells, cell, lut, a, down, smooth=smooth, mask=plane, mask_down=mask_down if plane is not None else None,
                 mask_thresh=t if plane is not None else 0, out=out)


def attention_pyramid(region: torch.Tensor, origins, scores: torch.Tensor, tile=256, stride=None, origin=(0, 0), alpha=102, downs=(1, 4, 16), lut=None,
                      score_range=(0, 1), outs=None, smooth: bool = False, mask=None, thresh=None, binarize: bool = False, blur=False) -> tuple:
    """``attention_canvas`` at several levels: a tuple of uint8 [Hr // down, Wr // down, 3] canvases in the order of ``downs``, each byte for byte
    ``attention_canvas`` at that ``down``. ``slide_cells`` builds the cell table ONCE, ``window_pyramid`` at (0, 0) renders every level from one read of
    the region. The lattice's cell must be at least max(downs) where that is 8 or more, a mask's ``mask_down`` a multiple of max(downs); ``smooth`` on a
    lattice whose cell is 4 is not done for more than one level. The other keywords: ``attention_canvas``; ``outs``: ``window_pyramid``."""
    _, hr, wr = ops._region_pitch(region, "attention_pyramid")
    ds = ops.heat_downs_arg("attention_pyramid", downs)
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    if max(ds) > cell:
        raise ValueError(f"attention_pyramid: down = {max(ds)}, the largest level, exceeds the lattice's cell = {cell} (tile {(h, w)}, stride {(sy, sx)}, "
                         f"origin {(x0, y0)}): a canvas box must lie in one cell")
    _alpha_arg(alpha)
    if not isinstance(scores, torch.Tensor) or scores.device != region.device:
        raise ValueError(f"attention_pyramid: scores must be a tensor on the region's device ({region.device}), got "
                         f"{scores.device if isinstance(scores, torch.Tensor) else type(scores).__name__}")
    if not isinstance(smooth, bool):
        raise ValueError(f"attention_pyramid: smooth must be a bool, got {smooth!r}")
    cells, cell = slide_cells((hr, wr), origins, scores, (h, w), (sy, sx), (x0, y0), score_range, thresh, binarize, blur, name="attention_pyramid")
    return window_pyramid(region, (0, 0), cells, cell, alpha=alpha, downs=ds, lut=lut, outs=outs, smooth=smooth, mask=mask)
