"""Tissue selection on the device: from the pixels of one decoded uint8 region to the ``origins`` the region calls read
(``ResNet_Baseline.forward_u8_region``, ``eval.region_attention_scores``).

The reference tree has no patching script; its bags come from CLAM's, which thresholds HSV saturation and keeps the tiles that hold tissue.
Here the region is already resident when the extractor is called, so the decision is made where it lies. There are two selectors.

``tissue_origins`` (csrc/tissue.hip) - one streaming pass over the region's bytes: tissue pixels per ``cell x cell`` cell, then per tile of a lattice
whose origin, tile shape and strides are multiples of the cell. The pixel predicate is exact integer arithmetic: with ``mx = max(r, g, b)`` and
``mn = min(r, g, b)`` a pixel is tissue iff ``mx >= val_min and 255 * (mx - mn) > sat_thresh * mx`` - HSV saturation above ``sat_thresh`` on the 8-bit
scale, written without the division. It is not OpenCV's rounded ``S`` channel. ``val_min`` removes black scanner margins, whose JPEG noise is fully
saturated; ``mx == 0`` is never tissue.

``segmented_tissue_origins`` (csrc/tissue_seg.hip) - CLAM's recipe, defined in integers:

1. box filter: ``down`` in 1, 2, 4, 8, 16, 32; ``Hp = Hr // down``, ``Wp = Wr // down``, partial boxes at the right and the bottom edge dropped; the
   mean pixel of a box is ``(sum + down * down // 2) // (down * down)`` per channel. An empty plane launches nothing.
2. saturation byte: on the mean pixel ``S = (255 * (mx - mn) + (mx >> 1)) // mx`` - ``255 (mx - mn) / mx`` rounded half up - and ``S = 0`` where
   ``mx == 0`` or ``mx < val_min``. Exact for every ``(mx, mn)``; not claimed to be bit-equal to OpenCV's ``COLOR_RGB2HSV``.
3. median: ``median`` = k in 1, 3, 5, 7; the ``(k * k) // 2``-th of the sorted ``k * k`` values of the window around each plane pixel, coordinates
   clamped to the plane (replicate border, as ``cv2.medianBlur``); k = 1 is the identity; planes smaller than the window are fine.
4. histogram: ``hist[v]`` = the pixels of the median plane equal to ``v``, int32 [256].
5. Otsu (``otsu_threshold``, on the host): with ``N = sum h``, ``MT = sum i h[i]``, ``W0(t) = sum_{i<=t} h[i]``, ``M0(t) = sum_{i<=t} i h[i]``,
   ``W1 = N - W0``, the smallest ``t`` in 0..254 that maximises ``(MT W0 - M0 N)^2 / (W0 W1)`` over the ``t`` with ``W0 > 0`` and ``W1 > 0`` - the
   between-class variance up to the constant ``N^2`` - and 0 if there is none. Fractions are compared by cross-multiplication in Python ints. First
   maximum, and 0 when degenerate, is what OpenCV's Otsu gives too.
6. tissue: a plane pixel is tissue iff its median-filtered ``S > t`` (``THRESH_BINARY``), ``t`` the caller's ``sat_thresh`` in 0..255 or Otsu's.
7. tiles: the lattice is given at the region's level and all six numbers must be multiples of ``4 * down``; in plane units it is then a lattice of
   multiples of 4 and ``lattice_cell`` applies unchanged. The extent is ``lattice(Hr, Wr, ...)``; a tile is kept iff its tissue count
   ``>= ceil(min_fraction * (H // down) * (W // down))``.

Between steps 6 and 7 the mask ``M0`` of step 6 may pass through the remaining steps of CLAM's ``segmentTissue`` (csrc/tissue_morph.hip), each switched
on by its keyword and skipped entirely at its default:

6a. closing: ``close`` = c in 0..8, 0 and 1 the identity; ``lo = c // 2``, ``hi = c - 1 - c // 2``. Dilation: ``D[y,x]`` is the OR of ``M0[y+dy, x+dx]``
    over ``-lo <= dy, dx <= hi``, the window clipped to the plane; erosion: ``M1[y,x]`` is the AND of ``D`` over the same offsets, clipped the same way.
    This is ``cv2.morphologyEx(m, MORPH_CLOSE, np.ones((c, c)))`` as OpenCV defines it - the default anchor ``(c // 2, c // 2)`` for both halves, which is
    why an even c shifts by a pixel; border pixels ignored - stated, not tested: not claimed bit-equal to OpenCV.
6b. small components: ``min_area`` = a >= 0 plane pixels. The 8-connected components of ``M1`` with fewer than a pixels are removed (kept iff
    ``count >= min_area``; CLAM keeps ``a > a_t``). This gives ``M2``. 0 and 1 remove nothing and launch nothing.
6c. small holes: ``min_hole`` = h >= 0 plane pixels. The 4-connected components of the complement of ``M2`` are labelled; one is a hole iff none of its
    pixels lies in row 0, row ``Hp - 1``, column 0 or column ``Wp - 1``; a hole with fewer than h pixels becomes tissue. This gives ``M3``, on which step
    7 runs unchanged. 0 launches nothing.

The order is closing, components, holes: after 6b every remaining component is kept, so a hole never needs to know its enclosing component, and an island
removed in 6b merges into the hole around it before 6c counts that hole. The areas are pixel counts of the unfilled component - CLAM's
``contourArea(outer) - sum(contourArea(holes))`` but for the polygon-versus-pixel difference. From CLAM's units (multiples of a 512 x 512 reference patch at
level 0): ``min_area = a_t * 512^2 / (level downsample * down)^2``, and ``min_hole`` from ``a_h`` alike.

Dust, JPEG speckle and single saturated pixels on glass are tissue for the first selector and vanish under the median of the second. Not done:
``max_n_holes``, polygon areas.

A slide that arrives in strips (``segment_tissue_strips``, ``segmented_slide_origins``; ``eval.slide_attention_heatmap(segment=...)``): only steps 1 and 2
touch the slide's pixels, and plane row ``r`` depends on the slide rows ``r down .. (r + 1) down`` alone. So the plane is put together from the strips -
``plane_strip_plan`` says which strip gives which rows, ``slide_saturation`` writes them in ONE launch for all strips (``ops.regions_saturation``,
``sat_plane_list_kernel``) - and is byte for byte the plane of the whole slide, provided every plane row lies whole in some strip. Steps 3 to 7 then run
once on that plane and see across the seams; there is one read-back for the slide. Several regions per call are done for steps 1 and 2 only.

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


def _min_fraction_arg(min_fraction):
    if not isinstance(min_fraction, (int, float)) or isinstance(min_fraction, bool) or not 0.0 <= min_fraction <= 1.0:
        raise ValueError(f"min_fraction must lie in [0, 1], got {min_fraction!r}")


def _kept(counts, need: int, x0: int, y0: int, sx: int, sy: int):
    """(origins, counts) of the lattice tiles whose count is >= need, from the device table int32 [ny,nx] (None: an empty lattice, nothing is copied).
    Origins int64 [B,2] of (x, y), row-major over the lattice - j (y) outer, i (x) inner; counts int64 [B]. The call's one copy and synchronisation."""
    if counts is None:
        return np.zeros((0, 2), dtype=np.int64), np.zeros((0,), dtype=np.int64)
    c = counts.cpu().numpy().astype(np.int64)
    j, i = np.nonzero(c >= need)
    return np.stack([x0 + i * sx, y0 + j * sy], axis=1).astype(np.int64), c[j, i]


def tissue_origins(region: torch.Tensor, tile=256, stride=None, min_fraction: float = 0.25, sat_thresh: int = 8, val_min: int = 0, origin=(0, 0),
                   return_counts: bool = False):
    """The origins of the lattice tiles that hold tissue: np.ndarray int64 [B,2] of (x, y) ON THE HOST (``ops.check_origins`` wants them there), in
    row-major order over the lattice, y outer and x inner. A tile is kept iff its tissue-pixel count >= ceil(min_fraction H W); min_fraction in [0, 1],
    0 keeps every tile, 1 only tiles that are tissue throughout. With ``return_counts`` also the kept tiles' counts, int64 [B].

    The call runs two launches and ONE device-to-host copy of ny nx int32 - its one synchronisation. A region smaller than one tile gives an empty
    [0,2] result, not an error.

    The defaults are API defaults in CLAM's units (its ``sthresh = 8``; min_fraction and val_min have no CLAM counterpart), not tuned values: CLAM
    thresholds a median-blurred, OpenCV-rounded saturation channel of a downsampled level, this is the exact per-pixel predicate at the region's level.
    ``segmented_tissue_origins`` is the selector that follows CLAM's recipe (box filter, median, fixed or Otsu threshold)."""
    _min_fraction_arg(min_fraction)
    counts, nx, ny = tissue_tile_fraction(region, tile, stride, origin, sat_thresh, val_min)
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    origins, kept = _kept(counts if nx and ny else None, math.ceil(min_fraction * h * w), x0, y0, sx, sy)
    return (origins, kept) if return_counts else origins


def otsu_threshold(hist) -> int:
    """Otsu's threshold of a 256-bin histogram (any 256-long integer sequence, numpy array or CPU tensor), in Python ints: with N = sum h,
    MT = sum i h[i], W0(t) = sum_{i<=t} h[i], M0(t) = sum_{i<=t} i h[i] and W1 = N - W0, the smallest t in 0..254 that maximises
    (MT W0 - M0 N)^2 / (W0 W1) over the t with W0 > 0 and W1 > 0; 0 if there is no such t (an empty or a one-bin histogram). The fractions are compared
    by cross-multiplication - the squares reach about 2^116, beyond float and int64. A pixel is then tissue iff its value > t."""
    if isinstance(hist, torch.Tensor):
        hist = hist.tolist()
    h = [int(v) for v in hist]
    if len(h) != 256 or any(v < 0 for v in h):
        raise ValueError(f"otsu_threshold: expected 256 non-negative counts, got {len(h)} values" + ("" if len(h) != 256 else ", some negative"))
    n, mt = sum(h), sum(i * v for i, v in enumerate(h))
    best, num, den = 0, -1, 1
    w0 = m0 = 0
    for t in range(255):
        w0 += h[t]
        m0 += t * h[t]
        w1 = n - w0
        if w0 <= 0 or w1 <= 0:
            continue
        a, d = (mt * w0 - m0 * n) ** 2, w0 * w1
        if a * den > num * d:                                       # strictly above the best so far: the FIRST maximum stays
            best, num, den = t, a, d
    return best


def _seg_args(down, median, sat_thresh, val_min):
    if down not in ops.SEG_DOWNS:
        raise ValueError(f"down must be one of {ops.SEG_DOWNS}, got {down!r}")
    if median not in ops.SEG_MEDIANS:
        raise ValueError(f"median must be one of {ops.SEG_MEDIANS}, got {median!r}")
    if sat_thresh != "otsu" and (not isinstance(sat_thresh, int) or isinstance(sat_thresh, bool) or not 0 <= sat_thresh <= 255):
        raise ValueError(f"sat_thresh must be 'otsu' or an int in [0, 255] (the 8-bit scale), got {sat_thresh!r}")
    if not isinstance(val_min, int) or isinstance(val_min, bool) or not 0 <= val_min <= 255:
        raise ValueError(f"val_min must be an int in [0, 255] (the 8-bit scale), got {val_min!r}")


def _morph_args(close, min_area, min_hole):
    if not isinstance(close, int) or isinstance(close, bool) or close not in ops.SEG_CLOSES:
        raise ValueError(f"close must be one of {ops.SEG_CLOSES}, got {close!r}")
    for name, v in (("min_area", min_area), ("min_hole", min_hole)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{name} must be a non-negative int (plane pixels), got {v!r}")
    return close > 1 or min_area > 1 or min_hole > 0


def _morph(plane: torch.Tensor, t: int, close: int, min_area: int, min_hole: int) -> torch.Tensor:
    """Steps 6a to 6c on the median plane: the 0 / 255 plane of M3. Only the active stages launch; the first of them reads the plane with t directly."""
    mask, th = plane, t
    if close > 1:
        mask, th = ops.plane_close(mask, close, th), 0
    if min_area > 1:
        labels, area = ops.plane_components(mask, th, 0, workspace=True)
        mask, th = ops.plane_area_select(labels, area, 0, min_area), 0
    if min_hole > 0:
        labels, area = ops.plane_components(mask, th, 1, workspace=True)
        mask, th = ops.plane_area_select(labels, area, 1, min_hole), 0
    return mask


def segment_tissue(region: torch.Tensor, down: int = 16, median: int = 7, sat_thresh=8, val_min: int = 0, close: int = 0, min_area: int = 0,
                   min_hole: int = 0, return_threshold: bool = False):
    """(plane, t): the median-filtered saturation plane of the region, uint8 [Hr // down, Wr // down] ON THE DEVICE (steps 1 to 3 of the module's
    definition), and the threshold used - a plane pixel is tissue iff it is > t. With an int ``sat_thresh`` t is that int and the call is two launches
    without any synchronisation. ``sat_thresh="otsu"`` also counts the plane's histogram and takes Otsu's threshold of it on the host
    (``otsu_threshold``): ONE extra device-to-host copy of 1 KB and its synchronisation. An empty plane gives t = 0 under "otsu".

    With ``close`` > 1, ``min_area`` > 1 or ``min_hole`` > 0 (steps 6a to 6c; the other values are the identity and launch nothing) the result is
    (mask, 0): mask = the 0 / 255 plane of M3, so "tissue iff > t" still holds for the pair. ``return_threshold`` appends the threshold that was applied
    to the median plane (``sat_thresh`` or Otsu's). Launches on top of the two: ``close`` 1; ``min_area`` 4 (3 labelling launches - 2 where the plane is
    one 64 x 16 tile - and the selection); ``min_hole`` 4 likewise; all three 9. No further synchronisation. An empty plane still launches nothing."""
    _seg_args(down, median, sat_thresh, val_min)
    active = _morph_args(close, min_area, min_hole)
    return _segment_plane(ops.region_saturation(region, down, val_min), median, sat_thresh, close, min_area, min_hole, active, return_threshold)


def _segment_plane(sat: torch.Tensor, median, sat_thresh, close=0, min_area=0, min_hole=0, active=False, return_threshold=False):
    """``segment_tissue`` from the saturation plane on (steps 3 to 6c): these steps do not care where the plane came from - one region, or a slide's
    strips (``slide_saturation``). The arguments have been checked."""
    if sat_thresh == "otsu":
        plane, hist = ops.plane_median(sat, median, want_hist=True)
        t = otsu_threshold(hist.cpu())                               # the 1 KB copy, the synchronisation
    else:
        plane, t = ops.plane_median(sat, median), sat_thresh
    out = (_morph(plane, t, close, min_area, min_hole), 0) if active and plane.numel() else (plane, t)
    return out + (t,) if return_threshold else out


def _seg_lattice(tile, stride, origin, down):
    """The lattice in plane units, after the 4 * down divisibility rule."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    for name, v in (("tile height", h), ("tile width", w), ("stride y", sy), ("stride x", sx), ("origin x", x0), ("origin y", y0)):
        if v % (4 * down):
            raise ValueError(f"{name} = {v} is not a multiple of 4 * down = {4 * down} (down = {down}): on the plane the tile shape, the strides and the "
                             "origin of a tissue lattice must all be multiples of 4")
    return h // down, w // down, sy // down, sx // down, x0 // down, y0 // down


def segmented_tissue_origins(region: torch.Tensor, tile=256, stride=None, min_fraction: float = 0.25, down: int = 16, median: int = 7, sat_thresh=8,
                             val_min: int = 0, origin=(0, 0), return_counts: bool = False, return_threshold: bool = False, close: int = 0,
                             min_area: int = 0, min_hole: int = 0, return_mask: bool = False):
    """``tissue_origins`` with CLAM's tissue decision (the module's steps 1 to 7): the region is box-filtered by ``down``, its saturation plane
    median-filtered (``median`` x ``median``), a plane pixel is tissue iff it is > ``sat_thresh`` - an int in 0..255 or ``"otsu"`` - and a lattice tile
    is kept iff its tissue count >= ceil(min_fraction (H // down) (W // down)). Result as for ``tissue_origins``: np.ndarray int64 [B,2] of (x, y) at the
    region's level ON THE HOST, row-major over the lattice; with ``return_counts`` also the kept tiles' counts (plane pixels), int64 [B]; with
    ``return_threshold`` also the threshold used, last. The tile shape, the strides and the origin must be multiples of ``4 * down``.

    Four launches and ONE device-to-host copy of ny nx int32, its one synchronisation; ``"otsu"`` adds a 1 KB memset and one more 1 KB copy with its
    synchronisation. An empty region or lattice gives an empty [0,2] result, not an error (and launches nothing; the threshold is then ``sat_thresh``,
    0 for ``"otsu"``).

    ``close``, ``min_area``, ``min_hole`` (the module's steps 6a to 6c: CLAM's ``close``, ``a_t`` and ``a_h`` in plane pixels) filter the mask before the
    tiles are counted; each is skipped entirely at 0 (``close`` and ``min_area`` at 1 as well). They add 1, 4 and 4 launches (9 together; a labelling is 2
    launches, not 3, where the plane is one 64 x 16 tile) and no synchronisation; ``return_threshold`` still gives the threshold applied to the median plane.

    ``return_mask`` appends ``(mask_plane, t)`` last: the uint8 [Hr // down, Wr // down] plane ON THE DEVICE the tile counts were taken from and the
    threshold it was read with (a plane pixel is tissue iff it is > t) - the median plane and the threshold applied, or the 0 / 255 plane of the filters
    and 0. Nothing is recomputed for it; with ``down`` it is the mask ``heatmap.attention_canvas`` takes. An empty lattice has no plane: ``(None, t)``.

    The defaults are CLAM's: ``sthresh = 8``, ``mthresh = 7``, a low-resolution level (``down = 16``); ``use_otsu`` is ``sat_thresh="otsu"``.
    CLAM's ``max_n_holes`` and its polygon areas are not done."""
    _min_fraction_arg(min_fraction)
    _seg_args(down, median, sat_thresh, val_min)
    active = _morph_args(close, min_area, min_hole)
    _, hr, wr = ops._region_pitch(region, "segmented_tissue_origins")
    return _origins_on_plane(lambda: ops.region_saturation(region, down, val_min), hr, wr, tile, stride, min_fraction, down, median, sat_thresh, origin,
                             return_counts, return_threshold, close, min_area, min_hole, active, return_mask)


def _origins_on_plane(saturation, hr, wr, tile, stride, min_fraction, down, median, sat_thresh, origin, return_counts, return_threshold, close, min_area,
                      min_hole, active, return_mask):
    """``segmented_tissue_origins`` from the saturation plane on: ``saturation()`` gives the uint8 [hr // down, wr // down] plane of the hr x wr image the
    lattice lies on and is called only where the lattice has a tile. The arguments have been checked."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    ph, pw, psy, psx, px0, py0 = _seg_lattice((h, w), (sy, sx), (x0, y0), down)
    nx, ny = lattice(hr, wr, (h, w), (sy, sx), (x0, y0))

    counts, t = None, 0 if sat_thresh == "otsu" else sat_thresh
    mask = (None, t)
    if nx and ny:
        plane, t = _segment_plane(saturation(), median, sat_thresh)
        cell = lattice_cell((ph, pw), (psy, psx), (px0, py0))
        mask = (_morph(plane, t, close, min_area, min_hole), 0) if active else (plane, t)
        cells = ops.plane_cells(mask[0], cell, mask[1])
        counts = ops.tissue_tile_counts(cells, cell, (px0, py0), (ph, pw), (psy, psx), (nx, ny))
    origins, kept = _kept(counts, math.ceil(min_fraction * ph * pw), x0, y0, sx, sy)
    out = (origins,) + ((kept,) if return_counts else ()) + ((t,) if return_threshold else ()) + ((mask,) if return_mask else ())
    return out if len(out) > 1 else origins


# ---- a slide that arrives in strips: the saturation plane is put together from the strips, everything behind it runs once on the slide's plane ----
def plane_strip_plan(slide_hw, strips, down: int):
    """Which strip gives which rows of the saturation plane of a slide of ``slide_hw`` = (Hs, Ws) pixels that arrives as full-width row strips. Host
    arithmetic only. ``strips`` = [(y_k, H_k)] as in ``heatmap.strip_plan``: strip k holds the slide's rows y_k .. y_k + H_k, sorted, each abutting or
    overlapping the one before, covering rows 0 .. Hs. One ``(p0, p1)`` per strip - the plane rows p0 <= r < p1 it gives; plane row r is made of the slide
    rows r down .. (r + 1) down and of nothing else, and belongs to the FIRST strip that holds them all:

        Hp = Hs // down,  p0_k = max(ceil(y_k / down), p1_{k-1}),  p1_k = max(p1_{k-1}, min((y_k + H_k) // down, Hp)),  p1_{-1} = 0

    (a strip that has no row left to give is ``(p1_{k-1}, p1_{k-1})``). The strip's rows p0 down - y_k .. p1 down - y_k are the sub-region whose
    ``ops.region_saturation`` IS rows p0 .. p1 of the slide's plane, byte for byte. Box rows below Hp down are dropped, as everywhere else.

    ValueError, in ``heatmap.strip_plan``'s words, for strips that are not sorted, leave a gap or do not cover 0 .. Hs; for a plane row that lies whole
    in no strip (its box rows straddle a seam: the strips must meet at multiples of ``down`` or overlap enough); and for a ``down`` outside 1 .. 32."""
    hs, ws = slide_hw
    if down not in ops.SEG_DOWNS:
        raise ValueError(f"plane_strip_plan: down must be one of {ops.SEG_DOWNS}, got {down!r}")
    strips = [(int(y), int(n)) for y, n in strips]
    if not strips or strips[0][0] != 0 or strips[-1][0] + strips[-1][1] != hs:
        raise ValueError(f"plane_strip_plan: the strips must cover rows 0 .. Hs = {hs}, got {strips!r}")
    hp, plan, end, p1 = hs // down, [], 0, 0
    for k, (y, n) in enumerate(strips):
        if n < 1 or y + n <= end or (k and y <= strips[k - 1][0]):
            raise ValueError(f"plane_strip_plan: strip {k} = (y, H) = {(y, n)} is empty or not sorted after the strips before it (rows up to {end})")
        if y > end:
            raise ValueError(f"plane_strip_plan: a gap between strip {k - 1}, which ends at row {end}, and strip {k}, which starts at row {y}")
        first, last = -(-y // down), max(p1, min((y + n) // down, hp))
        if last > p1 and first > p1:                                 # the strip has rows to give, and the next row to be given starts above it
            raise ValueError(f"plane_strip_plan: plane row {p1} (slide rows {p1 * down} .. {(p1 + 1) * down}) lies whole in no strip: strip {k - 1} ends at "
                             f"row {end} and strip {k} starts at row {y}; strips must meet at multiples of down = {down} or overlap by the rest of the box")
        plan.append((min(max(first, p1), last), last))
        end, p1 = y + n, last
    return plan


def _strip_shapes(name: str, strips, ws: int):
    shapes = []
    for k, (region, y) in enumerate(strips):
        if not isinstance(region, torch.Tensor) or region.dim() != 3 or region.shape[1] != ws or region.shape[2] != 3:
            got = tuple(region.shape) if isinstance(region, torch.Tensor) else type(region).__name__
            raise ValueError(f"{name}: strip {k} must be a full-width uint8 [H_k,{ws},3] region, got {got}")
        shapes.append((y, region.shape[0]))
    return shapes


def slide_saturation(strips, slide_hw, down: int, val_min: int = 0, batch: bool = True) -> torch.Tensor:
    """The saturation plane of a slide of ``slide_hw`` = (Hs, Ws) pixels that arrives strip by strip: ONE contiguous uint8 [Hs // down, Ws // down] plane on
    the device, byte for byte ``ops.region_saturation`` of the whole slide. ``strips`` is a sequence of ``(region, y_k)`` as in
    ``eval.slide_attention_heatmap`` - a decoded uint8 [H_k,Ws,3] full-width strip on the device and the slide row of its first row. Each strip writes the
    plane rows ``plane_strip_plan`` gives it (whose ValueErrors come before anything is launched), from the sub-region of its rows that holds their boxes.
    ``batch=True``: one ``ops.regions_saturation`` call - one launch per ``ops.SAT_LIST_MAX`` strips; ``batch=False``: one
    ``ops.region_saturation(..., out=view)`` call per strip. The bytes are the same. No synchronisation; every strip is read once."""
    hs, ws = slide_hw
    strips = list(strips)
    plan = plane_strip_plan((hs, ws), _strip_shapes("slide_saturation", strips, ws), down)
    if not isinstance(batch, bool):
        raise ValueError(f"slide_saturation: batch must be a bool, got {batch!r}")
    plane = torch.empty((hs // down, ws // down), dtype=torch.uint8, device=strips[0][0].device)
    subs = [(region[p0 * down - y:p1 * down - y], plane[p0:p1]) for (region, y), (p0, p1) in zip(strips, plan) if p1 > p0]
    if batch:
        ops.regions_saturation([r for r, _ in subs], down, val_min, outs=[o for _, o in subs])
    else:
        for r, o in subs:
            ops.region_saturation(r, down, val_min, out=o)
    return plane


def segment_tissue_strips(strips, slide_hw, down: int = 16, median: int = 7, sat_thresh=8, val_min: int = 0, close: int = 0, min_area: int = 0,
                          min_hole: int = 0, return_threshold: bool = False):
    """``segment_tissue`` of a slide that arrives strip by strip (``strips`` and ``slide_hw`` as in ``slide_saturation``): the same plane bytes and the
    same ``t`` as on the whole slide, ``"otsu"`` included, with no seam - only the saturation plane reads the pixels, and that is put together from the
    strips in one launch (``slide_saturation``); the median, the histogram, the closing and the component filters run once, on the slide's plane.
    Launches and copies: ``segment_tissue``'s."""
    _seg_args(down, median, sat_thresh, val_min)
    active = _morph_args(close, min_area, min_hole)
    return _segment_plane(slide_saturation(strips, slide_hw, down, val_min), median, sat_thresh, close, min_area, min_hole, active, return_threshold)


def segmented_slide_origins(strips, slide_hw, tile=256, stride=None, min_fraction: float = 0.25, down: int = 16, median: int = 7, sat_thresh=8,
                            val_min: int = 0, origin=(0, 0), return_counts: bool = False, return_threshold: bool = False, close: int = 0,
                            min_area: int = 0, min_hole: int = 0, return_mask: bool = False):
    """``segmented_tissue_origins`` of a slide that arrives strip by strip (``strips`` and ``slide_hw`` as in ``slide_saturation``): the result is what
    that call gives on the whole slide - origins in SLIDE coordinates, row-major over the slide's lattice, and the counts, the threshold and the mask
    plane of the whole slide where asked for. The strips are read once, in one launch, for the slide's saturation plane; everything behind it runs once
    on that plane, so there is ONE read-back of ny nx int32 for the whole slide (and Otsu's 1 KB), not one per strip. The strips' ValueErrors
    (``plane_strip_plan``) come before anything is launched, an empty lattice included."""
    _min_fraction_arg(min_fraction)
    _seg_args(down, median, sat_thresh, val_min)
    active = _morph_args(close, min_area, min_hole)
    hs, ws = slide_hw
    strips = list(strips)
    plane_strip_plan((hs, ws), _strip_shapes("segmented_slide_origins", strips, ws), down)
    return _origins_on_plane(lambda: slide_saturation(strips, (hs, ws), down, val_min), hs, ws, tile, stride, min_fraction, down, median, sat_thresh,
                             origin, return_counts, return_threshold, close, min_area, min_hole, active, return_mask)
