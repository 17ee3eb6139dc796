"""The reference of the tissue-morphology tests (csrc/tissue_morph.hip; the close / min_area / min_hole keywords of toad_amd/tissue.py): numpy and Python
ints, exactly steps 6a to 6c of include/toad_hip.h ("segmented tissue selection"). Not collected by pytest; shared by test_tissue_morph_host.py (which
tests the reference itself) and test_gpu_tissue_morph.py. No scipy here: the machine with the GPU may not have it.

  M0 = P > t on the median plane P of [Hp, Wp] (step 6, tests/tissue_seg_ref.py).
  6a closing     close = c in 0 .. 8, 0 and 1 the identity; lo = c // 2, hi = c - 1 - c // 2. D[y,x] = OR of M0[y+dy, x+dx] over -lo <= dy, dx <= hi, the
                 window clipped to the plane; M1[y,x] = AND of D over the same offsets, clipped the same way. cv2.morphologyEx(m, MORPH_CLOSE,
                 np.ones((c, c))) as OpenCV defines it (anchor (c // 2, c // 2) for both halves, border pixels ignored); not claimed bit-equal to OpenCV.
  6b components  min_area = a >= 0: the 8-connected components of M1 with fewer than a pixels are removed -> M2.
  6c holes       min_hole = h >= 0: the 4-connected components of the complement of M2 that touch neither row 0, row Hp-1, column 0 nor column Wp-1 are
                 holes; a hole with fewer than h pixels becomes tissue -> M3. Step 7 then runs on M3.
  Labels are canonical: the smallest y * Wp + x of the component, -1 on unselected pixels; area[label] = the pixel count + 2^30 iff the component touches
  the plane's outer rows or columns, 0 at every other index."""
import functools
import math

import numpy as np

from tests import tissue_seg_ref as seg
from tests.tissue_ref import slide

CLOSES = tuple(range(9))
BORDER = 1 << 30
COUNT = BORDER - 1

# the end-to-end cases of test_gpu_tissue_morph.py on holey_slide(300, 520, 1): (down, median) x sat_thresh x configuration, one lattice
E2E_KEY = (300, 520, 1)
E2E_DM = ((1, 3), (2, 5), (4, 7))
E2E_SAT = (8, "otsu")
E2E_LATTICE = ((64, 64), (32, 32), (0, 0))
E2E_CLOSE, E2E_MIN_AREA, E2E_MIN_HOLE = 4, 2000, 2000               # the areas at down = 1; a case at `down` takes area // down^2


def e2e_configs(down):
    """(close, min_area, min_hole): each parameter alone, then all together."""
    a, h = E2E_MIN_AREA // (down * down), E2E_MIN_HOLE // (down * down)
    return ((E2E_CLOSE, 0, 0), (0, a, 0), (0, 0, h), (E2E_CLOSE, a, h))


# ---- 6a ----------------------------------------------------------------------------------------------------------------------------------------------------
def _window_reduce(m, lo, hi, union):
    """out[y,x] = OR (union) or AND of m[y+dy, x+dx] over -lo <= dy, dx <= hi, offsets that leave the plane left out: explicit clipped windows."""
    hp, wp = m.shape
    out = np.zeros_like(m) if union else np.ones_like(m)
    for dy in range(-lo, hi + 1):
        for dx in range(-lo, hi + 1):
            ys, ye = max(0, -dy), min(hp, hp - dy)                  # the y with 0 <= y + dy < hp
            xs, xe = max(0, -dx), min(wp, wp - dx)
            if ys >= ye or xs >= xe:
                continue
            src = m[ys + dy:ye + dy, xs + dx:xe + dx]
            if union:
                out[ys:ye, xs:xe] |= src
            else:
                out[ys:ye, xs:xe] &= src
    return out


def closing(m0, c):
    """bool [Hp,Wp] -> bool [Hp,Wp]: step 6a."""
    m0 = np.asarray(m0).astype(bool)
    if c <= 1 or m0.size == 0:
        return m0.copy()
    lo, hi = c // 2, c - 1 - c // 2
    return _window_reduce(_window_reduce(m0, lo, hi, True), lo, hi, False)


# ---- components ------------------------------------------------------------------------------------------------------------------------------------------------
def components(sel, conn):
    """(labels int64 [Hp,Wp], area int64 [Hp*Wp]) of the selected pixels (bool [Hp,Wp]) under connectivity 4 or 8: a two-pass union-find in Python ints that
    always links the larger root below the smaller, so a root is its component's smallest index."""
    sel = np.asarray(sel).astype(bool)
    hp, wp = sel.shape
    flat = sel.ravel().tolist()
    parent = list(range(hp * wp))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def union(i, j):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for y in range(hp):
        for x in range(wp):
            i = y * wp + x
            if not flat[i]:
                continue
            if x > 0 and flat[i - 1]:
                union(i, i - 1)
            if y > 0:
                if flat[i - wp]:
                    union(i, i - wp)
                if conn == 8:
                    if x > 0 and flat[i - wp - 1]:
                        union(i, i - wp - 1)
                    if x < wp - 1 and flat[i - wp + 1]:
                        union(i, i - wp + 1)
    labels = np.array([find(i) if flat[i] else -1 for i in range(hp * wp)], dtype=np.int64).reshape(hp, wp)
    area = np.bincount(labels[sel], minlength=hp * wp).astype(np.int64)
    edge = np.zeros((hp, wp), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    area[np.unique(labels[sel & edge])] += BORDER
    return labels, area


def plane_components(plane, thresh, background):
    """What toad_plane_components_u8 computes: selected = (plane > thresh) != background, connectivity 8 for background 0 and 4 for background 1."""
    sel = (np.asarray(plane).astype(np.int64) > thresh) != bool(background)
    return components(sel, 4 if background else 8)


def area_select(labels, area, mode, limit):
    """bool [Hp,Wp]: the two selections of toad_plane_area_select_u8."""
    labels = np.asarray(labels)
    a = np.asarray(area)[np.maximum(labels, 0)]
    count, border = a & COUNT, (a & BORDER) != 0
    if mode == 0:
        return (labels >= 0) & (count >= limit)
    return (labels < 0) | ((count < limit) & ~border)


def drop_small(m1, min_area):
    """Step 6b."""
    if min_area <= 1 or m1.size == 0:
        return m1.copy()
    labels, area = components(m1, 8)
    return area_select(labels, area, 0, min_area)


def fill_holes(m2, min_hole):
    """Step 6c."""
    if min_hole <= 0 or m2.size == 0:
        return m2.copy()
    labels, area = components(~m2, 4)
    return area_select(labels, area, 1, min_hole)


def component_sizes(sel, conn):
    """(sizes of the components that do not touch the plane's border, sizes of those that do), each sorted."""
    _, area = components(sel, conn)
    a = area[area > 0]
    return sorted(int(v) for v in a[a < BORDER]), sorted(int(v & COUNT) for v in a[a >= BORDER])


# ---- the whole selector ----------------------------------------------------------------------------------------------------------------------------------------
def _source(region, key):
    return holey_slide(*key) if key is not None else region


@functools.lru_cache(maxsize=None)
def _plane(key, down, median, val_min):
    plane = seg.median_plane(seg.saturation_plane(holey_slide(*key), down, val_min), median)
    plane.setflags(write=False)
    return plane, seg.otsu(seg.histogram(plane))


def segmented(region, down, median, sat_thresh, val_min=0, key=None):
    """(median plane, t): steps 1 to 6 by tests/tissue_seg_ref.py. `key` = the (hr, wr, seed) of a holey_slide lets repeated calls share the plane."""
    if key is not None:
        plane, t = _plane(key, down, median, val_min)
        return plane, (t if sat_thresh == "otsu" else sat_thresh)
    return seg.segmented(region, down, median, sat_thresh, val_min)


@functools.lru_cache(maxsize=None)
def _stages_cached(key, down, median, sat_thresh, val_min, close, min_area, min_hole):
    return _stages(None, down, median, sat_thresh, val_min, close, min_area, min_hole, key)


def _stages(region, down, median, sat_thresh, val_min, close, min_area, min_hole, key):
    plane, t = segmented(region, down, median, sat_thresh, val_min, key)
    m0 = plane > t
    m1 = closing(m0, close)
    m2 = drop_small(m1, min_area)
    m3 = fill_holes(m2, min_hole)
    for m in (m0, m1, m2, m3):
        m.setflags(write=False)
    return m0, m1, m2, m3, t


def stages(region, down, median, sat_thresh, val_min=0, close=0, min_area=0, min_hole=0, key=None):
    """(M0, M1, M2, M3, t), bool [Hp,Wp] each."""
    if key is not None:
        return _stages_cached(key, down, median, sat_thresh, val_min, close, min_area, min_hole)
    return _stages(region, down, median, sat_thresh, val_min, close, min_area, min_hole, None)


def mask(region, down, median, sat_thresh, val_min=0, close=0, min_area=0, min_hole=0, key=None):
    """M3, bool [Hp,Wp]."""
    return stages(region, down, median, sat_thresh, val_min, close, min_area, min_hole, key)[3]


def selection(region, tile, stride, origin, min_fraction, down, median, sat_thresh, val_min=0, close=0, min_area=0, min_hole=0, key=None):
    """(origins int64 [B,2] of (x, y) at the region's level, row-major; the tile counts int64 [ny,nx]; threshold used): step 7 of tests/tissue_seg_ref.py on
    the 0 / 255 plane of M3."""
    region = _source(region, key)
    m0, m1, m2, m3, t = stages(region, down, median, sat_thresh, val_min, close, min_area, min_hole, key)
    c = seg.tile_counts(m3.astype(np.int64) * 255, 0, tile, stride, origin, down, np.asarray(region).shape[:2])
    (h, w), (sy, sx), (x0, y0) = tile, stride, origin
    need = math.ceil(min_fraction * (h // down) * (w // down))
    keep = [(x0 + i * sx, y0 + j * sy) for j in range(c.shape[0]) for i in range(c.shape[1]) if c[j, i] >= need]
    return np.array(keep, dtype=np.int64).reshape(-1, 2), c, t


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def holey_slide(hr, wr, seed):
    """tissue_ref.slide(hr, wr, seed) (read-only; cached) with, inside or near its pink ellipse: a large glass hole with a pink island in it, a medium and a
    small glass hole, a glass crack 1 to 3 pixels wide right across the ellipse below the holes (a median leaves slits of it), and two detached pink specks, a small and a larger one.
    Positions and radii are fractions of the slide, so that a 4096 x 8192 slide has the same features."""
    img = slide(hr, wr, seed).copy()
    rng = np.random.default_rng(seed + 1000)
    glass = np.minimum(rng.integers(230, 254, size=(hr, wr, 1)) + rng.integers(0, 3, size=(hr, wr, 3)), 255)
    pink = np.stack([rng.integers(180, 231, size=(hr, wr)), rng.integers(80, 141, size=(hr, wr)), rng.integers(150, 201, size=(hr, wr))], axis=2)
    y, x = np.mgrid[0:hr, 0:wr]

    def disc(cx, cy, rx, ry=None):
        ry = rx if ry is None else ry
        return ((x - cx * wr) / max(rx * hr, 0.6)) ** 2 + ((y - cy * hr) / max(ry * hr, 0.6)) ** 2 <= 1.0

    ellipse = ((x - 0.33 * wr) / (0.2 * wr)) ** 2 + ((y - 0.45 * hr) / (0.3 * hr)) ** 2 <= 1.0
    width = 1 + (x // 23) % 3                                       # the crack's width, 1 to 3 pixels, changing along x
    crack = ellipse & (np.abs(y - (0.62 * hr + 0.1 * (x - 0.33 * wr))) * 2 < width)
    holes = disc(0.30, 0.45, 0.12) | disc(0.438, 0.433, 0.066) | disc(0.42, 0.30, 0.018) | crack
    pinks = disc(0.30, 0.45, 0.035) | disc(0.55, 0.90, 0.02) | disc(0.62, 0.62, 0.073)
    img[holes] = glass[holes]
    img[pinks] = pink[pinks]
    img = img.astype(np.uint8)
    img.setflags(write=False)
    return img


def random_field(hp, wp, density, seed):
    return np.random.default_rng(seed).random((hp, wp)) < density


def checkerboard(hp, wp):
    y, x = np.mgrid[0:hp, 0:wp]
    return (x + y) % 2 == 0


def spiral(hp, wp, outward=False):
    """A one-pixel path wound from (0, 0) clockwise inwards, arms two apart: ring k (its corners at 2 k from the border) without its pixel (2 k + 1, 2 k),
    joined to ring k + 1 by the pixel (2 k + 2, 2 k + 1). `outward`: the same turned by 180 degrees, its outer end at the plane's last pixel."""
    m = np.zeros((hp, wp), dtype=bool)
    k = 0
    while 2 * k <= hp - 1 - 2 * k and 2 * k <= wp - 1 - 2 * k:
        t, b, l, r = 2 * k, hp - 1 - 2 * k, 2 * k, wp - 1 - 2 * k
        m[t, l:r + 1] = m[b, l:r + 1] = True
        m[t:b + 1, l] = m[t:b + 1, r] = True
        if b - t >= 2 and r > l:
            m[t + 1, l] = False
            if r - l >= 2 and b - t >= 2 and t + 2 <= hp - 1 - 2 * (k + 1):
                m[t + 2, l + 1] = True
        k += 1
    return m[::-1, ::-1].copy() if outward else m


def serpentine(hp, wp):
    """Every second row set, joined at alternating ends: one long 4-connected chain."""
    m = np.zeros((hp, wp), dtype=bool)
    m[0::2] = True
    m[1::4, wp - 1] = True
    m[3::4, 0] = True
    return m


def rings(hp, wp):
    """Concentric square rings at spacing 2, the outermost on the plane's border: nested holes and islands, and no background that touches the border."""
    y, x = np.mgrid[0:hp, 0:wp]
    return np.minimum(np.minimum(y, hp - 1 - y), np.minimum(x, wp - 1 - x)) % 2 == 0


def corner_contacts(hp, wp, anti=False):
    """Two pixels touching diagonally (or anti-diagonally) across every point (cy, cx) with cy and cx multiples of 16 - the four-tile corners of tiles of
    16, 32 and 64 among them: one 8-component and two 4-components each."""
    m = np.zeros((hp, wp), dtype=bool)
    for cy in range(16, hp, 16):
        for cx in range(16, wp, 16):
            if anti:
                m[cy - 1, cx] = m[cy, cx - 1] = True
            else:
                m[cy - 1, cx - 1] = m[cy, cx] = True
    return m


def patterns(hp, wp):
    """name -> bool [hp,wp]: the inputs of the component tests."""
    out = {f"random{d}": random_field(hp, wp, d, int(d * 1000) + hp * 7 + wp) for d in (0.35, 0.5, 0.593, 0.65, 0.9)}
    out.update(checkerboard=checkerboard(hp, wp), spiral_in=spiral(hp, wp), spiral_out=spiral(hp, wp, True), serpentine=serpentine(hp, wp),
               rings=rings(hp, wp), ones=np.ones((hp, wp), dtype=bool), zeros=np.zeros((hp, wp), dtype=bool),
               corners=corner_contacts(hp, wp), corners_anti=corner_contacts(hp, wp, True))
    return out
