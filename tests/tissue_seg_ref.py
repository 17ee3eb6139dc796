"""The reference of the segmented tissue-selection tests (toad_amd/tissue.py segmented_tissue_origins, csrc/tissue_seg.hip): numpy int64 and Python ints,
exactly the definition of include/toad_hip.h ("segmented tissue selection"). Not collected by pytest; shared by test_tissue_seg_host.py (which tests
the reference itself) and test_gpu_tissue_seg.py.

  1 box filter  down in 1, 2, 4, 8, 16, 32; Hp = Hr // down, Wp = Wr // down, partial boxes at the right and the bottom edge dropped; the mean pixel of a
                box is (sum + down * down // 2) // (down * down) per channel.
  2 saturation  on the mean pixel, S = (255 * (mx - mn) + (mx >> 1)) // mx, and S = 0 where mx == 0 or mx < val_min. Not claimed to equal OpenCV's S.
  3 median      k in 1, 3, 5, 7: the (k * k) // 2-th of the sorted k * k window, coordinates clamped to the plane (replicate border).
  4 histogram   hist[v] = the pixels of the median plane equal to v, [256].
  5 Otsu        N = sum h, MT = sum i h[i], W0(t) = sum_{i<=t} h[i], M0(t) = sum_{i<=t} i h[i], W1 = N - W0: the smallest t in 0..254 that maximises
                (MT W0 - M0 N)^2 / (W0 W1) over the t with W0 > 0 and W1 > 0; 0 if there is none. Cross-multiplied Python ints.
  6 tissue      median-filtered S > t.
  7 tiles       lattice at the region's level, all six numbers multiples of 4 * down; kept iff count >= ceil(min_fraction * (H // down) * (W // down))."""
import functools
import math

import numpy as np

from tests.tissue_ref import lattice_extent, probe_blocks, slide  # noqa: F401  (re-exported for the tests)

DOWNS = (1, 2, 4, 8, 16, 32)
MEDIANS = (1, 3, 5, 7)

# the end-to-end cases of test_gpu_tissue_seg.py: (down, median) x sat_thresh x lattice (tile, stride, origin) x min_fraction on slide(300, 520, 1)
E2E_DM = ((1, 3), (2, 5), (4, 7), (8, 3))
E2E_SAT = (8, 40, "otsu")
E2E_LATTICES = (((64, 64), (32, 32), (0, 0)), ((64, 64), (64, 64), (32, 64)))
E2E_FRACTIONS = (0, 0.25, 1)


def lattice_allowed(lat, down):
    """The divisibility rule of definition 7."""
    return all(v % (4 * down) == 0 for pair in lat for v in pair)


def saturation_plane(region, down, val_min=0):
    """int64 [Hr // down, Wr // down] from uint8 [Hr,Wr,3]: definitions 1 and 2."""
    px = np.asarray(region).astype(np.int64)
    hp, wp = px.shape[0] // down, px.shape[1] // down
    box = px[:hp * down, :wp * down].reshape(hp, down, wp, down, 3).sum(axis=(1, 3))
    mean = (box + down * down // 2) // (down * down)
    mx, mn = mean.max(axis=2), mean.min(axis=2)
    s = (255 * (mx - mn) + (mx >> 1)) // np.maximum(mx, 1)
    return np.where((mx == 0) | (mx < val_min), 0, s)


def median_plane(plane, k):
    """Definition 3: np.pad(mode="edge"), sliding_window_view, sort, the middle element."""
    p = np.asarray(plane).astype(np.int64)
    if p.size == 0 or k == 1:
        return p.copy()
    r = k // 2
    win = np.lib.stride_tricks.sliding_window_view(np.pad(p, r, mode="edge"), (k, k))
    return np.sort(win.reshape(p.shape[0], p.shape[1], k * k), axis=2)[:, :, (k * k) // 2]


def histogram(plane):
    return np.bincount(np.asarray(plane).astype(np.int64).ravel(), minlength=256)


def otsu(hist):
    """Definition 5 in Python ints."""
    h = [int(v) for v in hist]
    assert len(h) == 256
    n, mt = sum(h), sum(i * v for i, v in enumerate(h))
    best, best_num, best_den = 0, None, None
    for t in range(255):
        w0, m0 = sum(h[:t + 1]), sum(i * h[i] for i in range(t + 1))
        w1 = n - w0
        if w0 > 0 and w1 > 0:
            num, den = (mt * w0 - m0 * n) ** 2, w0 * w1
            if best_num is None or num * best_den > best_num * den:
                best, best_num, best_den = t, num, den
    return best


def plane_cell_counts(plane, cell, thresh):
    """int64 [ceil(Hp/cell), ceil(Wp/cell)]: the pixels > thresh per cell; zero-pad the mask to a multiple of the cell, then a reshape-sum."""
    m = (np.asarray(plane).astype(np.int64) > thresh).astype(np.int64)
    hp, wp = m.shape
    gy, gx = -(-hp // cell), -(-wp // cell)
    pad = np.zeros((gy * cell, gx * cell), dtype=np.int64)
    pad[:hp, :wp] = m
    return pad.reshape(gy, cell, gx, cell).sum(axis=(1, 3))


@functools.lru_cache(maxsize=None)
def _segmented(key, down, median, val_min):
    """(median plane, Otsu threshold) of a cached slide, computed once per (slide, down, median, val_min)."""
    region = slide(*key)
    plane = median_plane(saturation_plane(region, down, val_min), median)
    plane.setflags(write=False)
    return plane, otsu(histogram(plane))


def segmented(region, down, median, sat_thresh, val_min=0, key=None):
    """(median plane, t): definitions 1 to 6. `key` = the (hr, wr, seed) of a tissue_ref.slide lets repeated calls share the plane."""
    if key is not None:
        plane, t = _segmented(key, down, median, val_min)
    else:
        plane = median_plane(saturation_plane(region, down, val_min), median)
        t = otsu(histogram(plane)) if sat_thresh == "otsu" else None
    return plane, (t if sat_thresh == "otsu" else sat_thresh)


def tile_counts(plane, t, tile, stride, origin, down, region_hw):
    """int64 [ny,nx] by slicing the plane's mask: tile (j, i) covers plane rows (y0 + j sy) // down : + H // down, and columns alike."""
    (h, w), (sy, sx), (x0, y0) = tile, stride, origin
    assert all(v % (4 * down) == 0 for v in (h, w, sy, sx, x0, y0))
    m = np.asarray(plane) > t
    nx, ny = lattice_extent(region_hw[0], region_hw[1], tile, stride, origin)
    out = np.zeros((ny, nx), dtype=np.int64)
    for j in range(ny):
        for i in range(nx):
            ys, xs = (y0 + j * sy) // down, (x0 + i * sx) // down
            assert ys + h // down <= m.shape[0] and xs + w // down <= m.shape[1]
            out[j, i] = m[ys:ys + h // down, xs:xs + w // down].sum()
    return out


def selection(region, tile, stride, origin, min_fraction, down, median, sat_thresh, val_min=0, key=None):
    """(origins int64 [B,2] of (x, y) at the region's level, row-major; total tiles; threshold used): definition 7."""
    plane, t = segmented(region, down, median, sat_thresh, val_min, key)
    c = tile_counts(plane, t, tile, stride, origin, down, np.asarray(region).shape[:2])
    (h, w), (sy, sx), (x0, y0) = tile, stride, origin
    need = math.ceil(min_fraction * (h // down) * (w // down))
    keep = [(x0 + i * sx, y0 + j * sy) for j in range(c.shape[0]) for i in range(c.shape[1]) if c[j, i] >= need]
    return np.array(keep, dtype=np.int64).reshape(-1, 2), c.size, t


@functools.lru_cache(maxsize=None)
def dusty_glass(hr, wr, seed):
    """uint8 [hr,wr,3] (read-only; cached): the glass of tissue_ref.slide - grey 230..253 plus a per-channel jitter of 0..2, so S <= 2 - with one pure-red
    pixel (255, 0, 0) at every (row, column) = (8 j + 3, 8 i + 5)."""
    rng = np.random.default_rng(seed)
    grey = rng.integers(230, 254, size=(hr, wr, 1))
    img = np.minimum(grey + rng.integers(0, 3, size=(hr, wr, 3)), 255).astype(np.uint8)
    img[3::8, 5::8] = (255, 0, 0)
    img.setflags(write=False)
    return img
