"""The reference of the per-pixel heat-map tests (toad_region_heat_blend_px_u8; toad_amd/heatmap.py, csrc/heatmap.hip heat_blend_px_kernel): numpy and
Python integers, written from the definition in include/toad_hip.h - a loop per canvas pixel for the tent. Not collected by pytest; shared by
test_heatmap_px_host.py (which tests the reference itself) and test_gpu_heatmap_px.py.

The definition, for canvas pixel (ox, oy) of a region box-filtered by ``down`` (m per channel as in heat_ref.box), ``own`` = the value of the cell that
holds the pixel, values above 255 reading as 255:
  index   smooth = 0: idx_px = own. smooth = 1: along x  p = 2 down ox + down - cell, g0 = floor(p / (2 cell)), f = p - 2 cell g0, weights 2 cell - f
          for cell g0 and f for g0 + 1; the same along y; each of the four neighbours contributes its value if it lies inside the table and is >= 0, and
          own otherwise;  idx_px = (sum wy wx v + 2 cell^2) >> (2 log2(cell) + 2).
  tissue  without a mask every pixel; with a uint8 [Hr // mask_down, Wr // mask_down] plane iff mx = (down ox) // mask_down and my = (down oy) //
          mask_down lie inside it and mask[my, mx] > mask_thresh.
  byte    (alpha lut[idx_px][c] + (256 - alpha) m + 128) >> 8 where own >= 0 and the pixel is tissue, m elsewhere."""
import numpy as np

from tests import heat_ref


def tent_axis(n_out, down, cell):
    """[(g0, w0, w1)] for the n_out canvas coordinates of one axis, Python ints: weights w0 for cell g0 (which may be -1) and w1 for g0 + 1."""
    out = []
    for o in range(n_out):
        p = 2 * down * o + down - cell
        g0 = p // (2 * cell)                                        # Python's floor division
        f = p - 2 * cell * g0
        assert 0 <= f < 2 * cell
        out.append((g0, 2 * cell - f, f))
    return out


def index_px(cell_idx, cell, down, ho, wo, smooth):
    """int64 [ho,wo]: the colour index of every canvas pixel, -1 where the pixel's own cell has no value."""
    c = np.minimum(np.asarray(cell_idx).astype(np.int64), 255).tolist()
    gy_n, gx_n = len(c), len(c[0]) if c else 0
    shift = 2 * (cell.bit_length() - 1) + 2
    assert 1 << (cell.bit_length() - 1) == cell and cell >= 4
    ys, xs = tent_axis(ho, down, cell), tent_axis(wo, down, cell)
    out = np.full((ho, wo), -1, dtype=np.int64)
    for oy in range(ho):
        gy0, wy0, wy1 = ys[oy]
        row = c[(down * oy) // cell]
        for ox in range(wo):
            own = row[(down * ox) // cell]
            if own < 0 or not smooth:
                out[oy, ox] = own
                continue
            gx0, wx0, wx1 = xs[ox]
            s = 0
            for gy, wy in ((gy0, wy0), (gy0 + 1, wy1)):
                for gx, wx in ((gx0, wx0), (gx0 + 1, wx1)):
                    v = c[gy][gx] if 0 <= gy < gy_n and 0 <= gx < gx_n else -1
                    s += wy * wx * (v if v >= 0 else own)
            assert 0 <= s <= 255 * 4 * cell * cell
            out[oy, ox] = (s + 2 * cell * cell) >> shift
    return out


def tissue_px(mask, mask_down, mask_thresh, down, ho, wo):
    """bool [ho,wo]: the canvas pixels that are tissue; mask None = all of them."""
    if mask is None:
        return np.ones((ho, wo), dtype=bool)
    m = np.asarray(mask)
    assert m.dtype == np.uint8 and m.ndim == 2 and mask_down % down == 0 and 0 <= mask_thresh <= 255
    hm, wm = m.shape
    my, mx = (np.arange(ho) * down) // mask_down, (np.arange(wo) * down) // mask_down
    inside = (my < hm)[:, None] & (mx < wm)[None, :]
    if not (hm and wm):
        return np.zeros((ho, wo), dtype=bool)
    return inside & (m[np.minimum(my, hm - 1)][:, np.minimum(mx, wm - 1)] > mask_thresh)


def canvas(region, cell_idx, cell, lut, alpha, down, smooth=False, mask=None, mask_down=None, mask_thresh=0):
    """uint8 [Hr // down, Wr // down, 3] from the cell values [Gy,Gx] (-1 and up; above 255 reads as 255)."""
    m = heat_ref.box(region, down)
    ho, wo = m.shape[:2]
    if mask is not None:
        assert np.asarray(mask).shape == (np.asarray(region).shape[0] // mask_down, np.asarray(region).shape[1] // mask_down)
    idx = index_px(cell_idx, cell, down, ho, wo, smooth)
    blend = (idx >= 0) & tissue_px(mask, mask_down, mask_thresh, down, ho, wo)
    col = np.asarray(lut).astype(np.int64)[np.maximum(idx, 0)]
    out = np.where(blend[..., None], (alpha * col + (256 - alpha) * m + 128) >> 8, m)
    assert out.size == 0 or (0 <= out.min() and out.max() <= 255)
    return out.astype(np.uint8)


def select(scores, q, thresh=None, binarize=False):
    """heatmap.select_scores on the host: int64 [B] from the raw scores and their quantised values."""
    s, q = np.asarray(scores, dtype=np.float32), np.asarray(q).astype(np.int64).copy()
    if thresh is not None:
        q[~(s >= np.float32(thresh))] = -1                          # a NaN is >= nothing
    if binarize:
        q[q >= 0] = 65535
    return q


def tables(gy, gx, seed):
    """The cell tables of the GPU tests, int64 [gy,gx] each: a 0..255 ramp, the ramp with an interior cell absent, a checkerboard of absent cells, and
    absent cells all along the table's border."""
    ramp = (np.arange(gy * gx, dtype=np.int64).reshape(gy, gx) * 255) // max(gy * gx - 1, 1)
    rng = np.random.default_rng(seed)
    noisy = rng.integers(0, 256, size=(gy, gx))
    hole = ramp.copy()
    hole[gy // 2, gx // 2] = -1
    checker = noisy.copy()
    checker[(np.add.outer(np.arange(gy), np.arange(gx)) & 1) == 1] = -1
    border = noisy.copy()
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = -1
    return {"ramp": ramp, "hole": hole, "checker": checker, "border": border}
