"""The reference of the windowed heat-map tests (toad_region_heat_window_u8; ops.region_heat_window, heatmap.window_canvas): tests/heat_px_ref.py's
per-pixel definition with the window's place (wx, wy) added to the coordinates, in Python integers, one canvas pixel at a time. Written from the
definition in include/toad_hip.h; it never builds or slices the canvas of the whole image. Not collected by pytest; shared by
test_heatmap_window_host.py (which tests it against slices of heat_px_ref.canvas) and test_gpu_heatmap_window.py.

For canvas pixel (ox, oy) of the window, X = down ox + wx and Y = down oy + wy being its box's corner in the image the table and the mask describe:
  m       per channel (sum of the window's down x down box + down^2 / 2) // down^2; partial boxes at the window's right and bottom edge are dropped.
  own     cells[Y // cell][X // cell], values above 255 reading as 255.
  index   smooth = 0: own. smooth = 1: p = 2 X + down - cell, g0 = floor(p / (2 cell)), f = p - 2 cell g0, weights 2 cell - f for cell g0 and f for
          g0 + 1, the same along y from Y; a neighbour inside the TABLE and >= 0 contributes its value wherever the window lies, any other one own;
          idx_px = (sum wy wx v + 2 cell^2) >> (2 log2(cell) + 2).
  tissue  no mask: every pixel; else iff mx = X // mask_down < Wm, my = Y // mask_down < Hm and mask[my][mx] > mask_thresh.
  byte    (alpha lut[idx_px][c] + (256 - alpha) m + 128) >> 8 where own >= 0 and the pixel is tissue, m elsewhere."""
import numpy as np

from tests import heat_ref


def tent(p, cell):
    """(g0, w0, w1) of one axis from its doubled coordinate p = 2 X + down - cell: weights w0 for cell g0 (which may be -1) and w1 for g0 + 1."""
    g0 = p // (2 * cell)                                            # Python's floor division
    f = p - 2 * cell * g0
    assert 0 <= f < 2 * cell
    return g0, 2 * cell - f, f


def canvas(region, window, cell_idx, cell, lut, alpha, down, smooth=False, mask=None, mask_down=None, mask_thresh=0):
    """uint8 [Hr // down, Wr // down, 3]: the canvas of the window `region` at `window` = (wx, wy) under the image's cell values [Gy,Gx] and mask plane."""
    return canvases(region, window, cell_idx, cell, lut, (alpha,), down, smooth, mask, mask_down, mask_thresh)[alpha]


def canvases(region, window, cell_idx, cell, lut, alphas, down, smooth=False, mask=None, mask_down=None, mask_thresh=0):
    """{alpha: canvas} for several alphas from one walk over the pixels: only the last line of the definition holds alpha."""
    wx, wy = window
    hr, wr = np.asarray(region).shape[:2]
    ho, wo = hr // down, wr // down
    means = heat_ref.box(region, down).tolist()                     # of the window's own pixels
    c = np.minimum(np.asarray(cell_idx).astype(np.int64), 255).tolist()
    gy_n, gx_n = len(c), len(c[0]) if c else 0
    assert cell in (4, 8, 16, 32, 64) and down in (1, 2, 4, 8, 16, 32) and wx >= 0 and wy >= 0 and wx % max(4, down) == 0 and wy % max(4, down) == 0
    assert -(-(wy + hr) // cell) <= gy_n and -(-(wx + wr) // cell) <= gx_n and (down <= 4 or down <= cell)
    shift = 2 * (cell.bit_length() - 1) + 2
    lut = np.asarray(lut).astype(np.int64).tolist()
    m_plane = None if mask is None else np.asarray(mask)
    if m_plane is not None:
        assert m_plane.dtype == np.uint8 and m_plane.ndim == 2 and mask_down % down == 0 and 0 <= mask_thresh <= 255
        hm, wm = m_plane.shape
        m_plane = m_plane.tolist()
    outs = {alpha: np.zeros((ho, wo, 3), dtype=np.uint8) for alpha in alphas}
    assert all(isinstance(alpha, int) and 0 <= alpha <= 256 for alpha in alphas)
    for oy in range(ho):
        y = down * oy + wy
        for ox in range(wo):
            x = down * ox + wx
            m = means[oy][ox]
            own = c[y // cell][x // cell]
            tissue = True
            if m_plane is not None:
                my, mx = y // mask_down, x // mask_down
                tissue = my < hm and mx < wm and m_plane[my][mx] > mask_thresh
            if own < 0 or not tissue:
                for out in outs.values():
                    out[oy, ox] = m
                continue
            idx = own
            if smooth:
                gx0, wx0, wx1 = tent(2 * x + down - cell, cell)
                gy0, wy0, wy1 = tent(2 * y + down - cell, cell)
                s = 0
                for gy, w_y in ((gy0, wy0), (gy0 + 1, wy1)):
                    for gx, w_x in ((gx0, wx0), (gx0 + 1, wx1)):
                        v = c[gy][gx] if 0 <= gy < gy_n and 0 <= gx < gx_n else -1
                        s += w_y * w_x * (v if v >= 0 else own)
                assert 0 <= s <= 255 * 4 * cell * cell
                idx = (s + 2 * cell * cell) >> shift
            for alpha, out in outs.items():
                out[oy, ox] = [(alpha * lut[idx][k] + (256 - alpha) * m[k] + 128) >> 8 for k in range(3)]
    return outs
