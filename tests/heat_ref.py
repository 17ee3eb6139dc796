"""The reference of the heat-map tests (toad_amd/heatmap.py, csrc/heatmap.hip): numpy and Python integers, written from the definition in
include/toad_hip.h ("attention heat map") - a loop over the tiles for S and n, a reshape-sum for the boxes. Not collected by pytest; shared by
test_heatmap_host.py (which tests the reference itself) and test_gpu_heatmap.py."""
import functools

import numpy as np

from tests import tissue_ref

# (region (hr, wr), tile (H, W), stride (sy, sx), origin (x, y), cell) of the lattice cases; the tiles are those tissue_ref.selection keeps at
# min_fraction 0.25, sat_thresh 8, val_min 0 on tissue_ref.slide(hr, wr, 1)
LATTICES = [((300, 520), (64, 64), (32, 32), (0, 0), 32), ((300, 520), (64, 64), (64, 64), (8, 4), 4), ((203, 333), (32, 64), (8, 16), (0, 0), 8),
            ((300, 520), (256, 256), (64, 64), (0, 0), 64), ((131, 67), (16, 16), (16, 16), (0, 0), 16), ((203, 334), (32, 64), (8, 16), (8, 4), 4)]


def jet():
    """uint8 [256,3]: channel k of entry i is clamp(765 - |8 i - 510 k|, 0, 510) // 2, k = 3, 2, 1 for r, g, b - in Python integers."""
    return np.array([[min(max(765 - abs(8 * i - 510 * k), 0), 510) // 2 for k in (3, 2, 1)] for i in range(256)], dtype=np.uint8)


def quantise(scores):
    """int64 [B] from float32 scores in the default range: round(clamp(s, 0, 1) * 65535) in float32, half to even as torch.round; NaN -> -1."""
    s = np.asarray(scores, dtype=np.float32)
    q = np.round(np.clip(s, np.float32(0), np.float32(1)) * np.float32(65535))
    return np.where(np.isnan(s), -1, q).astype(np.int64)


def table(origins, q, tile, stride, origin, n):
    """int64 [ny,nx]: -1, and q at the tiles of origins."""
    (sy, sx), (x0, y0), (nx, ny) = stride, origin, n
    t = np.full((ny, nx), -1, dtype=np.int64)
    for (x, y), v in zip(np.asarray(origins).tolist(), np.asarray(q).tolist()):
        assert (x - x0) % sx == 0 and (y - y0) % sy == 0
        t[(y - y0) // sy, (x - x0) // sx] = v
    return t


def coverage(tile_q, cell, tile, stride, origin, region_hw):
    """(n, S) int64 [Gy,Gx]: the present tiles that cover each cell and the sum of their q - a loop over the tiles."""
    (h, w), (sy, sx), (x0, y0), (hr, wr) = tile, stride, origin, region_hw
    gy, gx = -(-hr // cell), -(-wr // cell)
    n, s = np.zeros((gy, gx), dtype=np.int64), np.zeros((gy, gx), dtype=np.int64)
    ny, nx = tile_q.shape
    for j in range(ny):
        for i in range(nx):
            q = int(tile_q[j, i])
            if q < 0:
                continue
            y, x = y0 + j * sy, x0 + i * sx
            assert x % cell == 0 and y % cell == 0 and h % cell == 0 and w % cell == 0
            n[y // cell:(y + h) // cell, x // cell:(x + w) // cell] += 1
            s[y // cell:(y + h) // cell, x // cell:(x + w) // cell] += q
    return n, s


def cells(tile_q, cell, tile, stride, origin, region_hw):
    """int64 [Gy,Gx]: (2 S + 257 n) // (514 n) where n > 0, else -1."""
    n, s = coverage(tile_q, cell, tile, stride, origin, region_hw)
    return np.where(n > 0, (2 * s + 257 * n) // np.maximum(514 * n, 1), -1)


def box(region, down):
    """int64 [Hr // down, Wr // down, 3]: (sum of the down x down box + down^2 / 2) // down^2, partial boxes dropped."""
    r = np.asarray(region).astype(np.int64)
    ho, wo = r.shape[0] // down, r.shape[1] // down
    s = r[:ho * down, :wo * down].reshape(ho, down, wo, down, 3).sum(axis=(1, 3))
    return (s + down * down // 2) // (down * down)


def canvas(region, cell_idx, cell, lut, alpha, down):
    """uint8 [Hr // down, Wr // down, 3] from the cell values [Gy,Gx] (-1 .. 255)."""
    m = box(region, down)
    ho, wo = m.shape[:2]
    idx = np.asarray(cell_idx).astype(np.int64)
    oy, ox = (np.arange(ho) * down) // cell, (np.arange(wo) * down) // cell
    per_px = idx[oy][:, ox] if ho and wo else np.zeros((ho, wo), dtype=np.int64)
    col = np.asarray(lut).astype(np.int64)[np.maximum(per_px, 0)]
    out = np.where((per_px >= 0)[..., None], (alpha * col + (256 - alpha) * m + 128) >> 8, m)
    assert out.size == 0 or (0 <= out.min() and out.max() <= 255)
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(k):
    """Lattice case k -> (slide uint8 [hr,wr,3], origins int64 [B,2], q int64 [B], tile_q int64 [ny,nx], (nx, ny)): the tiles kept at 0.25 / 8 / 0, with q
    from a seeded generator and 0 and 65535 among them. Read-only, cached."""
    (hr, wr), tile, stride, origin, _ = LATTICES[k]
    s = tissue_ref.slide(hr, wr, 1)
    origins, _ = tissue_ref.selection(s, tile, stride, origin, 0.25, 8, 0)
    q = np.random.default_rng(100 + k).integers(0, 65536, size=len(origins))
    q[0], q[-1] = 0, 65535
    nx, ny = tissue_ref.lattice_extent(hr, wr, tile, stride, origin)
    t = table(origins, q, tile, stride, origin, (nx, ny))
    for a in (origins, q, t):
        a.setflags(write=False)
    return s, origins, q, t, (nx, ny)
