"""The reference of the cell-table blur tests (toad_heat_cells_blur; toad_amd/heatmap.py, csrc/heatmap.hip heat_cells_blur_kernel): numpy int64 and Python
ints, written from the definition in include/toad_hip.h - NON-separably, a loop over the (2 r + 1)^2 offsets of the window that accumulates N and D
over the whole table, so that it shares nothing with a row / column split. Not collected by pytest; shared by test_heatmap_blur_host.py (which tests
the reference itself) and test_gpu_heatmap_blur.py.

The definition: cells int [Gy,Gx], -1 = no value, values above 255 read as 255; a half-kernel w[0 .. r] of ints, 1 <= r <= 16, w[0] >= 1, w[d] >= 0,
w[0] + 2 sum w[1:] <= 1024. A cell without a value keeps none. Otherwise, over dy, dx in -r .. r such that (gy + dy, gx + dx) lies inside the table and
holds a value v:  N = sum w[|dy|] w[|dx|] min(v, 255),  D = sum w[|dy|] w[|dx|],  out = (2 N + D) // (2 D).

gaussian_taps_exact restates heatmap.gaussian_taps in 60-digit decimals: g[d] = exp(-d^2 / (2 sigma^2)), G = g[0] + 2 sum g[1:],
w[d] = floor((1023 - 2 r) g[d] / G + 1/2), r = ceil(3 sigma) unless given."""
import decimal

import numpy as np


def check_taps(taps):
    w = [int(t) for t in taps]
    r = len(w) - 1
    assert 1 <= r <= 16 and w[0] >= 1 and min(w) >= 0 and w[0] + 2 * sum(w[1:]) <= 1024, w
    return w, r


def blur(cells, taps):
    """int64 [Gy,Gx] from the cell values [Gy,Gx] (-1 and up; above 255 reads as 255) and the half-kernel taps."""
    w, r = check_taps(taps)
    c = np.asarray(cells).astype(np.int64)
    assert c.ndim == 2
    gy, gx = c.shape
    present = (c >= 0).astype(np.int64)
    v = np.minimum(c, 255) * present
    # the table inside a frame of r cells without a value: a shifted window is then a slice
    pv = np.zeros((gy + 2 * r, gx + 2 * r), dtype=np.int64)
    pp = np.zeros_like(pv)
    pv[r:r + gy, r:r + gx] = v
    pp[r:r + gy, r:r + gx] = present
    n = np.zeros((gy, gx), dtype=np.int64)
    d = np.zeros((gy, gx), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            k = w[abs(dy)] * w[abs(dx)]
            if k:
                n += k * pv[r + dy:r + dy + gy, r + dx:r + dx + gx]
                d += k * pp[r + dy:r + dy + gy, r + dx:r + dx + gx]
    assert n.size == 0 or (n.max() <= 255 * 1024 * 1024 and (d[present == 1] >= 1).all())
    return np.where(present == 1, (2 * n + d) // np.maximum(2 * d, 1), -1)


def gaussian_taps_exact(sigma, radius=None):
    """heatmap.gaussian_taps from 60-digit decimals; sigma a float, a str or a Decimal (a float is taken at its exact binary value)."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        s = decimal.Decimal(sigma)
        r = int((3 * s).to_integral_value(rounding=decimal.ROUND_CEILING)) if radius is None else int(radius)
        r = max(r, 1)
        g = [(-decimal.Decimal(d * d) / (2 * s * s)).exp() for d in range(r + 1)]
        total = g[0] + 2 * sum(g[1:])
        return tuple(int(((1023 - 2 * r) * gd / total + decimal.Decimal("0.5")).to_integral_value(rounding=decimal.ROUND_FLOOR)) for gd in g)


def box_taps(r):
    """A box of radius r whose full kernel sums to at most 1024."""
    return (1024 // (2 * r + 1),) * (r + 1)


IDENTITY = (7, 0, 0)

# the tables of the GPU tests against a workgroup tile of 16 x 64 cells: smaller than any radius, a row and a column longer than a tile, exactly one tile,
# one past the seam in both directions, and two seams each way
TABLES = [(1, 1), (1, 70), (70, 1), (16, 64), (17, 65), (33, 130)]


def kernels(gaussian_taps):
    """The half-kernels of the GPU tests: Gaussians of radius 1, 5 and 16 (the widest), a box of radius 3 and the identity."""
    return {"gauss1": gaussian_taps(0.5, 1), "gauss5": gaussian_taps(1.6, 5), "gauss16": gaussian_taps(5.3, 16), "box3": box_taps(3), "identity": IDENTITY}


def patterns(gy, gx):
    """The cell tables of the GPU tests, int64 [gy,gx] each: the four of heat_px_ref.tables, a table without any value, and one with values up to 300
    and a fifth of its cells absent."""
    from tests import heat_px_ref
    p = dict(heat_px_ref.tables(gy, gx, 7 * gy + gx))
    p["absent"] = np.full((gy, gx), -1, dtype=np.int64)
    rng = np.random.default_rng(1000 * gy + gx)
    over = rng.integers(0, 301, size=(gy, gx))
    over[rng.random((gy, gx)) < 0.2] = -1
    over.reshape(-1)[0] = 300
    if over.size > 1:
        over.reshape(-1)[-1] = -1
    p["over"] = over
    return p
