"""CPU: tissue selection (toad_region_tissue_cells_u8, toad_tissue_tile_counts: an additive extension of ABI 15; toad_amd/tissue.py). The entry points exist
in the header, the library and the ctypes table and refuse what the host can see before any device access; the lattice arithmetic is host code; and the
numpy reference the GPU tests compare against (tests/tissue_ref.py) is itself tested here, on the inputs of those tests: every "mixed outcome" condition
the GPU tests rely on is a fact about the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tissue_ref as ref

TISSUE_SYMBOLS = ("toad_region_tissue_cells_u8", "toad_tissue_tile_counts")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (region (hr, wr), tile (H, W), stride (sy, sx), origin (x, y)) of the tile-count cases of test_gpu_tissue.py
LATTICES = [((300, 520), (64, 64), (32, 32), (0, 0)), ((300, 520), (64, 64), (64, 64), (8, 4)), ((203, 333), (32, 64), (8, 16), (0, 0)),
            ((300, 520), (256, 256), (64, 64), (0, 0)), ((131, 67), (16, 16), (16, 16), (0, 0))]


def test_tissue_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in TISSUE_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert "NOT OpenCV's rounded S" in header and "255 * (mx - mn) > sat_thresh * mx" in header      # the header states the predicate and what it is not


def test_tissue_entries_report_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # a region at an odd address is fine; int32 arrays there are refused
    two = ctypes.c_void_p((1 << 21) + 2)

    def cells(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, cell=16, sat=8, vmin=0, c=one):
        return lib.toad_region_tissue_cells_u8(r, pitch, hr, wr, cell, sat, vmin, c, None)

    def tiles(c=one, gy=5, gx=9, cell=16, x0=16, y0=0, h=32, w=64, sx=16, sy=16, nx=4, ny=3, t=one):
        return lib.toad_tissue_tile_counts(c, gy, gx, cell, x0, y0, h, w, sx, sy, nx, ny, t, None)      # ends at x = 16 + 48 + 64 = 128 <= 144, y = 64 <= 80

    a, b = "toad_region_tissue_cells_u8", "toad_tissue_tile_counts"
    cases = [
        (a, lambda: cells(r=None), -1, "null pointer"), (a, lambda: cells(c=None), -1, "null pointer"),
        (a, lambda: cells(sat=-1), -1, "sat_thresh"), (a, lambda: cells(sat=256), -1, "sat_thresh"),
        (a, lambda: cells(vmin=-1), -1, "val_min"), (a, lambda: cells(vmin=256), -1, "val_min"),
        (a, lambda: cells(cell=0), -2, "cell"), (a, lambda: cells(cell=12), -2, "cell"), (a, lambda: cells(cell=128), -2, "cell"), (a, lambda: cells(cell=2), -2, "cell"),
        (a, lambda: cells(hr=0), -2, "bad shape"), (a, lambda: cells(wr=0), -2, "bad shape"), (a, lambda: cells(hr=-3), -2, "bad shape"),
        (a, lambda: cells(pitch=3 * 31 - 1), -2, "pitch"), (a, lambda: cells(pitch=0), -2, "pitch"), (a, lambda: cells(pitch=-94), -2, "pitch"),
        (a, lambda: cells(wr=715827883, pitch=1 << 32), -2, "2^31"),                   # 3 Wr = 2^31 + 1
        (a, lambda: cells(c=odd), -4, "4-byte aligned"), (a, lambda: cells(c=two), -4, "4-byte aligned"),
        (b, lambda: tiles(c=None), -1, "null pointer"), (b, lambda: tiles(t=None), -1, "null pointer"),
        (b, lambda: tiles(cell=24), -2, "cell"), (b, lambda: tiles(cell=1), -2, "cell"),
        (b, lambda: tiles(nx=0), -2, "bad shape"), (b, lambda: tiles(ny=0), -2, "bad shape"), (b, lambda: tiles(h=0), -2, "bad shape"),
        (b, lambda: tiles(w=0), -2, "bad shape"), (b, lambda: tiles(sx=0), -2, "bad shape"), (b, lambda: tiles(sy=-16), -2, "bad shape"),
        (b, lambda: tiles(gy=0), -2, "bad shape"),
        (b, lambda: tiles(x0=-16), -2, "x0"), (b, lambda: tiles(y0=-16), -2, "y0"), (b, lambda: tiles(x0=8), -2, "x0"), (b, lambda: tiles(y0=4), -2, "y0"),
        (b, lambda: tiles(h=40), -2, "H = 40"), (b, lambda: tiles(w=72), -2, "W = 72"), (b, lambda: tiles(sx=24), -2, "sx"), (b, lambda: tiles(sy=8), -2, "sy"),
        (b, lambda: tiles(nx=6), -2, "last tile"),                                     # ends at x = 16 + 80 + 64 = 160 > 144
        (b, lambda: tiles(ny=5), -2, "last tile"),                                     # ends at y = 64 + 32 = 96 > 80
        (b, lambda: tiles(c=two), -4, "4-byte aligned"), (b, lambda: tiles(t=odd), -4, "4-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)
    # the largest lattice that is taken ends exactly at Gx * cell, Gy * cell: only the later alignment check stops these calls
    assert tiles(nx=5, ny=4, t=odd) == -4 and tiles(x0=0, nx=6, ny=4, t=odd) == -4
    assert cells(wr=715827882, pitch=1 << 32, c=odd) == -4                              # 3 Wr = 2^31 - 2 is taken


def test_lattice_cell():
    from toad_amd.tissue import lattice_cell
    assert lattice_cell(256, 256, (0, 0)) == 64 and lattice_cell(256) == 64
    assert lattice_cell(256, 64, (8, 4)) == 4
    assert lattice_cell(256, 48) == 16
    assert lattice_cell((32, 64), (8, 16)) == 8 and lattice_cell(64, 32) == 32 and lattice_cell(64, 64, (8, 4)) == 4 and lattice_cell((8, 256)) == 8
    with pytest.raises(ValueError, match=r"30.*multiple of 4"):
        lattice_cell(256, 30)
    with pytest.raises(ValueError, match=r"origin y = 2 .*multiple of 4"):
        lattice_cell(256, 64, (8, 2))
    with pytest.raises(ValueError, match="multiple of 4"):
        lattice_cell(250)
    with pytest.raises(ValueError):
        lattice_cell(256, 64, (-4, 0))


def test_lattice_extent():
    from toad_amd.tissue import lattice
    assert lattice(300, 520, 256, 64) == (5, 1)
    assert lattice(300, 520, 256) == (2, 1) and lattice(4096, 8192, 256) == (32, 16)
    assert lattice(255, 520, 256) == (2, 0) and lattice(300, 255, 256) == (0, 1) and lattice(7, 5, 16) == (0, 0)          # a region smaller than the tile
    assert lattice(203, 333, (32, 64), (8, 16)) == (17, 22)                                # non-square: (333 - 64) // 16 + 1, (203 - 32) // 8 + 1
    assert lattice(40, 1100, (8, 256), (8, 256)) == (4, 5)
    assert lattice(300, 520, 64, 64, (8, 4)) == (8, 4) and lattice(300, 520, 64, 64, (460, 240)) == (0, 0) and lattice(300, 520, 64, 64, (456, 236)) == (1, 1)
    for (hr, wr), tile, stride, origin in LATTICES:                                         # ... and the reference's own extent agrees
        assert lattice(hr, wr, tile, stride, origin) == ref.lattice_extent(hr, wr, tile, stride, origin)
    # every tile of the extent lies inside the region, and one more in either direction does not
    for (hr, wr), (h, w), (sy, sx), (x0, y0) in LATTICES:
        nx, ny = lattice(hr, wr, (h, w), (sy, sx), (x0, y0))
        assert x0 + (nx - 1) * sx + w <= wr < x0 + nx * sx + w and y0 + (ny - 1) * sy + h <= hr < y0 + ny * sy + h


def test_tissue_origins_refusals_cpu(monkeypatch):
    """Each refusal comes with the region wrappers' exception and before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.tissue import tissue_origins, tissue_tile_fraction

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    region = torch.zeros(300, 520, 3, dtype=torch.uint8)
    for bad in (-0.01, 1.01, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="min_fraction"):
            tissue_origins(region, 64, min_fraction=bad)
    for call in (lambda r: tissue_origins(r, 64), lambda r: tissue_tile_fraction(r, 64), lambda r: ops.region_tissue_cells(r, 16, 8, 0)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call(region)                                               # on the CPU
    # what comes after the device test, on a stand-in that claims to be on the device
    meta = torch.zeros(300, 1040, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for call in (lambda r: tissue_origins(r, 64), lambda r: tissue_tile_fraction(r, 64), lambda r: ops.region_tissue_cells(r, 16, 8, 0)):
        with pytest.raises(TypeError, match="uint8"):
            call(meta.float())
        with pytest.raises(ValueError, match=r"stride\(1\) == 3"):
            call(meta[:, ::2])                                         # stride(1) == 6
        with pytest.raises(ValueError, match=r"\[Hr,Wr,3\]"):
            call(torch.zeros(3, 300, 520, dtype=torch.uint8, device="meta"))
        with pytest.raises(ValueError, match=r"\[Hr,Wr,3\]"):
            call(torch.zeros(2, 300, 520, 3, dtype=torch.uint8, device="meta"))
    reg = meta[:, :520]
    with pytest.raises(ValueError, match="multiple of 4"):
        tissue_origins(reg, 64, 30)
    for k in (dict(sat_thresh=256), dict(val_min=-1), dict(sat_thresh=8.0)):
        with pytest.raises(ValueError, match=r"\[0, 255\]"):
            tissue_origins(reg, 64, **k)
    with pytest.raises(ValueError, match="cell"):
        ops.region_tissue_cells(reg, 12, 8, 0)
    # a region smaller than one tile: an empty result, and still nothing is launched
    small = torch.zeros(40, 50, 3, dtype=torch.uint8, device="meta")
    o = tissue_origins(small, 64)
    assert isinstance(o, np.ndarray) and o.shape == (0, 2) and o.dtype == np.int64
    o, c = tissue_origins(small, 64, return_counts=True)
    assert o.shape == (0, 2) and c.shape == (0,)


# ---- the reference itself, on the inputs of the GPU tests ---------------------------------------------------------------------------------------------
def test_reference_predicate_by_hand():
    px = np.array([[[0, 0, 0], [1, 0, 0], [128, 128, 128], [255, 247, 255], [255, 246, 255], [200, 100, 150], [15, 0, 0], [16, 0, 0]]], dtype=np.uint8)
    # sat 8: 255 (mx - mn) > 8 mx; (255, 247, 255): 2040 > 2040 is false, (255, 246, 255): 2295 > 2040
    assert ref.tissue_mask(px, 8, 0).tolist() == [[False, True, False, False, True, True, True, True]]
    assert ref.tissue_mask(px, 8, 16).tolist() == [[False, False, False, False, True, True, False, True]]
    assert not ref.tissue_mask(px, 255, 0).any()                       # 255 (mx - mn) > 255 mx never holds
    assert ref.tissue_mask(px, 0, 0).tolist() == [[False, True, False, True, True, True, True, True]]
    assert ref.cell_counts(px, 4, 8, 0).tolist() == [[1, 4]] and ref.cell_counts(px, 8, 8, 0).tolist() == [[5]]


def test_reference_cells_and_tiles_agree_and_the_slide_is_mixed():
    s = ref.slide(300, 520, 1)
    assert s.shape == (300, 520, 3) and s.dtype == np.uint8 and np.array_equal(s, ref.slide(300, 520, 1))
    for sat, vmin in ((8, 0), (8, 16), (40, 16)):
        c = ref.cell_counts(s, 16, sat, vmin)
        assert c.shape == (19, 33) and int(c.sum()) == int(ref.tissue_mask(s, sat, vmin).sum())
        full = np.minimum(16, 300 - 16 * np.arange(19))[:, None] * np.minimum(16, 520 - 16 * np.arange(33))[None, :]
        assert (c == 0).any() and (c == full).any() and ((c > 0) & (c < full)).any()          # empty, full and partial cells all occur
    # the pale blob is tissue at sat_thresh 8 and not at 40; the black margin at val_min 0 and not at 16
    blob = (slice(int(0.82 * 300) - 5, int(0.82 * 300) + 5), slice(int(0.8 * 520) - 5, int(0.8 * 520) + 5))
    assert ref.tissue_mask(s, 8, 16)[blob].all() and not ref.tissue_mask(s, 40, 16)[blob].any()
    assert ref.tissue_mask(s, 8, 0)[:, -5:].any() and not ref.tissue_mask(s, 8, 16)[:, -5:].any()
    # ... which changes the selection on a lattice that reaches the margin (8 x 8 tiles; the 64 x 64 lattice at stride 32 ends at column 511)
    k0, k16 = ref.selection(s, (8, 8), (8, 8), (0, 0), 0.25, 8, 0)[0], ref.selection(s, (8, 8), (8, 8), (0, 0), 0.25, 8, 16)[0]
    assert len(k16) < len(k0) and (k0[:, 0] == 512).any() and not (k16[:, 0] == 512).any()
    # tiles of whole cells: the slices of the mask equal the sums of the cells
    for (hr, wr), (h, w), (sy, sx), (x0, y0) in LATTICES:
        r = ref.slide(hr, wr, 1)
        t = ref.tile_counts(r, (h, w), (sy, sx), (x0, y0), 8, 0)
        c = ref.cell_counts(r, 4, 8, 0)
        for j, i in ((0, 0), (t.shape[0] - 1, t.shape[1] - 1), (t.shape[0] // 2, t.shape[1] // 3)):
            y, x = (y0 + j * sy) // 4, (x0 + i * sx) // 4
            assert t[j, i] == c[y:y + h // 4, x:x + w // 4].sum()
        assert t.min() < t.max()


@pytest.mark.parametrize("case", range(len(LATTICES)))
def test_reference_selection_is_mixed(case):
    (hr, wr), tile, stride, origin = LATTICES[case]
    r = ref.slide(hr, wr, 1)
    kept, total = ref.selection(r, tile, stride, origin, 0.25, 8, 0)
    assert 0 < len(kept) < total, (len(kept), total)
    every, _ = ref.selection(r, tile, stride, origin, 0.0, 8, 0)
    assert len(every) == total and every[0].tolist() == list(origin)
    if case == 0:
        assert total == 120
        for f in (0.05, 0.5, 1.0):
            k, _ = ref.selection(r, tile, stride, origin, f, 8, 0)
            assert 0 < len(k) < total, (f, len(k))
    if case == 3:
        assert total == 5 and len(kept) == 4                           # a single row of 5 tiles, 4 of 5 kept at 0.25
    p, t = ref.selection(ref.slide(40, 1100, 1), (8, 256), (8, 256), (0, 0), 0.25, 8, 0)      # the pipeline case
    assert t == 20 and 0 < len(p) < t


def test_reference_on_the_exhaustive_probe_blocks():
    img, mx, mn = ref.probe_blocks()
    assert img.shape == (1536, 1028, 3) and int((img != 128).any(axis=2).reshape(384, 4, 257, 4).sum(axis=(1, 3)).max()) <= 1
    for sat in (0, 8, 15, 254, 255):
        for vmin in (0, 1, 50, 255):
            want = (mx >= vmin) & (255 * (mx - mn) > sat * mx)
            got = ref.cell_counts(img, 4, sat, vmin)
            assert np.array_equal(got, want.astype(np.int64))
            assert (not want.any()) if sat == 255 else (want.any() and not want.all())
    assert int(((255 * (mx - mn) > 8 * mx)).sum()) == 3 * 31743            # 31,743 of the 32,896 (mx, mn) pairs, in each of the 3 positions
