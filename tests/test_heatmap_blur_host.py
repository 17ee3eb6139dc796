"""CPU: the blur of the heat-map cell table (toad_heat_cells_blur: an additive extension of ABI 15; ops.heat_cells_blur, heatmap.gaussian_taps and the blur
keyword of heatmap.attention_canvas and eval.region_tissue_attention_heatmap). The entry point exists in the header, the library and the ctypes table and
refuses what the host can see, in the documented order, before any device access; the Python wrappers refuse before the library is loaded; the Gaussian
taps are held to a 60-digit recomputation; and the numpy reference the GPU tests compare against (tests/heat_blur_ref.py) is itself tested here, by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import heat_blur_ref as ref
from tests import heat_px_ref

NAME = "toad_heat_cells_blur"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blur_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\bint\s+" + NAME + r"\s*\(const int \*cells, int Gy, int Gx, const int \*taps", header), f"{NAME} is not declared in include/toad_hip.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 7
    for text in ("N = sum w[|dy|] * w[|dx|] * min(v, 255)", "D = sum w[|dy|] * w[|dx|]", "out = (2 * N + D) / (2 * D)", "<= 1024", "1 <= radius <= 16"):
        assert text in header, text


def test_blur_entry_reports_argument_errors_in_order_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one, other = ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22)      # non-null fake pointers: every check below comes before a device access
    odd, two = ctypes.c_void_p((1 << 21) + 1), ctypes.c_void_p((1 << 22) + 2)
    arr = lambda *w: (ctypes.c_int * len(w))(*w)              # noqa: E731  (the taps are read on the host: a real array)
    good = arr(4, 2, 1)

    def blur(c=one, gy=3, gx=5, taps=good, r=2, out=other):
        return lib.toad_heat_cells_blur(c, gy, gx, taps, r, out, None)

    cases = [
        (lambda: blur(c=None), -1, "null pointer"), (lambda: blur(out=None), -1, "null pointer"),
        (lambda: blur(gy=0), -2, "bad shape"), (lambda: blur(gx=0), -2, "bad shape"), (lambda: blur(gy=-3), -2, "bad shape"),
        (lambda: blur(gy=1 << 16, gx=1 << 15), -2, "bad shape"), (lambda: blur(gy=(1 << 31) - 1, gx=2), -2, "bad shape"),
        (lambda: blur(r=0), -2, "radius"), (lambda: blur(r=17), -2, "radius"), (lambda: blur(r=-1), -2, "radius"),
        (lambda: blur(taps=None), -1, "null taps"),
        (lambda: blur(taps=arr(0, 1, 1)), -1, "taps[0]"), (lambda: blur(taps=arr(-4, 1, 1)), -1, "taps[0]"), (lambda: blur(taps=arr(4, -1, 1)), -1, "taps[1]"),
        (lambda: blur(taps=arr(4, 1, -1)), -1, "taps[2]"), (lambda: blur(taps=arr(1023, 1, 0)), -1, "sum to 1025"),
        (lambda: blur(taps=arr(1, 256, 256)), -1, "sum to 1025"), (lambda: blur(taps=arr(1 << 30, 1 << 30, 1 << 30)), -1, "taps"),
        (lambda: blur(out=one), -1, "must not be cells"),
        (lambda: blur(c=odd), -4, "4-byte aligned"), (lambda: blur(out=two), -4, "4-byte aligned"),
    ]
    for call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # the order: of two faults the earlier check reports
    for call, rc, text in [
        (lambda: blur(gy=0, r=0), -2, "bad shape"), (lambda: blur(gx=1 << 30, gy=2, taps=None), -2, "bad shape"),
        (lambda: blur(r=17, taps=None), -2, "radius"), (lambda: blur(r=0, taps=arr(0), out=one), -2, "radius"),
        (lambda: blur(taps=None, out=one), -1, "null taps"), (lambda: blur(taps=arr(0, 0, 0), out=one), -1, "taps[0]"),
        (lambda: blur(taps=arr(1000, 20, 0), c=odd, out=odd), -1, "sum to 1040"),
        (lambda: blur(c=odd, out=odd), -1, "must not be cells"),
    ]:
        got = call()
        msg = err()
        assert got == rc and text in msg, (text, got, msg)
    # what is taken: only the later alignment check stops these calls. Only taps[0 .. radius] are read.
    for ok in (dict(taps=arr(1024, 0, 0)), dict(taps=arr(1, 0, 0)), dict(taps=arr(2, 511, 0)), dict(taps=arr(4, 2, 1, -9), r=2), dict(taps=arr(1, 0), r=1),
               dict(taps=arr(*([32] + [31] * 16)), r=16), dict(gy=(1 << 31) - 1, gx=1), dict(gy=1, gx=(1 << 31) - 1), dict(gy=46340, gx=46340)):
        assert blur(c=odd, **ok) == -4, ok


def test_blur_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, heatmap, ops
    from toad_amd.eval import region_tissue_attention_heatmap
    from toad_amd.heatmap import attention_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.heat_cells_blur(torch.zeros(4, 4, dtype=torch.int32), (2, 1))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells = torch.zeros(4, 6, dtype=torch.int32, device="meta")
    bad_taps = (((3,), "radius"), ((1,) * 18, "radius"), ((), "radius"), ((0, 1), r"taps\[0\]"), ((4, -1), "every tap"), ((1000, 13), "exceeds 1024"),
                ((2.0, 1), "ints"), ((True, 1), "ints"), ("21", "sequence"), (5, "sequence"), (None, "sequence"), (torch.tensor([2, 1]), "sequence"))
    for taps, text in bad_taps:
        with pytest.raises(ValueError, match=text):
            ops.heat_cells_blur(cells, taps)
    with pytest.raises(ValueError, match=r"\[Gy,Gx\]"):
        ops.heat_cells_blur(cells.view(2, 2, 6), (2, 1))
    with pytest.raises(TypeError, match="int32"):
        ops.heat_cells_blur(cells.float(), (2, 1))
    with pytest.raises(ValueError, match="contiguous"):
        ops.heat_cells_blur(cells[:, ::2], (2, 1))
    assert ops.heat_blur_taps("x", [np.int64(4), np.int32(2), 1]) == (4, 2, 1) and ops.heat_blur_taps("x", np.array([1022, 1])) == (1022, 1)
    # an empty table launches nothing
    for shape in ((0, 6), (4, 0), (0, 0)):
        got = ops.heat_cells_blur(torch.zeros(shape, dtype=torch.int32, device="meta"), (2, 1))
        assert got.dtype == torch.int32 and tuple(got.shape) == shape

    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    none = (np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"))
    for tile, k, text in ((16, dict(blur="yes"), "sequence"), (16, dict(blur=-1.0), "positive and finite"), (16, dict(blur=0), "positive and finite"),
                          (16, dict(blur=float("nan")), "positive and finite"), (16, dict(blur=float("inf")), "positive and finite"),
                          (16, dict(blur=(0, 1)), r"taps\[0\]"), (16, dict(blur=(5, -1)), "every tap"), (16, dict(blur=(1000, 20)), "exceeds 1024"),
                          (16, dict(blur=(3,)), "radius"), (16, dict(blur=[1] * 18), "radius"), (16, dict(blur=(2.5, 1.0)), "ints"),
                          ((16, 32), dict(blur=True), "square tile"),
                          (16, dict(blur=100.0), "limit of 16 cells"),                     # sigma = 6.25 cells: ceil(3 sigma) = 19
                          (4, dict(blur=30), "limit of 16 cells")):                       # sigma = 7.5 cells
        with pytest.raises(ValueError, match=text):
            attention_canvas(meta, *none, tile, **k)
        with pytest.raises(ValueError, match=text):                  # the pipeline call refuses before the selection runs: no extractor, no model
            region_tissue_attention_heatmap(None, None, meta, tile=tile, **k)
    # CLAM's usual lattice, 256 / 64, is inside the limit; 256 / 16 is not
    assert len(heatmap.blur_taps(True, (256, 256), 64)) == 9 and len(heatmap.blur_taps(True, (256, 256), 32)) == 16
    with pytest.raises(ValueError, match="limit of 16 cells"):
        heatmap.blur_taps(True, (256, 256), 16)
    assert heatmap.blur_taps(False, (16, 32), 16) is None and heatmap.blur_taps(None, (16, 32), 16) is None
    assert heatmap.blur_taps(24.1, (16, 32), 16) == heatmap.gaussian_taps(24.1 / 16) and heatmap.blur_taps([4, 2, 1], (16, 32), 16) == (4, 2, 1)
    assert heatmap.blur_taps(True, (64, 64), 32) == heatmap.gaussian_taps(38.9 / 32) == heatmap.blur_taps(38.9, (64, 64), 32)
    # empty origins launch no blur, and blur=False / None launch none either
    monkeypatch.setattr(ops, "heat_cells_blur", lambda *a, **k: no_launch())
    monkeypatch.setattr(ops, "region_heat_blend_px", lambda region, cells, *a, **k: cells)
    monkeypatch.setattr(ops, "heat_cells", lambda *a, **k: torch.zeros(4, 4, dtype=torch.int32, device="meta"))
    for b in (True, 20.0, (4, 2, 1)):
        assert tuple(attention_canvas(meta, *none, 16, blur=b).shape) == (4, 4)
    some = (np.array([[0, 0]]), torch.zeros(1, device="meta"))
    monkeypatch.setattr(heatmap, "tile_table", lambda *a, **k: torch.zeros(4, 4, dtype=torch.int32, device="meta"))
    for b in (False, None):
        assert tuple(attention_canvas(meta, *some, 16, blur=b).shape) == (4, 4)
    with pytest.raises(AssertionError, match="library was reached"):      # ... and a blur with origins does reach it
        attention_canvas(meta, *some, 16, blur=True)


# ---- gaussian_taps ------------------------------------------------------------------------------------------------------------------------------------
def test_gaussian_taps():
    from toad_amd.heatmap import gaussian_taps
    for sigma in (0.3, 1, 2.41, 4.81):
        w = gaussian_taps(sigma)
        r = len(w) - 1
        assert r == max(1, int(np.ceil(3 * sigma))) and all(isinstance(t, int) for t in w)
        assert w == ref.gaussian_taps_exact(sigma), sigma
        assert all(a >= b for a, b in zip(w, w[1:])) and w[0] >= 1 and min(w) >= 0
        assert 1024 - 2 * (2 * r + 1) <= w[0] + 2 * sum(w[1:]) <= 1024, (sigma, w)
        ref.check_taps(w)
    assert gaussian_taps(2.41) == (167, 153, 118, 77, 42, 19, 8, 2, 1)       # CLAM's width on the 256 / 64 lattice
    for sigma in np.linspace(0.05, 5.33, 89).tolist():
        for radius in (None, 1, 7, 16):
            w = gaussian_taps(sigma, radius)
            r = len(w) - 1
            assert r == (radius or max(1, int(np.ceil(3 * sigma)))) and w == ref.gaussian_taps_exact(sigma, radius), (sigma, radius)
            assert all(a >= b for a, b in zip(w, w[1:])) and w[0] >= 1 and 1024 - 2 * (2 * r + 1) <= w[0] + 2 * sum(w[1:]) <= 1024
    assert gaussian_taps(1e-3) == (1021, 0) and gaussian_taps(1e6, 16) == (30,) * 17       # the ends: a spike and a box, both legal
    with pytest.raises(ValueError, match=r"sigma = 9\.6 cells.*limit of 16 cells"):
        gaussian_taps(9.6)
    assert len(gaussian_taps(9.6, 16)) == 17
    for bad in (0, -1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="sigma"):
            gaussian_taps(bad)
    for bad in (0, 17, -3, 2.0, True):
        with pytest.raises(ValueError, match="radius"):
            gaussian_taps(1.0, bad)


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------------------
def test_reference_three_by_three_by_hand():
    """taps (2, 1): the cell itself weighs 4, an edge neighbour 2, a corner neighbour 1; 300 reads as 255."""
    c = np.array([[10, 20, -1], [40, 50, 60], [-1, 80, 300]])
    # (1, 1): N = 4 * 50 + 2 * (20 + 40 + 60 + 80) + (10 + 255) = 865, D = 4 + 8 + 2 = 14 -> 1744 // 28 = 62
    # (0, 0): N = 4 * 10 + 2 * 20 + 2 * 40 + 50 = 210, D = 9 -> 429 // 18 = 23           (0, 1): N = 80 + 20 + 100 + 40 + 60 = 300, D = 10 -> 30
    # (1, 0): N = 160 + 20 + 100 + 20 + 80 = 380, D = 10 -> 770 // 20 = 38               (1, 2): N = 240 + 510 + 100 + 20 + 80 = 950, D = 10 -> 95
    # (2, 1): N = 320 + 510 + 100 + 40 + 60 = 1030, D = 10 -> 2070 // 20 = 103           (2, 2): N = 1020 + 160 + 120 + 50 = 1350, D = 9 -> 2709 // 18 = 150
    assert ref.blur(c, (2, 1)).tolist() == [[23, 30, -1], [38, 62, 95], [-1, 103, 150]]
    assert ref.blur(c, (2, 1, 0, 0)).tolist() == ref.blur(c, (2, 1)).tolist()          # zero taps beyond the first widen nothing
    assert ref.blur(c, (1, 0)).tolist() == [[10, 20, -1], [40, 50, 60], [-1, 80, 255]]
    # rounding half up: values 0 and 1 side by side with a box -> N / D = 1 / 2 -> 1
    assert ref.blur(np.array([[0, 1]]), (1, 1)).tolist() == [[1, 1]] and ref.blur(np.array([[0, 0, 1]]), (1, 1)).tolist() == [[0, 0, 1]]


def test_reference_properties():
    rng = np.random.default_rng(12)
    kernels = [(2, 1), ref.box_taps(3), (167, 153, 118, 77, 42, 19, 8, 2, 1), (30,) * 17, (1024 - 2 * 16, 1) + (0,) * 14 + (15,)]
    for gy, gx in ((1, 1), (1, 9), (7, 1), (12, 19), (37, 41)):
        holes = rng.random((gy, gx)) < 0.35
        noisy = rng.integers(0, 256, size=(gy, gx))
        noisy[holes] = -1
        for w in kernels:
            for value in (0, 1, 127, 255):                           # a constant field with holes comes back unchanged
                const = np.where(holes, -1, value)
                assert np.array_equal(ref.blur(const, w), const), (gy, gx, w, value)
            got = ref.blur(noisy, w)
            assert np.array_equal(got < 0, noisy < 0) and (got[noisy >= 0] <= 255).all()              # absent stays absent, present stays present
            pres = noisy[noisy >= 0]
            if pres.size:
                assert got[noisy >= 0].min() >= pres.min() and got[noisy >= 0].max() <= pres.max()      # a weighted mean
            assert np.array_equal(ref.blur(np.full((gy, gx), -1), w), np.full((gy, gx), -1))
            big = np.where(holes, -1, noisy + 200)                   # values above 255 read as 255
            assert (big.max() > 255 or holes.all()) and np.array_equal(ref.blur(big, w), ref.blur(np.minimum(big, 255), w))
            single = np.full((gy, gx), -1)                           # a single present cell keeps its value
            single[gy // 2, gx // 2] = 201
            assert np.array_equal(ref.blur(single, w), single)
        for ident in (ref.IDENTITY, (1, 0), (1024,) + (0,) * 16):     # identity taps return the input (read at 255)
            assert np.array_equal(ref.blur(noisy, ident), noisy)
    # a linear ramp is unchanged at r cells or more from the table's border (the kernel is symmetric), and changed at a border
    yy, xx = np.mgrid[0:40, 0:50]
    ramp = 3 * yy + 2 * xx
    assert ramp.max() <= 255
    for w in kernels:
        r = len(w) - 1
        got = ref.blur(ramp, w)
        assert np.array_equal(got[r:-r, r:-r], ramp[r:-r, r:-r]) and got[0, 0] > ramp[0, 0] and got[-1, -1] < ramp[-1, -1], w
    # smoothing does smooth: the largest step between neighbours of a noisy table shrinks
    t = rng.integers(0, 256, size=(30, 30))
    assert np.abs(np.diff(ref.blur(t, (167, 153, 118, 77, 42, 19, 8, 2, 1)), axis=1)).max() < np.abs(np.diff(t, axis=1)).max() // 4


def test_reference_tables_are_what_the_gpu_tests_need():
    from toad_amd.heatmap import gaussian_taps
    KERNELS, TABLES, patterns = ref.kernels(gaussian_taps), ref.TABLES, ref.patterns
    assert TABLES == [(1, 1), (1, 70), (70, 1), (16, 64), (17, 65), (33, 130)]
    assert [len(w) - 1 for w in KERNELS.values()] == [1, 5, 16, 3, 2] and KERNELS["box3"] == (146,) * 4 and KERNELS["identity"] == ref.IDENTITY
    assert KERNELS["gauss16"] == gaussian_taps(5.3, 16) and KERNELS["gauss16"][16] >= 1      # the widest kernel reaches its last tap
    for w in KERNELS.values():
        ref.check_taps(w)
    for gy, gx in TABLES:
        p = patterns(gy, gx)
        assert set(p) == set(heat_px_ref.tables(gy, gx, 0)) | {"absent", "over"} and (p["absent"] == -1).all() and p["over"].max() == 300
        if gy * gx > 1:
            assert (p["over"] > 255).any() and (p["over"] == -1).any() and (p["checker"] == -1).any()
            for name in ("ramp", "checker", "over"):                 # the blur changes these tables
                assert not np.array_equal(ref.blur(p[name], KERNELS["gauss5"]), np.minimum(p[name], 255)), (gy, gx, name)
