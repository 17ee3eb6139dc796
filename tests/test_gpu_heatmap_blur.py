"""GPU: the blur of the heat-map cell table (csrc/heatmap.hip heat_cells_blur_kernel, toad_heat_cells_blur; ops.heat_cells_blur, heatmap.gaussian_taps and
the blur keyword of heatmap.attention_canvas and eval.region_tissue_attention_heatmap). Integers throughout, so every comparison is == on whole arrays:
the kernel against the non-separable numpy reference of tests/heat_blur_ref.py (tested on its own, by hand, in test_heatmap_blur_host.py), the canvas
against tests/heat_px_ref.canvas of the reference-blurred cells."""
import functools

import numpy as np
import pytest
import torch

from tests import heat_blur_ref as ref
from tests import heat_px_ref
from tests import heat_ref
from tests import tissue_ref
from tests.test_gpu_heatmap import POISON, dev, same_cells, same_px


def blur_into_poison(cells: torch.Tensor, taps) -> torch.Tensor:
    """toad_heat_cells_blur into a table pre-filled with 0x7f7f7f7f: equality with the reference then also proves every element is written."""
    import ctypes
    from toad_amd import _lib
    out = torch.full(tuple(cells.shape), POISON, dtype=torch.int32, device=cells.device)
    w = (ctypes.c_int * len(taps))(*taps)
    _lib.check(_lib.load().toad_heat_cells_blur(cells.data_ptr(), cells.shape[0], cells.shape[1], w, len(taps) - 1, out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "toad_heat_cells_blur")
    return out


# ---- 1. the kernel against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gy,gx", ref.TABLES)
def test_blurred_cells_equal_the_reference_and_every_element_is_written(cuda, gy, gx):
    """Tables smaller than the radius, longer than a workgroup tile (16 x 64 cells) along one axis, exactly one tile, one past the seam both ways and two
    seams each way; Gaussians of radius 1, 5 and 16, a box and the identity; ramps, holes, a checkerboard, an absent border, nothing at all, values to 300."""
    from toad_amd import ops
    from toad_amd.heatmap import gaussian_taps
    for pname, tab in ref.patterns(gy, gx).items():
        cells = dev(tab, cuda, torch.int32)
        for kname, w in ref.kernels(gaussian_taps).items():
            want = ref.blur(tab, w)
            got = blur_into_poison(cells, w)
            assert same_cells(got, want), (pname, kname)
            assert torch.equal(ops.heat_cells_blur(cells, w), got), (pname, kname)
            assert same_cells(cells, tab)                            # the input is left as it was
            if kname == "identity":
                assert np.array_equal(want, np.minimum(tab, 255))


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------------------------------
HR, WR, TILE, STRIDE, CELL = 192, 320, 64, 32, 32
E2E_TAPS = (100, 80, 40, 9, 1)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """(region uint8 [192,320,3], origins [B,2], scores float32 [B], cells int64 [6,10]): tiles of 64 at stride 32 (cell 32, 9 x 5 tiles), about half of
    them present, a NaN score among them. Read-only, cached."""
    rng = np.random.default_rng(2024)
    region = rng.integers(0, 256, size=(HR, WR, 3), dtype=np.uint8)
    nx, ny = (WR - TILE) // STRIDE + 1, (HR - TILE) // STRIDE + 1
    keep = rng.random((ny, nx)) < 0.5
    keep[0, 0] = keep[2, 4] = True
    origins = np.array([(STRIDE * i, STRIDE * j) for j in range(ny) for i in range(nx) if keep[j, i]], dtype=np.int64)
    scores = rng.random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[2] = 0.0, 1.0, np.nan
    q = heat_ref.quantise(scores)
    t = heat_ref.table(origins[q >= 0], q[q >= 0], (TILE, TILE), (STRIDE, STRIDE), (0, 0), (nx, ny))
    cells = heat_ref.cells(t, CELL, (TILE, TILE), (STRIDE, STRIDE), (0, 0), (HR, WR))
    assert (nx, ny) == (9, 5) and cells.shape == (6, 10) and (cells == -1).any() and len(np.unique(cells)) > 8
    for a in (region, origins, scores, cells):
        a.setflags(write=False)
    return region, origins, scores, cells


@functools.lru_cache(maxsize=None)
def e2e_mask(md):
    rng = np.random.default_rng(77 + md)
    m = rng.integers(0, 256, size=(HR // md, WR // md), dtype=np.uint8)
    m.setflags(write=False)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [True, 20.0, E2E_TAPS], ids=["clam", "sigma20px", "taps"])
def test_attention_canvas_blur_equals_the_reference(cuda, blur):
    from toad_amd.heatmap import attention_canvas, gaussian_taps
    s, origins, scores, cells = e2e_case()
    taps = gaussian_taps((0.6 * TILE + 0.5) / CELL) if blur is True else gaussian_taps(20.0 / CELL) if blur == 20.0 else E2E_TAPS
    assert len(taps) - 1 == (4 if blur is True else 2 if blur == 20.0 else 4)
    blurred = ref.blur(cells, taps)
    assert not np.array_equal(blurred, cells) and np.array_equal(blurred < 0, cells < 0)
    region, sd, lut = dev(s, cuda), dev(scores, cuda), heat_ref.jet()
    lat = dict(tile=TILE, stride=STRIDE)
    md = 32                                                          # a multiple of every down below
    m = e2e_mask(md)
    mask = (dev(m, cuda), 100, md)
    for down in (1, 4, 8, 32):
        for smooth in (False, True):
            for masked in (False, True):
                kw = dict(mask=m, mask_down=md, mask_thresh=100) if masked else {}
                want = heat_px_ref.canvas(s, blurred, CELL, lut, 102, down, smooth=smooth, **kw)
                got = attention_canvas(region, origins, sd, down=down, smooth=smooth, mask=mask if masked else None, blur=blur, **lat)
                assert same_px(got, want), (down, smooth, masked)
                if not masked:                                       # the blur is not a no-op on the canvas
                    assert not np.array_equal(want, heat_px_ref.canvas(s, cells, CELL, lut, 102, down, smooth=smooth)), (down, smooth)


@pytest.mark.gpu
def test_blur_false_is_todays_canvas_and_a_constant_field_is_unchanged(cuda):
    from toad_amd import ops
    from toad_amd.heatmap import attention_canvas
    s, origins, scores, cells = e2e_case()
    region, sd = dev(s, cuda), dev(scores, cuda)
    lat = dict(tile=TILE, stride=STRIDE)
    called = []
    real = ops.heat_cells_blur
    ops.heat_cells_blur = lambda *a, **kw: called.append(a) or real(*a, **kw)
    try:
        for down in (1, 4, 8, 32):
            for smooth in (False, True):
                base = attention_canvas(region, origins, sd, down=down, smooth=smooth, **lat)
                assert same_px(base, heat_px_ref.canvas(s, cells, CELL, heat_ref.jet(), 102, down, smooth=smooth))
                assert torch.equal(attention_canvas(region, origins, sd, down=down, smooth=smooth, blur=False, **lat), base)
                assert torch.equal(attention_canvas(region, origins, sd, down=down, smooth=smooth, blur=None, **lat), base)
                assert not called                                    # no blur launch without the keyword
                # binarize gives every present tile the same score: a constant field, which the blur reproduces exactly
                flat = attention_canvas(region, origins, sd, down=down, smooth=smooth, binarize=True, **lat)
                for b in (True, 20.0, E2E_TAPS):
                    assert torch.equal(attention_canvas(region, origins, sd, down=down, smooth=smooth, binarize=True, blur=b, **lat), flat), (down, smooth, b)
                assert len(called) == 3
                del called[:]
        # thresh acts before the blur: the tiles below it carry no weight
        q = heat_px_ref.select(scores, heat_ref.quantise(scores), thresh=0.5)
        t = heat_ref.table(origins[q >= 0], q[q >= 0], (TILE, TILE), (STRIDE, STRIDE), (0, 0), (9, 5))
        kept = heat_ref.cells(t, CELL, (TILE, TILE), (STRIDE, STRIDE), (0, 0), (HR, WR))
        want = heat_px_ref.canvas(s, ref.blur(kept, E2E_TAPS), CELL, heat_ref.jet(), 102, 1)
        assert same_px(attention_canvas(region, origins, sd, thresh=0.5, blur=E2E_TAPS, **lat), want)
        # empty origins: the box-filtered region, and no blur launch
        del called[:]
        none = attention_canvas(region, np.zeros((0, 2), dtype=np.int64), sd[:0], down=4, blur=True, **lat)
        assert same_px(none, heat_ref.box(s, 4).astype(np.uint8)) and not called
    finally:
        ops.heat_cells_blur = real


@pytest.mark.gpu
def test_region_tissue_attention_heatmap_with_blur(cuda):
    """The synthetic slide of test_gpu_heatmap.py through the pipeline call, on square 8 x 8 tiles (blur=True is CLAM's width and needs a square tile):
    cell 8, sigma = 5.3 / 8 cells, and a table of 5 x 138 cells - three workgroup tiles wide."""
    from toad_amd.eval import region_tissue_attention_heatmap
    from toad_amd.heatmap import gaussian_taps
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    s = tissue_ref.slide(40, 1100, 1)
    region = dev(s, cuda)
    kept, total = tissue_ref.selection(s, (8, 8), (8, 8), (0, 0), 0.25, 8, 0)
    assert total == 5 * 137 and 0 < len(kept) < total
    o0, s0, plain = region_tissue_attention_heatmap(extractor, mil, region, tile=8)
    origins, scores, canvas = region_tissue_attention_heatmap(extractor, mil, region, tile=8, blur=True)
    assert np.array_equal(origins, kept) and np.array_equal(o0, kept) and torch.equal(scores, s0)
    q = heat_ref.quantise(scores.cpu().numpy())
    cells = heat_ref.cells(heat_ref.table(origins, q, (8, 8), (8, 8), (0, 0), (137, 5)), 8, (8, 8), (8, 8), (0, 0), (40, 1100))
    taps = gaussian_taps(5.3 / 8)
    assert cells.shape == (5, 138) and len(taps) == 3
    assert same_px(plain, heat_px_ref.canvas(s, cells, 8, heat_ref.jet(), 102, 1))
    assert same_px(canvas, heat_px_ref.canvas(s, ref.blur(cells, taps), 8, heat_ref.jet(), 102, 1))
    assert not torch.equal(canvas, plain)
