"""GPU: several levels of the heat-map pyramid from one read of the window (heat_pyramid_kernel in csrc/heatmap.hip behind toad_region_heat_pyramid_u8;
ops.region_heat_pyramid, heatmap.window_pyramid / attention_pyramid, a sequence as ``down`` of eval.slide_attention_heatmap). Every level is defined
from the region's own box sums, so every comparison is == on whole arrays: each level against the per-pixel windowed reference of
tests/heat_window_ref.py AND against ops.region_heat_window called for that level alone."""
import numpy as np
import pytest
import torch

from tests import heat_ref
from tests import heat_window_ref as wref
from tests import tissue_ref
from tests.test_gpu_heatmap import dev, embedded, odd_pads, same_px
from tests.test_gpu_heatmap_px import random_mask
from tests.test_gpu_heatmap_window import table_with_large_values, windows

DOWNS = (1, 2, 4, 8, 16, 32)
CELLS = (4, 8, 16, 64)
ALPHAS = (102, 0, 256)
SETS = ((1, 2), (1, 2, 4), (8, 16, 32), (1, 4, 16), (2, 32), (4, 8), DOWNS)
GUARD = 0x7F


def legal_cells(ds):
    return [c for c in CELLS if max(ds) <= 4 or c >= max(ds)]


_CASES, _WANT = {}, {}


def case(hs, ws, cell):
    """(px, idx, lut) of one slide and cell, the same for every level set: the references below are computed once and shared."""
    if (hs, ws, cell) not in _CASES:
        _CASES[hs, ws, cell] = table_with_large_values(hs, ws, cell, 17 * hs + ws + cell)
    return _CASES[hs, ws, cell]


def want_canvases(hs, ws, cell, win, down, smooth, md):
    """{alpha: canvas} of the windowed reference for one level, cached: read-only."""
    key = (hs, ws, cell, win, down, smooth, md)
    if key not in _WANT:
        px, idx, lut = case(hs, ws, cell)
        wx, wy, w, h = win
        kw = {} if md is None else dict(mask=random_mask(hs, ws, md, hs + md + cell, True), mask_down=md, mask_thresh=8)
        _WANT[key] = wref.canvases(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, ALPHAS, down, smooth, **kw)
    return _WANT[key]


# ---- 1. every level against the reference and against the per-level call ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", SETS, ids=lambda ds: "-".join(map(str, ds)))
def test_every_level_equals_the_windowed_reference(cuda, ds):
    """Every legal cell on the 67 x 131 slide (the whole slide among the windows) and the smallest and the largest on 300 x 520; smooth off and on (on at
    cell 4 is refused); no mask and the slide's plane at every legal mask_down, grey values around the threshold; alpha 102, 0 and 256; table values above
    255. The regions are views into the slide tensor."""
    from toad_amd import ops
    top = max(ds)
    cells_of = {(67, 131): legal_cells(ds), (300, 520): sorted({legal_cells(ds)[0], legal_cells(ds)[-1]})}
    mds = [m for m in DOWNS if m % top == 0]
    checked = 0
    for (hs, ws), cells in cells_of.items():
        for cell in cells:
            px, idx, lut = case(hs, ws, cell)
            slide, cells_d, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
            wins = windows(hs, ws, top, whole=hs == 67)
            for md in [None] + mds:
                kd = {} if md is None else dict(mask=dev(random_mask(hs, ws, md, hs + md + cell, True), cuda), mask_down=md, mask_thresh=8)
                some = wins if md is None else wins[-2:]             # with a plane: the edge window and the small one
                for win in some:
                    wx, wy, w, h = win
                    region = slide[wy:wy + h, wx:wx + w]
                    for smooth in (False, True):
                        if smooth and cell == 4:
                            with pytest.raises(ValueError, match="smooth at cell = 4"):
                                ops.region_heat_pyramid(region, (wx, wy), cells_d, cell, lut_d, 102, ds, smooth=True, **kd)
                            continue
                        for alpha in ALPHAS:
                            got = ops.region_heat_pyramid(region, (wx, wy), cells_d, cell, lut_d, alpha, ds, smooth=smooth, **kd)
                            assert isinstance(got, tuple) and len(got) == len(ds)
                            for d, g in zip(ds, got):
                                want = want_canvases(hs, ws, cell, win, d, smooth, md)[alpha]
                                assert want.shape == (h // d, w // d, 3) and same_px(g, want), (hs, ws, cell, md, win, smooth, alpha, d)
                                assert torch.equal(g, ops.region_heat_window(region, (wx, wy), cells_d, cell, lut_d, alpha, d, smooth=smooth, **kd)), (cell, md, win, smooth, alpha, d)
                                checked += 1
    assert checked >= 120                                            # 8 windows x 3 alphas x 2 levels x (smooth off and on at one cell) without any plane


# ---- 2. every level keeps its own extent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_levels_keep_their_own_extents(cuda):
    from toad_amd import ops
    hs, ws, cell = 300, 520, 64
    px, idx, lut = case(hs, ws, cell)
    slide, cells_d, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
    m = random_mask(hs, ws, 32, 77, True)
    kw, kd = dict(mask=m, mask_down=32, mask_thresh=8), dict(mask=dev(m, cuda), mask_down=32, mask_thresh=8)
    # 69 x 295 at D = 32: level 1 has all 69 rows and 295 columns, level 32 has 2 rows of 9
    wx, wy, w, h = 32, 64, 295, 69
    region = slide[wy:wy + h, wx:wx + w]
    got = ops.region_heat_pyramid(region, (wx, wy), cells_d, cell, lut_d, 102, DOWNS, smooth=True, **kd)
    assert [tuple(g.shape) for g in got] == [(h // d, w // d, 3) for d in DOWNS] and tuple(got[0].shape) == (69, 295, 3) and tuple(got[5].shape) == (2, 9, 3)
    for d, g in zip(DOWNS, got):
        assert same_px(g, wref.canvas(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, 102, d, True, **kw)), d
    # D - 1 = 31 rows: the coarse level is empty and unwritten, the fine ones are complete
    h = 31
    region = slide[wy:wy + h, wx:wx + w]
    parent = torch.full((3, w // 32, 3), GUARD, dtype=torch.uint8, device=cuda)
    outs = [torch.full((h // d, w // d, 3), GUARD, dtype=torch.uint8, device=cuda) for d in (1, 4)] + [parent[1:1]]
    got = ops.region_heat_pyramid(region, (wx, wy), cells_d, cell, lut_d, 102, (1, 4, 32), outs=outs)
    assert all(g is o for g, o in zip(got, outs)) and tuple(got[2].shape) == (0, 9, 3) and bool((parent == GUARD).all())
    for d, g in zip((1, 4), got):
        assert same_px(g, wref.canvas(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, 102, d)), d
    # every level empty: tensors of the right shapes, nothing launched
    got = ops.region_heat_pyramid(slide[wy:wy + 1, wx:wx + w], (wx, wy), cells_d, cell, lut_d, 102, (2, 4, 32))
    assert [tuple(g.shape) for g in got] == [(0, w // 2, 3), (0, w // 4, 3), (0, w // 32, 3)]
    got = ops.region_heat_pyramid(slide[wy:wy + 40, wx:wx + 3], (wx, wy), cells_d, cell, lut_d, 102, (4, 8))
    assert [tuple(g.shape) for g in got] == [(10, 0, 3), (5, 0, 3)]


# ---- 3. odd parents and guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", ((1, 4, 16), (8, 16, 32), DOWNS, (1, 2)), ids=lambda ds: "-".join(map(str, ds)))
def test_pyramid_inside_odd_parents_writes_only_its_rows_and_columns(cuda, ds):
    """The slide inside a parent of another colour padded by odd byte counts, and each level's canvas written into its rows and columns of a guard-filled
    parent at an odd base and pitch: every level equals the reference, every parent keeps its guard outside the view, the region's parent is unchanged."""
    from toad_amd import ops
    hs, ws, top = 300, 520, max(ds)
    cell, md = max(legal_cells(ds)[0], 8), 32 if top == 32 else 2 * top
    px, idx, lut = case(hs, ws, cell)
    px = (px >> 1).astype(np.uint8)                               # pixels below 128, the surroundings 255
    sparent, slide = embedded(px, *odd_pads(ws, 2, 3, 1, 6), 255, cuda)
    assert slide.stride(0) % 2 == 1 and slide.data_ptr() % 2 == 1
    before = sparent.clone()
    m = random_mask(hs, ws, md, 3 * hs + md, True)
    cells_d, lut_d, mask_d = dev(idx, cuda, torch.int32), dev(lut, cuda), dev(m, cuda)
    parents, views = zip(*(embedded(np.full((hs // d, ws // d, 3), GUARD, dtype=np.uint8), *odd_pads(ws // d, 2, 3, 1, 6), GUARD, cuda) for d in ds))
    assert all(v.stride(0) % 2 == 1 and v.data_ptr() % 2 == 1 for v in views)
    for wx, wy, w, h in windows(hs, ws, top, False):
        outs = [v[wy // d:wy // d + h // d, wx // d:wx // d + w // d] for d, v in zip(ds, views)]
        got = ops.region_heat_pyramid(slide[wy:wy + h, wx:wx + w], (wx, wy), cells_d, cell, lut_d, 102, ds, smooth=True, mask=mask_d, mask_down=md, mask_thresh=8,
                                      outs=outs)
        for d, g, out, parent in zip(ds, got, outs, parents):
            want = wref.canvas(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, 102, d, True, m, md, 8)
            assert g is out and same_px(out, want), (wx, wy, w, h, d)
            assert want.size == 0 or bool((out != GUARD).any())
            out.fill_(GUARD)
            assert bool((parent == GUARD).all()), (wx, wy, w, h, d)   # nothing outside the window's rows and columns of this level was written
    assert torch.equal(sparent, before)


# ---- 4. no seams, at every level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_strips_and_blocks_assemble_to_every_levels_whole_slide_canvas(cuda):
    """Lattice case 0 (64 x 64 tiles at stride 32 on 300 x 520: cell 32), levels (1, 4, 16): three uneven strips and a 2 x 3 grid of blocks rendered with
    window_pyramid into views of per-level slide canvases; each level equals attention_canvas of the whole slide - flat, tent + mask, blur. Seams at
    multiples of 16, inside cells and tiles."""
    from toad_amd.heatmap import attention_canvas, slide_cells, window_pyramid
    ds = (1, 4, 16)
    (hs, ws), tile, stride, origin, cell = heat_ref.LATTICES[0]
    s, origins, _, _, _ = heat_ref.case(0)
    slide = dev(s, cuda)
    scores = np.random.default_rng(61).random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[2] = 0.0, 1.0, np.nan
    sd = dev(scores, cuda)
    lat = dict(tile=tile, stride=stride, origin=origin)
    mask = (dev(random_mask(hs, ws, 16, 91, True), cuda), 100, 16)
    ys, xs, row = (0, 112, 240, hs), (0, 176, 336, ws), (0, 144, hs)
    assert all(v % 16 == 0 and v % cell for v in ys[1:-1] + xs[1:-1] + row[1:-1])
    strips = [(0, y0, ws, y1 - y0) for y0, y1 in zip(ys, ys[1:])]
    blocks = [(x0, y0, x1 - x0, y1 - y0) for y0, y1 in zip(row, row[1:]) for x0, x1 in zip(xs, xs[1:])]
    for name, kw, blur in (("flat", {}, False), ("both", dict(smooth=True, mask=mask), False), ("blur", dict(smooth=True), True)):
        wholes = [attention_canvas(slide, origins, sd, down=d, blur=blur, **kw, **lat) for d in ds]
        cells, c = slide_cells((hs, ws), origins, sd, blur=blur, **lat)
        assert c == cell
        for pieces in (strips, blocks):
            canvases = [torch.full((hs // d, ws // d, 3), GUARD, dtype=torch.uint8, device=cuda) for d in ds]
            for wx, wy, w, h in pieces:
                outs = [cv[wy // d:wy // d + h // d, wx // d:wx // d + w // d] for d, cv in zip(ds, canvases)]
                got = window_pyramid(slide[wy:wy + h, wx:wx + w], (wx, wy), cells, cell, downs=ds, outs=outs, **kw)
                assert all(g is o for g, o in zip(got, outs))
            for d, cv, whole in zip(ds, canvases, wholes):
                assert torch.equal(cv, whole), (name, d, len(pieces))


# ---- 5. the whole walk ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slide_attention_heatmap_renders_every_level_in_one_walk(cuda):
    """The 256 x 1100 slide of the window tests as 3 overlapping strips (seams at 112 and 208), tiles of 64 x 256 (cell 64): down = (1, 4, 16) gives, per
    level, the canvas of the same call with that int down; attention_pyramid gives attention_canvas per level."""
    from toad_amd.eval import slide_attention_heatmap
    from toad_amd.heatmap import attention_canvas, attention_pyramid
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    hs, ws, ds = 256, 1100, (1, 4, 16)
    slide = dev(tissue_ref.slide(hs, ws, 1), cuda)
    tile = stride = (64, 256)
    strips = [(slide[y:y + n], y) for y, n in ((0, 112), (64, 144), (176, 80))]
    kw = dict(tile=tile, stride=stride, smooth=True, blur=96.0)
    origins, scores, canvases = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=ds, **kw)
    assert isinstance(canvases, dict) and tuple(canvases) == ds and 4 < len(origins) < 16
    for d in ds:
        o1, s1, c1 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=d, **kw)
        assert np.array_equal(o1, origins) and torch.equal(s1, scores)
        assert tuple(canvases[d].shape) == (hs // d, ws // d, 3) and torch.equal(canvases[d], c1), d
    out = {d: torch.full((hs // d, ws // d, 3), GUARD, dtype=torch.uint8, device=cuda) for d in ds}
    _, _, c2 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=ds, origins=origins, out=out, **kw)
    assert all(c2[d] is out[d] and torch.equal(out[d], canvases[d]) for d in ds)
    got = attention_pyramid(slide, origins, scores, downs=ds, **kw)
    for d, g in zip(ds, got):
        assert torch.equal(g, attention_canvas(slide, origins, scores, down=d, **kw)), d
