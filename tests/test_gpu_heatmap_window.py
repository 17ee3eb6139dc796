"""GPU: heat maps rendered window by window (csrc/heatmap.hip behind toad_region_heat_window_u8; ops.region_heat_window, heatmap.slide_cells /
window_canvas / strip_plan, eval.slide_attention_heatmap). The canvas is defined in integers, so every comparison is == on whole arrays: windows against
the per-pixel windowed reference of tests/heat_window_ref.py (checked against slices of the whole-image reference in test_heatmap_window_host.py), and
canvases put together from strips and blocks against the whole-slide canvas of the entry points that were there before."""
import numpy as np
import pytest
import torch

from tests import heat_ref
from tests import heat_window_ref as wref
from tests import tissue_ref
from tests.test_gpu_heatmap import dev, embedded, odd_pads, random_case, same_px
from tests.test_gpu_heatmap_px import random_mask

DOWNS = (1, 2, 4, 8, 16, 32)
CELLS = (4, 8, 16, 64)
ALPHAS = (102, 0, 256)


def legal_cells(down):
    return [c for c in CELLS if down <= 4 or c >= down]


def windows(hs, ws, down, whole):
    """(wx, wy, w, h): offsets that are multiples of max(4, down) and of no cell above it; a window wider than a 256-pixel chunk; one a lane (a box) wide;
    widths and heights that are no multiples of 4 or of down; one that ends at the slide's right and bottom edge, in the table's partial last cell."""
    step = max(4, down)
    al = lambda v: max(v, 0) // step * step                          # noqa: E731
    cand = [(step, 3 * step, 263 + down, 37 + down), (al(ws // 2) + step, al(hs // 3) + step, step, 21 + 2 * down),
            (al(ws - 75), al(hs - 50), ws, hs), (3 * step, step, 2 * step + 3, 3 * step + 1)]
    out = [(0, 0, ws, hs)] if whole else []
    for wx, wy, w, h in cand:
        if wx < ws and wy < hs:
            out.append((wx, wy, min(w, ws - wx), min(h, hs - wy)))
    return out


def table_with_large_values(hs, ws, cell, seed):
    px, idx, lut = random_case(hs, ws, cell, seed)
    idx = idx.copy()
    idx[idx > 250] = 300                                           # values above 255 read as 255, as own and as tent neighbours
    return px, idx, lut


# ---- 1. windows against the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_windows_equal_the_windowed_reference(cuda, down):
    """Every legal cell on the 67 x 131 slide (the whole slide as window (0, 0) among the windows) and the smallest and the largest on 300 x 520; smooth on
    and off; no mask and the slide's plane at every legal mask_down, grey values around the threshold; alpha 102, 0 and 256. The regions are views into the
    slide tensor: pitched rows, bases at any multiple of 12 bytes."""
    from toad_amd import ops
    cells_of = {(67, 131): legal_cells(down), (300, 520): sorted({legal_cells(down)[0], legal_cells(down)[-1]})}
    mds = [m for m in DOWNS if m % down == 0]
    checked = 0
    for (hs, ws), cells in cells_of.items():
        for cell in cells:
            px, idx, lut = table_with_large_values(hs, ws, cell, 13 * hs + ws + cell + down)
            slide, cells_d, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
            wins = windows(hs, ws, down, whole=hs == 67)
            for md in [None] + mds:
                m = None if md is None else random_mask(hs, ws, md, hs + md + cell, True)
                kw = {} if md is None else dict(mask=m, mask_down=md, mask_thresh=8)
                kd = {} if md is None else dict(kw, mask=dev(m, cuda))
                some = wins if md in (None, down, 32) else wins[-2:]      # the other box sizes: the edge window and the small one
                for wx, wy, w, h in some:
                    if (w, h) == (ws, hs) and md not in (None, down):
                        continue
                    region = slide[wy:wy + h, wx:wx + w]
                    for smooth in (False, True):
                        want = wref.canvases(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, ALPHAS, down, smooth, **kw)
                        for alpha in ALPHAS:
                            got = ops.region_heat_window(region, (wx, wy), cells_d, cell, lut_d, alpha, down, smooth=smooth, **kd)
                            assert want[alpha].shape == (h // down, w // down, 3) and same_px(got, want[alpha]), (hs, ws, cell, md, (wx, wy, w, h), smooth, alpha)
                            checked += 1
    assert checked >= 90
    # a window with no canvas row launches nothing; a table larger than the slide is fine (the window only has to lie inside it)
    if down > 1:
        assert tuple(ops.region_heat_window(slide[:down - 1], (0, 0), cells_d, cell, lut_d, 102, down).shape) == (0, ws // down, 3)
    wide = torch.full((idx.shape[0] + 2, idx.shape[1] + 3), 77, dtype=torch.int32, device=cuda)
    wide[:idx.shape[0], :idx.shape[1]] = cells_d
    wx, wy, w, h = windows(hs, ws, down, False)[0]
    want = wref.canvas(px[wy:wy + h, wx:wx + w], (wx, wy), wide.cpu().numpy(), cell, lut, 102, down, True)
    assert same_px(ops.region_heat_window(slide[wy:wy + h, wx:wx + w], (wx, wy), wide, cell, lut_d, 102, down, smooth=True), want)


# ---- 2. odd parents and guard bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_windows_inside_odd_parents_write_only_their_rows_and_columns(cuda, down):
    """The slide inside a parent of another colour padded by odd byte counts, the plane likewise (its surroundings would be tissue), and each window's
    canvas written into its rows and columns of ONE sentinel-filled canvas parent at an odd base and pitch: every window equals the reference, and after
    each call the parent is unchanged outside that window's rows and columns."""
    from toad_amd import ops
    hs, ws = 300, 520
    cell, md = max(legal_cells(down)[0], 8), 32 if down == 32 else 2 * down
    px, idx, lut = table_with_large_values(hs, ws, cell, 5 * hs + ws + down)
    px = (px >> 1).astype(np.uint8)                               # pixels below 128, the surroundings 255
    _, slide = embedded(px, *odd_pads(ws, 2, 3, 1, 6), 255, cuda)
    assert slide.stride(0) % 2 == 1 and slide.data_ptr() % 2 == 1
    m = random_mask(hs, ws, md, 3 * hs + md, True)
    top, left, bottom, right = odd_pads(m.shape[1], 2, 3, 1, 5)
    mparent = torch.full((m.shape[0] + top + bottom, m.shape[1] + left + right), 255, dtype=torch.uint8, device=cuda)
    mview = mparent[top:top + m.shape[0], left:left + m.shape[1]]
    mview.copy_(torch.from_numpy(m.copy()))
    assert mview.stride(0) % 2 == 1 and mview.data_ptr() % 2 == 1
    cells_d, lut_d = dev(idx, cuda, torch.int32), dev(lut, cuda)
    ho, wo = hs // down, ws // down
    parent, view = embedded(np.full((ho, wo, 3), 0x7F, dtype=np.uint8), *odd_pads(wo, 2, 3, 1, 6), 0x7F, cuda)
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 2 == 1
    for wx, wy, w, h in windows(hs, ws, down, False):
        want = wref.canvas(px[wy:wy + h, wx:wx + w], (wx, wy), idx, cell, lut, 102, down, True, m, md, 8)
        out = view[wy // down:wy // down + h // down, wx // down:wx // down + w // down]
        got = ops.region_heat_window(slide[wy:wy + h, wx:wx + w], (wx, wy), cells_d, cell, lut_d, 102, down, smooth=True, mask=mview, mask_down=md, mask_thresh=8,
                                     out=out)
        assert got is out and same_px(out, want), (wx, wy, w, h)
        assert want.size == 0 or bool((out != 0x7F).any())
        out.fill_(0x7F)
        assert bool((parent == 0x7F).all()), (wx, wy, w, h)         # nothing outside the window's rows and columns was written


# ---- 3. no seams ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", (1, 4, 16))
def test_strips_and_blocks_assemble_to_the_whole_slide_canvas(cuda, down):
    """Lattice case 0 (64 x 64 tiles at stride 32 on 300 x 520: cell 32). The canvas put together from 3 uneven strips, and from a 2 x 3 grid of blocks, is the
    whole-slide canvas of attention_canvas - the entry points that were there before - flat, with the tent, with a mask, with both and with the blur. Every
    seam falls inside a cell and inside a tile. The same strips rendered one by one with attention_canvas do show seams under the tent."""
    from toad_amd.heatmap import attention_canvas, slide_cells, window_canvas
    (hs, ws), tile, stride, origin, cell = heat_ref.LATTICES[0]
    s, origins, _, _, _ = heat_ref.case(0)
    slide = dev(s, cuda)
    scores = np.random.default_rng(61).random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[2] = 0.0, 1.0, np.nan
    sd = dev(scores, cuda)
    lat = dict(tile=tile, stride=stride, origin=origin)
    mask = (dev(random_mask(hs, ws, 16, 91, True), cuda), 100, 16)
    ys, xs = ((0, 112, 240, hs), (0, 176, 336, ws)) if down == 16 else ((0, 100, 232, hs), (0, 172, 348, ws))
    row = (0, 144, hs) if down == 16 else (0, 148, hs)
    assert all(v % max(4, down) == 0 and v % cell for v in ys[1:-1] + xs[1:-1] + row[1:-1])
    strips = [(0, y0, ws, y1 - y0) for y0, y1 in zip(ys, ys[1:])]
    blocks = [(x0, y0, x1 - x0, y1 - y0) for y0, y1 in zip(row, row[1:]) for x0, x1 in zip(xs, xs[1:])]

    def assemble(pieces, cells, **kw):
        canvas = torch.full((hs // down, ws // down, 3), 0x7F, dtype=torch.uint8, device=cuda)
        for wx, wy, w, h in pieces:
            out = canvas[wy // down:wy // down + h // down, wx // down:wx // down + w // down]
            assert window_canvas(slide[wy:wy + h, wx:wx + w], (wx, wy), cells, cell, down=down, out=out, **kw) is out
        return canvas

    wholes = {}
    for name, kw, blur in (("flat", {}, False), ("smooth", dict(smooth=True), False), ("mask", dict(mask=mask), False),
                           ("both", dict(smooth=True, mask=mask), False), ("blur", dict(smooth=True), True)):
        whole = wholes[name] = attention_canvas(slide, origins, sd, down=down, blur=blur, **kw, **lat)
        cells, c = slide_cells((hs, ws), origins, sd, blur=blur, **lat)
        assert c == cell and tuple(cells.shape) == (-(-hs // cell), -(-ws // cell))
        assert torch.equal(assemble(strips, cells, **kw), whole), name
        assert torch.equal(assemble(blocks, cells, **kw), whole), name
    assert len({w.cpu().numpy().tobytes() for w in wholes.values()}) == 5      # every keyword does something on this slide
    # the guard: each strip as a region of its own - its whole tiles, its own lattice origin, today's call - does not give the slide's canvas under the tent
    alone = []
    for _, y0, _, h in strips:
        keep = (origins[:, 1] >= y0) & (origins[:, 1] + tile[0] <= y0 + h)
        local = (0, -(-y0 // stride[0]) * stride[0] - y0)
        alone.append(attention_canvas(slide[y0:y0 + h], origins[keep] - np.array([0, y0]), sd[torch.from_numpy(keep).to(cuda)], tile=tile, stride=stride,
                                      origin=local, down=down, smooth=True))
    assert not torch.equal(torch.cat(alone, dim=0), wholes["smooth"])


# ---- 4. the whole walk ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slide_attention_heatmap_over_overlapping_strips(cuda):
    """A 256 x 1100 synthetic slide as 3 overlapping strips, tiles of 64 x 256 (cell 64): the origins are those of tissue_origins on the whole slide, the
    scores those of ONE percentile ranking over the bag of the same per-strip extractor calls, the canvas that of attention_canvas on the whole slide."""
    from toad_amd.eval import attention_heatmap_scores, slide_attention_heatmap
    from toad_amd.heatmap import attention_canvas, strip_plan
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    hs, ws = 256, 1100
    s = tissue_ref.slide(hs, ws, 1)
    slide = dev(s, cuda)
    tile = stride = (64, 256)
    spans = [(0, 112), (64, 144), (176, 80)]                         # rows 0 .. 112, 64 .. 208, 176 .. 256: seams at 112 and 208, inside cells and tiles
    strips = [(slide[y:y + n], y) for y, n in spans]
    want_o = tissue_origins(slide, tile=tile, stride=stride)
    assert np.array_equal(want_o, tissue_ref.selection(s, tile, stride, (0, 0), 0.25, 8, 0)[0]) and 4 < len(want_o) < 16
    plan = strip_plan((hs, ws), spans, tile, stride, (0, 0), 16)
    assert [p["rows"] for p in plan] == [(0, 1), (1, 3), (3, 4)] and [p["render"] for p in plan] == [(0, 112), (112, 208), (208, 256)]
    bags = []
    for (region, y), p in zip(strips, plan):
        mine = want_o[(want_o[:, 1] // 64 >= p["rows"][0]) & (want_o[:, 1] // 64 < p["rows"][1])]
        assert len(mine)
        with torch.no_grad():
            bags.append(extractor.forward_u8_region(region, mine - np.array([0, y]), tile=tile, out_dtype=torch.float16))
    want_s = attention_heatmap_scores(mil, torch.cat(bags, dim=0), percentile=True)
    for down in (1, 16):
        kw = dict(tile=tile, stride=stride, down=down, smooth=True, blur=96.0)
        origins, scores, canvas = slide_attention_heatmap(extractor, mil, strips, (hs, ws), **kw)
        assert np.array_equal(origins, want_o) and origins.dtype == np.int64 and torch.equal(scores, want_s)
        want_c = attention_canvas(slide, origins, scores, **kw)
        assert tuple(canvas.shape) == (hs // down, ws // down, 3) and torch.equal(canvas, want_c)
        assert not torch.equal(want_c, attention_canvas(slide, origins, scores, tile=tile, stride=stride, down=down))      # the tent and the blur did something
    # the caller's selection, in slide coordinates, and the caller's canvas
    out = torch.full((hs // 16, ws // 16, 3), 0x7F, dtype=torch.uint8, device=cuda)
    o2, s2, c2 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), origins=want_o, out=out, **kw)
    assert np.array_equal(o2, want_o) and torch.equal(s2, want_s) and c2 is out and torch.equal(out, want_c)
    fewer = want_o[1::2]
    o3, s3, c3 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), origins=fewer, **kw)
    assert np.array_equal(o3, fewer) and len(s3) == len(fewer) and torch.equal(c3, attention_canvas(slide, fewer, s3, **kw))
    with pytest.raises(ValueError, match="off the lattice"):
        slide_attention_heatmap(None, None, strips, (hs, ws), origins=want_o + np.array([0, 4]), **kw)
    with pytest.raises(ValueError, match="lies whole in no strip"):
        slide_attention_heatmap(None, None, [strips[0], (slide[104:], 104)], (hs, ws), **kw)
    # a slide of glass: no tile, no extractor, no model - the box-filtered slide
    glass = torch.full((hs, ws, 3), 240, dtype=torch.uint8, device=cuda)
    o4, s4, c4 = slide_attention_heatmap(None, None, [(glass[y:y + n], y) for y, n in spans], (hs, ws), **kw)
    assert o4.shape == (0, 2) and s4.shape == (0,) and tuple(c4.shape) == (hs // 16, ws // 16, 3) and bool((c4 == 240).all())
