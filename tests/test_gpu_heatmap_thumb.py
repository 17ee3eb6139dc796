"""GPU: the overview heat-map canvas (csrc/heatmap.hip heat_thumb_kernel<DOWN>, toad_region_heat_thumb_u8; ops.region_heat_thumb; down = 8, 16, 32 of
toad_amd/heatmap.py and eval.region_tissue_attention_heatmap). The canvas is defined in integers, so every comparison is == on whole arrays: against the
numpy reference of tests/heat_px_ref.py, which states the per-pixel definition for any down (checked at the new values by hand in
test_heatmap_thumb_host.py), and against the down = 4 canvas of the existing kernel where the two must agree."""
import numpy as np
import pytest
import torch

from tests import heat_px_ref as ref
from tests import heat_ref
from tests import tissue_ref
from tests import tissue_seg_ref
from tests.test_gpu_heatmap import dev, embedded, odd_pads, random_case, same_px
from tests.test_gpu_heatmap_px import random_mask

DOWNS = (8, 16, 32)
CELLS = (8, 16, 32, 64)
# (7, 5): empty at every down. (8, 8): one box. (31, 33): partial boxes dropped on both axes. (64, 64): whole strips. (67, 131) / (131, 67): the partial last
# cell, edge lanes, more than one 16-row strip. (203, 333): two 256-pixel chunks, seven 32-row strips. (300, 520): three chunks, the last 8 pixels wide.
SHAPES = [(7, 5), (8, 8), (31, 33), (64, 64), (67, 131), (131, 67), (203, 333), (300, 520)]


def pairs():
    """Every (down, cell) the entry point takes."""
    return [(d, c) for d in DOWNS for c in CELLS if c >= d]


# ---- 1. shapes and edges, against the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr", SHAPES)
def test_thumb_canvas_shapes_and_edges(cuda, hr, wr):
    """Every down with every cell >= down on the ramp / hole / checker / border tables, smooth x mask in all four combinations, alpha 102, 0 and 256. The mask
    is a random 0 / 255 plane of down-sized boxes: one byte per canvas pixel."""
    from toad_amd import ops
    px, _, lut = random_case(hr, wr, 8, 1000 * hr + wr)
    region, lut_d = dev(px, cuda), dev(lut, cuda)
    for down, cell in pairs():
        m = random_mask(hr, wr, down, hr + wr + down)
        m_d = dev(m, cuda)
        for name, tab in ref.tables(-(-hr // cell), -(-wr // cell), cell + down).items():
            cells = dev(tab, cuda, torch.int32)
            for smooth in (False, True):
                for mask in (None, m):
                    kw = dict(mask=mask, mask_down=down, mask_thresh=0) if mask is not None else {}
                    kd = dict(kw, mask=m_d) if mask is not None else {}
                    for alpha in (102, 0, 256):
                        want = ref.canvas(px, tab, cell, lut, alpha, down, smooth=smooth, **kw)
                        got = ops.region_heat_thumb(region, cells, cell, lut_d, alpha, down, smooth=smooth, **kd)
                        assert want.shape == (hr // down, wr // down, 3) and same_px(got, want), (down, cell, name, smooth, mask is not None, alpha)
    if (hr, wr) == (7, 5):
        assert ops.region_heat_thumb(region, cells, cell, lut_d, 102, 8).shape == (0, 0, 3)            # empty: nothing is launched
    if (hr, wr) == (300, 520):                                     # values above 255 read as 255, also as tent neighbours
        over = ref.tables(-(-hr // 16), -(-wr // 16), 7)["checker"] * 3
        assert over.max() > 255
        assert same_px(ops.region_heat_thumb(region, dev(over, cuda, torch.int32), 16, lut_d, 200, 8, smooth=True), ref.canvas(px, over, 16, lut, 200, 8, smooth=True))


# ---- 2. the mask ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_every_mask_box_size_against_the_reference(cuda, down):
    """Every legal (mask_down, down) pair - mask_down in down .. 32 - on extents that are no multiples of mask_down: the dropped strip must come out
    unblended. A random 0 / 255 plane, and a grey plane at thresholds 0, 8 and 254."""
    from toad_amd import ops
    for hr, wr, cell in ((203, 333, max(down, 16)), (131, 67, 64), (70, 301, down)):
        px, idx, lut = random_case(hr, wr, cell, 17 * hr + wr + cell)
        idx[idx < 0] = 5                                            # everything covered: only the mask decides
        region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
        plain = heat_ref.box(px, down).astype(np.uint8)
        for md in [m for m in DOWNS if m % down == 0]:
            assert hr % md and wr % md
            dropped_y, dropped_x = (hr // md) * md // down, (wr // md) * md // down              # canvas rows / columns past the plane
            for grey, thresholds in ((False, (0,)), (True, (0, 8, 254))):
                m = random_mask(hr, wr, md, hr + md, grey)
                m_d = dev(m, cuda)
                for t in thresholds:
                    for smooth in (False, True) if t in (0, 8) else (False,):
                        want = ref.canvas(px, idx, cell, lut, 128, down, smooth=smooth, mask=m, mask_down=md, mask_thresh=t)
                        got = ops.region_heat_thumb(region, cells, cell, lut_d, 128, down, smooth=smooth, mask=m_d, mask_down=md, mask_thresh=t)
                        assert same_px(got, want), (hr, wr, md, grey, t, smooth)
                    assert np.array_equal(want[dropped_y:], plain[dropped_y:]) and np.array_equal(want[:, dropped_x:], plain[:, dropped_x:])
                    inside = (want != plain).any(axis=2)[:dropped_y, :dropped_x]
                    assert inside.any() == bool((m > t).any()) and (not inside.all()) == bool((m <= t).any()), (hr, wr, md, grey, t)


# ---- 3. pitch, base and surroundings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr,inner,corner", [(67, 131, (2, 3, 1, 5), (1, 4, 0, 0)), (300, 520, (2, 3, 1, 6), (2, 5, 0, 0))])
def test_thumb_pitched_region_canvas_and_mask_views(cuda, hr, wr, inner, corner):
    """As test_px_pitched_region_canvas_and_mask_views: the region inside a parent of another colour, then in its last rows, so that the view ends where the
    allocation ends; the canvas, pre-filled with 0x7f, and the mask as odd-pitch, odd-base windows of sentinel-filled parents - the canvas parent untouched
    outside the view, the mask read nowhere outside its window (its surroundings would be tissue)."""
    from toad_amd import ops
    for cell, md in ((8, 8), (32, 16), (64, 32)):
        px, idx, lut = random_case(hr, wr, cell, 7 * hr + wr + cell + md)
        px = (px >> 1).astype(np.uint8)                           # pixels below 128, the surroundings 255
        cells, lut_d = dev(idx, cuda, torch.int32), dev(lut, cuda)
        m = random_mask(hr, wr, md, 3 * hr + md, True)
        downs = [d for d in DOWNS if md % d == 0 and d <= cell]
        wants = {d: ref.canvas(px, idx, cell, lut, 102, d, smooth=True, mask=m, mask_down=md, mask_thresh=8) for d in downs}
        mviews = []
        for top, left, bottom, right in (odd_pads(m.shape[1], *inner), odd_pads(m.shape[1], *corner)):
            parent = torch.full((m.shape[0] + top + bottom, m.shape[1] + left + right), 255, dtype=torch.uint8, device=cuda)
            mv = parent[top:top + m.shape[0], left:left + m.shape[1]]
            mv.copy_(torch.from_numpy(m.copy()))
            assert mv.stride(0) % 2 == 1 and mv.data_ptr() % 2 == 1 and not mv.is_contiguous()
            mviews.append(mv)
        for (top, left, bottom, right), mv in zip((inner, corner), mviews):
            _, v = embedded(px, top, left, bottom, right, 255, cuda)
            assert v.stride(0) % 2 == 1 and v.data_ptr() % 2 == 1
            if (bottom, right) == (0, 0):
                assert v.storage_offset() + (hr - 1) * v.stride(0) + 3 * wr == v.untyped_storage().nbytes()
            for d in downs:
                got = ops.region_heat_thumb(v, cells, cell, lut_d, 102, d, smooth=True, mask=mv, mask_down=md, mask_thresh=8)
                assert same_px(got, wants[d]), (cell, md, top, left, d)
        region = dev(px, cuda)
        for d in downs:
            want = wants[d]
            for pads in (odd_pads(want.shape[1], *inner), odd_pads(want.shape[1], *corner)):
                parent, view = embedded(np.full_like(want, 0x7F), *pads, 0x7F, cuda)
                assert view.stride(0) % 2 == 1 and view.data_ptr() % 2 == 1
                assert ops.region_heat_thumb(region, cells, cell, lut_d, 102, d, smooth=True, mask=mviews[0], mask_down=md, mask_thresh=8, out=view) is view
                assert same_px(view, want), (cell, md, pads, d)
                view.fill_(0x7F)
                assert bool((parent == 0x7F).all()), (cell, md, pads, d)      # nothing outside the view was written
        with pytest.raises(ValueError, match="share storage"):
            ops.region_heat_thumb(v, cells, cell, lut_d, 102, 8, smooth=True, out=v[:hr // 8, :wr // 8])      # a canvas-sized window of the region itself


# ---- 4. against the existing kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_flat_colour_equals_the_down_4_canvas_subsampled(cuda, down):
    """With every cell covered and alpha = 256 a canvas pixel is its cell's colour, whatever the box: the overview canvas is the down = 4 canvas of
    ops.region_heat_blend at every (down / 4)-th pixel, cropped to Ho x Wo. And where cell == down the tent is the own value: smooth changes nothing."""
    from toad_amd import ops
    for hr, wr in ((67, 131), (300, 520)):
        for cell in [c for c in CELLS if c >= down]:
            px, idx, lut = random_case(hr, wr, cell, 31 * hr + wr + cell)
            idx[idx < 0] = 200
            region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
            got = ops.region_heat_thumb(region, cells, cell, lut_d, 256, down)
            four = ops.region_heat_blend(region, cells, cell, lut_d, 256, 4)
            assert torch.equal(got, four[::down // 4, ::down // 4][:hr // down, :wr // down]), (hr, wr, cell)
            assert got.shape == (hr // down, wr // down, 3) and len(got.unique()) > 2
    for hr, wr in ((67, 131), (203, 333)):
        px, idx, lut = random_case(hr, wr, down, 5 * hr + wr + down)      # absent cells among them
        region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
        flat = ops.region_heat_thumb(region, cells, down, lut_d, 102, down)
        assert torch.equal(ops.region_heat_thumb(region, cells, down, lut_d, 102, down, smooth=True), flat)
        assert same_px(flat, ref.canvas(px, idx, down, lut, 102, down))
        _, idx2, _ = random_case(hr, wr, 64, 5 * hr + wr)              # a coarser table: there the tent is not the flat index in disguise
        c2 = dev(idx2, cuda, torch.int32)
        assert not torch.equal(ops.region_heat_thumb(region, c2, 64, lut_d, 102, down, smooth=True), ops.region_heat_thumb(region, c2, 64, lut_d, 102, down))


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_attention_canvas_at_overview_scale_equals_the_reference(cuda):
    """Lattice case 0 (64 x 64 tiles at stride 32 on 300 x 520: cell 32) at down = 8, 16 and 32 against the reference chain tile table -> cells -> canvas;
    down = 4 on the same case still gives today's canvas through today's call."""
    from toad_amd import ops
    from toad_amd.heatmap import attention_canvas
    (hr, wr), tile, stride, origin, cell = heat_ref.LATTICES[0]
    s, origins, _, _, n = heat_ref.case(0)
    region = dev(s, cuda)
    rng = np.random.default_rng(61)
    scores = rng.random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[2], scores[-1] = 0.0, 1.0, np.nan, 0.5
    sd = dev(scores, cuda)
    lat = dict(tile=tile, stride=stride, origin=origin)
    md = 16
    m = random_mask(hr, wr, md, 91, True)
    mask = (dev(m, cuda), 100, md)

    def want(down, smooth=False, masked=False, thresh=None, binarize=False):
        q = ref.select(scores, heat_ref.quantise(scores), thresh, binarize)
        t = heat_ref.table(origins[q >= 0], q[q >= 0], tile, stride, origin, n)
        cells = heat_ref.cells(t, cell, tile, stride, origin, (hr, wr))
        kw = dict(mask=m, mask_down=md, mask_thresh=100) if masked else {}
        return ref.canvas(s, cells, cell, heat_ref.jet(), 102, down, smooth=smooth, **kw)

    for down in (8, 16):
        assert same_px(attention_canvas(region, origins, sd, down=down, **lat), want(down)), down
        assert same_px(attention_canvas(region, origins, sd, down=down, smooth=True, **lat), want(down, smooth=True)), down
        assert same_px(attention_canvas(region, origins, sd, down=down, mask=mask, **lat), want(down, masked=True)), down
        got = attention_canvas(region, origins, sd, down=down, smooth=True, mask=mask, thresh=0.5, binarize=True, **lat)
        assert same_px(got, want(down, True, True, 0.5, True)), down
        for other in (want(down, smooth=True), want(down, masked=True), want(down, thresh=0.5)):
            assert not np.array_equal(other, want(down))           # every keyword does something at this scale too
    assert same_px(attention_canvas(region, origins, sd, down=32, smooth=True, **lat), want(32, smooth=True))      # cell == down
    assert same_px(attention_canvas(region, np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device=cuda), down=16, **lat), heat_ref.box(s, 16).astype(np.uint8))
    out = torch.full((hr // 8, wr // 8, 3), 0x7F, dtype=torch.uint8, device=cuda)
    assert attention_canvas(region, origins, sd, down=8, out=out, **lat) is out and same_px(out, want(8))
    # one launch of the new call at 8, 16, 32; down = 1, 2, 4 take today's route
    called = []
    real_thumb, real_px = ops.region_heat_thumb, ops.region_heat_blend_px
    ops.region_heat_thumb = lambda *a, **kw: called.append("thumb") or real_thumb(*a, **kw)
    ops.region_heat_blend_px = lambda *a, **kw: called.append("px") or real_px(*a, **kw)
    try:
        four = attention_canvas(region, origins, sd, down=4, smooth=True, mask=mask, **lat)
        attention_canvas(region, origins, sd, down=8, **lat)
        assert called == ["px", "thumb"]
    finally:
        ops.region_heat_thumb, ops.region_heat_blend_px = real_thumb, real_px
    assert same_px(four, want(4, smooth=True, masked=True))
    with pytest.raises(ValueError, match="cell = 4"):               # lattice case 1: cell 4
        attention_canvas(region, np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device=cuda), tile=(64, 64), stride=(64, 64), origin=(8, 4), down=8)


@pytest.mark.gpu
def test_region_tissue_attention_heatmap_at_overview_scale(cuda):
    from toad_amd.eval import region_tissue_attention_heatmap
    from toad_amd.heatmap import attention_canvas
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import segmented_tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    key = (64, 1100, 1)                                            # the slide of the px test, tall enough for a tile of 4 * 16 rows (the rule of the
    s = tissue_ref.slide(*key)                                     # segmented selection at down = 16)
    region = dev(s, cuda)
    tile = stride = (64, 256)                                      # cell 64
    seg = dict(down=16, median=3)
    want_o, total, want_t = tissue_seg_ref.selection(s, tile, stride, (0, 0), 0.25, 16, 3, 8, key=key)
    assert total == 4 and 0 < len(want_o) < total and want_t == 8
    o_sel, (plane, t) = segmented_tissue_origins(region, tile=tile, stride=stride, return_mask=True, **seg)
    assert np.array_equal(o_sel, want_o) and t == 8 and tuple(plane.shape) == (4, 68)
    m = plane.cpu().numpy()
    assert np.array_equal(m, tissue_seg_ref.segmented(s, 16, 3, 8, key=key)[0])
    origins, scores, canvas = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=16, segment=seg, tissue_mask=True)
    assert np.array_equal(origins, want_o) and tuple(canvas.shape) == (4, 68, 3)
    assert torch.equal(canvas, attention_canvas(region, origins, scores, tile=tile, stride=stride, down=16, mask=(plane, t, 16)))
    q = heat_ref.quantise(scores.cpu().numpy())
    cells = heat_ref.cells(heat_ref.table(origins, q, tile, stride, (0, 0), (4, 1)), 64, tile, stride, (0, 0), (64, 1100))
    assert same_px(canvas, ref.canvas(s, cells, 64, heat_ref.jet(), 102, 16, mask=m, mask_down=16, mask_thresh=t))
    plain = heat_ref.box(s, 16).astype(np.uint8)
    changed = (canvas.cpu().numpy() != plain).any(axis=2)
    assert changed.any() and not changed[~(m > t)].any()            # no pixel outside the returned mask is coloured
    unmasked = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=16, segment=seg)[2]
    assert not torch.equal(unmasked, canvas)                        # the glass inside a selected tile is what the mask takes out
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=32, segment=seg, tissue_mask=True)
