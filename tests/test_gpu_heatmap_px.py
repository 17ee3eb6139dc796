"""GPU: the per-pixel heat-map blend (csrc/heatmap.hip heat_blend_px_kernel<DOWN,SMOOTH,MASK>, toad_region_heat_blend_px_u8; the smooth / mask / thresh /
binarize keywords of toad_amd/heatmap.py; eval.region_tissue_attention_heatmap(tissue_mask=True)). The canvas is defined in integers, so every comparison
is == on whole arrays: against the flat call (ops.region_heat_blend, itself held to tests/heat_ref.py) where the two must agree, and against the numpy
reference of tests/heat_px_ref.py (tested on its own, by hand, in test_heatmap_px_host.py) everywhere else."""
import functools

import numpy as np
import pytest
import torch

from tests import heat_px_ref as ref
from tests import heat_ref
from tests import tissue_ref
from tests import tissue_seg_ref
from tests.test_gpu_heatmap import dev, embedded, odd_pads, random_case, same_px

DOWNS = (1, 2, 4)
MASK_DOWNS = (1, 2, 4, 8, 16, 32)
SHAPES = [(1, 1), (7, 5), (64, 64), (67, 131), (131, 67), (203, 333), (300, 520)]


@functools.lru_cache(maxsize=None)
def random_mask(hr, wr, mask_down, seed, grey=False):
    """uint8 [hr // mask_down, wr // mask_down]: a random 0 / 255 plane, or a grey one with 0, 8, 9, 254 and 255 among its values. Read-only, cached."""
    rng = np.random.default_rng(seed)
    shape = (hr // mask_down, wr // mask_down)
    m = rng.integers(0, 256, size=shape, dtype=np.uint8) if grey else (rng.integers(0, 2, size=shape) * 255).astype(np.uint8)
    if grey and m.size >= 5:
        m.reshape(-1)[:5] = (0, 8, 9, 254, 255)
    m.setflags(write=False)
    return m


# ---- 1. against the flat call ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_flat_index_and_full_mask_equal_todays_kernel(cuda, down):
    from toad_amd import ops
    for hr, wr in ((67, 131), (300, 520)):
        for cell in (4, 16, 64):
            px, idx, lut = random_case(hr, wr, cell, 31 * hr + wr + cell)
            region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
            for alpha in (102, 0, 256):
                flat = ops.region_heat_blend(region, cells, cell, lut_d, alpha, down)
                assert same_px(flat, heat_ref.canvas(px, idx, cell, lut, alpha, down)), (hr, wr, cell, alpha)      # both calls below launch flat's kernel
                assert torch.equal(ops.region_heat_blend_px(region, cells, cell, lut_d, alpha, down), flat), (hr, wr, cell, alpha)
                for md in [m for m in MASK_DOWNS if m % down == 0]:
                    full = torch.full((hr // md, wr // md), 255, dtype=torch.uint8, device=cuda)
                    got = ops.region_heat_blend_px(region, cells, cell, lut_d, alpha, down, mask=full, mask_down=md, mask_thresh=254)
                    if hr % md == 0 and wr % md == 0:
                        assert torch.equal(got, flat), (hr, wr, cell, alpha, md)
                    else:                                           # the strip the plane dropped is not tissue: the reference decides
                        assert same_px(got, ref.canvas(px, idx, cell, lut, alpha, down, mask=full.cpu().numpy(), mask_down=md, mask_thresh=254)), (cell, md)
            if down == 1:                                          # whole multiples of 32: every mask_down covers the region, all must equal today's canvas
                sub = region[:64, :128]
                sub_cells = cells[:-(-64 // cell), :-(-128 // cell)].contiguous()
                flat = ops.region_heat_blend(sub, sub_cells, cell, lut_d, 102, 1)
                for md in MASK_DOWNS:
                    full = torch.full((64 // md, 128 // md), 255, dtype=torch.uint8, device=cuda)
                    assert torch.equal(ops.region_heat_blend_px(sub, sub_cells, cell, lut_d, 102, 1, mask=full, mask_down=md), flat), (cell, md)


# ---- 2. against the reference: the tent ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 4])
def test_the_tent_equals_the_reference_on_the_lattice_cases(cuda, k):
    """Cells 32, 4, 8 and 16 on the slides of heat_ref.LATTICES, and a 64-cell table on case 0's slide; a 0..255 ramp, an interior absent cell, a checkerboard
    of absent cells and absent cells on the table's border, at every down."""
    from toad_amd import ops
    (hr, wr), _, _, _, cell = heat_ref.LATTICES[k]
    s = heat_ref.case(k)[0]
    region, lut = dev(s, cuda), heat_ref.jet()
    lut_d = dev(lut, cuda)
    for c in (cell, 64) if k == 0 else (cell,):
        for name, tab in ref.tables(-(-hr // c), -(-wr // c), 70 + k).items():
            cells = dev(tab, cuda, torch.int32)
            for down in DOWNS:
                want = ref.canvas(s, tab, c, lut, 102, down, smooth=True)
                got = ops.region_heat_blend_px(region, cells, c, lut_d, 102, down, smooth=True)
                assert same_px(got, want), (c, name, down)
                if c != down:                                       # the tent is not the flat index in disguise
                    assert not np.array_equal(want, heat_ref.canvas(s, tab, c, lut, 102, down)), (c, name, down)
    over = ref.tables(-(-hr // cell), -(-wr // cell), 70 + k)["checker"] * 3      # values above 255 read as 255
    assert over.max() > 255
    assert same_px(ops.region_heat_blend_px(region, dev(over, cuda, torch.int32), cell, lut_d, 200, 1, smooth=True), ref.canvas(s, over, cell, lut, 200, 1, smooth=True))


# ---- 3. shapes and edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr", SHAPES)
def test_px_canvas_shapes_and_edges(cuda, hr, wr):
    """The edge lanes, the partial last cell and the dropped partial boxes: tent, mask (an 8-box plane where 8 is legal, else a 4-box one) and both."""
    from toad_amd import ops
    for cell in (4, 8, 64):
        px, idx, lut = random_case(hr, wr, cell, 1000 * hr + wr + cell + 1)
        region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
        for down in DOWNS:
            md = 4 if cell == 8 else 8
            m = random_mask(hr, wr, md, hr + wr + md)
            m_d = dev(m, cuda)
            for smooth, mask in ((True, None), (False, m), (True, m)):
                kw = dict(mask=mask, mask_down=md, mask_thresh=0) if mask is not None else {}
                want = ref.canvas(px, idx, cell, lut, 102, down, smooth=smooth, **kw)
                if mask is not None:
                    kw["mask"] = m_d
                got = ops.region_heat_blend_px(region, cells, cell, lut_d, 102, down, smooth=smooth, **kw)
                assert want.shape == (hr // down, wr // down, 3) and same_px(got, want), (cell, down, smooth, mask is not None)
    if (hr, wr) == (1, 1):
        assert ops.region_heat_blend_px(region, cells, cell, lut_d, 102, 4, smooth=True).shape == (0, 0, 3)      # empty: nothing is launched
        none = torch.zeros((0, 0), dtype=torch.uint8, device=cuda)                                                # an empty plane: nothing is tissue
        assert same_px(ops.region_heat_blend_px(region, cells, cell, lut_d, 102, 1, mask=none, mask_down=2), px)


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_every_mask_box_size_against_the_reference(cuda, down):
    """Every legal (mask_down, down) pair, on extents that are no multiples of mask_down - the dropped strip must come out unblended - with a random 0 / 255
    plane and a grey plane at thresholds 0, 8 and 254."""
    from toad_amd import ops
    for hr, wr, cell in ((203, 333, 8), (131, 67, 4), (70, 301, 32)):
        px, idx, lut = random_case(hr, wr, cell, 17 * hr + wr + cell)
        idx[idx < 0] = 5                                            # everything covered: only the mask decides
        region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
        plain = heat_ref.box(px, down).astype(np.uint8)
        for md in [m for m in MASK_DOWNS if m % down == 0]:
            assert hr % md or wr % md or md == 1
            dropped_y, dropped_x = (hr // md) * md // down, (wr // md) * md // down              # canvas rows / columns past the plane
            for grey, thresholds in ((False, (0,)), (True, (0, 8, 254))):
                m = random_mask(hr, wr, md, hr + md, grey)
                m_d = dev(m, cuda)
                for t in thresholds:
                    for smooth in (False, True) if t in (0, 8) else (False,):
                        want = ref.canvas(px, idx, cell, lut, 128, down, smooth=smooth, mask=m, mask_down=md, mask_thresh=t)
                        got = ops.region_heat_blend_px(region, cells, cell, lut_d, 128, down, smooth=smooth, mask=m_d, mask_down=md, mask_thresh=t)
                        assert same_px(got, want), (hr, wr, md, grey, t, smooth)
                    assert np.array_equal(want[dropped_y:], plain[dropped_y:]) and np.array_equal(want[:, dropped_x:], plain[:, dropped_x:])
                    inside = (want != plain).any(axis=2)[:dropped_y, :dropped_x]
                    assert inside.any() == bool((m > t).any()) and (not inside.all()) == bool((m <= t).any()), (hr, wr, md, grey, t)


# ---- 5. pitch, base and surroundings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr,inner,corner", [(67, 131, (2, 3, 1, 5), (1, 4, 0, 0)), (300, 520, (2, 3, 1, 6), (2, 5, 0, 0))])
def test_px_pitched_region_canvas_and_mask_views(cuda, hr, wr, inner, corner):
    """As test_pitched_region_and_canvas_views: the region inside a parent of another colour, then in its last rows, so that the view ends where the
    allocation ends; the canvas, pre-filled with 0x7f, and the mask as odd-pitch, odd-base windows of poisoned parents - the canvas parent untouched outside
    the view, the mask read nowhere outside its window (its surroundings would be tissue)."""
    from toad_amd import ops
    for cell, md in ((4, 1), (4, 2), (32, 4)):
        px, idx, lut = random_case(hr, wr, cell, 7 * hr + wr + cell + md)
        px = (px >> 1).astype(np.uint8)                           # pixels below 128, the surroundings 255
        cells, lut_d = dev(idx, cuda, torch.int32), dev(lut, cuda)
        m = random_mask(hr, wr, md, 3 * hr + md, True)
        downs = [d for d in DOWNS if md % d == 0]
        wants = {d: ref.canvas(px, idx, cell, lut, 102, d, smooth=True, mask=m, mask_down=md, mask_thresh=8) for d in downs}
        # the mask: values 0 .. 255 inside a parent of 255 (tissue at every threshold), last rows and columns included
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
                got = ops.region_heat_blend_px(v, cells, cell, lut_d, 102, d, smooth=True, mask=mv, mask_down=md, mask_thresh=8)
                assert same_px(got, wants[d]), (cell, md, top, left, d)
        region = dev(px, cuda)
        for d in downs:
            want = wants[d]
            for pads in (odd_pads(want.shape[1], *inner), odd_pads(want.shape[1], *corner)):
                parent, view = embedded(np.full_like(want, 0x7F), *pads, 0x7F, cuda)
                assert view.stride(0) % 2 == 1 and view.data_ptr() % 2 == 1
                assert ops.region_heat_blend_px(region, cells, cell, lut_d, 102, d, smooth=True, mask=mviews[0], mask_down=md, mask_thresh=8, out=view) is view
                assert same_px(view, want), (cell, md, pads, d)
                view.fill_(0x7F)
                assert bool((parent == 0x7F).all()), (cell, md, pads, d)      # nothing outside the view was written
        with pytest.raises(ValueError, match="share storage"):
            ops.region_heat_blend_px(v, cells, cell, lut_d, 102, 1, smooth=True, out=v)


# ---- 6. Python ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_attention_canvas_keywords_equal_the_reference(cuda, k):
    from toad_amd import ops
    from toad_amd.heatmap import attention_canvas
    (hr, wr), tile, stride, origin, cell = heat_ref.LATTICES[k]
    s, origins, _, _, n = heat_ref.case(k)
    region = dev(s, cuda)
    rng = np.random.default_rng(60 + k)
    scores = rng.random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[2], scores[-1] = 0.0, 1.0, np.nan, 0.5
    sd = dev(scores, cuda)
    lat = dict(tile=tile, stride=stride, origin=origin)
    md = 4
    m = random_mask(hr, wr, md, 90 + k, True)
    mask = (dev(m, cuda), 100, md)

    def want(down, smooth=False, masked=False, thresh=None, binarize=False):
        q = ref.select(scores, heat_ref.quantise(scores), thresh, binarize)
        t = heat_ref.table(origins[q >= 0], q[q >= 0], tile, stride, origin, n)
        cells = heat_ref.cells(t, cell, tile, stride, origin, (hr, wr))
        kw = dict(mask=m, mask_down=md, mask_thresh=100) if masked else {}
        return ref.canvas(s, cells, cell, heat_ref.jet(), 102, down, smooth=smooth, **kw)

    for down in DOWNS:
        got = attention_canvas(region, origins, sd, down=down, smooth=True, mask=mask, thresh=0.5, binarize=True, **lat)
        assert same_px(got, want(down, True, True, 0.5, True)), down
        assert same_px(attention_canvas(region, origins, sd, down=down, smooth=True, **lat), want(down, smooth=True)), down
        assert same_px(attention_canvas(region, origins, sd, down=down, mask=mask, **lat), want(down, masked=True)), down
    assert same_px(attention_canvas(region, origins, sd, thresh=0.5, **lat), want(1, thresh=0.5))
    assert same_px(attention_canvas(region, origins, sd, binarize=True, **lat), want(1, binarize=True))
    assert same_px(attention_canvas(region, origins, sd, thresh=0.25, smooth=True, **lat), want(1, smooth=True, thresh=0.25))
    base = want(1)
    for other in (want(1, smooth=True), want(1, masked=True), want(1, thresh=0.5), want(1, binarize=True)):
        assert not np.array_equal(other, base)                      # every keyword does something on these inputs
    # one blend call with or without the keywords (smooth=False and mask=None launch the flat kernel behind it), and it is what region_heat_blend gives
    called = []
    real = ops.region_heat_blend_px
    ops.region_heat_blend_px = lambda *a, **kw: called.append((a, kw)) or real(*a, **kw)
    try:
        got = attention_canvas(region, origins, sd, thresh=0.5, binarize=True, **lat)
        assert same_px(got, want(1, thresh=0.5, binarize=True)) and len(called) == 1
        (a, kw), = called
        assert len(a) == 6 and kw["smooth"] is False and kw["mask"] is None and torch.equal(got, ops.region_heat_blend(*a))
        attention_canvas(region, origins, sd, smooth=True, **lat)
        assert len(called) == 2 and called[1][1]["smooth"] is True
    finally:
        ops.region_heat_blend_px = real


@pytest.mark.gpu
def test_region_tissue_attention_heatmap_colours_tissue_pixels_only(cuda):
    from toad_amd.eval import region_tissue_attention_heatmap, region_tissue_attention_scores
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
    key = (48, 1100, 1)
    s = tissue_ref.slide(*key)
    region = dev(s, cuda)
    tile = stride = (16, 256)
    seg = dict(down=4, median=3, sat_thresh="otsu")
    want_o, total, want_t = tissue_seg_ref.selection(s, tile, stride, (0, 0), 0.25, 4, 3, "otsu", key=key)
    want_plane, _ = tissue_seg_ref.segmented(s, 4, 3, "otsu", key=key)
    assert total == 12 and 0 < len(want_o) < total
    o_ref, s_ref = region_tissue_attention_scores(extractor, mil, region, tile=tile, stride=stride, percentile=True, segment=seg)
    o_sel, (plane, t) = segmented_tissue_origins(region, tile=tile, stride=stride, return_mask=True, **seg)
    o_cnt, counts, t2, (plane2, t3) = segmented_tissue_origins(region, tile=tile, stride=stride, return_counts=True, return_threshold=True, return_mask=True, **seg)
    assert np.array_equal(o_sel, want_o) and np.array_equal(o_cnt, want_o) and np.array_equal(o_ref, want_o) and (t, t2, t3) == (want_t,) * 3
    assert plane.dtype == torch.uint8 and np.array_equal(plane.cpu().numpy(), want_plane) and torch.equal(plane, plane2)
    m = plane.cpu().numpy()
    tissue = np.repeat(np.repeat(m > t, 4, axis=0), 4, axis=1)      # at the region's level; 48 x 1100 are multiples of 4
    # the counts of the kept tiles were taken from this very plane
    assert [int((m[y // 4:(y + 16) // 4, x // 4:(x + 256) // 4] > t).sum()) for x, y in o_ref.tolist()] == counts.tolist()
    assert tissue.any() and not tissue.all()
    for down in (1, 4):
        origins, scores, canvas = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=down, segment=seg, tissue_mask=True,
                                                                  smooth=True)
        assert np.array_equal(origins, o_ref) and torch.equal(scores, s_ref)
        by_hand = attention_canvas(region, origins, scores, tile=tile, stride=stride, down=down, smooth=True, mask=(plane, t, 4))
        assert torch.equal(canvas, by_hand)
        plain = heat_ref.box(s, down).astype(np.uint8)
        changed = (canvas.cpu().numpy() != plain).any(axis=2)
        assert changed.any() and not changed[~tissue[::down, ::down]].any(), down      # no pixel outside the returned mask is coloured
        q = heat_ref.quantise(scores.cpu().numpy())
        cells = heat_ref.cells(heat_ref.table(origins, q, tile, stride, (0, 0), (4, 3)), 16, tile, stride, (0, 0), (48, 1100))
        assert same_px(canvas, ref.canvas(s, cells, 16, heat_ref.jet(), 102, down, smooth=True, mask=m, mask_down=4, mask_thresh=t)), down
        unmasked = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=down, segment=seg, smooth=True)[2]
        assert not torch.equal(unmasked, canvas)                    # the glass inside a selected tile is what the mask takes out
    # the morphology filters: the mask is then the 0 / 255 plane the tiles were counted on, read with threshold 0
    o_m, (plane_m, t_m) = segmented_tissue_origins(region, tile=tile, stride=stride, return_mask=True, close=3, min_area=4, **seg)
    assert t_m == 0 and set(plane_m.unique().tolist()) <= {0, 255} and tuple(plane_m.shape) == tuple(plane.shape)
    canvas_m = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, segment=dict(close=3, min_area=4, **seg), tissue_mask=True)[2]
    assert torch.equal(canvas_m, attention_canvas(region, o_m, region_tissue_attention_scores(extractor, mil, region, tile=tile, stride=stride, percentile=True,
                                                  segment=dict(close=3, min_area=4, **seg))[1], tile=tile, stride=stride, mask=(plane_m, 0, 4)))
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=4, segment=dict(down=2, median=3), tissue_mask=True)
