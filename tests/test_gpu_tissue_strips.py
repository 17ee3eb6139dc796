"""GPU: the saturation plane of a list of windows in one launch (csrc/tissue_seg.hip sat_plane_list_kernel<DOWN>, toad_regions_saturation_u8,
ops.regions_saturation) and the segmented tissue selection of a slide that arrives in strips (toad_amd/tissue.py slide_saturation,
segment_tissue_strips, segmented_slide_origins; the segment= and tissue_mask= keywords of eval.slide_attention_heatmap). Everything is defined in
integers, so every comparison is exact: against the single-window calls on the whole slide, and against the numpy reference of tests/tissue_seg_ref.py.

The test slide is tissue_ref.slide(200, 600, seed): its rows reach all four waves at every down; at down = 32 Hp = 6 with 8 rows dropped and Wp = 18 with
24 columns dropped; three 256-pixel column chunks, two on the plain path and one partial."""
import numpy as np
import pytest
import torch

from tests import tissue_morph_ref as mref
from tests import tissue_seg_ref as ref

DOWNS = (1, 2, 4, 8, 16, 32)
GUARD = 0x7F
HS, WS = 200, 600
SPANS = [(0, 96), (64, 96), (160, 40)]                               # three uneven strips, the first two overlapping: rows 0 .. 96, 64 .. 160, 160 .. 200
BLOCKS = [(y, x, h, w) for y, h in ((0, 96), (96, 104)) for x, w in ((0, 192), (192, 224), (416, 184))]      # a 2 x 3 grid: x cuts at 192 and 416, y cut at 96
WALK_HW = (256, 1100)
WALK_SPANS = [(0, 112), (64, 144), (176, 80)]                        # the spans of test_slide_attention_heatmap_over_overlapping_strips
WALK_TILE = (64, 256)


def dev(a: np.ndarray, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                   # a copy: the cached inputs are read-only


def same_plane(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def guarded_plane(hp, wp, cuda, top=1, left=3):
    """(parent, view): a uint8 [hp,wp] view at an odd pitch and offset inside a parent filled with 0x7f."""
    width = wp + left + 2
    width += 1 - width % 2
    parent = torch.full((hp + top + 2, width), GUARD, dtype=torch.uint8, device=cuda)
    return parent, parent[top:top + hp, left:left + wp]


def guards_untouched(parent, view_shape, top=1, left=3) -> bool:
    p = parent.clone()
    p[top:top + view_shape[0], left:left + view_shape[1]] = GUARD
    return bool((p == GUARD).all())


@pytest.fixture(scope="module")
def slide(cuda):
    """(numpy slide, device slide, {(down, vmin): whole-slide plane by ops.region_saturation}) - computed once, left unchanged."""
    from toad_amd import ops
    s = ref.slide(HS, WS, 1)
    d = dev(s, cuda)
    whole = {(down, vmin): ops.region_saturation(d, down, vmin) for down in DOWNS for vmin in (0, 40)}
    return s, d, whole


def strip_windows(d, plane, down):
    """The strips' sub-regions and their rows of `plane`, by plane_strip_plan."""
    from toad_amd.tissue import plane_strip_plan
    plan = plane_strip_plan((HS, WS), SPANS, down)
    regions = [d[y:y + n][p0 * down - y:p1 * down - y] for (y, n), (p0, p1) in zip(SPANS, plan)]
    return regions, [plane[p0:p1] for p0, p1 in plan]


def block_windows(d, plane, down):
    return [d[y:y + h, x:x + w] for y, x, h, w in BLOCKS], [plane[y // down:y // down + h // down, x // down:x // down + w // down] for y, x, h, w in BLOCKS]


# ---- 1. strips and blocks into views of one plane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_strips_and_blocks_in_one_call_are_the_plane_of_the_slide(cuda, slide, down):
    from toad_amd import ops
    s, d, whole = slide
    hp, wp = HS // down, WS // down
    for vmin in (0, 40):
        want = ref.saturation_plane(s, down, vmin)
        assert same_plane(whole[down, vmin], want)
        for windows in (strip_windows, block_windows):
            parent, plane = guarded_plane(hp, wp, cuda)
            regions, outs = windows(d, plane, down)
            got = ops.regions_saturation(regions, down, vmin, outs=outs)      # ONE call
            assert len(got) == len(outs) and all(g is o for g, o in zip(got, outs))
            assert torch.equal(plane, whole[down, vmin]) and same_plane(plane, want), (down, vmin, windows.__name__)
            assert guards_untouched(parent, (hp, wp)), (down, vmin, windows.__name__)
    if down == 32:
        assert (hp, wp) == (6, 18) and HS - 32 * hp == 8 and WS - 32 * wp == 24


# ---- 2. each window against the single-window call -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_each_window_of_a_list_equals_region_saturation(cuda, slide, down):
    from toad_amd import ops
    s, d, whole = slide
    regions = [d[y:y + n] for y, n in SPANS] + [d[y:y + h, x:x + w] for y, x, h, w in BLOCKS] + [d[3:70, 5:266], d[:, 1:]]
    for vmin in (0, 40):
        got = ops.regions_saturation(regions, down, vmin)
        assert len(got) == len(regions)
        for k, (r, g) in enumerate(zip(regions, got)):
            assert g.is_contiguous() and torch.equal(g, ops.region_saturation(r, down, vmin)), (down, vmin, k)
        one, = ops.regions_saturation([d], down, vmin)               # a list of one window
        assert torch.equal(one, whole[down, vmin])


# ---- 3. windows without a plane pixel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS[1:])
def test_empty_windows_write_nothing_and_the_others_are_written(cuda, slide, down):
    from toad_amd import ops
    s, d, whole = slide
    flat, thin = d[:down - 1], d[:, :down - 1]                       # Hr < down, Wr < down
    hp, wp = HS // down, WS // down
    full = [d[:96], d[64:160, 100:500], d[96:]]
    want = [ops.region_saturation(r, down) for r in full]
    orders = dict(first=[flat, thin] + full, middle=[full[0], flat, full[1], thin, full[2]], last=full + [thin, flat])
    for where, regs in orders.items():
        got = ops.regions_saturation(regs, down)
        assert [tuple(g.shape) for r, g in zip(regs, got) if r is flat or r is thin] == [(0, wp) if r is flat else (hp, 0) for r in regs if r is flat or r is thin]
        live = [g for r, g in zip(regs, got) if r is not flat and r is not thin]
        assert len(live) == 3 and all(torch.equal(g, w) for g, w in zip(live, want)), (down, where)
        # ... and with outs: the empty windows' views lie in a guard-filled parent, which stays as it was
        guard = torch.full((hp + 4, wp + 8), GUARD, dtype=torch.uint8, device=cuda)
        planes = [torch.full_like(w, GUARD) for w in want]
        it = iter(planes)
        outs = [guard[2:2, 3:3 + wp] if r is flat else guard[1:1 + hp, 5:5] if r is thin else next(it) for r in regs]
        got = ops.regions_saturation(regs, down, outs=outs)
        assert all(g is o for g, o in zip(got, outs)) and bool((guard == GUARD).all())
        assert all(torch.equal(p, w) for p, w in zip(planes, want)), (down, where)
    # only empty windows, and no window at all: nothing is launched
    assert [tuple(g.shape) for g in ops.regions_saturation([flat, thin, flat], down)] == [(0, WS // down), (HS // down, 0), (0, WS // down)]
    assert ops.regions_saturation([], down) == ()


# ---- 4. a list longer than one launch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", (1, 4, 16))
def test_thirty_three_windows_are_two_launches_with_the_same_bytes(cuda, slide, down):
    from toad_amd import ops
    s, d, whole = slide
    assert ops.SAT_LIST_MAX == 32
    regions = [d[(5 * k) % 184:(5 * k) % 184 + 16, (16 * k + 3) % 536:(16 * k + 3) % 536 + 64] for k in range(33)]
    got = ops.regions_saturation(regions, down, 40)
    assert len(got) == 33
    for k, (r, g) in enumerate(zip(regions, got)):
        assert tuple(g.shape) == (16 // down, 64 // down) and torch.equal(g, ops.region_saturation(r, down, 40)), (down, k)
    assert same_plane(got[32], ref.saturation_plane(s[160:176, 515:579], down, 40))      # the one window of the second launch, against the reference


# ---- 5. odd addresses and pitches ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_regions_and_planes_at_odd_addresses_and_pitches(cuda, slide, down):
    """Every region at byte offset 1 with pitch 3 Wr + 5, every plane at byte offset 3 with pitch Wp + 7, in buffers filled with 0x7f."""
    from toad_amd import ops
    s, d, whole = slide
    regions, outs, parents = [], [], []
    for y, n in SPANS:
        buf = torch.full((1 + n * (3 * WS + 5),), GUARD, dtype=torch.uint8, device=cuda)
        r = torch.as_strided(buf, (n, WS, 3), (3 * WS + 5, 3, 1), 1)
        r.copy_(d[y:y + n])
        assert r.data_ptr() % 2 == 1 and r.stride(0) == 3 * WS + 5
        hp, wp = n // down, WS // down
        pbuf = torch.full((3 + max(hp, 1) * (wp + 7),), GUARD, dtype=torch.uint8, device=cuda)
        o = torch.as_strided(pbuf, (hp, wp), (wp + 7, 1), 3)
        regions.append(r), outs.append(o), parents.append(pbuf)
    ops.regions_saturation(regions, down, 0, outs=outs)
    for k, ((y, n), o, pbuf) in enumerate(zip(SPANS, outs, parents)):
        want = ref.saturation_plane(s[y:y + n], down)
        assert same_plane(o, want), (down, k)
        expect = torch.full_like(pbuf, GUARD)
        torch.as_strided(expect, tuple(o.shape), (o.shape[1] + 7, 1), 3).copy_(o)
        assert torch.equal(pbuf, expect), (down, k)                  # nothing outside y * pitch + [0, Wp) was written


# ---- 6. slide_saturation ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_slide_saturation_in_one_call_and_strip_by_strip(cuda, slide, down):
    from toad_amd.tissue import slide_saturation
    s, d, whole = slide
    strips = [(d[y:y + n], y) for y, n in SPANS]
    for vmin in (0, 40):
        for batch in (True, False):
            got = slide_saturation(strips, (HS, WS), down, vmin, batch=batch)
            assert got.is_contiguous() and torch.equal(got, whole[down, vmin]), (down, vmin, batch)
    assert torch.equal(slide_saturation([(d, 0)], (HS, WS), down), whole[down, 0])


# ---- 7. the segmented calls ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk_slide(cuda):
    s = ref.slide(*WALK_HW, 1)
    d = dev(s, cuda)
    return s, d, [(d[y:y + n], y) for y, n in WALK_SPANS]


SEG_CASES = [dict(down=16, median=7, sat_thresh=8), dict(down=16, median=7, sat_thresh="otsu"), dict(down=8, median=5, sat_thresh=8),
             dict(down=16, median=7, sat_thresh=8, close=4, min_area=8, min_hole=8)]
SEG_KEPT = [9, 6, 8, None]                                            # of 16 tiles, by tests/tissue_seg_ref.selection on the CPU (the last: tissue_morph_ref, below)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(SEG_CASES)))
def test_segmented_calls_on_strips_equal_the_whole_slide(cuda, walk_slide, case):
    from toad_amd.tissue import segment_tissue, segment_tissue_strips, segmented_slide_origins, segmented_tissue_origins
    s, d, strips = walk_slide
    kw = SEG_CASES[case]
    morph = {k: kw.get(k, 0) for k in ("close", "min_area", "min_hole")}
    if any(morph.values()):
        cpu_o, cpu_c, cpu_t = mref.selection(s, WALK_TILE, WALK_TILE, (0, 0), 0.25, kw["down"], kw["median"], kw["sat_thresh"], **morph)
    else:
        cpu_o, total, cpu_t = ref.selection(s, WALK_TILE, WALK_TILE, (0, 0), 0.25, kw["down"], kw["median"], kw["sat_thresh"], key=(*WALK_HW, 1))
        assert total == 16 and len(cpu_o) == SEG_KEPT[case]
    assert 4 < len(cpu_o) < 16                                       # a selector that returns nothing or everything cannot pass
    # the plane and the threshold
    want_p, want_pt, want_t = segment_tissue(d, return_threshold=True, **kw)
    got_p, got_pt, got_t = segment_tissue_strips(strips, WALK_HW, return_threshold=True, **kw)
    assert torch.equal(got_p, want_p) and got_pt == want_pt and got_t == want_t == cpu_t
    assert segment_tissue_strips(strips, WALK_HW, **kw)[1] == want_pt
    # origins, counts, threshold and the mask
    sel = dict(tile=WALK_TILE, stride=WALK_TILE, return_counts=True, return_threshold=True, return_mask=True, **kw)
    want_o, want_c, want_t2, (want_m, want_mt) = segmented_tissue_origins(d, **sel)
    got_o, got_c, got_t2, (got_m, got_mt) = segmented_slide_origins(strips, WALK_HW, **sel)
    assert np.array_equal(want_o, cpu_o)
    assert np.array_equal(got_o, want_o) and got_o.dtype == np.int64 and np.array_equal(got_c, want_c) and got_t2 == want_t2 == cpu_t
    assert torch.equal(got_m, want_m) and got_mt == want_mt
    assert np.array_equal(segmented_slide_origins(strips, WALK_HW, tile=WALK_TILE, stride=WALK_TILE, **kw), want_o)


# ---- 8. the walk ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slide_attention_heatmap_with_the_segmented_selector_across_strips(cuda, walk_slide):
    """The slide, spans, extractor and model of test_slide_attention_heatmap_over_overlapping_strips (same seeds), selected with segment=dict(down=16) on
    the whole slide's plane and rendered with its mask: origins, scores and canvas are those of the one-region calls on the whole slide."""
    from toad_amd.eval import attention_heatmap_scores, slide_attention_heatmap
    from toad_amd.heatmap import attention_canvas, strip_plan
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import segmented_tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    s, d, strips = walk_slide
    hs, ws = WALK_HW
    tile = stride = WALK_TILE
    want_o, (plane, t) = segmented_tissue_origins(d, tile=tile, stride=stride, down=16, return_mask=True)
    cpu_o = ref.selection(s, tile, stride, (0, 0), 0.25, 16, 7, 8, key=(hs, ws, 1))[0]
    assert np.array_equal(want_o, cpu_o) and 4 < len(want_o) < 16
    plan = strip_plan((hs, ws), WALK_SPANS, tile, stride, (0, 0), 16)
    bags = []
    for (region, y), p in zip(strips, plan):
        mine = want_o[(want_o[:, 1] // 64 >= p["rows"][0]) & (want_o[:, 1] // 64 < p["rows"][1])]
        if len(mine):
            with torch.no_grad():
                bags.append(extractor.forward_u8_region(region, mine - np.array([0, y]), tile=tile, out_dtype=torch.float16))
    want_s = attention_heatmap_scores(mil, torch.cat(bags, dim=0), percentile=True)
    base = dict(tile=tile, stride=stride, smooth=True)
    for down in (1, 16):
        origins, scores, canvas = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=down, segment=dict(down=16), tissue_mask=True, **base)
        assert np.array_equal(origins, want_o) and origins.dtype == np.int64 and torch.equal(scores, want_s)
        want_c = attention_canvas(d, origins, scores, down=down, mask=(plane, t, 16), **base)
        assert tuple(canvas.shape) == (hs // down, ws // down, 3) and torch.equal(canvas, want_c)
        assert not torch.equal(want_c, attention_canvas(d, origins, scores, down=down, **base))       # the mask did something
    levels = (1, 4, 16)
    origins, scores, canvases = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=levels, segment=dict(down=16), tissue_mask=True, **base)
    assert np.array_equal(origins, want_o) and torch.equal(scores, want_s) and set(canvases) == set(levels)
    for lv in levels:
        assert torch.equal(canvases[lv], attention_canvas(d, origins, scores, down=lv, mask=(plane, t, 16), **base)), lv
    # the selection alone, without the mask: the unmasked canvas of the same tiles
    o2, s2, c2 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=16, segment=dict(down=16), **base)
    assert np.array_equal(o2, want_o) and torch.equal(s2, want_s) and torch.equal(c2, attention_canvas(d, want_o, want_s, down=16, **base))
    # segment=None: the bytes of the call without the new keywords
    o3, s3, c3 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=16, **base)
    o4, s4, c4 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), down=16, segment=None, tissue_mask=False, **base)
    assert np.array_equal(o3, o4) and torch.equal(s3, s4) and torch.equal(c3, c4)
