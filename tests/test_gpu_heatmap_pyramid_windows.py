"""GPU: several pyramid levels for a list of windows of one slide rendered in one call (csrc/heatmap.hip: heat_pyramid_list_kernel behind
toad_region_heat_pyramid_windows_u8; ops.region_heat_pyramid_windows, heatmap.windows_pyramid, eval.slide_attention_heatmap(batch_levels=True)). Every
canvas is defined in integers, so every comparison is == on whole arrays. The references are the whole-slide canvases of the entry points that were
there before any window entry (region_heat_blend_px, region_heat_thumb), the single-window pyramid call, the single-level list call and - so that it
is not only sibling kernels - the per-pixel windowed reference of tests/heat_window_ref.py on one block per set of levels.

The scene is test_gpu_heatmap_windows.py's: the 200 x 600 slide, its 4 x 10 table of 64-pixel cells, its 50 x 150 table of 4-pixel cells and its mask
plane at mask_down 32, the uneven 2 x 3 block grids whose seams are multiples of max(4, down) inside cells, and the guard-filled parents."""
import numpy as np
import pytest
import torch

from tests import heat_window_ref as wref
from tests.test_gpu_heatmap import same_px
from tests.test_gpu_heatmap_windows import GUARD, HS, MD, THRESH, WS, _Rows, grid, guard_untouched, scene, variants, whole_canvas      # noqa: F401

DOWNS = (1, 2, 4, 8, 16, 32)
SETS = ((1, 4, 16), (2, 8), (8, 16, 32), DOWNS)                       # RB 16 and 32; levels finished in the lane only, in the tail only, both
BOTH = dict(smooth=True, mask_down=MD, mask_thresh=THRESH)


def both(sc):
    return dict(BOTH, mask=sc["mask_d"])


@pytest.fixture(scope="module")
def wholes(cuda, scene):
    """The whole slide at every level and in every variant through the older entry points, cell 64; computed once, never written."""
    return {(d, name): whole_canvas(scene, 64, d, **kw) for d in DOWNS for name, kw in variants(scene)}


def parents(ds, device):
    """Per level a guard-filled parent larger than the slide's canvas, and the slide's canvas inside it."""
    ps = {d: torch.full((HS // d + 3, WS // d + 5, 3), GUARD, dtype=torch.uint8, device=device) for d in ds}
    return ps, {d: p[1:1 + HS // d, 2:2 + WS // d] for d, p in ps.items()}


def views(canvases, ds, blocks):
    return [[canvases[d][wy // d:wy // d + h // d, wx // d:wx // d + w // d] for d in ds] for wx, wy, w, h in blocks]


def regions_of(sc, blocks):
    return [sc["slide"][wy:wy + h, wx:wx + w] for wx, wy, w, h in blocks], [(wx, wy) for wx, wy, _, _ in blocks]


# ---- (a) a block grid in one call is every level's whole-slide canvas -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", SETS, ids=str)
def test_block_grid_in_one_call_is_every_levels_whole_slide_canvas(cuda, scene, wholes, ds):
    """The uneven 2 x 3 grid of the largest level, flat / smooth / mask / both: every level's canvas, put together from the six views, equals the
    whole-slide canvas of the older entry, and the parent around it keeps its guard bytes. Then the grid trimmed to 198 x 598 pixels: widths that are
    no multiple of 4, and rows and columns that the coarse levels drop and the fine ones keep."""
    from toad_amd import ops
    blocks = grid(max(ds))
    trimmed = [(wx, wy, min(w, 598 - wx), min(h, 198 - wy)) for wx, wy, w, h in blocks]
    assert trimmed[2][2] % 4 == 2 and trimmed[5][3] % 4 == 2
    cells, lut = scene["cells"][64], scene["lut_d"]
    for name, kw in variants(scene):
        for wins, (hc, wc) in ((blocks, (HS, WS)), (trimmed, (198, 598))):
            ps, canvases = parents(ds, cuda)
            regions, places = regions_of(scene, wins)
            outs = views(canvases, ds, wins)
            got = ops.region_heat_pyramid_windows(regions, places, cells, 64, lut, 102, ds, outs=outs, **kw)
            assert len(got) == 6 and all(len(g) == len(ds) and all(a is b for a, b in zip(g, o)) for g, o in zip(got, outs))
            for d in ds:
                assert torch.equal(canvases[d][:hc // d, :wc // d], wholes[d, name][:hc // d, :wc // d]), (name, d, hc)
                assert guard_untouched(ps[d], hc // d, wc // d), (name, d, hc)
    for d in ds:                                                      # every keyword does something at every level (cell 64 > down)
        assert len({wholes[d, name].cpu().numpy().tobytes() for name, _ in variants(scene)}) == 4


# ---- (b) each window against the single-window call -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", SETS, ids=str)
def test_each_windows_tuple_is_region_heat_pyramid_of_that_window(cuda, scene, ds):
    from toad_amd import ops
    blocks = grid(max(ds))
    blocks = blocks + [(wx, wy, min(w, 598 - wx), min(h, 198 - wy)) for wx, wy, w, h in blocks[3:]]
    regions, places = regions_of(scene, blocks)
    cells, lut = scene["cells"][64], scene["lut_d"]
    for name, kw in variants(scene):
        got = ops.region_heat_pyramid_windows(regions, places, cells, 64, lut, 102, ds, **kw)
        assert isinstance(got, tuple) and len(got) == len(blocks)
        for k, (g, region, place) in enumerate(zip(got, regions, places)):
            want = ops.region_heat_pyramid(region, place, cells, 64, lut, 102, ds, **kw)
            assert isinstance(g, tuple) and len(g) == len(ds)
            for d, a, b in zip(ds, g, want):
                assert tuple(a.shape) == (region.shape[0] // d, region.shape[1] // d, 3) and torch.equal(a, b), (name, k, d)


# ---- (c) levels that are empty for some windows only ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", ((1, 4, 16), (4, 16), (8, 16, 32), (2, 32), DOWNS), ids=str)
def test_empty_levels_write_nothing_and_the_others_are_rendered(cuda, scene, ds):
    """The first, a middle and the last window are empty at SOME levels only - D - 1 rows, D - 1 columns, and one box of the smallest level - and, where
    the set does not hold level 1, two more windows are empty at every level. An empty level's canvas has no pixel and the guard-filled buffer its view
    comes from keeps every byte; every other canvas equals region_heat_window at that level and nothing around it is written."""
    from toad_amd import ops
    lo, top = min(ds), max(ds)
    step = max(4, top)
    partial = [(0, 0, 300, top - 1), (2 * step, step, top - 1, 40 + top), (3 * step, 3 * step, lo, lo)]
    live = [(step, 2 * step, 263, 37 + top), (4 * step, step, 2 * step + 3, 3 * step + 1)]
    empty = [(0, step, 300, lo - 1), (step, 0, lo - 1, lo - 1)] if lo > 1 else []
    wins = [partial[0], live[0]] + empty[:1] + [partial[1], live[1]] + empty[1:] + [partial[2]]
    cells, lut, kw = scene["cells"][64], scene["lut_d"], both(scene)
    bufs = [[torch.full((max(h // d, 1) + 2, 3 * max(w // d, 1) + 7), GUARD, dtype=torch.uint8, device=cuda) for d in ds] for _, _, w, h in wins]
    outs = [[b[1:1 + h // d, 2:2 + 3 * (w // d)].unflatten(1, (w // d, 3)) for b, d in zip(bs, ds)] for bs, (_, _, w, h) in zip(bufs, wins)]
    regions, places = regions_of(scene, wins)
    got = ops.region_heat_pyramid_windows(regions, places, cells, 64, lut, 102, ds, outs=outs, **kw)
    seen = set()
    for k, (gs, os_, bs, region, (wx, wy, w, h)) in enumerate(zip(got, outs, bufs, regions, wins)):
        for d, g, o, b in zip(ds, gs, os_, bs):
            assert g is o and tuple(g.shape) == (h // d, w // d, 3)
            if h // d == 0 or w // d == 0:
                assert g.numel() == 0 and bool((b == GUARD).all()), (k, d)
                seen.add(((wx, wy, w, h) in empty, "empty"))
            else:
                assert torch.equal(g, ops.region_heat_window(region, (wx, wy), cells, 64, lut, 102, d, **kw)), (k, d)
                g.fill_(GUARD)
                assert bool((b == GUARD).all()), (k, d)                # nothing around the view was written
                seen.add(((wx, wy, w, h) in partial, "live"))
        assert all((h // d == 0 or w // d == 0) for d in ds) == ((wx, wy, w, h) in empty)
    assert (False, "empty") in seen and (True, "live") in seen      # partial windows had both kinds of level
    if empty:                                                         # a list of windows that are empty at every level launches nothing
        regions, places = regions_of(scene, empty)
        got = ops.region_heat_pyramid_windows(regions, places, cells, 64, lut, 102, ds)
        assert [[g.numel() for g in gs] for gs in got] == [[0] * len(ds)] * 2


# ---- (d) more windows than one launch takes -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", ((1, 4, 16), DOWNS), ids=str)
def test_a_list_longer_than_one_launch(cuda, scene, ds):
    """ops.HEAT_PYR_LIST_MAX + 1 windows of 16 x 16 to 48 x 56 pixels at distinct places: the call crosses one launch, the last window is alone in the
    second. Each tuple equals region_heat_pyramid."""
    from toad_amd import ops
    from toad_amd.heatmap import windows_pyramid
    n = ops.HEAT_PYR_LIST_MAX + 1
    assert n == 17
    rng = np.random.default_rng(11 + len(ds))
    step = max(4, max(ds))
    wins = []
    for k in range(n):
        h, w = (16, 16) if k == 0 else (48, 56) if k == n - 1 else (int(rng.integers(16, 49)), int(rng.integers(16, 57)))
        wx, wy = (k % 9) * 64 + int(rng.integers(0, 2)) * step, (k // 9) * 64 + int(rng.integers(0, 2)) * step
        wins.append((wx, wy, w, h))
    assert len({(wx, wy) for wx, wy, _, _ in wins}) == n and all(wx + w <= WS and wy + h <= HS for wx, wy, w, h in wins)
    regions, places = regions_of(scene, wins)
    cells, lut = scene["cells"][64], scene["lut_d"]
    got = windows_pyramid(regions, places, cells, 64, downs=ds, lut=lut, smooth=True, mask=(scene["mask_d"], THRESH, MD))
    assert len(got) == n
    for k, (gs, region, place) in enumerate(zip(got, regions, places)):
        want = ops.region_heat_pyramid(region, place, cells, 64, lut, 102, ds, **both(scene))
        assert all(torch.equal(a, b) for a, b in zip(gs, want)) and len(gs) == len(ds), (k, wins[k])


# ---- (e) one window, and one level ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", SETS, ids=str)
def test_a_list_of_one_window_is_region_heat_pyramid(cuda, scene, ds):
    from toad_amd import ops
    step = max(4, max(ds))
    cells, lut = scene["cells"][64], scene["lut_d"]
    for wx, wy, w, h in ((step, 3 * step, 263 + step, 37 + step), (0, 0, WS, HS), (3 * step, step, 2 * step + 3, 3 * step + 1)):
        region = scene["slide"][wy:wy + h, wx:wx + w]
        for name, kw in variants(scene):
            got = ops.region_heat_pyramid_windows([region], [(wx, wy)], cells, 64, lut, 102, ds, **kw)
            want = ops.region_heat_pyramid(region, (wx, wy), cells, 64, lut, 102, ds, **kw)
            assert isinstance(got, tuple) and len(got) == 1 and len(got[0]) == len(ds)
            assert all(torch.equal(a, b) for a, b in zip(got[0], want)), ((wx, wy, w, h), name)


@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_one_level_is_region_heat_windows(cuda, scene, down):
    """A set of one level is the single-level list call: the grid, a window that is empty at that level in the middle, cell 64 and (down <= 4) cell 4."""
    from toad_amd import ops
    blocks = grid(down)
    blocks = blocks[:3] + [(0, 0, 300, down - 1)] * (down > 1) + blocks[3:]
    regions, places = regions_of(scene, blocks)
    for cell in (64, 4) if down <= 4 else (64,):
        cells, lut = scene["cells"][cell], scene["lut_d"]
        for name, kw in variants(scene):
            got = ops.region_heat_pyramid_windows(regions, places, cells, cell, lut, 102, (down,), **kw)
            want = ops.region_heat_windows(regions, places, cells, cell, lut, 102, down, **kw)
            assert len(got) == len(blocks) and all(len(g) == 1 and torch.equal(g[0], w) for g, w in zip(got, want)), (cell, name)


# ---- (f) the cell-4 table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_cell_4_table_flat_and_masked_and_the_smooth_refusal(cuda, scene):
    from toad_amd import ops
    ds = (1, 2, 4)
    blocks = grid(4)
    cells, lut = scene["cells"][4], scene["lut_d"]
    regions, places = regions_of(scene, blocks)
    for name, kw in variants(scene):
        if kw.get("smooth"):
            with pytest.raises(ValueError, match="smooth at cell = 4 is not done for more than one level"):
                ops.region_heat_pyramid_windows(regions, places, cells, 4, lut, 102, ds, **kw)
            continue
        ps, canvases = parents(ds, cuda)
        ops.region_heat_pyramid_windows(regions, places, cells, 4, lut, 102, ds, outs=views(canvases, ds, blocks), **kw)
        for d in ds:
            assert torch.equal(canvases[d], whole_canvas(scene, 4, d, **kw)), (name, d)
            assert guard_untouched(ps[d], HS // d, WS // d), (name, d)


# ---- (g) pitched views at odd addresses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", ((1, 4, 16), DOWNS), ids=str)
def test_regions_and_canvases_at_odd_addresses_and_pitches(cuda, scene, ds):
    """Every region is a view of a larger buffer of its own, filled with another colour, that starts at an odd byte address and has an odd pitch - a byte
    read outside the view would change a box mean - and every canvas of every level a view at an odd address and an odd pitch inside a guard-filled
    buffer, which keeps its guard bytes. Widths that are no multiple of 4 and heights that are no multiple of 4 or of the levels."""
    from toad_amd import ops
    top = max(ds)
    step = max(4, top)
    wins = [(step, 3 * step, 263 + top, 37 + top), (2 * step, 0, 2 * step + 3, 3 * step + 1), (5 * step, 2 * step, 297, 101), (0, step, 75, 50 + top)]
    cells, lut, kw = scene["cells"][64], scene["lut_d"], both(scene)
    regions, outs, bufs = [], [], []
    for k, (wx, wy, w, h) in enumerate(wins):
        pitch = 3 * w + 5 + (3 * w) % 2                              # odd
        flat = torch.full(((h + 2) * pitch + 1,), 255 - k, dtype=torch.uint8, device=cuda)
        view = flat[pitch + 8:pitch + 8 + h * pitch].view(h, pitch)[:, :3 * w].unflatten(1, (w, 3))
        view.copy_(scene["slide"][wy:wy + h, wx:wx + w])
        assert view.data_ptr() % 2 == 1 and view.stride(0) % 2 == 1 and not view.is_contiguous()
        regions.append(view)
        o, b = [], []
        for d in ds:
            ho, wo = h // d, w // d
            opitch = 3 * wo + 7 + (3 * wo) % 2                       # odd
            buf = torch.full(((ho + 2) * opitch + 1,), GUARD, dtype=torch.uint8, device=cuda)
            out = buf[opitch + 6:opitch + 6 + ho * opitch].view(ho, opitch)[:, :3 * wo].unflatten(1, (wo, 3))
            assert out.data_ptr() % 2 == 1 and out.stride(0) % 2 == 1
            o.append(out)
            b.append(buf)
        outs.append(o)
        bufs.append(b)
    got = ops.region_heat_pyramid_windows(regions, [(wx, wy) for wx, wy, _, _ in wins], cells, 64, lut, 102, ds, outs=outs, **kw)
    for k, (gs, os_, bs, (wx, wy, w, h)) in enumerate(zip(got, outs, bufs, wins)):
        want = ops.region_heat_pyramid(scene["slide"][wy:wy + h, wx:wx + w], (wx, wy), cells, 64, lut, 102, ds, **kw)
        for d, g, o, b, wd in zip(ds, gs, os_, bs, want):
            assert g is o and torch.equal(o, wd) and bool((o != GUARD).any()), (k, d)
            o.fill_(GUARD)
            assert bool((b == GUARD).all()), (k, d)


# ---- (h) against the per-pixel reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ds", SETS, ids=str)
def test_one_block_against_the_per_pixel_reference(cuda, scene, ds):
    """Not only sibling kernels: the bottom middle block of the grid, the one that spans two chunks, rendered in the list call between its neighbours,
    against tests/heat_window_ref.py at every level, tent and mask on."""
    from toad_amd import ops
    blocks = grid(max(ds))[3:]
    regions, places = regions_of(scene, blocks)
    got = ops.region_heat_pyramid_windows(regions, places, scene["cells"][64], 64, scene["lut_d"], 102, ds, **both(scene))
    wx, wy, w, h = blocks[1]
    assert w > 256
    for d, g in zip(ds, got[1]):
        want = wref.canvas(scene["px"][wy:wy + h, wx:wx + w], (wx, wy), scene["idx"][64], 64, scene["lut"], 102, d, True, scene["mask"], MD, THRESH)
        assert same_px(g, want), d


# ---- (i) the strip walk with one render call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slide_attention_heatmap_batch_levels_equals_the_strip_by_strip_walk(cuda, scene):
    """Three uneven overlapping strips of the 200 x 600 slide, tiles of 64 at stride 64 (cell 64), the caller's tiles: with batch_levels=True pass 2 is one
    call, and origins, scores and every level's canvas are those of batch_levels=False."""
    from toad_amd.eval import slide_attention_heatmap
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    spans = [(0, 80), (64, 96), (128, 72)]                           # rows 0 .. 80, 64 .. 160, 128 .. 200: seams at 80 and 160, inside cells
    strips = [(scene["slide"][y:y + n], y) for y, n in spans]
    rng = np.random.default_rng(5)
    tiles = np.array([(x, y) for y in (0, 64, 128) for x in range(0, WS - 63, 64)], dtype=np.int64)
    tiles = tiles[np.sort(rng.permutation(len(tiles))[:19])]
    downs = (1, 4, 16)
    kw = dict(tile=64, stride=64, origins=tiles, down=downs, smooth=True, mask=(scene["mask_d"], THRESH, MD), blur=(2, 1))
    o0, s0, c0 = slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), **kw)
    out = {d: torch.full((HS // d, WS // d, 3), GUARD, dtype=torch.uint8, device=cuda) for d in downs}
    o1, s1, c1 = slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), batch_levels=True, out=out, **kw)
    assert np.array_equal(o0, tiles) and np.array_equal(o1, o0) and torch.equal(s1, s0) and len(s0) == len(tiles)
    assert list(c1) == list(downs) == list(c0)
    for d in downs:
        assert c1[d] is out[d] and tuple(c0[d].shape) == (HS // d, WS // d, 3) and torch.equal(c1[d], c0[d]), d
    flat = slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), **dict(kw, smooth=False, blur=False))[2]
    assert not any(torch.equal(c0[d], flat[d]) for d in downs)      # the keywords did something
