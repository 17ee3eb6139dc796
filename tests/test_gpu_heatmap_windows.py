"""GPU: a list of windows of one slide rendered in one call (csrc/heatmap.hip: heat_blend_px_list_kernel, heat_thumb_list_kernel behind
toad_region_heat_windows_u8; ops.region_heat_windows, heatmap.windows_canvas, eval.slide_attention_heatmap(batch_render=True)). The canvas is defined in
integers, so every comparison is == on whole arrays. The reference is ops.region_heat_window called once per window - and, so that it is not only the
sibling kernel, the per-pixel windowed reference of tests/heat_window_ref.py on one block per ``down`` and the whole-slide canvas of the entry points
that were there before.

The slide is 200 x 600 random pixels. Its cell tables are drawn directly, as in test_gpu_heatmap_window.py: 4 x 10 cells of 64 pixels - the cell of a
lattice of 256-pixel tiles at stride 64, which every ``down`` up to 32 is legal on - and 50 x 150 cells of 4 pixels for the nine-neighbour tent at
``down`` 1 and 2; about a third of the cells hold -1, the value of a cell no present tile covers. The mask plane is the slide's at mask_down 32, the only
plane pitch that every ``down`` divides, with grey values around the threshold."""
import numpy as np
import pytest
import torch

from tests import heat_window_ref as wref
from tests.test_gpu_heatmap import dev, same_px
from tests.test_gpu_heatmap_px import random_mask
from tests.test_gpu_heatmap_window import table_with_large_values

HS, WS = 200, 600
DOWNS = (1, 2, 4, 8, 16, 32)
GUARD = 0x7F
MD, THRESH = 32, 8


@pytest.fixture(scope="module")
def scene(cuda):
    """The slide, its two tables, colours and mask plane, on the host and on the device; built once, never written."""
    px, idx64, lut = table_with_large_values(HS, WS, 64, 20261)
    _, idx4, _ = table_with_large_values(HS, WS, 4, 20262)
    mask = random_mask(HS, WS, MD, 20263, True)
    assert idx64.shape == (4, 10) and idx4.shape == (50, 150) and mask.shape == (6, 18) and (idx64 < 0).any() and (idx4 < 0).any()
    return dict(px=px, lut=lut, mask=mask, idx={64: idx64, 4: idx4}, slide=dev(px, cuda), lut_d=dev(lut, cuda), mask_d=dev(mask, cuda),
                cells={64: dev(idx64, cuda, torch.int32), 4: dev(idx4, cuda, torch.int32)})


def variants(sc):
    m = dict(mask=sc["mask_d"], mask_down=MD, mask_thresh=THRESH)
    return (("flat", {}), ("smooth", dict(smooth=True)), ("mask", m), ("both", dict(smooth=True, **m)))


def grid(down):
    """An uneven 2 x 3 block grid over the slide as (wx, wy, w, h). Seams are multiples of max(4, down) that lie inside cells of 64. Widths: one below a
    256-pixel chunk, one spanning two chunks, one more below a chunk. Heights are no multiples of 16 or of strip_rows(down) wherever the arithmetic
    allows it: a seam is a multiple of max(4, down) and 200 = 8 mod 16, so from down = 8 on one of two heights is a multiple of 16 - it is the first
    one, and the last one is not. (Every width of a grid that covers 600 columns with such seams is a multiple of 4: the width that is not one is the
    trimmed grid's, below, and those of the other tests.)"""
    ys, xs = {1: ((0, 100, HS), (0, 172, 484, WS)), 2: ((0, 100, HS), (0, 172, 484, WS)), 4: ((0, 100, HS), (0, 172, 484, WS)),
              8: ((0, 112, HS), (0, 168, 488, WS)), 16: ((0, 112, HS), (0, 176, 496, WS)), 32: ((0, 96, HS), (0, 160, 480, WS))}[down]
    step = max(4, down)
    assert all(v % step == 0 and v % 64 for v in ys[1:-1] + xs[1:-1])
    widths, heights = [b - a for a, b in zip(xs, xs[1:])], [b - a for a, b in zip(ys, ys[1:])]
    assert widths[0] < 256 < widths[1] and widths[2] < 256 and heights[-1] % 16 and (down >= 8 or all(h % 16 for h in heights))
    return [(x0, y0, x1 - x0, y1 - y0) for y0, y1 in zip(ys, ys[1:]) for x0, x1 in zip(xs, xs[1:])]


def whole_canvas(sc, cell, down, **kw):
    """The whole slide through the entry points that were there before the window entry."""
    from toad_amd import ops
    blend = ops.region_heat_thumb if down >= 8 else ops.region_heat_blend_px
    return blend(sc["slide"], sc["cells"][cell], cell, sc["lut_d"], 102, down, **kw)


def list_into_canvas(sc, blocks, cell, down, **kw):
    """The blocks through ONE call, each canvas a view into one guard-filled parent that is larger than the slide's canvas -> (parent, slide canvas view)."""
    from toad_amd import ops
    ho, wo = HS // down, WS // down
    parent = torch.full((ho + 3, wo + 5, 3), GUARD, dtype=torch.uint8, device=sc["slide"].device)
    canvas = parent[1:1 + ho, 2:2 + wo]
    outs = [canvas[wy // down:wy // down + h // down, wx // down:wx // down + w // down] for wx, wy, w, h in blocks]
    got = ops.region_heat_windows([sc["slide"][wy:wy + h, wx:wx + w] for wx, wy, w, h in blocks], [(wx, wy) for wx, wy, _, _ in blocks], sc["cells"][cell], cell,
                                  sc["lut_d"], 102, down, outs=outs, **kw)
    assert len(got) == len(outs) and all(g is o for g, o in zip(got, outs))
    return parent, canvas


def guard_untouched(parent, ho, wo):
    """Every byte of the parent outside rows 1 .. 1 + ho and columns 2 .. 2 + wo still holds the guard."""
    p = parent.clone()
    p[1:1 + ho, 2:2 + wo] = GUARD
    return bool((p == GUARD).all())


# ---- (a) a block grid in one call is the whole-slide canvas ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_block_grid_in_one_call_is_the_whole_slide_canvas(cuda, scene, down):
    """The uneven 2 x 3 grid, flat / smooth / mask / both, on the cell-64 table for every down and on the cell-4 table where down <= 4: the one canvas the
    six views lie in equals the whole-slide canvas of the older entry, and the parent around it keeps its guard bytes. Then the grid trimmed to 198 x 598
    pixels - a last column whose width is no multiple of 4, last rows that end inside a lane's 4 rows: what it covers equals the whole-slide canvas,
    what it does not cover keeps the guard. One block per down is also checked against the per-pixel reference of tests/heat_window_ref.py."""
    ho, wo = HS // down, WS // down
    blocks = grid(down)
    wholes = {}
    for cell in (64, 4) if down <= 4 else (64,):
        for name, kw in variants(scene):
            whole = wholes[cell, name] = whole_canvas(scene, cell, down, **kw)
            parent, canvas = list_into_canvas(scene, blocks, cell, down, **kw)
            assert torch.equal(canvas, whole), (cell, name)
            assert guard_untouched(parent, ho, wo), (cell, name)
            # trimmed: the right column ends at 598, the bottom row at 198
            trimmed = [(wx, wy, min(w, 598 - wx), min(h, 198 - wy)) for wx, wy, w, h in blocks]
            assert trimmed[2][2] % 4 == 2 and trimmed[5][3] % 4 == 2
            hc, wc = 198 // down, 598 // down
            parent, canvas = list_into_canvas(scene, trimmed, cell, down, **kw)
            assert torch.equal(canvas[:hc, :wc], whole[:hc, :wc]), (cell, name)
            assert guard_untouched(parent, hc, wc), (cell, name)
        assert len({w.cpu().numpy().tobytes() for (c, _), w in wholes.items() if c == cell}) == (4 if cell != down else 2)      # every keyword does something
    # not only the sibling kernels: the bottom middle block, the one that spans two chunks, against the per-pixel reference, tent and mask on
    wx, wy, w, h = blocks[4]
    want = wref.canvas(scene["px"][wy:wy + h, wx:wx + w], (wx, wy), scene["idx"][64], 64, scene["lut"], 102, down, True, scene["mask"], MD, THRESH)
    assert same_px(wholes[64, "both"][wy // down:wy // down + h // down, wx // down:wx // down + w // down], want)


# ---- (b) empty windows in the list ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS[1:])
def test_empty_windows_write_nothing_and_the_others_are_rendered(cuda, scene, down):
    """The first, a middle and the last window have fewer than ``down`` rows or columns (at down = 1 no such window exists): their canvases have no
    pixel, and the guard-filled buffers their views come from keep every byte; the others equal region_heat_window."""
    from toad_amd import ops
    step = max(4, down)
    live = [(step, 2 * step, 263, 37 + down), (4 * step, step, 2 * step + 3, 3 * step + 1), (WS - 75 - (WS - 75) % step, HS - 50 - (HS - 50) % step, 75, 50)]
    empty = [(0, 0, 300, down - 1), (2 * step, step, down - 1, 40), (3 * step, 3 * step, down - 1, down - 1)]
    wins = [empty[0], live[0], live[1], empty[1], live[2], empty[2]]
    cells, lut = scene["cells"][64], scene["lut_d"]
    kw = dict(smooth=True, mask=scene["mask_d"], mask_down=MD, mask_thresh=THRESH)
    bufs = [torch.full((max(h // down, 1) + 2, 3 * max(w // down, 1) + 7), GUARD, dtype=torch.uint8, device=cuda) for _, _, w, h in wins]
    outs = [b[1:1 + h // down, 2:2 + 3 * (w // down)].unflatten(1, (w // down, 3)) for b, (_, _, w, h) in zip(bufs, wins)]
    regions = [scene["slide"][wy:wy + h, wx:wx + w] for wx, wy, w, h in wins]
    got = ops.region_heat_windows(regions, [(wx, wy) for wx, wy, _, _ in wins], cells, 64, lut, 102, down, outs=outs, **kw)
    for k, (g, o, b, region, (wx, wy, w, h)) in enumerate(zip(got, outs, bufs, regions, wins)):
        assert g is o and tuple(g.shape) == (h // down, w // down, 3)
        if (wx, wy, w, h) in empty:
            assert g.numel() == 0 and bool((b == GUARD).all()), k
        else:
            assert torch.equal(g, ops.region_heat_window(region, (wx, wy), cells, 64, lut, 102, down, **kw)) and bool((g != GUARD).any()), k
            g.fill_(GUARD)
            assert bool((b == GUARD).all()), k                     # nothing around the view was written
    # a list of empty windows launches nothing and returns its empty canvases
    got = ops.region_heat_windows([regions[0], regions[5]], [(0, 0), (3 * step, 3 * step)], cells, 64, lut, 102, down)
    assert [g.numel() for g in got] == [0, 0]


# ---- (c) one window -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_a_list_of_one_window_is_region_heat_window(cuda, scene, down):
    from toad_amd import ops
    step = max(4, down)
    for cell in (64, 4) if down <= 4 else (64,):
        cells, lut = scene["cells"][cell], scene["lut_d"]
        for wx, wy, w, h in ((step, 3 * step, 263 + down, 37 + down), (0, 0, WS, HS), (3 * step, step, 2 * step + 3, 3 * step + 1)):
            region = scene["slide"][wy:wy + h, wx:wx + w]
            for name, kw in variants(scene):
                got = ops.region_heat_windows([region], [(wx, wy)], cells, cell, lut, 102, down, **kw)
                assert isinstance(got, tuple) and len(got) == 1
                assert torch.equal(got[0], ops.region_heat_window(region, (wx, wy), cells, cell, lut, 102, down, **kw)), (cell, (wx, wy, w, h), name)


# ---- (d) more windows than one launch takes -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", (1, 4, 16))
def test_a_list_longer_than_one_launch(cuda, scene, down):
    """ops.HEAT_LIST_MAX + 1 windows of 16 x 16 to 48 x 80 pixels at distinct places, all sizes different from their neighbours': the call crosses one
    launch, the last window is alone in the second. Each canvas equals region_heat_window."""
    from toad_amd import ops
    from toad_amd.heatmap import windows_canvas
    n = ops.HEAT_LIST_MAX + 1
    assert n == 33
    rng = np.random.default_rng(7 + down)
    step = max(4, down)
    wins = []
    for k in range(n):
        h, w = (16, 16) if k == 0 else (48, 80) if k == n - 1 else (int(rng.integers(16, 49)), int(rng.integers(16, 81)))
        wx, wy = (k % 8) * 64 + int(rng.integers(0, 2)) * step, (k // 8) * 32 + int(rng.integers(0, 2)) * step
        wins.append((wx, wy, w, h))
    assert len({(wx, wy) for wx, wy, _, _ in wins}) == n and all(wx + w <= WS and wy + h <= HS for wx, wy, w, h in wins)
    regions = [scene["slide"][wy:wy + h, wx:wx + w] for wx, wy, w, h in wins]
    cells, lut = scene["cells"][64], scene["lut_d"]
    mask = (scene["mask_d"], THRESH, MD)
    got = windows_canvas(regions, [(wx, wy) for wx, wy, _, _ in wins], cells, 64, down=down, lut=lut, smooth=True, mask=mask)
    assert len(got) == n
    for k, (g, region, (wx, wy, w, h)) in enumerate(zip(got, regions, wins)):
        want = ops.region_heat_window(region, (wx, wy), cells, 64, lut, 102, down, smooth=True, mask=mask[0], mask_down=MD, mask_thresh=THRESH)
        assert tuple(g.shape) == (h // down, w // down, 3) and torch.equal(g, want), (k, (wx, wy, w, h))


# ---- (e) pitched views at odd addresses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down", DOWNS)
def test_regions_and_canvases_at_odd_addresses_and_pitches(cuda, scene, down):
    """Every region is a view of a larger buffer of its own, filled with another colour, that starts at an odd byte address and has an odd pitch - a byte
    read outside the view would change a box mean - and every canvas a view at an odd address and an odd pitch inside a guard-filled buffer, which keeps
    its guard bytes. Widths that are no multiple of 4 and heights that are no multiple of 4 or of down."""
    from toad_amd import ops
    step = max(4, down)
    wins = [(step, 3 * step, 263 + down, 37 + down), (2 * step, 0, 2 * step + 3, 3 * step + 1), (5 * step, 2 * step, 297, 101), (0, step, 75, 50 + down)]
    cells, lut = scene["cells"][64], scene["lut_d"]
    kw = dict(smooth=True, mask=scene["mask_d"], mask_down=MD, mask_thresh=THRESH)
    regions, outs, bufs = [], [], []
    for k, (wx, wy, w, h) in enumerate(wins):
        pitch = 3 * w + 5 + (3 * w) % 2                              # odd
        flat = torch.full(((h + 2) * pitch + 1,), 255 - k, dtype=torch.uint8, device=cuda)
        view = flat[pitch + 8:pitch + 8 + h * pitch].view(h, pitch)[:, :3 * w].unflatten(1, (w, 3))
        view.copy_(scene["slide"][wy:wy + h, wx:wx + w])
        assert view.data_ptr() % 2 == 1 and view.stride(0) % 2 == 1 and not view.is_contiguous()
        regions.append(view)
        ho, wo = h // down, w // down
        opitch = 3 * wo + 7 + (3 * wo) % 2                           # odd
        buf = torch.full(((ho + 2) * opitch + 1,), GUARD, dtype=torch.uint8, device=cuda)
        out = buf[opitch + 6:opitch + 6 + ho * opitch].view(ho, opitch)[:, :3 * wo].unflatten(1, (wo, 3))
        assert out.data_ptr() % 2 == 1 and out.stride(0) % 2 == 1
        outs.append(out)
        bufs.append(buf)
    got = ops.region_heat_windows(regions, [(wx, wy) for wx, wy, _, _ in wins], cells, 64, lut, 102, down, outs=outs, **kw)
    for k, (g, o, b, (wx, wy, w, h)) in enumerate(zip(got, outs, bufs, wins)):
        want = ops.region_heat_window(scene["slide"][wy:wy + h, wx:wx + w], (wx, wy), cells, 64, lut, 102, down, **kw)
        assert g is o and torch.equal(o, want) and bool((o != GUARD).any()), (k, (wx, wy, w, h))
        o.fill_(GUARD)
        assert bool((b == GUARD).all()), k


# ---- (f) the strip walk with one render call ------------------------------------------------------------------------------------------------------------
class _Rows:
    """Stands in for the extractor: bag rows that depend only on the tiles' first pixels, so that two walks over the same strips give the same bag."""

    def forward_u8_region(self, region, origins, tile=256, out_dtype=torch.float32, shrink=1):
        o = torch.as_tensor(np.asarray(origins), device=region.device)
        first = region[o[:, 1], o[:, 0]].to(torch.float32)          # [B,3]
        ramp = torch.arange(1024, device=region.device, dtype=torch.float32)
        return (torch.sin(first.sum(dim=1, keepdim=True) * 0.37 + ramp * 0.011) * 0.5).to(out_dtype)


@pytest.mark.gpu
def test_slide_attention_heatmap_batch_render_equals_the_strip_by_strip_walk(cuda, scene):
    """Three uneven overlapping strips of the 200 x 600 slide, tiles of 64 at stride 64 (cell 64), the caller's tiles: with batch_render=True pass 2 is one
    call, and origins, scores and canvas are those of batch_render=False."""
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
    mask = (scene["mask_d"], THRESH, MD)
    for down in (1, 16):
        kw = dict(tile=64, stride=64, origins=tiles, down=down, smooth=True, mask=mask, blur=(2, 1))
        o0, s0, c0 = slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), **kw)
        out = torch.full((HS // down, WS // down, 3), GUARD, dtype=torch.uint8, device=cuda)
        o1, s1, c1 = slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), batch_render=True, out=out, **kw)
        assert np.array_equal(o0, tiles) and np.array_equal(o1, o0) and torch.equal(s1, s0) and len(s0) == len(tiles)
        assert c1 is out and tuple(c0.shape) == (HS // down, WS // down, 3) and torch.equal(c1, c0)
        assert not torch.equal(c0, slide_attention_heatmap(_Rows(), mil, strips, (HS, WS), **dict(kw, smooth=False, blur=False))[2])      # the keywords did something
