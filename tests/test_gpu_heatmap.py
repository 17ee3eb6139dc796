"""GPU: attention heat maps of a decoded uint8 region (csrc/heatmap.hip heat_cells_kernel, heat_blend_px_kernel<DOWN,0,false>; toad_amd/heatmap.py;
eval.region_tissue_attention_heatmap). The canvas is defined in integers, so every comparison is exact, against the numpy reference of tests/heat_ref.py
(tested on its own, by hand and on these very inputs, in test_heatmap_host.py - that the cases have covered and uncovered cells, overlap and several
colours is asserted there)."""
import numpy as np
import pytest
import torch

from tests import heat_ref as ref
from tests import tissue_ref

CELLS = (4, 8, 16, 32, 64)
DOWNS = (1, 2, 4)
POISON = 0x7F7F7F7F


def dev(a: np.ndarray, device, dtype=None) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return (t if dtype is None else t.to(dtype)).to(device)


def same_cells(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.int32 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def same_px(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)


def cells_into_poison(tile_q, cell, origin, tile, stride, n, region_hw):
    """toad_heat_cells into a table pre-filled with 0x7f7f7f7f: equality with the reference then also proves every element is written."""
    from toad_amd import _lib
    (x0, y0), (h, w), (sy, sx), (nx, ny), (hr, wr) = origin, tile, stride, n, region_hw
    cells = torch.full((-(-hr // cell), -(-wr // cell)), POISON, dtype=torch.int32, device=tile_q.device)
    _lib.check(_lib.load().toad_heat_cells(tile_q.data_ptr(), nx, ny, cell, x0, y0, h, w, sx, sy, cells.shape[0], cells.shape[1], cells.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "toad_heat_cells")
    return cells


def random_case(hr, wr, cell, seed):
    """(pixels uint8 [hr,wr,3], cells int64 [Gy,Gx] with -1, 0 and 255 among the values, lut uint8 [256,3]) from a seeded generator."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(hr, wr, 3), dtype=np.uint8)
    idx = rng.integers(-1, 256, size=(-(-hr // cell), -(-wr // cell)))
    idx[rng.random(idx.shape) < 0.3] = -1
    flat = idx.reshape(-1)
    flat[0] = 255
    if flat.size > 2:
        flat[1], flat[2] = -1, 0
    return px, idx, rng.integers(0, 256, size=(256, 3), dtype=np.uint8)


# ---- 1. cells, exact ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(ref.LATTICES)))
def test_cell_values_equal_the_reference_and_every_element_is_written(cuda, k):
    from toad_amd import ops
    (hr, wr), tile, stride, origin, cell = ref.LATTICES[k]
    _, origins, q, t, n = ref.case(k)
    tq = dev(t, cuda, torch.int32)
    for fine in [c for c in CELLS if c <= cell]:                  # the lattice's own cell and every finer one
        want = ref.cells(t, fine, tile, stride, origin, (hr, wr))
        assert (want == -1).any() and (want >= 0).any() and want.max() <= 255
        got = cells_into_poison(tq, fine, origin, tile, stride, n, (hr, wr))
        assert same_cells(got, want), fine
        assert torch.equal(ops.heat_cells(tq, fine, origin, tile, stride, n, (hr, wr)), got)
    none = torch.full_like(tq, -1)                                # no tile present: no cell has a value
    assert same_cells(cells_into_poison(none, cell, origin, tile, stride, n, (hr, wr)), np.full((-(-hr // cell), -(-wr // cell)), -1))
    with pytest.raises(RuntimeError, match="last tile"):        # more columns of tiles than the cells hold
        cells_into_poison(tq, cell, origin, tile, stride, (n[0] + 1000, n[1]), (hr, wr))


# ---- 2. the blend arithmetic, exhaustively --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_blend_on_every_colour_pixel_pair(cuda):
    """1024 x 1024 at cell 4: cell (gy, gx) has idx = gy and pixels (gx, 255 - gx, gx ^ 0x55); lut[i] = (i, 255 - i, i ^ 0xAA). Every (colour, pixel)
    pair of every channel occurs."""
    from toad_amd import ops
    g = np.arange(256)
    cell_px = np.stack([g, 255 - g, g ^ 0x55], axis=1).astype(np.uint8)                       # [gx, 3]
    px = np.ascontiguousarray(np.broadcast_to(np.repeat(cell_px, 4, axis=0)[None], (1024, 1024, 3)))
    idx = np.ascontiguousarray(np.broadcast_to(g[:, None], (256, 256)))
    lut = np.stack([g, 255 - g, g ^ 0xAA], axis=1).astype(np.uint8)
    region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
    for alpha in (0, 1, 77, 128, 255, 256):
        want = ref.canvas(px, idx, 4, lut, alpha, 1)
        assert same_px(ops.region_heat_blend(region, cells, 4, lut_d, alpha, 1), want), alpha
    assert np.array_equal(ref.canvas(px, idx, 4, lut, 0, 1), px) and np.array_equal(ref.canvas(px, idx, 4, lut, 256, 1)[::4, 0], lut)


# ---- 3. shapes and edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr", [(1, 1), (7, 5), (64, 64), (67, 131), (131, 67), (203, 333), (203, 334), (300, 520)])
def test_canvas_shapes_and_edges(cuda, hr, wr):
    from toad_amd import ops
    for cell in (4, 16, 64):
        px, idx, lut = random_case(hr, wr, cell, 1000 * hr + wr + cell)
        region, cells, lut_d = dev(px, cuda), dev(idx, cuda, torch.int32), dev(lut, cuda)
        for down in DOWNS:
            want = ref.canvas(px, idx, cell, lut, 102, down)
            got = ops.region_heat_blend(region, cells, cell, lut_d, 102, down)
            assert want.shape == (hr // down, wr // down, 3) and same_px(got, want), (cell, down)
    if (hr, wr) == (1, 1):
        assert ops.region_heat_blend(region, cells, cell, lut_d, 102, 4).shape == (0, 0, 3)      # empty: nothing is launched


# ---- 4. pitch, base and surroundings ----------------------------------------------------------------------------------------------------------------
def embedded(px: np.ndarray, top, left, bottom, right, fill, device):
    """px as rows [top, top + Hr) x columns [left, left + Wr) of a wider, taller image filled with `fill`: a pitch above 3 Wr, a base at byte
    top * pitch + 3 * left."""
    hr, wr, _ = px.shape
    wide = torch.full((hr + top + bottom, wr + left + right, 3), fill, dtype=torch.uint8, device=device)
    v = wide[top:top + hr, left:left + wr]
    v.copy_(torch.from_numpy(px.copy()))
    assert not v.is_contiguous() and v.stride() == (3 * (wr + left + right), 3, 1)
    return wide, v


def odd_pads(w, top, left, bottom, right):
    """The pads moved by one where needed, so that a view of width w has an odd pitch 3 (w + left + right) and an odd base top * pitch + 3 * left."""
    if (w + left + right) % 2 == 0:
        left += 1
    if (top + left) % 2 == 0:
        top += 1
    return top, left, bottom, right


@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr,inner,corner", [(67, 131, (2, 3, 1, 5), (1, 4, 0, 0)), (300, 520, (2, 3, 1, 6), (2, 5, 0, 0))])
def test_pitched_region_and_canvas_views(cuda, hr, wr, inner, corner):
    """The region inside a parent of another colour at an odd base address with an odd pitch, then in the parent's last rows and columns, so that its final
    row ends where the allocation ends: the canvas equals that of the contiguous copy (a byte read outside the view would change a box mean). Then the
    canvas as a view inside a poisoned parent at an odd base and pitch: the view equals the reference and every other byte of the parent keeps the poison."""
    from toad_amd import ops
    for cell in (4, 32):
        px, idx, lut = random_case(hr, wr, cell, 7 * hr + wr + cell)
        px = (px >> 1).astype(np.uint8)                           # pixels below 128, the surroundings 255
        cells, lut_d = dev(idx, cuda, torch.int32), dev(lut, cuda)
        for top, left, bottom, right in (inner, corner):
            _, v = embedded(px, top, left, bottom, right, 255, cuda)
            assert v.stride(0) % 2 == 1 and v.data_ptr() % 2 == 1
            if (bottom, right) == (0, 0):
                assert v.storage_offset() + (hr - 1) * v.stride(0) + 3 * wr == v.untyped_storage().nbytes()
            for down in DOWNS:
                want = ref.canvas(px, idx, cell, lut, 102, down)
                assert same_px(ops.region_heat_blend(v, cells, cell, lut_d, 102, down), want), (cell, top, left, down)
        region = dev(px, cuda)
        for down in DOWNS:
            want = ref.canvas(px, idx, cell, lut, 102, down)
            for top, left, bottom, right in (odd_pads(want.shape[1], *inner), odd_pads(want.shape[1], *corner)):
                parent, view = embedded(np.full_like(want, 0xA5), top, left, bottom, right, 0xA5, cuda)
                assert view.stride(0) % 2 == 1 and view.data_ptr() % 2 == 1
                assert ops.region_heat_blend(region, cells, cell, lut_d, 102, down, out=view) is view
                assert same_px(view, want), (cell, top, left, down)
                view.fill_(0xA5)
                assert bool((parent == 0xA5).all()), (cell, top, left, down)      # nothing outside the view was written
        with pytest.raises(ValueError, match="share storage"):
            ops.region_heat_blend(v, cells, cell, lut_d, 102, 1, out=v)


# ---- 5. attention_canvas ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_attention_canvas_equals_the_reference(cuda, k):
    from toad_amd.heatmap import attention_canvas, jet_lut, quantise_scores
    (hr, wr), tile, stride, origin, cell = ref.LATTICES[k]
    s, origins, _, _, n = ref.case(k)
    region = dev(s, cuda)
    rng = np.random.default_rng(50 + k)
    scores = rng.random(len(origins)).astype(np.float32)
    scores[0], scores[1], scores[-1] = 0.0, 1.0, 1.5              # the ends of the range, and one beyond it
    lat = dict(tile=tile, stride=stride, origin=origin)

    def want(sc, alpha, down, lut):
        q = ref.quantise(sc)
        t = ref.table(origins[q >= 0], q[q >= 0], tile, stride, origin, n)
        return ref.canvas(s, ref.cells(t, cell, tile, stride, origin, (hr, wr)), cell, lut, alpha, down)

    sd = dev(scores, cuda)
    assert np.array_equal(jet_lut(cuda).cpu().numpy(), ref.jet())
    for down in DOWNS:
        got = attention_canvas(region, origins, sd, down=down, **lat)
        assert same_px(got, want(scores, 102, down, ref.jet())), down
        assert torch.equal(attention_canvas(region, origins, sd, down=down, **lat), got)         # run to run
    assert same_px(attention_canvas(region, origins, sd, alpha=0.4, **lat), want(scores, 102, 1, ref.jet()))       # round(256 * 0.4) = 102
    assert same_px(attention_canvas(region, origins, sd, alpha=0.75, down=2, **lat), want(scores, 192, 2, ref.jet()))
    lut = np.random.default_rng(9).integers(0, 256, size=(256, 3), dtype=np.uint8)
    assert same_px(attention_canvas(region, origins, sd, alpha=200, lut=dev(lut, cuda), **lat), want(scores, 200, 1, lut))
    # a NaN score: its tile is absent, it never becomes a colour
    holes = scores.copy()
    holes[[2, len(holes) // 2]] = np.nan
    w_nan = want(holes, 102, 1, ref.jet())
    assert not np.array_equal(w_nan, want(scores, 102, 1, ref.jet()))
    assert same_px(attention_canvas(region, origins, dev(holes, cuda), **lat), w_nan)
    # no origins: the box-filtered region
    for down in DOWNS:
        got = attention_canvas(region, np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device=cuda), down=down, **lat)
        assert same_px(got, ref.box(s, down).astype(np.uint8))
    # another score range: the quantisation agrees with the same float32 formula on the CPU to +-1, compared on its own
    wide = torch.from_numpy((rng.random(len(origins)).astype(np.float32) * 12 - 4))
    q_dev, q_cpu = quantise_scores(wide.to(cuda), (-3.0, 7.5)), quantise_scores(wide, (-3.0, 7.5))
    assert int((q_dev.cpu() - q_cpu).abs().max()) <= 1 and q_cpu.min() == 0 and q_cpu.max() == 65535 and len(q_cpu.unique()) > 8
    got = attention_canvas(region, origins, wide.to(cuda), score_range=(-3.0, 7.5), **lat)
    qd = q_dev.cpu().numpy().astype(np.int64)
    assert same_px(got, ref.canvas(s, ref.cells(ref.table(origins, qd, tile, stride, origin, n), cell, tile, stride, origin, (hr, wr)), cell, ref.jet(), 102, 1))
    with pytest.raises(ValueError, match="off the lattice"):
        attention_canvas(region, origins + 1, sd, **lat)


# ---- 6. through the pipeline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_region_tissue_attention_heatmap_draws_the_selected_tiles(cuda):
    from toad_amd.eval import region_tissue_attention_heatmap, region_tissue_attention_scores
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
    tile = stride = (8, 256)
    kept, total = tissue_ref.selection(s, tile, stride, (0, 0), 0.25, 8, 0)
    assert total == 20 and 0 < len(kept) < total
    o_ref, s_ref = region_tissue_attention_scores(extractor, mil, region, tile=tile, stride=stride, percentile=True)
    for down in (1, 4):
        origins, scores, canvas = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, down=down)
        assert np.array_equal(origins, kept) and np.array_equal(origins, o_ref) and torch.equal(scores, s_ref)
        q = ref.quantise(scores.cpu().numpy())
        assert q.min() == 0 and q.max() == 65535 and len(np.unique(q)) == len(kept)              # percentile ranks: all different, the ends reached
        cells = ref.cells(ref.table(origins, q, tile, stride, (0, 0), (4, 5)), 8, tile, stride, (0, 0), (40, 1100))
        assert (cells == -1).any() and (cells >= 0).any()
        assert same_px(canvas, ref.canvas(s, cells, 8, ref.jet(), 102, down)), down
