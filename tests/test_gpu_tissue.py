"""GPU: tissue selection on a decoded uint8 region (csrc/tissue.hip tissue_cells_kernel<CELL>, tissue_tile_counts_kernel; toad_amd/tissue.py;
eval.region_tissue_attention_scores). The result is defined in integers, so every comparison is exact, against the numpy reference of tests/tissue_ref.py
(tested on its own, on these very inputs, in test_tissue_host.py - the "mixed outcome" assertions below are facts about that reference)."""
import numpy as np
import pytest
import torch

from tests import tissue_ref as ref

CELLS = (4, 8, 16, 32, 64)
THRESHOLDS = ((8, 0), (8, 16), (40, 16))
POISON = 0x7F7F7F7F
# (region (hr, wr), tile (H, W), stride (sy, sx), origin (x, y))
LATTICES = [((300, 520), (64, 64), (32, 32), (0, 0)), ((300, 520), (64, 64), (64, 64), (8, 4)), ((203, 333), (32, 64), (8, 16), (0, 0)),
            ((300, 520), (256, 256), (64, 64), (0, 0)), ((131, 67), (16, 16), (16, 16), (0, 0))]


def cells_into_poison(region, cell, sat, vmin):
    """toad_region_tissue_cells_u8 into a counts array pre-filled with 0x7f7f7f7f: equality with the reference then also proves every element is written."""
    from toad_amd import _lib, ops
    pitch, hr, wr = ops._region_pitch(region, "test")
    counts = torch.full((-(-hr // cell), -(-wr // cell)), POISON, dtype=torch.int32, device=region.device)
    _lib.check(_lib.load().toad_region_tissue_cells_u8(region.data_ptr(), pitch, hr, wr, cell, sat, vmin, counts.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream), "toad_region_tissue_cells_u8")
    return counts


def same(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.int32 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def embedded(region: np.ndarray, top, left, bottom, right, dev):
    """The region as rows [top, top + Hr) x columns [left, left + Wr) of a wider, taller image of saturated red (tissue under every threshold used here):
    a pitch above 3 Wr, a base at byte top * pitch + 3 * left."""
    hr, wr, _ = region.shape
    wide = torch.zeros((hr + top + bottom, wr + left + right, 3), dtype=torch.uint8, device=dev)
    wide[..., 0] = 255
    v = wide[top:top + hr, left:left + wr]
    v.copy_(torch.from_numpy(region.copy()))
    assert not v.is_contiguous() and v.stride() == (3 * (wr + left + right), 3, 1)
    return v


# ---- 1. cells, exact ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr", [(1, 1), (7, 5), (7, 6), (64, 64), (67, 131), (131, 67), (66, 134), (300, 520)])
def test_cell_counts_equal_the_reference_and_every_element_is_written(cuda, hr, wr):
    from toad_amd import ops
    s = ref.slide(hr, wr, 1)
    region = torch.from_numpy(s.copy()).to(cuda)
    for cell in CELLS:
        for sat, vmin in THRESHOLDS:
            want = ref.cell_counts(s, cell, sat, vmin)
            got = cells_into_poison(region, cell, sat, vmin)
            assert same(got, want), (cell, sat, vmin)
            assert torch.equal(ops.region_tissue_cells(region, cell, sat, vmin), got)
    if (hr, wr) == (300, 520):                                  # empty, full and partial cells all occur
        c = ref.cell_counts(s, 16, 8, 0)
        full = np.minimum(16, hr - 16 * np.arange(c.shape[0]))[:, None] * np.minimum(16, wr - 16 * np.arange(c.shape[1]))[None, :]
        assert (c == 0).any() and (c == full).any() and ((c > 0) & (c < full)).any()


# ---- 2. pitch, base and surroundings --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr,inner,corner", [(67, 131, (2, 3, 1, 5), (1, 4, 0, 0)), (300, 520, (2, 3, 1, 6), (2, 5, 0, 0))])
def test_pitched_views_count_like_the_contiguous_copy(cuda, hr, wr, inner, corner):
    """The region inside a parent of saturated red, at an odd base address with an odd pitch; then in the parent's last rows and columns, so that its final
    row ends where the allocation ends. A byte read outside the view and counted would show: every red pixel is tissue."""
    s = ref.slide(hr, wr, 1)
    for top, left, bottom, right in (inner, corner):
        v = embedded(s, top, left, bottom, right, cuda)
        assert v.stride(0) % 2 == 1 and v.data_ptr() % 2 == 1
        if (bottom, right) == (0, 0):
            assert v.storage_offset() + (hr - 1) * v.stride(0) + 3 * wr == v.untyped_storage().nbytes()
        for cell in CELLS:
            for sat, vmin in THRESHOLDS:
                assert same(cells_into_poison(v, cell, sat, vmin), ref.cell_counts(s, cell, sat, vmin)), (top, left, cell, sat, vmin)


# ---- 3. the predicate, exhaustively -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_predicate_on_every_max_min_pair(cuda):
    """One probe pixel per 4 x 4 block for every (mx, mn <= mx, position of mx among r, g, b); everything else is grey 128, never tissue. With CELL = 4 the
    counts are the predicate's 0 / 1."""
    img, mx, mn = ref.probe_blocks()
    region = torch.from_numpy(img.copy()).to(cuda)
    for sat in (0, 8, 15, 254, 255):
        for vmin in (0, 1, 50, 255):
            want = (mx >= vmin) & (255 * (mx - mn) > sat * mx)
            assert (not want.any()) if sat == 255 else (want.any() and not want.all())
            assert same(cells_into_poison(region, 4, sat, vmin), want.astype(np.int64)), (sat, vmin)
            # the first 63 block columns as a view narrower than a wave's 256 pixels: every row ends inside its one chunk, so the kernel's edge path
            # is checked on a quarter of the pairs as well
            assert same(cells_into_poison(region[:, :252], 4, sat, vmin), want[:, :63].astype(np.int64)), (sat, vmin)
    assert int((255 * (mx - mn) > 8 * mx).sum()) == 3 * 31743


# ---- 4. tile counts, exact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LATTICES)))
def test_tile_counts_equal_direct_sums_over_the_tiles(cuda, case):
    from toad_amd import ops
    from toad_amd.tissue import lattice, lattice_cell, tissue_tile_fraction
    (hr, wr), tile, stride, origin = LATTICES[case]
    s = ref.slide(hr, wr, 1)
    region = torch.from_numpy(s.copy()).to(cuda)
    cell = lattice_cell(tile, stride, origin)
    assert cell == (32, 4, 8, 64, 16)[case]
    nx, ny = lattice(hr, wr, tile, stride, origin)
    for sat, vmin in THRESHOLDS:
        want = ref.tile_counts(s, tile, stride, origin, sat, vmin)
        assert want.shape == (ny, nx) and want.min() < want.max()
        got, gx, gy = tissue_tile_fraction(region, tile, stride, origin, sat, vmin)
        assert (gx, gy) == (nx, ny) and same(got, want), (sat, vmin)
        # ... and from every finer cell size
        for fine in [c for c in CELLS if c <= cell]:
            cells = ops.region_tissue_cells(region, fine, sat, vmin)
            out = ops.tissue_tile_counts(cells, fine, origin, tile, stride, (nx, ny))
            assert same(out, want), (fine, sat, vmin)
    with pytest.raises(RuntimeError, match="last tile"):       # more columns of tiles than the cells hold
        ops.tissue_tile_counts(cells, fine, origin, tile, stride, (nx + 1000, ny))


# ---- 5. tissue_origins ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tissue_origins_equal_the_reference_selection(cuda):
    from toad_amd import ops
    from toad_amd.tissue import tissue_origins
    hr, wr, tile, stride = 300, 520, (64, 64), (32, 32)
    s = ref.slide(hr, wr, 1)
    region = torch.from_numpy(s.copy()).to(cuda)
    for sat, vmin in ((8, 0), (8, 16)):
        for f in (0, 0.05, 0.25, 0.5, 1.0):
            want, total = ref.selection(s, tile, stride, (0, 0), f, sat, vmin)
            assert total == 120 and (len(want) == total if f == 0 else 0 < len(want) < total), (f, len(want))
            got = tissue_origins(region, 64, 32, min_fraction=f, sat_thresh=sat, val_min=vmin)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), f
            assert ops.check_origins(got, hr, wr, 64, 64).tolist() == want.tolist()              # the region calls take them unchanged
            again, counts = tissue_origins(region, 64, 32, min_fraction=f, sat_thresh=sat, val_min=vmin, return_counts=True)
            assert np.array_equal(again, got)                                                    # run to run
            tc = ref.tile_counts(s, tile, stride, (0, 0), sat, vmin)
            assert counts.dtype == np.int64 and np.array_equal(counts, tc[got[:, 1] // 32, got[:, 0] // 32])
    full, _ = ref.selection(s, tile, stride, (0, 0), 1.0, 8, 0)
    assert all(ref.tissue_mask(s, 8, 0)[y:y + 64, x:x + 64].all() for x, y in full)               # at 1.0 only full tiles
    # val_min changes the selection where the lattice reaches the black margin: 8 x 8 tiles, the last column of tiles at x = 512
    k0, k16 = ref.selection(s, (8, 8), (8, 8), (0, 0), 0.25, 8, 0)[0], ref.selection(s, (8, 8), (8, 8), (0, 0), 0.25, 8, 16)[0]
    assert len(k16) < len(k0) and (k0[:, 0] == 512).any() and not (k16[:, 0] == 512).any()
    assert np.array_equal(tissue_origins(region, 8), k0) and np.array_equal(tissue_origins(region, 8, val_min=16), k16)
    # an origin off (0, 0) and non-square tiles; a pitched view
    want, total = ref.selection(s, (32, 64), (8, 16), (8, 4), 0.25, 8, 0)
    assert 0 < len(want) < total
    assert np.array_equal(tissue_origins(region, (32, 64), (8, 16), origin=(8, 4)), want)
    assert np.array_equal(tissue_origins(embedded(s, 2, 3, 1, 6, cuda), (32, 64), (8, 16), origin=(8, 4)), want)
    # a region smaller than the tile
    small = tissue_origins(region[:60], 64)
    assert small.shape == (0, 2) and small.dtype == np.int64


# ---- 6. through the pipeline ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_region_tissue_attention_scores_score_the_selected_tiles(cuda):
    from toad_amd.eval import region_attention_scores, region_tissue_attention_scores
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    s = ref.slide(40, 1100, 1)
    region = torch.from_numpy(s.copy()).to(cuda)
    want, total = ref.selection(s, (8, 256), (8, 256), (0, 0), 0.25, 8, 0)
    assert total == 20 and 0 < len(want) < total
    origins, scores = region_tissue_attention_scores(extractor, mil, region, tile=(8, 256), stride=(8, 256))
    assert np.array_equal(origins, want) and np.array_equal(origins, tissue_origins(region, (8, 256), (8, 256)))
    assert scores.shape == (len(want),) and torch.equal(scores, region_attention_scores(extractor, mil, region, origins, tile=(8, 256)))
    assert torch.isfinite(scores).all()
    o32, s32 = region_tissue_attention_scores(extractor, mil, region, tile=(8, 256), stride=(8, 256), bag_dtype=torch.float32, percentile=True)
    assert np.array_equal(o32, want)
    assert torch.equal(s32, region_attention_scores(extractor, mil, region, want, tile=(8, 256), bag_dtype=torch.float32, percentile=True))
    # nothing selected: empty results, and the extractor is not called
    o0, s0 = region_tissue_attention_scores(None, None, region, tile=(8, 256), stride=(8, 256), sat_thresh=255)
    assert o0.shape == (0, 2) and s0.shape == (0,) and s0.device == region.device
