"""GPU: segmented tissue selection on a decoded uint8 region (csrc/tissue_seg.hip sat_plane_kernel<DOWN>, plane_median_kernel<K>, plane_cells_kernel<CELL>;
toad_amd/tissue.py segment_tissue, segmented_tissue_origins; the segment= keyword of the eval calls). The result is defined in integers, so every
comparison is exact, against the numpy reference of tests/tissue_seg_ref.py (tested on its own, on these very inputs, in test_tissue_seg_host.py - the
"mixed outcome" conditions are facts about that reference, asserted there)."""
import numpy as np
import pytest
import torch

from tests import tissue_ref as ref0
from tests import tissue_seg_ref as ref
from tests.tissue_seg_ref import E2E_DM, E2E_FRACTIONS, E2E_LATTICES, E2E_SAT, lattice_allowed

DOWNS = (1, 2, 4, 8, 16, 32)
MEDIANS = (1, 3, 5, 7)
CELLS = (4, 8, 16, 32, 64)
POISON8 = 0x7F
POISON32 = 0x7F7F7F7F


def dev(a: np.ndarray, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                   # a copy: the cached inputs are read-only


def stream():
    return torch.cuda.current_stream().cuda_stream


def poisoned_view(hp, wp, cuda, top=1, left=3):
    """(parent, view): a uint8 [hp,wp] view at an odd pitch and offset inside a parent filled with 0x7f."""
    width = wp + left + 2
    width += 1 - width % 2                                           # an odd pitch
    parent = torch.full((hp + top + 2, width), POISON8, dtype=torch.uint8, device=cuda)
    view = parent[top:top + hp, left:left + wp]
    assert view.stride(0) % 2 == 1 and view.stride(1) == 1
    return parent, view


def only_the_view_was_written(parent, view_shape, top=1, left=3) -> bool:
    p = parent.clone()
    p[top:top + view_shape[0], left:left + view_shape[1]] = POISON8
    return bool((p == POISON8).all())


def pitch_of(view):
    return view.stride(0) if view.shape[0] > 1 else max(view.stride(0), view.shape[1])


def sat_into_poison(region, down, vmin):
    """toad_region_saturation_u8 into a pitched view of a poisoned parent -> (parent, view)."""
    from toad_amd import _lib, ops
    pitch, hr, wr = ops._region_pitch(region, "test")
    hp, wp = hr // down, wr // down
    parent, view = poisoned_view(hp, wp, region.device)
    _lib.check(_lib.load().toad_region_saturation_u8(region.data_ptr(), pitch, hr, wr, down, vmin, view.data_ptr(), pitch_of(view), stream()),
               "toad_region_saturation_u8")
    return parent, view


def same_plane(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def same_counts(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.int32 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def embedded(region: np.ndarray, top, left, bottom, right, cuda):
    """The region as rows [top, top + Hr) x columns [left, left + Wr) of a wider, taller image of saturated red (S = 255 wherever it leaks into a box)."""
    hr, wr, _ = region.shape
    wide = torch.zeros((hr + top + bottom, wr + left + right, 3), dtype=torch.uint8, device=cuda)
    wide[..., 0] = 255
    v = wide[top:top + hr, left:left + wr]
    v.copy_(torch.from_numpy(region.copy()))
    assert not v.is_contiguous() and v.stride() == (3 * (wr + left + right), 3, 1)
    return v


# ---- 1. the saturation byte, exhaustively -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_saturation_on_every_max_min_pair(cuda):
    """One probe pixel per 4 x 4 block for every (mx, mn <= mx, position of mx among r, g, b), at down = 1: the division is exact on all 32,896 pairs."""
    from toad_amd import ops
    img, mx, mn = ref.probe_blocks()
    region = dev(img, cuda)
    for vmin in (0, 1, 50, 255):
        want = ref.saturation_plane(img, 1, vmin)
        parent, view = sat_into_poison(region, 1, vmin)
        assert same_plane(view, want), vmin
        assert only_the_view_was_written(parent, want.shape)
        assert torch.equal(ops.region_saturation(region, 1, vmin), view)
        # a view narrower than a wave's 256 pixels: every row ends inside its one chunk, so the edge path sees a quarter of the pairs as well
        assert same_plane(ops.region_saturation(region[:, :251], 1, vmin), want[:, :251]), vmin
    probe = ref.saturation_plane(img, 1).reshape(384, 4, 257, 4).max(axis=(1, 3))
    assert np.array_equal(probe, (255 * (mx - mn) + (mx >> 1)) // np.maximum(mx, 1))


# ---- 2. shapes, every box filter ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr", [(1, 1), (7, 5), (7, 6), (31, 33), (67, 131), (131, 67), (66, 134), (300, 520), (70, 1037)])
def test_saturation_planes_equal_the_reference_and_nothing_else_is_written(cuda, hr, wr):
    """(70, 1037) is the last-lane case beyond four 256-pixel chunks. The plane lies in a parent poisoned with 0x7f, at an odd pitch and offset."""
    from toad_amd import ops
    s = ref.slide(hr, wr, 1)
    region = dev(s, cuda)
    for down in DOWNS:
        for vmin in (0, 16):
            want = ref.saturation_plane(s, down, vmin)
            assert want.shape == (hr // down, wr // down)
            if want.size == 0:                                      # an empty plane: returned empty, nothing launched
                got = ops.region_saturation(region, down, vmin)
                assert tuple(got.shape) == want.shape and got.dtype == torch.uint8
                continue
            parent, view = sat_into_poison(region, down, vmin)
            assert same_plane(view, want), (down, vmin)
            assert only_the_view_was_written(parent, want.shape), (down, vmin)
            assert torch.equal(ops.region_saturation(region, down, vmin), view)
            out_parent, out_view = poisoned_view(want.shape[0], want.shape[1], cuda)
            assert ops.region_saturation(region, down, vmin, out=out_view) is out_view and same_plane(out_view, want)
    if (hr, wr) == (300, 520):
        w = ref.saturation_plane(s, 4)
        assert (w == 0).any() and (w > 100).any() and ((w > 8) & (w < 40)).any()       # glass, pink and the pale blob


# ---- 3. pitch, base and surroundings of the region ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hr,wr,inner,corner", [(67, 131, (2, 3, 1, 5), (1, 4, 0, 0)), (300, 520, (2, 3, 1, 6), (2, 5, 0, 0))])
def test_pitched_region_views_give_the_plane_of_the_contiguous_copy(cuda, hr, wr, inner, corner):
    """The region inside a parent of saturated red, at an odd base address with an odd pitch; then in the parent's last rows and columns, so that its final
    row ends where the allocation ends. A byte read outside the view and summed into a box would show: red is S = 255."""
    s = ref.slide(hr, wr, 1)
    for top, left, bottom, right in (inner, corner):
        v = embedded(s, top, left, bottom, right, cuda)
        assert v.stride(0) % 2 == 1 and v.data_ptr() % 2 == 1
        if (bottom, right) == (0, 0):
            assert v.storage_offset() + (hr - 1) * v.stride(0) + 3 * wr == v.untyped_storage().nbytes()
        for down in DOWNS:
            want = ref.saturation_plane(s, down, 0)
            parent, view = sat_into_poison(v, down, 0)
            assert same_plane(view, want) and only_the_view_was_written(parent, want.shape), (top, left, down)


# ---- 4. the median and its histogram ------------------------------------------------------------------------------------------------------------------------
def median_contents(hp, wp):
    rng = np.random.default_rng(hp * 1000 + wp)
    y, x = np.mgrid[0:hp, 0:wp]
    return {"random": rng.integers(0, 256, size=(hp, wp)), "constant": np.full((hp, wp), 201), "checkerboard": 255 * ((x + y) % 2),
            "ties": rng.choice(np.array([0, 7, 8, 255]), size=(hp, wp)), "ramp": (y * 37 + 5) % 256}


@pytest.mark.gpu
@pytest.mark.parametrize("hp,wp", [(1, 1), (1, 7), (2, 3), (3, 300), (67, 259), (130, 64)])
def test_median_planes_and_histograms_equal_the_reference(cuda, hp, wp):
    from toad_amd import _lib, ops
    lib = _lib.load()
    for name, plane in median_contents(hp, wp).items():
        src_parent, src = poisoned_view(hp, wp, cuda, top=2, left=5)
        src.copy_(dev(plane.astype(np.uint8), cuda))
        for k in MEDIANS:
            want = ref.median_plane(plane, k)
            dst_parent, dst = poisoned_view(hp, wp, cuda)
            hist = torch.full((256,), POISON32, dtype=torch.int32, device=cuda)       # garbage: the launcher zeroes it
            _lib.check(lib.toad_plane_median_u8(src.data_ptr(), pitch_of(src), hp, wp, k, dst.data_ptr(), pitch_of(dst), hist.data_ptr(), stream()),
                       "toad_plane_median_u8")
            assert same_plane(dst, want), (name, k)
            assert only_the_view_was_written(dst_parent, (hp, wp)), (name, k)
            h = hist.cpu().numpy().astype(np.int64)
            assert np.array_equal(h, np.bincount(want.ravel(), minlength=256)) and h.sum() == hp * wp, (name, k)
            # a second call into the histogram as it stands gives the same histogram; and no histogram at all is fine
            dst2_parent, dst2 = poisoned_view(hp, wp, cuda)
            _lib.check(lib.toad_plane_median_u8(src.data_ptr(), pitch_of(src), hp, wp, k, dst2.data_ptr(), pitch_of(dst2), hist.data_ptr(), stream()),
                       "toad_plane_median_u8")
            assert np.array_equal(hist.cpu().numpy().astype(np.int64), h) and torch.equal(dst2, dst)
            m, hh = ops.plane_median(src, k, want_hist=True)
            assert m.is_contiguous() and torch.equal(m, dst) and torch.equal(hh, hist)
            assert torch.equal(ops.plane_median(src, k), dst)
        assert only_the_view_was_written(src_parent, (hp, wp), top=2, left=5) and same_plane(src, plane.astype(np.int64))      # the source is untouched
    with pytest.raises(RuntimeError, match="overlap"):
        lib_rc = lib.toad_plane_median_u8(src.data_ptr(), pitch_of(src), hp, wp, 3, src.data_ptr(), pitch_of(src), None, stream())
        _lib.check(lib_rc, "toad_plane_median_u8")


# ---- 5. plane cells ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hp,wp", [(1, 1), (5, 7), (67, 131), (300, 520)])
def test_plane_cell_counts_equal_the_reference_and_every_element_is_written(cuda, hp, wp):
    from toad_amd import _lib, ops
    rng = np.random.default_rng(hp + wp)
    plane = np.where(rng.random((hp, wp)) < 0.5, rng.integers(0, 256, size=(hp, wp)), rng.choice(np.array([0, 8, 9, 254, 255]), size=(hp, wp)))
    parent, view = poisoned_view(hp, wp, cuda, top=2, left=5)
    view.copy_(dev(plane.astype(np.uint8), cuda))
    for cell in CELLS:
        for thresh in (0, 8, 254, 255):
            want = ref.plane_cell_counts(plane, cell, thresh)
            counts = torch.full(want.shape, POISON32, dtype=torch.int32, device=cuda)
            _lib.check(_lib.load().toad_plane_cells_u8(view.data_ptr(), pitch_of(view), hp, wp, cell, thresh, counts.data_ptr(), stream()),
                       "toad_plane_cells_u8")
            assert same_counts(counts, want), (cell, thresh)
            assert torch.equal(ops.plane_cells(view, cell, thresh), counts)
            assert thresh < 255 or not want.any()                   # nothing is above 255
    # a plane that ends where its allocation ends
    flat = dev(plane.astype(np.uint8), cuda)
    assert same_counts(ops.plane_cells(flat, 4, 8), ref.plane_cell_counts(plane, 4, 8))


# ---- 6. segmented_tissue_origins ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down,median", E2E_DM)
def test_segmented_tissue_origins_equal_the_reference_selection(cuda, down, median):
    from toad_amd import ops
    from toad_amd.tissue import segment_tissue, segmented_tissue_origins
    key = (300, 520, 1)
    s = ref.slide(*key)
    region = dev(s, cuda)
    ran = 0
    for lat in E2E_LATTICES:
        if not lattice_allowed(lat, down):
            continue
        tile, stride, origin = lat
        for sat in E2E_SAT:
            plane_ref, t_ref = ref.segmented(s, down, median, sat, key=key)
            plane, t = segment_tissue(region, down, median, sat)
            assert same_plane(plane, plane_ref) and t == t_ref and isinstance(t, int)
            for f in E2E_FRACTIONS:
                want, total, _ = ref.selection(s, tile, stride, origin, f, down, median, sat, key=key)
                got, counts, thr = segmented_tissue_origins(region, tile, stride, min_fraction=f, down=down, median=median, sat_thresh=sat, origin=origin,
                                                            return_counts=True, return_threshold=True)
                assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (lat, sat, f)
                assert thr == t_ref
                tc = ref.tile_counts(plane_ref, t_ref, tile, stride, origin, down, (300, 520))
                assert counts.dtype == np.int64 and np.array_equal(counts, tc[(got[:, 1] - origin[1]) // stride[0], (got[:, 0] - origin[0]) // stride[1]])
                assert ops.check_origins(got, 300, 520, *tile).tolist() == want.tolist()          # the region calls take them unchanged
                assert np.array_equal(segmented_tissue_origins(region, tile, stride, min_fraction=f, down=down, median=median, sat_thresh=sat,
                                                               origin=origin), got)                # run to run, and the bare result
            ran += 1
    assert ran == 6
    # a pitched view; val_min; a region smaller than the tile
    tile, stride, origin = E2E_LATTICES[0]
    want, _, _ = ref.selection(s, tile, stride, origin, 0.25, down, median, 8, key=key)
    assert np.array_equal(segmented_tissue_origins(embedded(s, 2, 3, 1, 6, cuda), tile, stride, down=down, median=median), want)
    want16, _, _ = ref.selection(s, tile, stride, origin, 0.25, down, median, 8, val_min=16, key=key)
    assert np.array_equal(segmented_tissue_origins(region, tile, stride, down=down, median=median, val_min=16), want16)
    small = segmented_tissue_origins(region[:60], 64, down=down, median=median)
    assert small.shape == (0, 2) and small.dtype == np.int64


@pytest.mark.gpu
def test_segmented_tissue_origins_at_the_defaults(cuda):
    """down = 16, median = 7, sat_thresh = 8 on a 1024 x 2048 slide, 256 x 256 tiles: CLAM's defaults."""
    from toad_amd.tissue import segmented_tissue_origins
    key = (1024, 2048, 2)
    s = ref.slide(*key)
    region = dev(s, cuda)
    want, total, _ = ref.selection(s, (256, 256), (256, 256), (0, 0), 0.25, 16, 7, 8, key=key)
    assert total == 32 and 0 < len(want) < total
    assert np.array_equal(segmented_tissue_origins(region), want)
    want_o, _, t = ref.selection(s, (256, 256), (128, 128), (0, 0), 0.25, 16, 7, "otsu", key=key)
    got, thr = segmented_tissue_origins(region, 256, 128, sat_thresh="otsu", return_threshold=True)
    assert thr == t == 57 and np.array_equal(got, want_o)


# ---- 7. the behaviour users want ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dust_on_glass_is_not_tissue_after_the_median(cuda):
    from toad_amd.tissue import segmented_tissue_origins, tissue_origins
    region = dev(ref.dusty_glass(256, 256, 1), cuda)
    assert len(tissue_origins(region, 64, min_fraction=1 / 64)) == 16                 # one red pixel in 64: every tile passes the per-pixel predicate
    assert len(segmented_tissue_origins(region, 64, min_fraction=1 / 64, down=1, median=1, sat_thresh=8)) == 16
    assert segmented_tissue_origins(region, 64, min_fraction=1 / 64, down=1, median=3, sat_thresh=8).shape == (0, 2)


# ---- 8. through the pipeline ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eval_calls_select_with_the_segment_keyword(cuda):
    from toad_amd.eval import region_attention_scores, region_tissue_attention_heatmap, region_tissue_attention_scores
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
    s = ref.slide(*key)
    region = dev(s, cuda)
    tile = stride = (16, 256)
    # segment=None is the call without the keyword
    o0, s0, c0 = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride)
    o1, s1, c1 = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, segment=None)
    assert np.array_equal(o0, o1) and torch.equal(s0, s1) and torch.equal(c0, c1)
    assert np.array_equal(o0, ref0.selection(s, tile, stride, (0, 0), 0.25, 8, 0)[0])
    # a dict selects with segmented_tissue_origins
    seg = dict(down=4, median=3, sat_thresh="otsu")
    want, total, _ = ref.selection(s, tile, stride, (0, 0), 0.25, 4, 3, "otsu", key=key)
    assert total == 12 and 0 < len(want) < total
    origins, scores, canvas = region_tissue_attention_heatmap(extractor, mil, region, tile=tile, stride=stride, segment=seg)
    assert np.array_equal(origins, want) and np.array_equal(origins, segmented_tissue_origins(region, tile, stride, **seg))
    assert torch.equal(scores, region_attention_scores(extractor, mil, region, origins, tile=tile, percentile=True))
    assert torch.equal(canvas, attention_canvas(region, origins, scores, tile=tile, stride=stride))
    o2, s2 = region_tissue_attention_scores(extractor, mil, region, tile=tile, stride=stride, segment=seg)
    assert np.array_equal(o2, want) and torch.equal(s2, region_attention_scores(extractor, mil, region, want, tile=tile))
    # keys the dict leaves out take the call's own sat_thresh / val_min
    o3, s3 = region_tissue_attention_scores(None, None, region, tile=tile, stride=stride, sat_thresh=255, segment=dict(down=4, median=3))
    assert o3.shape == (0, 2) and s3.shape == (0,) and s3.device == region.device
