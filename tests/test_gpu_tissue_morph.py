"""GPU: closing, connected components with areas, and the two area selections on a plane of bytes (csrc/tissue_morph.hip plane_close_kernel<C>,
cc_local_kernel, cc_seam_kernel, cc_flatten_kernel, area_select_kernel; the close / min_area / min_hole keywords of toad_amd/tissue.py and of the segment=
dict of the eval calls). Everything is defined in integers and the labelling is canonical, so every comparison is exact, against the numpy reference of
tests/tissue_morph_ref.py (tested on its own, on these very inputs, in test_tissue_morph_host.py - that every stage acts on every end-to-end case is a
fact about that reference, asserted there). The kernels' tile is 64 x 16: (130, 257) is eight tiles and two rows by four tiles and one column."""
import functools

import numpy as np
import pytest
import torch

from tests import tissue_morph_ref as ref

SHAPES = ((1, 1), (1, 200), (200, 1), (63, 65), (129, 131), (130, 257))
POISON8 = 0x7F
POISON32 = 0x7F7F7F7F
THRESH = 8


def dev(a: np.ndarray, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                   # a copy: the cached inputs are read-only


def stream():
    return torch.cuda.current_stream().cuda_stream


def poisoned_view(hp, wp, cuda, top=1, left=2):
    """(parent, view): a uint8 [hp,wp] view at an odd pitch and an odd offset inside a parent filled with 0x7f."""
    width = wp + left + 2
    width += 1 - width % 2                                           # an odd pitch
    parent = torch.full((hp + top + 2, width), POISON8, dtype=torch.uint8, device=cuda)
    view = parent[top:top + hp, left:left + wp]
    assert view.stride(0) % 2 == 1 and view.stride(1) == 1 and view.data_ptr() % 2 == 1
    return parent, view


def untouched_outside(parent, view_shape, top=1, left=2) -> bool:
    p = parent.clone()
    p[top:top + view_shape[0], left:left + view_shape[1]] = POISON8
    return bool((p == POISON8).all())


def pitch_of(view):
    return view.stride(0) if view.shape[0] > 1 else max(view.stride(0), view.shape[1])


def plane_of(m: np.ndarray, seed: int) -> np.ndarray:
    """A uint8 plane whose pixels > THRESH are exactly m: values 9 .. 255 on m and 0 .. 8 elsewhere, so the comparison at the threshold is exercised."""
    rng = np.random.default_rng(seed)
    return np.where(m, rng.integers(THRESH + 1, 256, size=m.shape), rng.integers(0, THRESH + 1, size=m.shape)).astype(np.uint8)


def source_view(plane: np.ndarray, cuda):
    parent, view = poisoned_view(plane.shape[0], plane.shape[1], cuda, top=2, left=5)
    view.copy_(dev(plane, cuda))
    return parent, view


@functools.lru_cache(maxsize=None)
def reference_components(hp, wp, name, background):
    m = ref.patterns(hp, wp)[name]
    labels, area = ref.components(~m if background else m, 4 if background else 8)
    labels.setflags(write=False)
    area.setflags(write=False)
    return labels, area


def same_mask(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want.astype(np.uint8) * 255)


# ---- 1. components ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hp,wp", SHAPES)
def test_components_labels_and_areas_equal_the_reference(cuda, hp, wp):
    """Every pattern in both polarities, whole arrays compared; labels and area start as 0x7f7f7f7f, so an element the call left alone would show. The
    plane is an odd-pitch, odd-offset view of a poisoned parent that must come back unchanged."""
    from toad_amd import _lib, ops
    lib = _lib.load()
    for i, (name, m) in enumerate(ref.patterns(hp, wp).items()):
        plane = plane_of(m, i)
        parent, view = source_view(plane, cuda)
        before = parent.clone()
        for background in (0, 1):
            want_l, want_a = reference_components(hp, wp, name, background)
            labels = torch.full((hp, wp), POISON32, dtype=torch.int32, device=cuda)
            area = torch.full((hp * wp,), POISON32, dtype=torch.int32, device=cuda)
            _lib.check(lib.toad_plane_components_u8(view.data_ptr(), pitch_of(view), hp, wp, THRESH, background, labels.data_ptr(), area.data_ptr(), stream()),
                       "toad_plane_components_u8")
            got_l, got_a = labels.cpu().numpy().astype(np.int64), area.cpu().numpy().astype(np.int64)
            assert np.array_equal(got_l, want_l), (name, background)
            assert np.array_equal(got_a, want_a), (name, background)
            l2, a2 = ops.plane_components(view, THRESH, background)
            assert l2.dtype == torch.int32 and tuple(l2.shape) == (hp, wp) and torch.equal(l2, labels) and torch.equal(a2, area)      # run to run as well
            l3, a3 = ops.plane_components(view, THRESH, background, workspace=True)
            assert torch.equal(l3, labels) and torch.equal(a3, area)
        assert torch.equal(parent, before), name                      # the plane and its surroundings are only read


# ---- 2. closing ------------------------------------------------------------------------------------------------------------------------------------------------
def closing_inputs(hp, wp):
    rng = np.random.default_rng(hp * 1000 + wp)
    ends = np.zeros((hp, wp), dtype=bool)                             # the plane's corners, and one pixel next to each: the clipped windows
    ends[0, 0] = ends[0, -1] = ends[-1, 0] = ends[-1, -1] = True
    ends[min(1, hp - 1), min(2, wp - 1)] = ends[max(hp - 3, 0), max(wp - 2, 0)] = True
    return {"random0.5": rng.random((hp, wp)) < 0.5, "random0.1": rng.random((hp, wp)) < 0.1, "random0.9": rng.random((hp, wp)) < 0.9,
            "serpentine": ref.serpentine(hp, wp), "corners of the plane": ends}


@pytest.mark.gpu
@pytest.mark.parametrize("hp,wp", SHAPES)
def test_closing_equals_the_reference_and_nothing_else_is_written(cuda, hp, wp):
    from toad_amd import _lib, ops
    lib = _lib.load()
    for i, (name, m) in enumerate(closing_inputs(hp, wp).items()):
        parent, view = source_view(plane_of(m, i), cuda)
        before = parent.clone()
        for c in ref.CLOSES:
            want = ref.closing(m, c)
            dst_parent, dst = poisoned_view(hp, wp, cuda)
            _lib.check(lib.toad_plane_close_u8(view.data_ptr(), pitch_of(view), hp, wp, THRESH, c, dst.data_ptr(), pitch_of(dst), stream()), "toad_plane_close_u8")
            assert same_mask(dst, want), (name, c)
            assert untouched_outside(dst_parent, (hp, wp)), (name, c)
            out = ops.plane_close(view, c, THRESH)
            assert out.is_contiguous() and torch.equal(out, dst), (name, c)
        assert torch.equal(parent, before), name
    with pytest.raises(RuntimeError, match="overlap"):
        _lib.check(lib.toad_plane_close_u8(view.data_ptr(), pitch_of(view), hp, wp, THRESH, 3, view.data_ptr(), pitch_of(view), stream()), "toad_plane_close_u8")
    assert torch.equal(parent, before)


# ---- 3. the selections -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hp,wp", [(63, 65), (130, 257)])
def test_area_selections_equal_the_reference_at_the_edges_of_the_limit(cuda, hp, wp):
    """Both modes on the labels of a field near the percolation threshold; limits 0 and 1, a component size that occurs and that size + 1 (the >= and the <
    edge), and a limit above every count."""
    from toad_amd import _lib
    lib = _lib.load()
    for mode, background in ((0, 0), (1, 1)):
        labels_np, area_np = reference_components(hp, wp, "random0.593", background)
        counts = area_np[area_np > 0]
        inner = np.sort(counts[counts < ref.BORDER]) if mode else np.sort(counts & ref.COUNT)
        sizes = np.unique(inner[(inner > 1) & (inner < int((counts & ref.COUNT).max()))])
        size = int(sizes[len(sizes) // 2])                          # a size that occurs, with components below and above it
        labels, area = dev(labels_np.astype(np.int32), cuda), dev(area_np.astype(np.int32), cuda)
        outs = []
        for limit in (0, 1, size, size + 1, int((counts & ref.COUNT).max()) + 1, 1 << 30):
            want = ref.area_select(labels_np, area_np, mode, limit)
            parent, dst = poisoned_view(hp, wp, cuda)
            _lib.check(lib.toad_plane_area_select_u8(labels.data_ptr(), area.data_ptr(), hp, wp, mode, limit, dst.data_ptr(), pitch_of(dst), stream()),
                       "toad_plane_area_select_u8")
            assert same_mask(dst, want), (mode, limit)
            assert untouched_outside(parent, (hp, wp)), (mode, limit)
            outs.append(int(want.sum()))
        assert outs[2] != outs[3]                                    # the edge is there: a component of exactly `size` pixels flips between the two limits
        if mode == 0:
            assert outs[0] == outs[1] == int((labels_np >= 0).sum()) and outs[4] == 0
        else:
            assert outs[0] == int((labels_np < 0).sum()) and outs[0] == outs[1] and outs[4] == outs[5] > outs[0]


@pytest.mark.gpu
def test_the_wrappers_chain_as_the_stages_do(cuda):
    """plane_close -> plane_components -> plane_area_select, twice, by hand: steps 6a to 6c on a random plane, against the reference's stages."""
    from toad_amd import ops
    m0 = ref.random_field(129, 131, 0.25, 9)
    view = source_view(plane_of(m0, 9), cuda)[1]
    m1 = ref.closing(m0, 2)
    m2 = ref.drop_small(m1, 40)
    m3 = ref.fill_holes(m2, 6)
    assert (m1 != m0).any() and (m2 != m1).any() and (m3 != m2).any() and m2.any()
    d1 = ops.plane_close(view, 2, THRESH)
    d2 = ops.plane_area_select(*ops.plane_components(d1, 0, 0), 0, 40)
    d3 = ops.plane_area_select(*ops.plane_components(d2, 0, 1), 1, 6)
    assert same_mask(d1, m1) and same_mask(d2, m2) and same_mask(d3, m3)
    # without the closing the components read the plane with its threshold directly
    assert same_mask(ops.plane_area_select(*ops.plane_components(view, THRESH, 0), 0, 40), ref.drop_small(m0, 40))


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("down,median", ref.E2E_DM)
def test_segmented_selection_with_closing_and_area_filters_equals_the_reference(cuda, down, median):
    from toad_amd import ops
    from toad_amd.tissue import segment_tissue, segmented_tissue_origins
    key = ref.E2E_KEY
    s = ref.holey_slide(*key)
    region = dev(s, cuda)
    tile, stride, origin = ref.E2E_LATTICE
    for sat in ref.E2E_SAT:
        plain, t_plain = segment_tissue(region, down, median, sat)
        for close, min_area, min_hole in ref.e2e_configs(down):
            kw = dict(close=close, min_area=min_area, min_hole=min_hole)
            m3 = ref.mask(None, down, median, sat, 0, key=key, **kw)
            want, counts_ref, t_ref = ref.selection(None, tile, stride, origin, 0.25, down, median, sat, 0, key=key, **kw)
            mask, zero, t = segment_tissue(region, down, median, sat, return_threshold=True, **kw)
            assert same_mask(mask, m3) and zero == 0 and t == t_ref == t_plain and isinstance(t, int), (sat, kw)
            assert segment_tissue(region, down, median, sat, **kw)[1] == 0
            got, counts, thr = segmented_tissue_origins(region, tile, stride, down=down, median=median, sat_thresh=sat, origin=origin, return_counts=True,
                                                        return_threshold=True, **kw)
            assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (sat, kw)
            assert thr == t_ref
            assert counts.dtype == np.int64 and np.array_equal(counts, counts_ref[(got[:, 1] - origin[1]) // stride[0], (got[:, 0] - origin[0]) // stride[1]])
            assert ops.check_origins(got, 300, 520, *tile).tolist() == want.tolist()
        # the inactive values are today's call: the same plane, the same threshold
        again, t_again = segment_tissue(region, down, median, sat, close=1, min_area=1, min_hole=0)
        assert torch.equal(again, plain) and t_again == t_plain


@pytest.mark.gpu
def test_eval_calls_take_the_three_keywords_in_segment(cuda):
    from toad_amd.eval import region_attention_scores, region_tissue_attention_scores
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    key = ref.E2E_KEY
    region = dev(ref.holey_slide(*key), cuda)
    tile = stride = (64, 64)
    seg = dict(down=1, median=3, close=4, min_area=ref.E2E_MIN_AREA, min_hole=ref.E2E_MIN_HOLE)
    want, counts, _ = ref.selection(None, tile, stride, (0, 0), 0.25, 1, 3, 8, 0, 4, ref.E2E_MIN_AREA, ref.E2E_MIN_HOLE, key=key)
    unfiltered, _, _ = ref.selection(None, tile, stride, (0, 0), 0.25, 1, 3, 8, 0, key=key)
    assert 0 < len(want) < counts.size and not np.array_equal(want, unfiltered)
    origins, scores = region_tissue_attention_scores(extractor, mil, region, tile=tile, stride=stride, segment=seg)
    assert np.array_equal(origins, want)
    assert torch.equal(scores, region_attention_scores(extractor, mil, region, want, tile=tile))
