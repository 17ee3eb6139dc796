"""GPU: the extractor's region calls with shrink = 2 - a tile is a (2 H, 2 W) footprint of the region, box-filtered to the (H, W) network tile while it is
read (csrc/stem_halo.inc box form, csrc/conv.hip tiles_u8_nhwc_to_nchw_kernel<true, 2>, ResNet_Baseline.forward_u8_region(shrink=2), the eval.region_*
calls). Every comparison is bitwise against the existing uint8 call on ops.box_tiles_u8(region, origins, tile, 2), the tiles materialised with torch integer
ops (tests/test_extractor_shrink_host.py checks that function against the formula): padding is the tile's, nothing outside the footprints is read, and no
tile copy exists on the new route."""
import numpy as np
import pytest
import torch

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
IDENTITY = ((0.0, 0.0, 0.0), (1.0 / 255.0,) * 3)

# 2 x 2 boxes (a b / c d) with the sums 0, 1, 2, 3, 509, 510, 1018, 1020: all residues mod 4, the half-up rounding and the top of the range
BOXES = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 1), (255, 254, 0, 0), (255, 0, 255, 0), (255, 255, 254, 254), (255, 255, 255, 255)]

# the 39 x 1043 region (pitch 3129 B, odd) with (16, 512) footprints = (8, 256) network tiles: both parities of x and of y, the tiles that touch the right
# and the bottom edge exactly, a duplicate, overlaps at odd offsets, an order that is not monotone; 9 tiles x 2 row pairs, so workgroup ranges begin
# inside a tile
ORIGINS_16x512 = [(0, 0), (1, 0), (2, 3), (3, 5), (531, 23), (2, 3), (0, 23), (531, 0), (257, 7)]
ORIGINS_512 = [(0, 0), (528, 88), (263, 13)]                  # 512 x 512 footprints in the 600 x 1040 region


def make_region(hr, wr, seed):
    """Uniform random uint8 [hr,wr,3] whose second quarter of rows is all 0, third all 255 and fourth the ramp x + 3 y + 85 c (a swapped row, column or
    channel shows); the first quarter stays random, except that its rows 0, 1 begin with the BOXES (box i at columns 2 i, 2 i + 1, channel c holding box
    (i + c) % 8), repeated along the row as often as they fit into its first half: a tile at an even origin there sees every rounding case."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 256, (hr, wr, 3), generator=g, dtype=torch.uint8)
    ramp = (torch.arange(wr).view(1, wr, 1) + 3 * torch.arange(hr).view(hr, 1, 1) + 85 * torch.arange(3).view(1, 1, 3)).remainder(256).to(torch.uint8)
    q = hr // 4
    r[q:2 * q] = 0; r[2 * q:3 * q] = 255; r[3 * q:] = ramp[3 * q:]
    n = len(BOXES)
    for i in range(wr // 4):
        for c in range(3):
            a, b, cc, d = BOXES[(i + c) % n]
            r[0, 2 * i, c], r[0, 2 * i + 1, c], r[1, 2 * i, c], r[1, 2 * i + 1, c] = a, b, cc, d
    return r


def pitched_view(region, top, left, bottom, right):
    """The same pixels as rows [top, top + Hr) x columns [left, left + Wr) of a wider, taller image filled with other bytes: a pitch above 3 Wr and a base
    at byte offset top * pitch + 3 * left."""
    hr, wr, _ = region.shape
    wide = torch.full((hr + top + bottom, wr + left + right, 3), 77, dtype=torch.uint8, device=region.device)
    v = wide[top:top + hr, left:left + wr]
    v.copy_(region)
    assert not v.is_contiguous() and v.stride() == (3 * (wr + left + right), 3, 1)
    return v


def boxed(region, origins, tile):
    from toad_amd import ops
    return ops.box_tiles_u8(region, origins, tile, 2)


# ---- the stem, 256-wide route ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stem_weights(cuda):
    g = torch.Generator().manual_seed(4242)
    wt = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    w8 = torch.zeros(64, 3, 8, 8); w8[:, :, 1:, 1:] = wt
    wf = w8.view(64, 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(64, 192).contiguous().to(cuda)
    return wf, torch.randn(64, generator=g).to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
@pytest.mark.parametrize("case", ["odd_pitch", "view_odd_base", "h256"])
def test_stem_with_shrink_is_bitwise_the_stem_on_the_box_filtered_tiles(cuda, stem_weights, case, norm):
    from toad_amd import ops
    wf, bias = stem_weights
    if case == "h256":
        region, origins, fp = make_region(600, 1040, 3).to(cuda), ORIGINS_512, (512, 512)
    else:
        region, origins, fp = make_region(39, 1043, 1).to(cuda), ORIGINS_16x512, (16, 512)
        if case == "view_odd_base":                                # wide[1:40, 3:1046] of a 41 x 1052 image: pitch 3156, base at byte 3165
            region = pitched_view(region, 1, 3, 1, 6)
            assert region.stride(0) == 3156 and region.data_ptr() % 2 == 1
        else:
            assert region.stride(0) == 3129
    h = fp[0] // 2
    tiles = boxed(region, origins, fp)
    assert tiles.shape == (len(origins), h, 256, 3)
    want = ops.stem_pool_nhwc_u8(tiles, wf, bias, *norm)
    got = ops.stem_pool_region_u8(region, origins, wf, bias, fp, *norm, shrink=2)
    assert got.shape == (len(origins), h // 4, 64, 64) and torch.equal(got, want)
    assert torch.equal(got, ops.stem_pool_region_u8(region, torch.tensor(origins), wf, bias, fp, *norm, shrink=2))       # run to run; origins as a CPU tensor
    assert float(want.abs().max()) > 0
    # the box filter is not the identity here: the stem on the footprint's even pixels differs
    assert not torch.equal(tiles, torch.stack([region[y:y + fp[0]:2, x:x + fp[1]:2] for x, y in origins]))


@pytest.mark.gpu
def test_padding_is_the_tiles_not_the_regions(cuda, stem_weights):
    """A region of 255s: the footprint at (100, 4) has 255s on every side, and the tile's border taps must still be 0 in normalised space."""
    from toad_amd import ops
    wf, bias = stem_weights
    region = torch.full((32, 1024, 3), 255, dtype=torch.uint8, device=cuda)
    alone = torch.full((1, 8, 256, 3), 255, dtype=torch.uint8, device=cuda)
    for norm in (IMAGENET, IDENTITY):
        want = ops.stem_pool_nhwc_u8(alone, wf, bias, *norm)
        assert torch.equal(ops.stem_pool_region_u8(region, [(100, 4)], wf, bias, (16, 512), *norm, shrink=2), want)
        assert not torch.equal(want[0, :, 0], want[0, :, 30])      # the standalone tile's border column is not its interior: the padding shows in `want`


@pytest.mark.gpu
def test_nothing_outside_the_footprints_decides_anything(cuda, stem_weights):
    """Two regions that agree inside the footprints and differ in every other byte give the same results, on the stem route and on the staged one."""
    from toad_amd import ops
    wf, bias = stem_weights
    for (hr, wr), fp, origins in (((39, 1043), (16, 512), [(1, 2), (530, 21), (3, 21)]), ((40, 62), (14, 18), [(1, 3), (43, 25), (20, 9)])):
        a = make_region(hr, wr, 21)
        inside = torch.zeros(hr, wr, dtype=torch.bool)
        for x, y in origins:
            inside[y:y + fp[0], x:x + fp[1]] = True
        b = torch.where(inside.unsqueeze(2), a, 255 - a)                       # every byte outside differs (255 - v != v)
        assert bool((a != b).any(dim=2)[~inside].all()) and torch.equal(a[inside], b[inside]) and not bool(inside.all())
        a, b = a.to(cuda), b.to(cuda)
        got_a, got_b = (ops.tiles_u8_region_to_f32(r, origins, fp, *IDENTITY, shrink=2) for r in (a, b))
        assert torch.equal(got_a, got_b) and torch.equal(got_a, boxed(a, origins, fp).permute(0, 3, 1, 2).float())
        if fp[1] == 512:
            assert torch.equal(ops.stem_pool_region_u8(a, origins, wf, bias, fp, shrink=2), ops.stem_pool_region_u8(b, origins, wf, bias, fp, shrink=2))


# ---- rounding on the device; the conversion op, staged shapes -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("h,w,hr,wr", [(7, 9, 40, 62), (40, 300, 128, 666), (8, 256, 39, 1043)])
def test_conversion_with_shrink_is_the_rounded_box_mean(cuda, h, w, hr, wr, pitched):
    from toad_amd import ops
    region = make_region(hr, wr, hr + wr).to(cuda)
    if pitched:
        region = pitched_view(region, 2, 5, 1, 2)                  # base at an odd byte offset (2 * pitch + 15), pitch 3 (wr + 7)
    fp = (2 * h, 2 * w)
    fh, fw = fp
    origins = [(wr - fw, hr - fh), (0, 0), (wr - fw, 0), (0, hr - fh), ((wr - fw) // 2 + 1, (hr - fh) // 2), (1, 1)]      # the far corners, both parities
    tiles = boxed(region, origins, fp)
    got = ops.tiles_u8_region_to_f32(region, origins, fp, *IDENTITY, shrink=2)
    assert got.shape == (6, 3, h, w) and got.dtype == torch.float32 and torch.equal(got, tiles.permute(0, 3, 1, 2).float())
    # the tile at (0, 0) holds the eight rounding cases in its first row, on every channel
    first = got[1, :, 0, :8].cpu()
    assert torch.equal(first, torch.tensor([[(sum(BOXES[(i + c) % 8]) + 2) // 4 for i in range(8)] for c in range(3)], dtype=torch.float32))
    assert torch.equal(ops.tiles_u8_region_to_f32(region, origins, fp, *IMAGENET, shrink=2), ops.tiles_u8_to_f32(tiles, *IMAGENET))


# ---- shrink = 1 is the call without it ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    return resnet50_baseline().eval().to(cuda)


@pytest.mark.gpu
def test_shrink_1_of_every_entry_and_keyword_is_the_existing_call(cuda, stem_weights, model):
    from toad_amd import _lib as L, ops
    from toad_amd.eval import attention_heatmap_scores, region_attention_scores
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    lib = L.load()
    wf, bias = stem_weights
    region = make_region(39, 1043, 1).to(cuda)
    origins = [(0, 0), (1, 0), (2, 3), (787, 31), (2, 3), (0, 31)]
    org = torch.tensor(origins, dtype=torch.int32, device=cuda)
    B, pitch, stream = len(origins), region.stride(0), torch.cuda.current_stream().cuda_stream
    norm = ops.norm_constants_u8()
    # the keywords
    want_stem = ops.stem_pool_region_u8(region, origins, wf, bias, (8, 256))
    want_conv = ops.tiles_u8_region_to_f32(region, origins, (7, 9))
    want_net = model.forward_u8_region(region, origins, (8, 256))
    want_staged = model.forward_u8_region(region, origins, (7, 9), out_dtype=torch.float16)
    assert torch.equal(ops.stem_pool_region_u8(region, origins, wf, bias, (8, 256), shrink=1), want_stem)
    assert torch.equal(ops.tiles_u8_region_to_f32(region, origins, (7, 9), shrink=1), want_conv)
    assert torch.equal(model.forward_u8_region(region, origins, (8, 256), shrink=1), want_net)
    assert torch.equal(model.forward_u8_region(region, origins, (7, 9), out_dtype=torch.float16, shrink=1), want_staged)
    assert torch.equal(ops.box_tiles_u8(region, origins, (8, 256), 1), torch.stack([region[y:y + 8, x:x + 256] for x, y in origins]))
    # the C entries
    got = torch.empty_like(want_stem)
    ws = torch.empty(lib.toad_linear_ws_bytes(B * 4 * 128, 64, 192), dtype=torch.uint8, device=cuda)
    L.check(lib.toad_stem_pool_region_box_u8(region.data_ptr(), pitch, 39, 1043, org.data_ptr(), norm, wf.data_ptr(), bias.data_ptr(), got.data_ptr(), B, 8, 256, 1,
                                             ws.data_ptr(), ws.numel(), stream), "toad_stem_pool_region_box_u8")
    assert torch.equal(got, want_stem)
    got = torch.empty_like(want_conv)
    L.check(lib.toad_tiles_u8_region_box_to_nchw_f32(region.data_ptr(), pitch, 39, 1043, org.data_ptr(), norm, got.data_ptr(), B, 7, 9, 1, stream),
            "toad_tiles_u8_region_box_to_nchw_f32")
    assert torch.equal(got, want_conv)
    _, _, wp, bp = model._folded
    for (h, w), want in (((8, 256), want_net), ((7, 9), want_staged)):
        got = torch.empty_like(want)
        ws = torch.empty(lib.toad_resnet50_trunc_u8_ws_bytes(B, h, w), dtype=torch.uint8, device=cuda)
        o32, o16 = (None, got.data_ptr()) if want.dtype == torch.float16 else (got.data_ptr(), None)
        L.check(lib.toad_resnet50_trunc_fwd_u8_region_box(region.data_ptr(), pitch, 39, 1043, org.data_ptr(), norm, wp, bp, o32, o16, B, h, w, 1, ws.data_ptr(), ws.numel(),
                                                          stream), "toad_resnet50_trunc_fwd_u8_region_box")
        assert torch.equal(got, want), (h, w)
    # the pipeline keyword
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    assert torch.equal(region_attention_scores(model, mil, region, origins, tile=(8, 256), shrink=1), region_attention_scores(model, mil, region, origins, tile=(8, 256)))
    assert torch.equal(region_attention_scores(model, mil, region, origins, tile=(8, 256), shrink=1), attention_heatmap_scores(mil, want_net.half(), False))


# ---- the whole network ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["512x512", "16x512", "14x18_staged"])
def test_forward_u8_region_with_shrink_is_bitwise_forward_u8_of_the_box_filtered_tiles(cuda, model, case):
    if case == "512x512":
        region, origins, tile = make_region(600, 1040, 3).to(cuda), ORIGINS_512, 512
    elif case == "16x512":
        region, origins, tile = make_region(39, 1043, 1).to(cuda), ORIGINS_16x512, (16, 512)
    else:
        region, origins, tile = pitched_view(make_region(40, 62, 51).to(cuda), 2, 5, 1, 2), [(44, 26), (0, 0), (44, 0), (0, 26), (23, 11)], (14, 18)
    tiles = boxed(region, origins, tile)
    want = model.forward_u8(tiles)
    got = model.forward_u8_region(region, origins, tile, shrink=2)
    assert got.dtype == torch.float32 and got.shape == (len(origins), 1024) and torch.equal(got, want)
    got16 = model.forward_u8_region(region, origins, tile, out_dtype=torch.float16, shrink=2)
    assert got16.dtype == torch.float16 and torch.equal(got16, model.forward_u8(tiles, out_dtype=torch.float16))
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    half = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                  # the constants are arguments
    assert torch.equal(model.forward_u8_region(region, origins, tile, *half, shrink=2), model.forward_u8(tiles, *half))


@pytest.mark.gpu
def test_forward_u8_region_with_shrink_chunks_by_the_network_tile(cuda, model, monkeypatch):
    """Nine origins with the cap at 4 tiles a call: three chunks into one result; the cap is asked for the NETWORK tile (8, 256), not the footprint."""
    from toad_amd import resnet_custom as rc
    asked = []

    def cap(h, w):
        asked.append((h, w))
        return 4
    region = make_region(39, 1043, 1).to(cuda)
    tiles = boxed(region, ORIGINS_16x512, (16, 512))
    want = model.forward_u8(tiles)
    monkeypatch.setattr(rc, "max_tiles_per_call", cap)
    got = model.forward_u8_region(region, ORIGINS_16x512, (16, 512), shrink=2)
    assert asked == [(8, 256)] and torch.equal(got, want)
    assert torch.equal(model.forward_u8_region(region, np.array(ORIGINS_16x512), (16, 512), out_dtype=torch.float16, shrink=2), want.half())


@pytest.mark.gpu
def test_forward_u8_region_shrink_refusals_on_the_device(cuda, model):
    region = make_region(39, 1043, 1).to(cuda)
    with pytest.raises(ValueError, match=r"origins\[1\]"):     # x + 512 == Wr + 1: the footprint is what has to fit
        model.forward_u8_region(region, [(0, 0), (532, 0)], (16, 512), shrink=2)
    with pytest.raises(ValueError, match=r"origins\[0\]"):     # y + 16 == Hr + 1
        model.forward_u8_region(region, [(0, 24)], (16, 512), shrink=2)
    with pytest.raises(ValueError, match="does not divide"):
        model.forward_u8_region(region, [(0, 0)], (8, 255), shrink=2)
    for bad in (0, 3, 4, True, 2.0):
        with pytest.raises(ValueError, match="shrink must be"):
            model.forward_u8_region(region, [(0, 0)], (16, 512), shrink=bad)


@pytest.mark.gpu
def test_no_tile_copy_on_the_shrink_route(cuda, model):
    """64 footprints of 512 x 512 at stride 128 from an 896 x 1920 region (5.2 MB; the footprints would be 50 MB, the box-filtered tiles 12.6 MB): over a warm
    call the allocator's peak rises by the output rows (256 KB) and the origins (512 B) - less than ONE network tile (196,608 B) above them."""
    region = make_region(896, 1920, 64).to(cuda)
    origins = [(128 * i, 128 * j) for j in range(4) for i in range(12)] + [(128 * i + 3, 383) for i in range(11)] + [(1408, 384)] * 5
    assert len(origins) == 64
    model.forward_u8_region(region, origins, 512, shrink=2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.forward_u8_region(region, origins, 512, shrink=2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak - before < 64 * 1024 * 4 + 64 * 8 + 256 * 256 * 3, (peak, before)
    assert out.shape == (64, 1024)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mil(cuda):
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    torch.manual_seed(3)
    m = TOAD_fc_mtl_concat()
    m.relocate()
    m.eval()
    return m


@pytest.mark.gpu
def test_region_attention_scores_with_shrink_equal_the_scores_of_the_materialised_bag(cuda, model, mil):
    """70 origins of (16, 512) footprints: at least 64 rows, so the fp16 bag takes the _x16 route of the MIL model."""
    from toad_amd.eval import attention_heatmap_scores, region_attention_scores
    region = make_region(39, 1043, 1).to(cuda)
    g = torch.Generator().manual_seed(8)
    origins = ORIGINS_16x512 + [(int(x), int(y)) for x, y in zip(torch.randint(0, 532, (61,), generator=g), torch.randint(0, 24, (61,), generator=g))]
    assert len(origins) == 70
    tiles = boxed(region, origins, (16, 512))
    bag16 = model.forward_u8(tiles, out_dtype=torch.float16)
    for pct in (False, True):
        got = region_attention_scores(model, mil, region, origins, tile=(16, 512), percentile=pct, shrink=2)
        assert got.shape == (70,) and torch.equal(got, attention_heatmap_scores(mil, bag16, pct)), pct
    got32 = region_attention_scores(model, mil, region, origins, tile=(16, 512), bag_dtype=torch.float32, shrink=2)
    assert torch.equal(got32, attention_heatmap_scores(mil, model.forward_u8(tiles), False))
    assert torch.isfinite(got32).all() and float(got32.abs().max()) > 0


@pytest.mark.gpu
def test_tissue_heatmap_of_a_40x_region(cuda, model, mil):
    """A 1024 x 1536 region, white but for a block of random colours: 512-pixel footprints on the 512 / 128 lattice, read at half the pitch; the selection
    and the canvas work on the footprint as they do without a shrink, only the extractor sees it."""
    from toad_amd.eval import attention_heatmap_scores, region_tissue_attention_heatmap, region_tissue_attention_scores
    from toad_amd.tissue import tissue_origins
    g = torch.Generator().manual_seed(40)
    r = torch.full((1024, 1536, 3), 255, dtype=torch.uint8)
    r[200:800, 400:1100] = torch.randint(0, 256, (600, 700, 3), generator=g, dtype=torch.uint8)      # the corner tiles hold 13 % of it: below min_fraction
    region = r.to(cuda)
    origins, scores, canvas = region_tissue_attention_heatmap(model, mil, region, tile=512, stride=128, shrink=2, down=4)
    assert canvas.shape == (256, 384, 3) and canvas.dtype == torch.uint8
    assert origins.shape[1] == 2 and 0 < origins.shape[0] < 5 * 9 and scores.shape == (origins.shape[0],)
    assert (origins % 128 == 0).all() and origins[:, 0].max() <= 1024 and origins[:, 1].max() <= 512
    assert np.array_equal(origins, tissue_origins(region, tile=512, stride=128))                               # the selection does not know of the shrink
    want = attention_heatmap_scores(mil, model.forward_u8(boxed(region, origins, 512), out_dtype=torch.float16), True)
    assert torch.equal(scores, want)
    o2, s2 = region_tissue_attention_scores(model, mil, region, tile=512, stride=128, shrink=2, percentile=True)
    assert np.array_equal(o2, origins) and torch.equal(s2, want)
    # the canvas: coloured where a tile was selected, the box-filtered white of the region elsewhere
    assert bool((canvas[:8, :8] == 255).all()) and not bool((canvas == 255).all())
