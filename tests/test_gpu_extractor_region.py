"""GPU: tiles read by origin from one decoded uint8 region (csrc/stem_halo.inc region form, csrc/conv.hip tiles_u8_nhwc_to_nchw_kernel<true>,
ResNet_Baseline.forward_u8_region, eval.region_attention_scores). Every comparison is bitwise against the existing route on the tiles materialised with
torch.stack([region[y:y+H, x:x+W] for x, y in origins]): padding is the tile's, not the region's, and no tile copy exists on the new route."""
import pytest
import torch

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
IDENTITY = ((0.0, 0.0, 0.0), (1.0 / 255.0,) * 3)

# the 23 x 531 region (pitch 1593 B, odd) with (8, 256) tiles: both parities of x and of y * pitch, the two tiles that touch the right and the bottom edge
# exactly, a duplicate, overlaps, an order that is not monotone; 7 tiles x 2 row pairs, so workgroup ranges begin inside a tile
ORIGINS_8x256 = [(0, 0), (1, 0), (2, 3), (3, 5), (275, 15), (2, 3), (0, 15)]
ORIGINS_256 = [(0, 0), (264, 44), (131, 7)]                   # 256 x 256 in the 300 x 520 region


def make_region(hr, wr, seed):
    """Uniform random uint8 [hr,wr,3] whose second quarter of rows is all 0, third all 255 and fourth the ramp x + 3 y + 85 c (a swapped row, column or
    channel shows); the first quarter stays random."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 256, (hr, wr, 3), generator=g, dtype=torch.uint8)
    ramp = (torch.arange(wr).view(1, wr, 1) + 3 * torch.arange(hr).view(hr, 1, 1) + 85 * torch.arange(3).view(1, 1, 3)).remainder(256).to(torch.uint8)
    q = hr // 4
    r[q:2 * q] = 0; r[2 * q:3 * q] = 255; r[3 * q:] = ramp[3 * q:]
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


def stacked(region, origins, h, w):
    return torch.stack([region[y:y + h, x:x + w] for x, y in origins])


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
def test_stem_by_origin_is_bitwise_the_stem_on_the_stacked_tiles(cuda, stem_weights, case, norm):
    from toad_amd import ops
    wf, bias = stem_weights
    if case == "h256":
        region, origins, h = make_region(300, 520, 3).to(cuda), ORIGINS_256, 256
    else:
        region, origins, h = make_region(23, 531, 1).to(cuda), ORIGINS_8x256, 8
        if case == "view_odd_base":                                # wide[1:24, 3:534] of a 25 x 540 image: pitch 1620, base at byte 1629
            region = pitched_view(region, 1, 3, 1, 6)
            assert region.stride(0) == 1620 and region.data_ptr() % 2 == 1
        else:
            assert region.stride(0) == 1593
    want = ops.stem_pool_nhwc_u8(stacked(region, origins, h, 256), wf, bias, *norm)
    got = ops.stem_pool_region_u8(region, origins, wf, bias, (h, 256), *norm)
    assert got.shape == (len(origins), h // 4, 64, 64) and torch.equal(got, want)
    assert torch.equal(got, ops.stem_pool_region_u8(region, torch.tensor(origins), wf, bias, (h, 256), *norm))       # run to run; origins as a CPU tensor
    assert float(want.abs().max()) > 0


@pytest.mark.gpu
def test_padding_is_the_tiles_not_the_regions(cuda, stem_weights):
    """A region of 255s: the tile at (100, 4) has 255s on every side, and its border taps must still be 0 in normalised space - what a standalone tile sees."""
    from toad_amd import ops
    wf, bias = stem_weights
    region = torch.full((16, 512, 3), 255, dtype=torch.uint8, device=cuda)
    alone = torch.full((1, 8, 256, 3), 255, dtype=torch.uint8, device=cuda)
    for norm in (IMAGENET, IDENTITY):
        want = ops.stem_pool_nhwc_u8(alone, wf, bias, *norm)
        assert torch.equal(ops.stem_pool_region_u8(region, [(100, 4)], wf, bias, (8, 256), *norm), want)
        assert not torch.equal(want[0, :, 0], want[0, :, 30])      # the standalone tile's border column is not its interior: the padding shows in `want`


# ---- the conversion op, staged shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("h,w,hr,wr", [(7, 9, 20, 31), (40, 300, 64, 333)])
def test_conversion_by_origin_equals_the_conversion_of_the_stacked_tiles(cuda, h, w, hr, wr, pitched, norm):
    from toad_amd import ops
    region = make_region(hr, wr, hr + wr).to(cuda)
    if pitched:
        region = pitched_view(region, 2, 5, 1, 2)                  # base at an odd byte offset (2 * pitch + 15), pitch 3 (wr + 7)
    origins = [(wr - w, hr - h), (0, 0), (wr - w, 0), (0, hr - h), ((wr - w) // 2 + 1, (hr - h) // 2)]       # both far corners among five
    want = ops.tiles_u8_to_f32(stacked(region, origins, h, w), *norm)
    got = ops.tiles_u8_region_to_f32(region, origins, (h, w), *norm)
    assert got.shape == (5, 3, h, w) and got.dtype == torch.float32 and torch.equal(got, want)
    if norm is IDENTITY:
        assert torch.equal(got, stacked(region, origins, h, w).permute(0, 3, 1, 2).float())


# ---- the whole network ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    return resnet50_baseline().eval().to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["256x256", "8x256", "7x9_staged"])
def test_forward_u8_region_is_bitwise_forward_u8_of_the_stacked_tiles(cuda, model, case):
    if case == "256x256":
        region, origins, tile = make_region(300, 520, 3).to(cuda), ORIGINS_256, 256
    elif case == "8x256":
        region, origins, tile = make_region(23, 531, 1).to(cuda), ORIGINS_8x256, (8, 256)
    else:
        region, origins, tile = pitched_view(make_region(20, 31, 51).to(cuda), 2, 5, 1, 2), [(22, 13), (0, 0), (22, 0), (0, 13), (12, 6)], (7, 9)
    h, w = (tile, tile) if isinstance(tile, int) else tile
    tiles = stacked(region, origins, h, w)
    want = model.forward_u8(tiles)
    got = model.forward_u8_region(region, origins, tile)
    assert got.dtype == torch.float32 and got.shape == (len(origins), 1024) and torch.equal(got, want)
    got16 = model.forward_u8_region(region, origins, tile, out_dtype=torch.float16)
    assert got16.dtype == torch.float16 and torch.equal(got16, model.forward_u8(tiles, out_dtype=torch.float16))
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    half = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                  # the constants are arguments
    assert torch.equal(model.forward_u8_region(region, origins, tile, *half), model.forward_u8(tiles, *half))


@pytest.mark.gpu
def test_forward_u8_region_chunks_the_origins(cuda, model):
    """4,097 origins of 4 x 256 tiles cross max_tiles_per_call (4,096 at this tile size): the origins are sliced, the region never is."""
    from toad_amd.resnet_custom import max_tiles_per_call
    assert max_tiles_per_call(4, 256) == 4096
    region = make_region(40, 300, 9).to(cuda)
    g = torch.Generator().manual_seed(5)
    origins = torch.stack([torch.randint(0, 300 - 256 + 1, (4097,), generator=g), torch.randint(0, 40 - 4 + 1, (4097,), generator=g)], dim=1)
    origins[0] = torch.tensor([44, 36]); origins[4096] = torch.tensor([43, 35])          # the far corner, and a last tile that is its own chunk
    idx_y = origins[:, 1].view(-1, 1) + torch.arange(4).view(1, 4)                       # the stacked tiles by one gather (4,097 slices are slow to build)
    idx_x = origins[:, 0].view(-1, 1) + torch.arange(256).view(1, 256)
    tiles = region[idx_y.to(cuda)[:, :, None], idx_x.to(cuda)[:, None, :]]
    assert tiles.shape == (4097, 4, 256, 3) and torch.equal(tiles[4096], region[35:39, 43:299]) and torch.equal(tiles[0], region[36:40, 44:300])
    want = model.forward_u8(tiles)
    assert torch.equal(model.forward_u8_region(region, origins, (4, 256)), want)
    assert torch.equal(model.forward_u8_region(region, origins.numpy(), (4, 256), out_dtype=torch.float16), model.forward_u8(tiles, out_dtype=torch.float16))


@pytest.mark.gpu
def test_forward_u8_region_refusals_on_the_device(cuda, model):
    region = make_region(23, 531, 1).to(cuda)
    with pytest.raises(ValueError, match=r"origins\[1\]"):     # x + W == Wr + 1
        model.forward_u8_region(region, [(0, 0), (276, 0)], (8, 256))
    with pytest.raises(ValueError, match=r"origins\[0\]"):
        model.forward_u8_region(region, [(0, -1)], (8, 256))
    with pytest.raises(ValueError, match="on the host"):
        model.forward_u8_region(region, torch.zeros(2, 2, dtype=torch.int32, device=cuda), (8, 256))
    with pytest.raises(TypeError, match="integers"):
        model.forward_u8_region(region, torch.zeros(2, 2), (8, 256))
    with pytest.raises(RuntimeError, match=r"stride\(1\) == 3"):
        model.forward_u8_region(torch.zeros(23, 1062, 3, dtype=torch.uint8, device=cuda)[:, ::2], [(0, 0)], (8, 256))
    with pytest.raises(RuntimeError, match="uint8"):
        model.forward_u8_region(region.float(), [(0, 0)], (8, 256))
    with pytest.raises(RuntimeError, match="HIP device"):
        model.forward_u8_region(region.cpu(), [(0, 0)], (8, 256))
    with pytest.raises(ValueError):                            # a tile larger than the region: no origin can be right
        model.forward_u8_region(region, [(0, 0)], 256)


@pytest.mark.gpu
def test_no_tile_copy_on_the_region_route(cuda, model):
    """64 tiles of 256 x 256 at stride 64 from a 448 x 960 region (1.3 MB; the tiles would be 12.6 MB): over a warm call the allocator's peak rises by the
    output rows (256 KB) and the origins (512 B) - less than ONE tile (196,608 B) above them, far from B * H * W * 3."""
    region = make_region(448, 960, 64).to(cuda)
    origins = [(64 * i, 64 * j) for j in range(4) for i in range(12)] + [(64 * i + 3, 191) for i in range(11)] + [(704, 192)] * 5
    assert len(origins) == 64
    model.forward_u8_region(region, origins, 256)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.forward_u8_region(region, origins, 256)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak - before < 64 * 1024 * 4 + 64 * 8 + 256 * 256 * 3, (peak, before)
    assert out.shape == (64, 1024)


# ---- heat-map scores ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_region_attention_scores_equal_the_scores_of_the_materialised_bag(cuda, model):
    """70 origins of (8, 256) tiles: at least 64 rows, so the fp16 bag takes the _x16 route of the MIL model."""
    from toad_amd.eval import attention_heatmap_scores, region_attention_scores
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    region = make_region(23, 531, 1).to(cuda)
    g = torch.Generator().manual_seed(8)
    origins = ORIGINS_8x256 + [(int(x), int(y)) for x, y in zip(torch.randint(0, 276, (63,), generator=g), torch.randint(0, 16, (63,), generator=g))]
    assert len(origins) == 70
    tiles = stacked(region, origins, 8, 256)
    bag16 = model.forward_u8(tiles, out_dtype=torch.float16)
    for pct in (False, True):
        got = region_attention_scores(model, mil, region, origins, tile=(8, 256), percentile=pct)
        assert got.shape == (70,) and torch.equal(got, attention_heatmap_scores(mil, bag16, pct)), pct
    got32 = region_attention_scores(model, mil, region, origins, tile=(8, 256), bag_dtype=torch.float32)
    assert torch.equal(got32, attention_heatmap_scores(mil, model.forward_u8(tiles), False))
    assert torch.isfinite(got32).all() and float(got32.abs().max()) > 0
