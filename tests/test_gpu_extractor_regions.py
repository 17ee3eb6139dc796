"""GPU: tiles read by origin from a LIST of regions (csrc/stem_halo.inc list forms, csrc/conv.hip tiles_u8_nhwc_to_nchw_kernel<true, ., true>,
ResNet_Baseline.forward_u8_regions, eval.slide_attention_heatmap(batch_extract=True)). Every comparison is bitwise against the existing route on the
tiles materialised with torch.stack([regions[k][y:y+H, x:x+W] for x, y, k in origins]): padding is the tile's, every tile is read from ITS region, and
with the same tiles in the same order the cut of the slide into regions is invisible in the bag."""
import numpy as np
import pytest
import torch

from tests import tissue_ref

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
IDENTITY = ((0.0, 0.0, 0.0), (1.0 / 255.0,) * 3)

# (8, 256) tiles of three regions - R0 23 x 531 (pitch 1593, odd), R1 a view of pitch 1620 at an odd address, R2 16 x 512 - interleaved so that consecutive
# tiles, hence a workgroup's carry tile (the tile above its range), come from different regions. Both parities of x and of y * pitch; the tiles touching each
# region's right and bottom edge exactly ((275, 15) in R0 and R1, (256, 8) in R2); a duplicate ((2, 3, 0)); one position, (2, 3), in R0 and R1, whose bytes
# differ there, so a wrong k shows; 14 tiles x 2 row pairs, so workgroup ranges begin inside a tile.
TRIPLES_8x256 = [(0, 0, 0), (1, 0, 1), (256, 8, 2), (2, 3, 0), (2, 3, 1), (275, 15, 0), (0, 0, 2), (275, 15, 1), (256, 0, 2), (3, 5, 1), (0, 8, 2), (2, 3, 0),
                 (0, 15, 1), (1, 1, 2)]


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


def stacked(regions, triples, h, w):
    return torch.stack([regions[k][y:y + h, x:x + w] for x, y, k in triples])


def boxed(regions, triples, fh, fw):
    """The 2 x 2 box-filtered footprints in triple order, by the stated reference of `shrink` (ops.box_tiles_u8 on each tile's own region)."""
    from toad_amd import ops
    return torch.cat([ops.box_tiles_u8(regions[k], [(x, y)], (fh, fw), 2) for x, y, k in triples])


@pytest.fixture(scope="module")
def three_regions(cuda):
    r0 = make_region(23, 531, 1).to(cuda)
    r1 = pitched_view(make_region(23, 531, 2).to(cuda), 1, 3, 1, 6)            # wide[1:24, 3:534] of a 25 x 540 image: pitch 1620, base at byte 1629
    r2 = make_region(16, 512, 5).to(cuda)
    assert r0.stride(0) == 1593 and r1.stride(0) == 1620 and r1.data_ptr() % 2 == 1 and r2.stride(0) == 1536
    assert not torch.equal(r0[3:11, 2:258], r1[3:11, 2:258])                   # the shared position holds other bytes in R0 than in R1
    return [r0, r1, r2]


@pytest.fixture(scope="module")
def stem_weights(cuda):
    g = torch.Generator().manual_seed(4242)
    wt = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    w8 = torch.zeros(64, 3, 8, 8); w8[:, :, 1:, 1:] = wt
    wf = w8.view(64, 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(64, 192).contiguous().to(cuda)
    return wf, torch.randn(64, generator=g).to(cuda)


@pytest.fixture(scope="module")
def model(cuda):
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    return resnet50_baseline().eval().to(cuda)


# ---- 1. the stem, 256-wide route -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
def test_stem_from_three_regions_is_bitwise_the_stem_on_the_stacked_tiles(cuda, stem_weights, three_regions, norm):
    from toad_amd import ops
    wf, bias = stem_weights
    assert len(TRIPLES_8x256) >= 11 and all(a[2] != b[2] for a, b in zip(TRIPLES_8x256, TRIPLES_8x256[1:]))
    want = ops.stem_pool_nhwc_u8(stacked(three_regions, TRIPLES_8x256, 8, 256), wf, bias, *norm)
    got = ops.stem_pool_regions_u8(three_regions, TRIPLES_8x256, wf, bias, (8, 256), *norm)
    assert got.shape == (len(TRIPLES_8x256), 2, 64, 64) and torch.equal(got, want)
    assert torch.equal(got, ops.stem_pool_regions_u8(tuple(three_regions), torch.tensor(TRIPLES_8x256), wf, bias, (8, 256), *norm))      # run to run
    assert float(want.abs().max()) > 0
    # a list of ONE region is the single-region call
    for k, region in enumerate(three_regions):
        mine = [(x, y) for x, y, kk in TRIPLES_8x256 if kk == k]
        one = ops.stem_pool_regions_u8([region], [(x, y, 0) for x, y in mine], wf, bias, (8, 256), *norm)
        assert torch.equal(one, ops.stem_pool_region_u8(region, mine, wf, bias, (8, 256), *norm))


# ---- 2. padding --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_padding_is_the_tiles_not_the_regions_in_a_list(cuda, stem_weights):
    """R0 all 255, R1 all 0: the tile in the middle of R0 has 255s on every side, and its border taps must still be 0 in normalised space."""
    from toad_amd import ops
    wf, bias = stem_weights
    regions = [torch.full((16, 512, 3), 255, dtype=torch.uint8, device=cuda), torch.zeros((16, 512, 3), dtype=torch.uint8, device=cuda)]
    alone = torch.stack([torch.full((8, 256, 3), 255, dtype=torch.uint8, device=cuda), torch.zeros((8, 256, 3), dtype=torch.uint8, device=cuda)])
    for norm in (IMAGENET, IDENTITY):
        want = ops.stem_pool_nhwc_u8(alone, wf, bias, *norm)
        assert torch.equal(ops.stem_pool_regions_u8(regions, [(100, 4, 0), (100, 4, 1)], wf, bias, (8, 256), *norm), want)
        assert not torch.equal(want[0, :, 0], want[0, :, 30])      # the standalone tile's border column is not its interior: the padding shows in `want`


# ---- 3. shrink = 2 through the stem ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
def test_box_stem_from_two_regions_is_the_stem_on_the_box_filtered_footprints(cuda, stem_weights, norm):
    from toad_amd import ops
    wf, bias = stem_weights
    ra = make_region(40, 600, 7).to(cuda)                                      # pitch 1800
    rb = pitched_view(make_region(33, 531, 8).to(cuda), 1, 3, 1, 6)            # pitch 1620, base at byte 1629
    assert rb.data_ptr() % 2 == 1 and ra.stride(0) != rb.stride(0)
    triples = [(0, 0, 0), (19, 17, 1), (88, 24, 0), (1, 0, 1), (87, 23, 0), (0, 1, 1), (3, 5, 0), (19, 17, 1), (88, 0, 0)]       # far corners of both; a duplicate
    want = ops.stem_pool_nhwc_u8(boxed([ra, rb], triples, 16, 512), wf, bias, *norm)
    got = ops.stem_pool_regions_u8([ra, rb], triples, wf, bias, (16, 512), *norm, shrink=2)
    assert got.shape == (len(triples), 2, 64, 64) and torch.equal(got, want) and float(want.abs().max()) > 0
    assert torch.equal(got, ops.stem_pool_regions_u8([ra, rb], triples, wf, bias, (16, 512), *norm, shrink=2))


# ---- 4. the staged converter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
@pytest.mark.parametrize("h,w,hr,wr,shrink", [(7, 9, 20, 31, 1), (40, 300, 64, 333, 1), (14, 18, 20, 31, 2)])
def test_conversion_from_two_regions_equals_the_conversion_of_the_stacked_tiles(cuda, h, w, hr, wr, shrink, norm):
    from toad_amd import ops
    ra = make_region(hr, wr, hr + wr).to(cuda)
    rb = pitched_view(make_region(hr + 3, wr + 2, hr).to(cuda), 2, 5, 1, 2)    # another extent; base at an odd byte offset (2 * pitch + 15), pitch 3 (wr + 9)
    regions = [ra, rb]
    triples = [(wr - w, hr - h, 0), (wr + 2 - w, hr + 3 - h, 1), (0, 0, 1), (wr - w, 0, 0), (0, hr + 3 - h, 1), ((wr - w) // 2 + 1, (hr - h) // 2, 0), (1, 1, 1)]
    tiles = stacked(regions, triples, h, w) if shrink == 1 else boxed(regions, triples, h, w)
    want = ops.tiles_u8_to_f32(tiles, *norm)
    got = ops.tiles_u8_regions_to_f32(regions, triples, (h, w), *norm, shrink=shrink)
    assert got.shape == (len(triples), 3, h // shrink, w // shrink) and got.dtype == torch.float32 and torch.equal(got, want)
    if norm is IDENTITY:
        assert torch.equal(got, tiles.permute(0, 3, 1, 2).float())


# ---- 5. the whole network ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["256x256", "8x256", "7x9_staged"])
def test_forward_u8_regions_is_bitwise_forward_u8_of_the_stacked_tiles(cuda, model, three_regions, case):
    if case == "256x256":
        r = make_region(300, 520, 3).to(cuda)
        regions, triples, tile = [r, pitched_view(r, 1, 3, 1, 6)], [(0, 0, 0), (264, 44, 1), (131, 7, 0), (131, 7, 1), (264, 44, 0)], 256
    elif case == "8x256":
        regions, triples, tile = three_regions, TRIPLES_8x256, (8, 256)
    else:
        regions = [pitched_view(make_region(20, 31, 51).to(cuda), 2, 5, 1, 2), make_region(9, 40, 52).to(cuda)]
        triples, tile = [(22, 13, 0), (31, 2, 1), (0, 0, 0), (22, 0, 0), (0, 0, 1), (0, 13, 0), (12, 6, 0)], (7, 9)
    h, w = (tile, tile) if isinstance(tile, int) else tile
    tiles = stacked(regions, triples, h, w)
    want = model.forward_u8(tiles)
    got = model.forward_u8_regions(regions, triples, tile)
    assert got.dtype == torch.float32 and got.shape == (len(triples), 1024) and torch.equal(got, want)
    got16 = model.forward_u8_regions(regions, np.array(triples), tile, out_dtype=torch.float16)
    assert got16.dtype == torch.float16 and torch.equal(got16, model.forward_u8(tiles, out_dtype=torch.float16))
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    half = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                  # the constants are arguments
    assert torch.equal(model.forward_u8_regions(regions, triples, tile, *half), model.forward_u8(tiles, *half))
    assert tuple(model.forward_u8_regions(regions, np.zeros((0, 3), dtype=np.int64), tile).shape) == (0, 1024)


@pytest.mark.gpu
def test_forward_u8_regions_with_shrink_2_is_forward_u8_of_the_box_filtered_footprints(cuda, model):
    ra = make_region(40, 600, 7).to(cuda)
    rb = pitched_view(make_region(33, 531, 8).to(cuda), 1, 3, 1, 6)
    triples = [(0, 0, 0), (19, 17, 1), (88, 24, 0), (1, 0, 1), (87, 23, 0)]
    want = model.forward_u8(boxed([ra, rb], triples, 16, 512))
    assert torch.equal(model.forward_u8_regions([ra, rb], triples, (16, 512), shrink=2), want) and float(want.abs().max()) > 0
    # ... and the whole-slide call's bits when the list is a cut of one region: strips of ra, the same tiles in the same order
    whole = model.forward_u8_region(ra, [(x, y) for x, y, k in triples if k == 0], (16, 512), shrink=2)
    cut = model.forward_u8_regions([ra[:20], ra[4:]], [(0, 0, 0), (88, 20, 1), (87, 19, 1)], (16, 512), shrink=2)
    assert torch.equal(cut, whole)


# ---- 6. chunking -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_u8_regions_chunks_the_triples(cuda, model):
    """4,097 triples of 4 x 256 tiles cross max_tiles_per_call (4,096 at this tile size): the triples are sliced, the regions never are, and every chunk
    gets the same list. 4,096 row pairs on at most 512 workgroups: every workgroup walks several tiles of different regions."""
    from toad_amd.resnet_custom import max_tiles_per_call
    assert max_tiles_per_call(4, 256) == 4096
    regions = [make_region(40, 300, 9).to(cuda), pitched_view(make_region(40, 300, 10).to(cuda), 1, 3, 1, 6), make_region(44, 311, 11).to(cuda)]
    assert len({r.stride(0) for r in regions}) == 3
    g = torch.Generator().manual_seed(5)
    n = 4097
    triples = torch.stack([torch.randint(0, 300 - 256 + 1, (n,), generator=g), torch.randint(0, 40 - 4 + 1, (n,), generator=g),
                           torch.randint(0, 3, (n,), generator=g)], dim=1)
    triples[0] = torch.tensor([55, 40, 2]); triples[4096] = torch.tensor([43, 35, 1])    # R2's far corner, and a last tile that is its own chunk
    idx_y = (triples[:, 1].view(-1, 1) + torch.arange(4).view(1, 4)).to(cuda)            # the stacked tiles by one gather per region
    idx_x = (triples[:, 0].view(-1, 1) + torch.arange(256).view(1, 256)).to(cuda)
    tiles = torch.empty((n, 4, 256, 3), dtype=torch.uint8, device=cuda)
    for k, region in enumerate(regions):
        sel = (triples[:, 2] == k).to(cuda)
        tiles[sel] = region[idx_y[sel][:, :, None], idx_x[sel][:, None, :]]
    assert torch.equal(tiles[4096], regions[1][35:39, 43:299]) and torch.equal(tiles[0], regions[2][40:44, 55:311])
    want = model.forward_u8(tiles)
    assert torch.equal(model.forward_u8_regions(regions, triples, (4, 256)), want)
    assert torch.equal(model.forward_u8_regions(regions, triples.numpy(), (4, 256), out_dtype=torch.float16), model.forward_u8(tiles, out_dtype=torch.float16))


# ---- 7. refusals of the Python layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_u8_regions_refusals_on_the_device(cuda, model, three_regions):
    from toad_amd import ops
    r0, r1, r2 = three_regions
    with pytest.raises(ValueError, match=r"origins\[1\].*region 2, which is 16 x 512"):      # inside R0 and R1, outside ITS region
        model.forward_u8_regions(three_regions, [(0, 0, 0), (275, 15, 2)], (8, 256))
    with pytest.raises(ValueError, match=r"origins\[0\].*k=3"):                              # k == n
        model.forward_u8_regions(three_regions, [(0, 0, 3)], (8, 256))
    with pytest.raises(ValueError, match=r"origins\[1\].*k=-1"):
        model.forward_u8_regions(three_regions, [(0, 0, 0), (0, 0, -1)], (8, 256))
    with pytest.raises(ValueError, match=r"\[B,3\]"):
        model.forward_u8_regions(three_regions, [(0, 0)], (8, 256))
    with pytest.raises(ValueError, match="on the host"):
        model.forward_u8_regions(three_regions, torch.zeros(2, 3, dtype=torch.int32, device=cuda), (8, 256))
    with pytest.raises(TypeError, match="integers"):
        model.forward_u8_regions(three_regions, torch.zeros(2, 3), (8, 256))
    with pytest.raises(RuntimeError, match=r"stride\(1\) == 3.*regions\[1\]"):
        model.forward_u8_regions([r0, torch.zeros(23, 1062, 3, dtype=torch.uint8, device=cuda)[:, ::2]], [(0, 0, 0)], (8, 256))
    with pytest.raises(RuntimeError, match=r"float32 as regions\[2\]"):
        model.forward_u8_regions([r0, r1, r2.float()], [(0, 0, 0)], (8, 256))
    with pytest.raises(RuntimeError, match=r"HIP device.*regions\[1\] on cpu"):
        model.forward_u8_regions([r0, r1.cpu()], [(0, 0, 0)], (8, 256))
    with pytest.raises(ValueError, match=r"regions\[1\].*stride\(1\) == 3"):
        ops.stem_pool_regions_u8([r0, torch.zeros(23, 1062, 3, dtype=torch.uint8, device=cuda)[:, ::2]], [(0, 0, 0)], None, None, (8, 256))
    with pytest.raises(TypeError, match=r"regions\[1\].*uint8"):
        ops.tiles_u8_regions_to_f32([r0, r1.float()], [(0, 0, 0)], (8, 256))
    with pytest.raises(RuntimeError, match=r"regions\[1\]"):
        ops.tiles_u8_regions_to_f32([r0, r1.cpu()], [(0, 0, 0)], (8, 256))
    many = [r2[i % 8:, i // 8:] for i in range(129)]                                         # 129 views of one small tensor
    with pytest.raises(ValueError, match="129 regions"):
        model.forward_u8_regions(many, [(0, 0, 0)], (8, 256))
    with pytest.raises(ValueError, match="129 regions"):
        ops.stem_pool_regions_u8(many, [(0, 0, 0)], None, None, (8, 256))
    with pytest.raises(ValueError):                                                          # a tile larger than every region: no triple can be right
        model.forward_u8_regions(three_regions, [(0, 0, 0)], 256)


@pytest.mark.gpu
def test_regions_on_different_devices_are_refused(cuda, model, three_regions):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from toad_amd import ops
    other = three_regions[2].to("cuda:1")
    with pytest.raises(RuntimeError, match=r"regions\[1\] is on cuda:1.*one device"):
        model.forward_u8_regions([three_regions[0], other], [(0, 0, 0)], (8, 256))
    with pytest.raises(ValueError, match=r"regions\[1\] is on cuda:1.*one device"):
        ops.tiles_u8_regions_to_f32([three_regions[0], other], [(0, 0, 0)], (8, 256))


# ---- 8. no tile copy -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_tile_copy_on_the_regions_route(cuda, model):
    """64 tiles of 256 x 256 at stride 64 from two 448 x 960 regions (the tiles would be 12.6 MB): over a warm call the allocator's peak rises by the output
    rows (256 KB) and the triples (768 B) - less than ONE tile (196,608 B) above them, far from B * H * W * 3. The descriptors live on the host."""
    regions = [make_region(448, 960, 64).to(cuda), make_region(448, 960, 65).to(cuda)]
    xy = [(64 * i, 64 * j) for j in range(4) for i in range(12)] + [(64 * i + 3, 191) for i in range(11)] + [(704, 192)] * 5
    triples = [(x, y, i % 2) for i, (x, y) in enumerate(xy)]
    assert len(triples) == 64
    model.forward_u8_regions(regions, triples, 256)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.forward_u8_regions(regions, triples, 256)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak - before < 64 * 1024 * 4 + 64 * 12 + 256 * 256 * 3, (peak, before)
    assert out.shape == (64, 1024)


# ---- 9. the walk over strips with one extractor call --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slide_attention_heatmap_batch_extract_gives_the_whole_slides_scores(cuda):
    """The 256 x 1100 synthetic slide of the walk's own test as 3 overlapping strips, tiles of 64 x 256: with batch_extract=True the scores are those of
    forward_u8_region on the WHOLE slide - the strips are invisible in the bag - and the canvas that of attention_canvas on the whole slide."""
    from toad_amd.eval import attention_heatmap_scores, slide_attention_heatmap
    from toad_amd.heatmap import attention_canvas
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import segmented_tissue_origins, tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    hs, ws = 256, 1100
    s = tissue_ref.slide(hs, ws, 1)
    slide = torch.from_numpy(np.ascontiguousarray(s).copy()).to(cuda)
    tile = stride = (64, 256)
    spans = [(0, 112), (64, 144), (176, 80)]
    strips = [(slide[y:y + n], y) for y, n in spans]
    want_o = tissue_origins(slide, tile=tile, stride=stride)
    assert 4 < len(want_o) < 16

    def whole_scores(o):
        with torch.no_grad():
            return attention_heatmap_scores(mil, extractor.forward_u8_region(slide, o, tile, out_dtype=torch.float16), percentile=True)
    want_s = whole_scores(want_o)
    for down in (1, 16):
        kw = dict(tile=tile, stride=stride, down=down, smooth=True, blur=96.0)
        origins, scores, canvas = slide_attention_heatmap(extractor, mil, strips, (hs, ws), batch_extract=True, **kw)
        assert np.array_equal(origins, want_o) and origins.dtype == np.int64 and torch.equal(scores, want_s)
        assert tuple(canvas.shape) == (hs // down, ws // down, 3) and torch.equal(canvas, attention_canvas(slide, origins, scores, **kw))
        o1, s1, c1 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), batch_extract=True, batch_render=True, **kw)
        assert np.array_equal(o1, want_o) and torch.equal(s1, want_s) and torch.equal(c1, canvas)
    # the caller's selection, in slide coordinates
    fewer = want_o[1::2]
    o2, s2, c2 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), origins=fewer, batch_extract=True, **kw)
    assert np.array_equal(o2, fewer) and torch.equal(s2, whole_scores(fewer)) and torch.equal(c2, attention_canvas(slide, fewer, s2, **kw))
    # the segmented selector on the whole slide's plane
    seg_o = segmented_tissue_origins(slide, tile=tile, stride=stride, down=16)
    assert len(seg_o)
    base = dict(tile=tile, stride=stride, smooth=True, down=16)
    o3, s3, c3 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), segment=dict(down=16), batch_extract=True, **base)
    assert np.array_equal(o3, seg_o) and torch.equal(s3, whole_scores(seg_o)) and torch.equal(c3, attention_canvas(slide, seg_o, s3, **base))
    # several levels in one walk, and in one launch
    for bl in (False, True):
        o4, s4, c4 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), tile=tile, stride=stride, smooth=True, down=(1, 16), batch_levels=bl,
                                             batch_extract=True)
        assert np.array_equal(o4, want_o) and torch.equal(s4, want_s)
        for lv in (1, 16):
            assert torch.equal(c4[lv], attention_canvas(slide, o4, s4, tile=tile, stride=stride, smooth=True, down=lv))


@pytest.mark.gpu
def test_slide_attention_heatmap_batch_extract_with_a_last_strip_shorter_than_the_tile(cuda):
    """A 300 x 1100 slide as strips of 256 and 44 rows, tiles of 64 x 256: the last strip owns no lattice row and only renders rows 256 .. 300. The per-strip
    walk skips it in pass 1; so does the one list call - it gets the strips that own tiles - and scores and canvas are the whole slide's."""
    from toad_amd.eval import attention_heatmap_scores, slide_attention_heatmap
    from toad_amd.heatmap import attention_canvas, strip_plan
    from toad_amd.model_toad import TOAD_fc_mtl_concat
    from toad_amd.resnet_custom import resnet50_baseline
    from toad_amd.tissue import tissue_origins
    torch.manual_seed(77)
    extractor = resnet50_baseline().eval().to(cuda)
    torch.manual_seed(3)
    mil = TOAD_fc_mtl_concat()
    mil.relocate()
    mil.eval()
    hs, ws = 300, 1100
    slide = torch.from_numpy(np.ascontiguousarray(tissue_ref.slide(hs, ws, 1)).copy()).to(cuda)
    tile = stride = (64, 256)
    spans = [(0, 256), (256, 44)]
    assert [p["rows"] for p in strip_plan((hs, ws), spans, tile, stride, (0, 0), 4)] == [(0, 4), (4, 4)]
    strips = [(slide[y:y + n], y) for y, n in spans]
    want_o = tissue_origins(slide, tile=tile, stride=stride)
    assert len(want_o) > 2
    with torch.no_grad():
        want_s = attention_heatmap_scores(mil, extractor.forward_u8_region(slide, want_o, tile, out_dtype=torch.float16), percentile=True)
    for down in (1, 4):
        kw = dict(tile=tile, stride=stride, down=down, smooth=True)
        o0, s0, c0 = slide_attention_heatmap(extractor, mil, strips, (hs, ws), **kw)                      # the walk as it was: the short strip is no obstacle
        origins, scores, canvas = slide_attention_heatmap(extractor, mil, strips, (hs, ws), batch_extract=True, **kw)
        assert np.array_equal(o0, want_o) and np.array_equal(origins, want_o) and torch.equal(scores, want_s)
        assert tuple(canvas.shape) == (hs // down, ws // down, 3) and torch.equal(canvas, attention_canvas(slide, origins, scores, **kw))
