"""GPU: uint8 NHWC tiles into the extractor (csrc/stem_halo.inc uint8 form, csrc/conv.hip tiles_u8_nhwc_to_nchw_kernel + the fp16 average pool,
ResNet_Baseline.forward_u8). Every comparison is bitwise: the expected fp32 NCHW tensor is built with the fp64 expression
(u.double() * a.double() + b.double()).float() - the single-rounded fma (tests/test_extractor_u8_host.py) - and the uint8 route must give exactly what
the existing fp32 route gives on it."""
import pytest
import torch

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
IDENTITY = ((0.0, 0.0, 0.0), (1.0 / 255.0,) * 3)


def make_tiles(b, h, w, seed):
    """Uniform random uint8 [b,h,w,3] with an all-0 image, an all-255 image and a ramp (x + 3 y + 85 c: a swapped channel, column or row order shows).
    With fewer than three images the three patterns are row bands of image 0 (its last quarter stays random)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    ramp = (torch.arange(w).view(1, w, 1) + 3 * torch.arange(h).view(h, 1, 1) + 85 * torch.arange(3).view(1, 1, 3)).remainder(256).to(torch.uint8)
    if b >= 3:
        t[b - 3] = 0; t[b - 2] = 255; t[b - 1] = ramp
    else:
        q = h // 4
        t[0, :q] = 0; t[0, q:2 * q] = 255; t[0, 2 * q:3 * q] = ramp[2 * q:3 * q]
    return t


def expected_nchw(tiles, mean, std):
    """fp32 [B,3,H,W]: the fp64 expression on the fp32-rounded constants (exact product and sum, one rounding in the cast)."""
    from toad_amd import ops
    n = torch.tensor(list(ops.norm_constants_u8(mean, std)), dtype=torch.float32, device=tiles.device).double()
    return (tiles.double() * n[:3] + n[3:]).float().permute(0, 3, 1, 2).contiguous()


def view_at_offset(tiles, off):
    """The same tiles as a contiguous view that starts `off` bytes into a larger allocation."""
    buf = torch.empty(tiles.numel() + 16, dtype=torch.uint8, device=tiles.device)
    v = buf[off:off + tiles.numel()].view(tiles.shape)
    v.copy_(tiles)
    assert v.data_ptr() == buf.data_ptr() + off and v.is_contiguous()
    return v


# ---- the conversion op ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, HALF, IDENTITY], ids=["imagenet", "half", "identity"])
@pytest.mark.parametrize("b,h,w", [(1, 1, 1), (2, 7, 9), (1, 40, 300), (3, 4, 256)])
def test_conversion_op_equals_the_fp64_expression(cuda, b, h, w, norm):
    from toad_amd import ops
    t = make_tiles(b, h, w, 11 * b + h + w).to(cuda)
    want = expected_nchw(t, *norm)
    got = ops.tiles_u8_to_f32(t, *norm)
    assert got.shape == (b, 3, h, w) and got.dtype == torch.float32 and torch.equal(got, want)
    for off in (1, 2):                                         # any base alignment of the source
        assert torch.equal(ops.tiles_u8_to_f32(view_at_offset(t, off), *norm), want), off
    if norm is IDENTITY:
        assert torch.equal(got, t.permute(0, 3, 1, 2).float())


@pytest.mark.gpu
def test_conversion_op_refuses_other_layouts(cuda):
    from toad_amd import ops
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        ops.tiles_u8_to_f32(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=cuda))
    with pytest.raises(TypeError):
        ops.tiles_u8_to_f32(torch.zeros(2, 8, 8, 3, device=cuda))
    with pytest.raises(ValueError):
        ops.tiles_u8_to_f32(torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda), std=(0.5, 0.0, 0.5))


# ---- the stem --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stem_weights(cuda):
    g = torch.Generator().manual_seed(4242)
    wt = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    w8 = torch.zeros(64, 3, 8, 8); w8[:, :, 1:, 1:] = wt
    wf = w8.view(64, 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(64, 192).contiguous().to(cuda)
    return wf, torch.randn(64, generator=g).to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [IMAGENET, IDENTITY], ids=["imagenet", "identity"])
@pytest.mark.parametrize("b,h", [(1, 256), (3, 256), (5, 64), (7, 4), (2, 12), (37, 128)])
def test_stem_from_uint8_tiles_is_bitwise_the_fp32_stem(cuda, stem_weights, b, h, norm):
    """(37, 128): 1,184 tiles, more than the grid - workgroups own ranges and recompute the carry tile. Constants compiled in, or b_c written into the
    padding, fail on every case (the identity set has b_c = 0 but a_c = 1; the default set has b_c != 0)."""
    from toad_amd import ops
    wf, bias = stem_weights
    t = make_tiles(b, h, 256, 100 * b + h).to(cuda)
    want = ops.stem_pool_nchw(expected_nchw(t, *norm), wf, bias)
    got = ops.stem_pool_nhwc_u8(t, wf, bias, *norm)
    assert got.shape == (b, h // 4, 64, 64) and torch.equal(got, want)
    assert torch.equal(got, ops.stem_pool_nhwc_u8(t, wf, bias, *norm))          # run to run
    assert float(want.abs().max()) > 0


@pytest.mark.gpu
def test_stem_from_uint8_tiles_shapes_and_alignment(cuda, stem_weights):
    from toad_amd import ops
    wf, bias = stem_weights
    t = make_tiles(2, 8, 256, 5).to(cuda)
    with pytest.raises(RuntimeError, match="W = 256"):
        ops.stem_pool_nhwc_u8(t[:, :, :128].contiguous(), wf, bias)
    with pytest.raises(RuntimeError, match="W = 256"):         # ... like the fp32 op
        ops.stem_pool_nchw(expected_nchw(t, *IMAGENET)[:, :, :, :128].contiguous(), wf, bias)
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        ops.stem_pool_nhwc_u8(t.permute(0, 3, 1, 2).contiguous(), wf, bias)
    want = ops.stem_pool_nchw(expected_nchw(t, *IMAGENET), wf, bias)
    for off in (1, 2, 6):                                      # odd address: copied once by the op; even addresses are read in place
        assert torch.equal(ops.stem_pool_nhwc_u8(view_at_offset(t, off), wf, bias), want), off


# ---- the whole network -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    from toad_amd.resnet_custom import resnet50_baseline
    torch.manual_seed(77)
    return resnet50_baseline().eval().to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,w", [(2, 256, 256), (3, 6, 256), (2, 7, 9), (1, 40, 300), (1, 1, 1)])
def test_forward_u8_is_bitwise_forward_of_the_normalised_tiles(cuda, model, b, h, w):
    """(3, 6, 256) is 256 wide but H % 4 != 0: the staging route, like every shape but the first."""
    t = make_tiles(b, h, w, 1000 + b + h + w).to(cuda)
    want = model(expected_nchw(t, *IMAGENET))
    got = model.forward_u8(t)
    assert got.dtype == torch.float32 and got.shape == (b, 1024) and torch.equal(got, want)
    got16 = model.forward_u8(t, out_dtype=torch.float16)
    assert got16.dtype == torch.float16 and torch.equal(got16, want.half())
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    got_half = model.forward_u8(t, *HALF)                      # the constants are arguments
    assert torch.equal(got_half, model(expected_nchw(t, *HALF)))
    if h * w > 1:
        assert not torch.equal(got_half, want)


@pytest.mark.gpu
def test_forward_u8_chunks_like_forward(cuda, model):
    """4,097 tiles of 4 x 256 cross max_tiles_per_call (4,096 at this tile size)."""
    from toad_amd.resnet_custom import max_tiles_per_call
    assert max_tiles_per_call(4, 256) == 4096
    t = make_tiles(4097, 4, 256, 9).to(cuda)
    want = model(expected_nchw(t, *IMAGENET))
    assert torch.equal(model.forward_u8(t), want)
    assert torch.equal(model.forward_u8(t, out_dtype=torch.float16), want.half())


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,w", [(2, 256, 256), (2, 7, 9)])
def test_forward_u8_takes_a_misaligned_view(cuda, model, b, h, w):
    t = make_tiles(b, h, w, 31 + h).to(cuda)
    want = model(expected_nchw(t, *IMAGENET))
    for off in (1, 2):
        assert torch.equal(model.forward_u8(view_at_offset(t, off)), want), off


@pytest.mark.gpu
def test_forward_u8_refusals_on_the_device(cuda, model):
    t = make_tiles(2, 8, 8, 3).to(cuda)
    with pytest.raises(RuntimeError, match=r"\[B,H,W,3\]"):
        model.forward_u8(t.permute(0, 3, 1, 2).contiguous())
    with pytest.raises(RuntimeError, match="uint8"):
        model.forward_u8(t.float())
    with pytest.raises(RuntimeError, match="out_dtype"):
        model.forward_u8(t, out_dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HIP device"):
        model.forward_u8(t.cpu())
    with pytest.raises(ValueError):
        model.forward_u8(t, std=(0.0, 1.0, 1.0))


@pytest.mark.gpu
def test_no_fp32_image_on_the_256_wide_route(cuda, model):
    """64 tiles of 256 x 256: over a warm call the allocator's peak stays below the size of the fp32 image (50 MB) above what was allocated before it -
    the output is 256 KB and the workspace is cached."""
    t = make_tiles(64, 256, 256, 64).to(cuda)
    model.forward_u8(t)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.forward_u8(t)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak - before < 64 * 3 * 256 * 256 * 4, (peak, before)
    assert out.shape == (64, 1024)
