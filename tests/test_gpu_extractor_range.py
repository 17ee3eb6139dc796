"""GPU: the extractor's kernels (csrc/conv.hip) on VALUES across the fp32 range and on zero operands, through the public per-op entry points and the whole
network, against float64 under the bound of the two-piece arithmetic (tests/ext_range_ref.py::nt_bound; tests/test_extractor_range_host.py shows on the CPU
that the bound is the arithmetic's). No internal scalar is read: a wrong, stale or clobbered abs-max scalar (ext_scratch_scalar / launch_gmax / a producer's
y_gmax), a wrong descale clamp (h2_arith.h) or a scale that leaks between weight rows, images or calls shows as a value outside the bound, a non-finite
value or a zero that is not exact.

Which kernel every shape reaches (narrow_ok, ext_linear, ext_conv_nhwc, launch_narrow_t, ext_stem_conv, stem_pool_from_tiles in conv.hip):

ops.linear_act_res_fwd (M, K, N)
  (300, 160, 64)            N <= 64: gemm_nt_h2_stream_kernel<2, 2, GATHER_NONE>, five k-stages + the zero stage
  (300, 64, 128)            64 < N <= 128: gemm_nt_h2_stream_kernel<2, 4, GATHER_NONE>
  (777, 64, 512) + residual N > 128 is narrow only with a residual and K <= kNarrowResKmax = 64: <2, 4, GATHER_NONE>, four column tiles, ragged M.
                            (K = 128, the shape the range issue listed for this route, is above kNarrowResKmax and runs on the 256x256 kernel.)
  (300, 576, 256)           not narrow: the persistent 256x256 kernel (launch_nt_h2, gemm_h2.inc) with the tensor-wide scalar at stride 0; two row tiles on
                            256 workgroups, so both are K-split into slabs and finished by the fix-up kernel
  (512, 256, 1024)          the same kernel, no residual, four column tiles x two row tiles (fewer tiles than workgroups: K-split as well, nt_half_tiles)
  (8200, 288, 64)           <2, 2, GATHER_NONE>; 2.36 M floats = 590,400 float4, past the 2048 x 256 = 524,288 float4 of gmax_kernel's first grid-stride pass
ops.conv_nhwc (b, h, w, cin, cout, k, s, p)
  (1, 16, 16, 32, 64, 3, 1, 1)            conv3x3_h2_halo_kernel<2>: one 256-pixel tile (the whole image), one 32-channel chunk
  (2, 32, 32, 128, 128, 3, 1, 1)          conv3x3_h2_halo_kernel<4>: eight image rows per tile, four channel chunks
  (4, 16, 16, 64, 192, 3, 1, 1) + residual  conv3x3_h2_halo_kernel<4>: one image per tile, ragged second column tile. (The halo kernel takes whole
                                          256-pixel ROW blocks of one image, H % (256 / W) == 0: the 8x8 images the range issue listed for it - four
                                          images per tile - go to the streamed kernel; that shape is kept in the zero-image test below for exactly
                                          that reason.)
  (1, 13, 9, 64, 64, 3, 2, 1)             gemm_nt_h2_stream_kernel<2, 2, GATHER_CONV>, stride 2, ragged M = 35
  (2, 13, 16, 96, 64, 3, 1, 1)            gemm_nt_h2_stream_kernel<2, 2, GATHER_CONV>, 27 k-stages (odd: the zero stage), taps inner over three channel
                                          chunks, ragged M = 416. (H = 16, the shape the range issue listed, is a whole row block: the halo kernel takes
                                          it whatever Cin is, so H = 13 here.)
  (1, 16, 16, 32, 256, 1, 1, 0)           gemm_nt_h2_stream_kernel<2, 4, GATHER_CONV>, K = 32: one real k-stage + the zero stage, two column tiles (the
                                          padded planes that once overran the abs-max scalar)
  (4, 8, 8, 64, 192, 3, 1, 1) + residual  (zero-image test only) gemm_nt_h2_stream_kernel<2, 4, GATHER_CONV>: four images inside one 256-row tile
ops.stem_conv (1, 3, 33, 35)          stem_s2d_kernel + gemm_nt_h2_stream_kernel<2, 2, GATHER_STEM>, tensor-wide scale (gmax_kernel over the space-to-depth image)
ops.stem_conv_pool (1, 3, 4, 256)     stem_s2d_kernel + gemm_nt_h2_stream_kernel<2, 2, GATHER_STEM_POOL>, tensor-wide scale
ops.stem_pool_nchw (B, 3, 4 n, 256)   stem_halo_pool_kernel<SH_F32>: one scale per tile of two conv rows
resnet50_baseline() on (2, 3, 64, 64)   the three-kernel stem, then toad_resnet50_trunc_fwd_f32's chain of y_gmax -> x_gmax scalars
resnet50_baseline() on (2, 3, 8, 256)   the fused stem (stem_nchw_pool_ok), then the same chain

Every test prints its figures (`EXTRANGE ...`, run with -s) before it asserts; profiles/extractor_range_bound.md records them."""
import functools

import pytest
import torch

from oracle import resnet_oracle as ro
from tests import ext_range_ref as er

pytestmark = pytest.mark.gpu

LINEAR = [(300, 160, 64, False, 1), (300, 64, 128, False, 0), (777, 64, 512, True, 1), (300, 576, 256, False, 1), (512, 256, 1024, False, 0)]
LINEAR_LONG = (8200, 288, 64, False, 1)
CONV = [(1, 16, 16, 32, 64, 3, 1, 1, False), (2, 32, 32, 128, 128, 3, 1, 1, False), (4, 16, 16, 64, 192, 3, 1, 1, True),
        (1, 13, 9, 64, 64, 3, 2, 1, False), (2, 13, 16, 96, 64, 3, 1, 1, False), (1, 16, 16, 32, 256, 1, 1, 0, False)]
STEM = [("stem_conv", (1, 3, 33, 35)), ("stem_conv_pool", (1, 3, 4, 256))]
A_CASES = ([("linear", s, f) for s in LINEAR for f in er.FAMILIES] + [("linear", LINEAR_LONG, f) for f in ("giant_last", "unit")] +
           [("conv", s, f) for s in CONV for f in er.FAMILIES] + [(op, s, f) for op, s in STEM for f in er.FAMILIES])


# ---- one description of every op: its float64 rows, its weights, how it is called, how its [M, N] pre-activations become the output -------------------
def _geom(op, shape):
    """(x shape, N, K of the weight rows, has residual, act, output shape before pooling, pooled)"""
    if op == "linear":
        m, k, n, res, act = shape
        return (m, k), n, k, res, act, (m, n), False
    if op == "conv":
        b, h, w, cin, cout, k, s, p, res = shape
        return (b, h, w, cin), cout, k * k * cin, res, 1, (b, er.conv_out(h, k, s, p), er.conv_out(w, k, s, p), cout), False
    b, _, h, w = shape
    return shape, 64, 147, False, 1, (b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64), op != "stem_conv"


def _rows(op, shape, x):
    if op == "linear":
        return x.double()
    if op == "conv":
        return er.unfold_nhwc(x, *shape[5:8])
    return er.unfold_stem(x)


def _amax(op, x):
    if op == "stem_pool_nchw":                                   # one scale per tile of two conv rows: a value per row of the product
        return er.stem_tile_amax(x).repeat_interleave(128, dim=1).reshape(-1)
    return x.abs().max().double()


def _call(op, shape, cuda, x, w, b, r):
    """w: the weight ROWS the reference uses ([N, K]; the stem's in (c, ky, kx) order, embedded into [64, 192] here)."""
    from toad_amd import ops
    d = lambda t: None if t is None else t.to(cuda)
    if op == "linear":
        return ops.linear_act_res_fwd(d(x), d(w), d(b), d(r), shape[4])
    if op == "conv":
        return ops.conv_nhwc(d(x), d(w), d(b), d(r), shape[5], shape[5], shape[6], shape[7], 1)
    wf = d(er.embed_stem(w))
    if op == "stem_conv":
        return ops.stem_conv(d(x), wf, d(b), 1)
    if op == "stem_conv_pool":
        return ops.stem_conv_pool(d(x), wf, d(b))
    return ops.stem_pool_nchw(d(x), wf, d(b))


def _reference(op, shape, x, w, b, r, amax=None, c=None):
    """(float64 reference, elementwise bound), both shaped like the op's output. r is shaped like the output (or None)."""
    _, n, _, _, act, oshape, pooled = _geom(op, shape)
    rows = _rows(op, shape, x)
    r2 = None if r is None else r.reshape(-1, n)
    pre = rows @ w.double().t()
    if b is not None:
        pre = pre + b.double().view(1, -1)
    if r2 is not None:
        pre = pre + r2.double()
    bound = er.nt_bound(rows, w, _amax(op, x) if amax is None else amax, b, r2, c)
    ref = (pre.clamp_min(0) if act else pre).view(oshape)
    bound = bound.view(oshape)
    if pooled:                                                   # an output's bound: the largest bound of the pre-activations it is taken over
        ref, bound = er.pool_max(ref), er.pool_max(bound)
    return ref, bound


@functools.lru_cache(maxsize=None)
def _case(op, shape, family):
    """One (op, shape, family): operands, the float64 reference and the bound - computed once, shared by the tests below, never modified."""
    xshape, n, k, res, _, oshape, _ = _geom(op, shape)
    x, w = er.make_a(family, xshape), er.make_w(n, k)
    b, r = er.make_bias_res(family, oshape[0] if op == "linear" else oshape[0] * oshape[1] * oshape[2], n, True, res)
    if r is not None:
        r = r.view(oshape)
    ref, bound = _reference(op, shape, x, w, b, r)
    return x, w, b, r, ref, bound


def _check(tag, y, ref, bound):
    y = y.cpu().double()
    err = (y - ref).abs()
    ratio = er.ratio(err, bound)
    print(f"EXTRANGE {tag} err/bound {ratio:.3f}")
    assert y.shape == ref.shape and torch.isfinite(y).all(), tag
    assert bool((err <= bound).all()), (tag, ratio)
    return ratio


def _rel(y, ref):
    return (y.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


# ---- A: every kernel, every family -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,shape,family", A_CASES, ids=lambda v: "x".join(str(int(e)) for e in v) if isinstance(v, tuple) else str(v))
def test_values_stay_within_the_two_piece_bound(cuda, op, shape, family):
    x, w, b, r, ref, bound = _case(op, shape, family)
    y = _call(op, shape, cuda, x, w, b, r)
    assert torch.equal(y, _call(op, shape, cuda, x, w, b, r))                 # a second call: bitwise the first
    _check(f"A {op} {shape} {family}", y, ref, bound)
    # (for the profile note only: the same error against the bound with the constant of exact accumulation, ext_range_ref.c_exact - see its docstring)
    k = _geom(op, shape)[2]
    print(f"EXTRANGE A {op} {shape} {family} err/bound(c_exact) {er.ratio((y.cpu().double() - ref).abs(), _reference(op, shape, x, w, b, r, c=er.c_exact(k))[1]):.3f}")
    if family in ("unit", "tiny", "huge"):
        # fp32-level RELATIVE accuracy at every magnitude; no bias (a unit bias hides a product of 1e-30), and a residual of zeros where the residual is what
        # selects the kernel
        r0 = None if r is None else torch.zeros_like(r)
        ref0, _ = _reference(op, shape, x, w, None, r0)
        rel = _rel(_call(op, shape, cuda, x, w, None, r0), ref0)
        print(f"EXTRANGE A {op} {shape} {family} rel {rel:.3e}")
        assert rel <= 1e-5, (op, shape, family, rel)


# ---- B: the cached workspace (and the abs-max scalar inside it) carries nothing from call to call --------------------------------------------------------
@pytest.mark.parametrize("op,shape", [("linear", LINEAR[0]), ("conv", CONV[0]), ("linear", LINEAR[4])], ids=["streamed", "halo", "wide"])
def test_nothing_is_carried_over_between_calls_of_very_different_magnitude(cuda, op, shape):
    """huge, tiny, unit, huge back to back on one stream: the same cached workspace, so a scalar left by the previous call would be off by 2^100 or more."""
    out = []
    for family in ("huge", "tiny", "unit", "huge"):
        x, w, b, r, ref, bound = _case(op, shape, family)
        out.append(_call(op, shape, cuda, x, w, b, r))                        # no synchronisation in between: the results are looked at afterwards
    for i, family in enumerate(("huge", "tiny", "unit", "huge")):
        _, _, _, _, ref, bound = _case(op, shape, family)
        _check(f"B {op} {shape} #{i} {family}", out[i], ref, bound)
    assert torch.equal(out[0], out[3])


# ---- C: zeros are exact ----------------------------------------------------------------------------------------------------------------------------
C_CASES = [("linear", s) for s in LINEAR] + [("conv", CONV[0]), ("conv", CONV[2]), ("conv", CONV[3]), ("conv", CONV[5])] + STEM + [("stem_pool_nchw", (2, 3, 8, 256))]


def _host_act_bias_res(op, shape, b, r):
    """act(bias + residual) as fp32 computes it, shaped like the op's output (a max-pool over equal values changes nothing)."""
    _, n, _, _, act, oshape, pooled = _geom(op, shape)
    if pooled:
        oshape = (oshape[0], (oshape[1] - 1) // 2 + 1, (oshape[2] - 1) // 2 + 1, n)
    e = b.view(*([1] * (len(oshape) - 1)), n).expand(oshape)
    if r is not None:
        e = e + r
    return (e.clamp_min(0) if act else e).contiguous()


@pytest.mark.parametrize("op,shape", C_CASES, ids=lambda v: "x".join(str(int(e)) for e in v) if isinstance(v, tuple) else str(v))
def test_zero_operands_and_a_zero_weight_row_are_exact(cuda, op, shape):
    x, w, b, r, _, _ = _case(op, shape, "unit")
    want = _host_act_bias_res(op, shape, b, r)
    y = _call(op, shape, cuda, torch.zeros_like(x), w, b, r).cpu()           # gmax == 0
    assert torch.equal(y, want), ("x = 0", (y - want).abs().max().item())
    y = _call(op, shape, cuda, x, torch.zeros_like(w), b, r).cpu()           # amax == 0 in every weight row
    assert torch.equal(y, want), ("w = 0", (y - want).abs().max().item())
    z = er.zero_row(w.shape[0])
    assert float(w[z].abs().max()) == 0.0
    y = _call(op, shape, cuda, x, w, b, r).cpu()
    assert torch.equal(y[..., z], want[..., z]), "the zero row's column"
    w2 = w.clone()
    w2[z] = torch.randn(w.shape[1], generator=torch.Generator().manual_seed(5)) / w.shape[1] ** 0.5
    y2 = _call(op, shape, cuda, x, w2, b, r).cpu()
    keep = torch.arange(w.shape[0]) != z
    assert torch.equal(y[..., keep], y2[..., keep]), "a row's scale touched its neighbours"


@pytest.mark.parametrize("shape", [(4, 8, 8, 64, 192, 3, 1, 1, True), CONV[2]], ids=["streamed_four_images_per_tile", "halo_one_image_per_tile"])
def test_zero_images_between_bright_ones_stay_exact(cuda, shape):
    """Images 0 and 2 at 1e6, images 1 and 3 zero: nothing crosses an image edge - inside a 256-row tile of the streamed kernel (8x8 images, four per tile),
    or between the tiles of the halo kernel - so the zero images give act(bias + residual) exactly, and the bright ones sit within the bound."""
    _, w, b, r, _, _ = _case("conv", shape, "unit")
    x = er.make_a("unit", _geom("conv", shape)[0], seed=1) * 1e6
    x[1] = 0.0; x[3] = 0.0
    y = _call("conv", shape, cuda, x, w, b, r)
    want = _host_act_bias_res("conv", shape, b, r)
    for i in (1, 3):
        assert torch.equal(y[i].cpu(), want[i]), i
    ref, bound = _reference("conv", shape, x, w, b, r)
    _check(f"C conv {shape} zero images", y, ref, bound)


# ---- D: the fused stem's scale is per tile -----------------------------------------------------------------------------------------------------------
def test_fused_stem_scales_every_tile_by_its_own_window(cuda):
    from toad_amd import ops
    op, shape = "stem_pool_nchw", (4, 3, 8, 256)
    bright = [1e-8, 1.0, 1e8, 0.0]
    x = er.make_a("unit", shape, seed=2) * torch.tensor(bright).view(4, 1, 1, 1)
    wt = er.make_w(64, 147)
    one = _call(op, shape, cuda, x, wt, None, None)
    ref, bound = _reference(op, shape, x, wt, None, None)                     # amax_a: every tile's own window
    fused_err = []
    for i in range(4):
        _check(f"D fused image {i} x{bright[i]:g}", one[i], ref[i], bound[i])
        fused_err.append((one[i].cpu().double() - ref[i]).abs().max().item())
        if bright[i]:
            rel = _rel(one[i], ref[i])
            print(f"EXTRANGE D fused image {i} rel {rel:.3e}")
            assert rel <= 1e-5, (i, rel)
    assert float(one[3].abs().max()) == 0.0
    # the same batch through the three-kernel route, whose scale is the batch's: it owes only the bound with the batch maximum ...
    two = ops.maxpool3x3s2_nhwc(_call("stem_conv", shape, cuda, x, wt, None, None))
    ref2, bound2 = _reference("stem_conv_pool", shape, x, wt, None, None, amax=x.abs().max().double())
    _check("D two-kernel route, batch maximum", two, ref2, bound2)
    # ... and that is a different rule: on the 1e-8 image it is further from the fused result than the fused result is from the truth
    apart = (two[0] - one[0]).abs().max().item()
    print(f"EXTRANGE D routes apart on the 1e-8 image {apart:.3e}, fused error there {fused_err[0]:.3e}")
    assert apart > fused_err[0]


def test_fused_stem_tiles_of_one_image_carry_their_own_scale(cuda):
    """Image rows 0 .. 7 at 1e-6, rows 8 .. 15 at 1: tile 0 (window = image rows 0 .. 5) sees small values only and must keep them."""
    op, shape = "stem_pool_nchw", (1, 3, 16, 256)
    x = er.make_a("unit", shape, seed=3)
    x[:, :, :8] *= 1e-6
    wt = er.make_w(64, 147)
    y = _call(op, shape, cuda, x, wt, None, None)
    ref, bound = _reference(op, shape, x, wt, None, None)
    _check("D one image, two magnitudes", y, ref, bound)
    rel0 = _rel(y[:, 0], ref[:, 0])                                           # pooled row 0 = conv rows 0, 1 = tile 0 alone
    print(f"EXTRANGE D pooled row 0 rel {rel0:.3e}")
    assert rel0 <= 1e-5, rel0


# ---- E: the scalar chain inside toad_resnet50_trunc_fwd_f32 -------------------------------------------------------------------------------------------
def _edited_params(kind):
    sd = ro.make_params(41)
    if kind == "dead_relu":                      # layer2.1's first ReLU is exactly zero: its 3x3 convolution is handed gmax == 0
        sd["layer2.1.bn1.weight"] = torch.zeros_like(sd["layer2.1.bn1.weight"])
        sd["layer2.1.bn1.bias"] = torch.full_like(sd["layer2.1.bn1.bias"], -1.0)
    elif kind == "growing":                      # activations grow by orders of magnitude along the chain
        for key in sd:
            if key.startswith("layer1.") and (key.endswith("bn3.weight") or key.endswith("downsample.1.weight")):
                sd[key] = sd[key] * 8.0
    return sd


@functools.lru_cache(maxsize=None)
def _model(kind):
    from toad_amd.resnet_custom import resnet50_baseline
    sd = _edited_params(kind)
    model = resnet50_baseline()
    model.load_state_dict(sd, strict=True)       # through load_state_dict: the folded-weight cache is dropped
    model.relocate().eval()
    return model, sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


E_ROUTES = {"three_kernel_stem": (2, 64, 64), "fused_stem": (2, 8, 256)}
E_CASES = ["x1e-4", "x50", "zero_tile", "brightness_1e6", "dead_relu", "growing", "after_a_bright_call"]


@pytest.mark.parametrize("case", E_CASES)
@pytest.mark.parametrize("route", list(E_ROUTES))
def test_extractor_chain_across_magnitudes(cuda, route, case):
    """Every producer's y_gmax is its consumer's x_gmax: inputs at 1e-4 and 50, a zero tile, tiles 1e6 apart, a dead ReLU layer (the next convolution is
    handed gmax == 0), activations growing 8x per block of layer1, and a call that follows one 2^40 brighter - against the oracle in float64, with the
    tolerance of test_extractor_matches_reference_features taken relative to the reference's scale: max(1e-4 max|feat64|, 4 dev64)."""
    b, h, w = E_ROUTES[route]
    x = ro.make_tiles(b, h, w, 900 + h)
    if case == "x1e-4":
        x = x * 1e-4
    elif case == "x50":
        x = x * 50.0
    elif case == "zero_tile":
        x[1] = 0.0
    elif case == "brightness_1e6":
        x[0] *= 1e-3; x[1] *= 1e3
    model, sd, sd64 = _model(case if case in ("dead_relu", "growing") else "plain")
    feat64 = ro.forward(sd64, x.double())
    dev64 = (ro.forward(sd, x).double() - feat64).abs().max().item()
    scale = feat64.abs().max().item()
    tol = max(1e-4 * scale, 4 * dev64)
    with torch.no_grad():
        if case == "after_a_bright_call":        # the same tiles 2^40 brighter, just before, in the same workspace: scaled by a scalar that call left in a slot,
            model((x * 2.0 ** 40).to(cuda))      # these activations would lie under fp16's smallest subnormal and vanish (trunc_fwd zeroes its slots per call)
        full = model(x.to(cuda))
        alone = [model(x[i:i + 1].to(cuda)) for i in range(b)]
    err = (full.cpu().double() - feat64).abs().max().item()
    apart = max((full[i:i + 1] - alone[i]).abs().max().item() for i in range(b))
    print(f"EXTRANGE E {route} {case} max|feat64| {scale:.3e} dev64 {dev64:.3e} tol {tol:.3e} err {err:.3e} batch-vs-alone {apart:.3e}")
    assert full.shape == (b, 1024) and torch.isfinite(full).all()
    assert err <= tol, (route, case, err, tol)
    if case != "brightness_1e6":
        # batch invariance (the bar of test_extractor_matches_reference_features). An activation's scale is its batch's maximum, so a tile is computed with the
        # same power of two alone and in a batch only where the batch's tiles share a magnitude: with tiles 1e6 apart the dim tile alone is scaled 2^20 finer
        # than beside the bright one, and the two results legitimately differ by the absolute term of the bound - skipped there.
        assert apart <= 1e-5 * max(full.abs().max().item(), 1.0), (route, case, apart)
