"""CPU: the error bound the extractor's kernels are held to (tests/ext_range_ref.py::nt_bound, asserted on the device by
tests/test_gpu_extractor_range.py) belongs to the fp16 two-piece arithmetic itself - its host emulation stays inside it for every operand family -
and the operand families are what they claim to be."""
import pytest
import torch

from tests import ext_range_ref as er

M, K, N = 512, 576, 64


@pytest.mark.parametrize("family", er.FAMILIES)
def test_emulated_two_piece_product_stays_within_the_bound(family):
    x, w = er.make_a(family, (M, K)), er.make_w(N, K)
    amax = x.abs().max().double()
    ref = x.double() @ w.double().t()
    # the representation alone (exact accumulation) under the constant of tests/test_gpu_h2.py::_nt_bound, c = max(6, 0.75 sqrt(K))
    got = er.emulate(x, w, amax)
    bound = er.nt_bound(x, w, amax, c=er.c_exact(K))
    r = er.ratio((got - ref).abs(), bound)
    # the same products through an fp32 accumulator, one rounding per product, under the bound the kernels are held to
    got32 = er.emulate(x, w, amax, acc32=True)
    bound32 = er.nt_bound(x, w, amax)
    r32 = er.ratio((got32 - ref).abs(), bound32)
    print(f"EXTRANGE host {family} err/bound: exact accumulation {r:.3f}, fp32 accumulation {r32:.3f}")
    assert torch.isfinite(got).all() and r <= 1.0, (family, r)
    assert torch.isfinite(got32).all() and r32 <= 1.0, (family, r32)
    assert r == er.host_ratio(family, False) and r32 == er.host_ratio(family)     # the figures the profile note prints are these
    z = er.zero_row(N)
    for g, b in ((got, bound), (got32, bound32)):
        assert float(g[:, z].abs().max()) == 0.0 and float(b[:, z].max()) == 0.0        # a zero weight row: exact, and the bound says so


def test_fp32_accumulation_of_a_dominated_sum_needs_the_accumulation_term():
    """Why c is not _nt_bound's max(6, 0.75 sqrt(K)) here (tests/ext_range_ref.py): with one product dominating the sum the fp32 accumulator rounds at the
    size of the whole sum from that product on, and over 38,400 elements the walk passes three standard deviations - on the host, with no kernel involved.
    The same chain on unit data stays inside the old constant, which is why no unit-magnitude test ever saw this."""
    m, k, n = 300, 64, 128
    for family, over in (("heavy", True), ("unit", False)):
        x, w = er.make_a(family, (m, k)), er.make_w(n, k)
        amax = x.abs().max().double()
        err = (er.emulate(x, w, amax, acc32=True) - x.double() @ w.double().t()).abs()
        r_old, r_new = er.ratio(err, er.nt_bound(x, w, amax, c=er.c_exact(k))), er.ratio(err, er.nt_bound(x, w, amax))
        print(f"EXTRANGE host fp32 chain {family} ({m}, {k}, {n}): err/bound {r_old:.3f} with c = max(6, 0.75 sqrt K), {r_new:.3f} with c = 6 + 6 sqrt K")
        assert (r_old > 1.0) == over and r_new <= 1.0, (family, r_old, r_new)


def test_a_per_row_scale_group_is_tighter_than_the_tensor_wide_one():
    """amax_a may be one value per row (the fused stem's tiles): rows 2^-40 below the tensor's maximum keep their relative accuracy under their own scale
    and lose everything under the tensor's - the bound must tell the two apart in the same way."""
    x, w = er.make_a("unit", (64, 160)), er.make_w(64, 160)
    x[:32] *= 2.0 ** -40
    ref = x.double() @ w.double().t()
    own = torch.cat([x[:32].abs().max().expand(32), x[32:].abs().max().expand(32)]).double()
    e_own = (er.emulate(x, w, own) - ref).abs()
    e_all = (er.emulate(x, w, x.abs().max().double()) - ref).abs()
    assert er.ratio(e_own, er.nt_bound(x, w, own)) <= 1.0 and er.ratio(e_all, er.nt_bound(x, w, x.abs().max().double())) <= 1.0
    assert er.ratio(e_all, er.nt_bound(x, w, own)) > 1.0     # the tensor-wide scale does NOT meet the per-group bound
    assert float(er.emulate(x, w, x.abs().max().double())[:32].abs().max()) == 0.0       # it flushes those rows


def test_families_and_weights_are_what_they_claim():
    w = er.make_w(N, K)
    z = er.zero_row(N)
    assert float(w[z].abs().max()) == 0.0 and z % 7 != 0
    assert int((w.abs().max(1).values == 0).sum()) == 1
    assert float(w[::7].abs().max()) < 1e-3 * float(w[1::7].abs().max())
    for shape in [(M, K), (8200, 288), (1, 16, 16, 32), (1, 3, 33, 35)]:
        x = er.make_a("giant_last", shape).reshape(-1)
        assert int(x.abs().argmax()) == x.numel() - 1 and float(x[-1]) == -2.0 ** 20
    assert 8200 * 288 // 4 > 2048 * 256                       # past what the first pass of gmax_kernel's 2048-block grid-stride loop covers
    assert 0 < float(er.make_a("tiny", (M, K)).abs().max()) < 1e-29 and float(er.make_a("huge", (M, K)).abs().max()) > 1e30
    h = er.make_a("heavy", (M, K)).abs()
    assert float(h.max()) <= 1e12 and float(h.max() / h.median()) > 2.0 ** 17          # elements in the absolute regime of the tensor's scale
    r = er.make_a("relu_sparse", (M, K))
    assert float(r.min()) == 0.0 and float(r.max()) == 3e4 and float((r == 0).float().mean()) > 0.9


def test_scale_exponent_and_its_clamps():
    k = er.exp_from_amax(torch.tensor([0.0, 1.0, 0.75, 2.0 ** 13, 3e38, 1e-45, 2.0 ** -126], dtype=torch.float64))
    assert k.tolist() == [14.0, 13.0, 14.0, 0.0, -114.0, 120.0, 120.0]


def test_stem_geometry_helpers():
    """The embedded [64, 192] weights and the 147-column unfold are the same convolution; the per-tile window is image rows 4t - 4 .. 4t + 5."""
    import torch.nn.functional as F
    wt, wf = er.stem_weights()
    x = er.make_a("unit", (1, 3, 8, 12))
    ref = F.conv2d(x.double(), wt.view(64, 3, 7, 7).double(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    assert (er.unfold_stem(x) @ wt.double().t() - ref).abs().max().item() <= 1e-12
    assert float(wf.abs().sum()) == float(wt.abs().sum()) and wf.shape == (64, 192)
    x = torch.zeros(1, 3, 16, 256)
    x[0, 0, 10, 5] = 3.0                                       # image row 10 is in the windows of tiles 2 (rows 4 .. 13) and 3 (rows 8 .. 15) only
    assert er.stem_tile_amax(x)[0].tolist() == [0.0, 0.0, 0.0, 0.0, 3.0, 3.0, 3.0, 3.0]
    x[0, 0, 5, 5] = 2.0                                        # row 5: tiles 0 (rows 0 .. 5), 1 (0 .. 9), 2
    assert er.stem_tile_amax(x)[0].tolist() == [2.0, 2.0, 2.0, 2.0, 3.0, 3.0, 3.0, 3.0]
