"""GPU: the fused gated-attention pool backward (toad_amd/csrc/gated_pool.hip) where tests/test_gpu_kernels.py does not reach.
  A. the abs-max array of dP (ops.gated_pool_bwd(want_amax=True)): an analytic per-row bound, folded per 256 rows, that fixes the scale of the
     fp16 two-piece operands downstream - it must bound the device's own dP in every block, sit in the right block, stay within 8x of the
     measured maximum on ordinary data (tests/test_pool_ref_host.py shows the exact arithmetic does), and cost the consumers no accuracy;
  B. the backward values against the float64 oracle at the covering shapes with few rows, under dropout, with saturated softmax / gates, and
     the rows past N left alone;
  C. the batched launch (one bound per row of the concatenation) on a ragged batch whose slides' gradients differ by 10^7.
The reference is oracle.toad_oracle.gated_pool_bwd on float64 inputs (tests/pool_ref.reference); dropout masks come from tests/drop_ref."""
import pytest
import torch
import torch.nn.functional as F

from oracle import toad_oracle as orc
from tests import pool_ref as R
from tests.helpers import SLOT2KEY, assert_grad_close, assert_grad_close_or_few_flips, grad_scale

pytestmark = pytest.mark.gpu

SLACK = 1.0 + 2.0 ** -18        # fewer than 32 fp32 roundings and a one-ulp reciprocal lie between the bound and the stored dP


def _rel(a, b, floor=1e-3):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), floor)


class _Case:
    """Inputs of one (D, L, T, n) on the host and on the device."""

    def __init__(self, cuda, d, l, t, n, scale=1.0, inputs=None):
        self.d, self.l, self.t, self.n, self.cuda = d, l, t, n, cuda
        self.p, self.h, self.wc, self.bc = R.pool_inputs(n, d, l, t, 1000 + n + d, scale) if inputs is None else inputs
        self.dm, self.da = R.grad_inputs(n, l, t, n)
        self.sa, self.sb = R.seeds(n, d)
        self.dev = {k: getattr(self, k).to(cuda) for k in ("p", "h", "wc", "bc", "dm", "da")}

    def masks(self, drop):
        return R.drop_masks(self.n, self.d, drop, self.sa, self.sb) if drop else (None, None)

    def fwd(self, drop=0.0):
        from toad_amd import ops
        v = self.dev
        return ops.gated_pool_fwd(v["p"], self.d, v["h"], v["wc"], v["bc"], drop, self.sa, self.sb)

    def bwd(self, fw, ext=None, drop=0.0, **kw):
        """ops.gated_pool_bwd on the device forward ``fw``; ``ext``: None, True (the family's da_ext) or a device tensor."""
        from toad_amd import ops
        v = self.dev
        a_raw, m, stats = fw
        ext = v["da"] if ext is True else ext
        return ops.gated_pool_bwd(v["p"], self.d, v["h"], v["wc"], a_raw, stats, m, v["dm"], ext, drop_p=drop, seed_a=self.sa, seed_b=self.sb, **kw)

    def ref(self, ext=False, drop=0.0, dtype=torch.float64):
        ma, mb = self.masks(drop)
        return R.reference(self.p, self.h, self.wc, self.bc, self.dm, self.da if ext else None, ma, mb, dtype)


def _check_amax(amax_dev, dp_dev, n, what, cap):
    """The bound of every 256-row block holds against the device's own dP; with ``cap`` it is within R.CAP of it. Returns the ratios."""
    nb = (n + R.ROWBLK - 1) // R.ROWBLK
    assert amax_dev.numel() >= nb
    amax = amax_dev[:nb].cpu().double()
    mx = R.fold256(dp_dev.cpu())
    assert torch.isfinite(amax).all() and (amax >= 0).all(), what
    nz = mx > 0
    r = amax[nz] / mx[nz]
    msg = f"{what}: bound / max |dP| per block from {r.min().item() if nz.any() else float('nan'):.3f} to {r.max().item() if nz.any() else float('nan'):.3f}"
    bad = amax * SLACK < mx
    assert not bad.any(), f"{msg}; blocks {bad.nonzero().flatten().tolist()[:4]} lie BELOW their maximum"
    if cap and nz.any():
        over = torch.zeros_like(nz); over[nz] = r > R.CAP
        assert not over.any(), f"{msg}; blocks {over.nonzero().flatten().tolist()[:4]} exceed {R.CAP:g} x their maximum"
    return r


# ---- A. the abs-max array, single-slide route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,scale", [(n, 1.0) for n in R.AMAX_NS] + [(513, 4.0)])
@pytest.mark.parametrize("d,l,t", R.EXACT_SHAPES + R.COVER_SHAPES)
def test_amax_bounds_dp_in_every_block_and_is_not_slack(cuda, d, l, t, n, scale):
    """n = 4097 / 12289 pass the 512-workgroup cap (a workgroup takes a second row step); 255 ... 513 put block edges everywhere in a step."""
    c = _Case(cuda, d, l, t, n, scale)
    lo, hi = float("inf"), 0.0
    for drop in (0.0, R.DROP_P):
        fw = c.fwd(drop)
        for ext in (None, True):
            dp, _, _, _, amax = c.bwd(fw, ext, drop, want_amax=True)
            r = _check_amax(amax, dp, n, f"{(d, l, t)} n={n} scale={scale:g} drop={drop} da_ext={ext is not None}", cap=(d, l, t) in R.ORDINARY_SHAPES)
            if r.numel():
                lo, hi = min(lo, r.min().item()), max(hi, r.max().item())
    print(f"POOLBWD ratio {(d, l, t)} n={n} scale={scale:g}: {lo:.3f} .. {hi:.3f}")


@pytest.mark.parametrize("r", [255, 256, 767, 999])
@pytest.mark.parametrize("d,l,t", [(384, 512, 2), (100, 200, 1)])
def test_amax_of_one_large_row_lands_in_its_own_block(cuda, d, l, t, r):
    """da_ext = 1e4 in row r only: block r // 256 must carry it, and no other block may - each stays within the cap of its OWN maximum
    (a fine-table entry folded into the wrong slot would lift a neighbour 10^4-fold, or leave r's block too small)."""
    n = 1000
    c = _Case(cuda, d, l, t, n)
    ext = torch.zeros(n, t); ext[r] = 1e4
    for drop in (0.0, R.DROP_P):
        fw = c.fwd(drop)
        dp, _, _, _, amax = c.bwd(fw, ext.to(cuda), drop, want_amax=True)
        ratios = _check_amax(amax, dp, n, f"{(d, l, t)} row {r} drop={drop}", cap=False)
        assert ratios.numel() == 4
        mx = R.fold256(dp.cpu())
        others = [b for b in range(4) if b != r // 256]
        assert all(ratios[b].item() <= R.CAP for b in others), (r, drop, ratios.tolist())
        assert mx[r // 256].item() > 100 * max(mx[b].item() for b in others)          # the row really dominates its block alone
        assert amax[r // 256].item() > 100 * max(amax[b].item() for b in others)


@pytest.mark.parametrize("d,l,t", [(384, 512, 2), (260, 520, 2)])
def test_options_change_no_other_output_and_runs_repeat_bitwise(cuda, d, l, t):
    n = 1000
    c = _Case(cuda, d, l, t, n)
    for drop in (0.0, R.DROP_P):
        fw = c.fwd(drop)
        plain = c.bwd(fw, True, drop)
        assert len(plain) == 4 and plain[1] is not None
        for want_amax in (False, True):
            for want_dh in (False, True):
                for _ in range(2):
                    out = c.bwd(fw, True, drop, want_amax=want_amax, want_dh=want_dh)
                    assert len(out) == (5 if want_amax else 4)
                    assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2]) and torch.equal(out[3], plain[3])
                    assert (out[1] is None) if not want_dh else torch.equal(out[1], plain[1])
                    if want_amax:
                        _check_amax(out[4], out[0], n, f"{(d, l, t)} want_dh={want_dh}", cap=True)
        a1, a2 = c.bwd(fw, True, drop, want_amax=True)[4], c.bwd(fw, True, drop, want_amax=True)[4]
        assert torch.equal(a1[:4], a2[:4])


@pytest.mark.parametrize("n", [257, 3000])
@pytest.mark.parametrize("d,l,t", R.EXACT_SHAPES)
def test_consumers_lose_nothing_to_the_bound(cuda, d, l, t, n):
    """The attention weight gradient and dgrad with dy_amax = the pool's bound against the same calls with the measured abs-max of dP:
    e_bound <= max(8 e_exact, the op's own bound in test_gpu_kernels.py) - the bound may cost at most the three bits the cap allows."""
    from toad_amd import ops
    c = _Case(cuda, d, l, t, n)
    fw = c.fwd()
    dp, _, _, _, amax = c.bwd(fw, True, want_amax=True, want_dh=False)
    h = c.dev["h"]
    exact = ops.absmax_rows256(dp)
    g = torch.Generator().manual_seed(n + d)
    w = torch.randn(2 * d, 512, generator=g) * 0.05
    wt = ops.transpose(w.to(cuda))
    dp64, h64 = dp.cpu().double(), c.h.double()
    ref_w, ref_x = dp64.t() @ h64, dp64 @ w.double()
    hmax = ops.absmax_rows256(h)
    err = {}
    for name, am in (("bound", amax), ("exact", exact)):
        dw, _ = ops.linear_wgrad(dp, h, dy_amax=am, x_amax=hmax)
        dx = ops.linear_dgrad(dp, wt, dy_amax=am)
        err[name] = (_rel(dw.cpu(), ref_w), _rel(dx.cpu(), ref_x))
    print(f"POOLBWD downstream {(d, l, t)} n={n}: wgrad e_exact {err['exact'][0]:.3e} e_bound {err['bound'][0]:.3e}; "
          f"dgrad e_exact {err['exact'][1]:.3e} e_bound {err['bound'][1]:.3e}")
    assert err["bound"][0] <= max(8 * err["exact"][0], 2e-5), err
    assert err["bound"][1] <= max(8 * err["exact"][1], 1e-5), err


# ---- B. values against float64 --------------------------------------------------------------------------------------------------------------
def _check_values(what, out, ref, ref32, n, ext):
    """(dP, dH, dWc, dbc) of the device against the float64 reference under the tolerances of test_gpu_kernels.py::test_gated_pool_bwd;
    where the fp32 round-off of the reference's own arithmetic (ref32 against ref) is larger than a tolerance, 10 x that round-off."""
    dp, dh, dwc, dbc = out
    fl = 0.1 if (n == 1 and not ext) else 1e-3
    for name, got, key, tol, floor in (("dP", dp, "dp", 5e-5, fl), ("dH", dh, "dh", 2e-5, 1e-3), ("dWc", dwc, "dwc", 5e-5, fl)):
        assert torch.isfinite(got).all(), (what, name)
        noise = _rel(ref32[key], ref[key], floor)
        err = _rel(got.cpu(), ref[key], floor)
        print(f"POOLBWD values {what} {name}: err {err:.2e} fp32 noise of the reference {noise:.2e}")
        assert err <= max(tol, 10 * noise), (what, name, err, noise)
    assert torch.isfinite(dbc).all(), (what, "dbc")
    noise = (ref32["dbc"].double() - ref["dbc"]).abs().max().item()
    err = (dbc.cpu().double() - ref["dbc"]).abs().max().item()
    print(f"POOLBWD values {what} dbc: abs err {err:.2e} fp32 noise of the reference {noise:.2e}")
    assert err <= max(5e-5 * max(ref["dbc"].abs().max().item(), 1.0), 10 * noise), (what, "dbc", err, noise)


@pytest.mark.parametrize("n", [1, 2, 3, 9, 65])
@pytest.mark.parametrize("d,l,t", R.COVER_SHAPES)
def test_covering_shapes_with_few_rows_against_fp64(cuda, d, l, t, n):
    from toad_amd import ops
    c = _Case(cuda, d, l, t, n)
    fw = c.fwd()
    for ext in (False, True):
        ref, ref32 = c.ref(ext), c.ref(ext, dtype=torch.float32)
        _check_values(f"{(d, l, t)} n={n} da_ext={ext}", c.bwd(fw, True if ext else None), ref, ref32, n, ext)
    # beta = 1 on top of an existing gradient (ref: the da_ext run above)
    g = torch.Generator().manual_seed(n)
    bw, bb = torch.randn(t, d, generator=g), torch.randn(t, generator=g)
    aw, ab = bw.to(cuda), bb.to(cuda)
    v = c.dev
    ops.gated_pool_bwd(v["p"], d, v["h"], v["wc"], fw[0], fw[2], fw[1], v["dm"], v["da"], aw, ab, 1.0)
    assert _rel(aw.cpu(), ref["dwc"] + bw) <= 5e-5 and _rel(ab.cpu(), ref["dbc"] + bb) <= 5e-5


@pytest.mark.parametrize("n", [9, 777])
@pytest.mark.parametrize("d,l,t", [(384, 512, 2), (100, 200, 1), (260, 520, 2)])
def test_dropout_backward_against_fp64_with_host_masks(cuda, d, l, t, n):
    """drop_p = 0.25 on both gate branches: the kernel recomputes the masks from the seeds; the reference takes them from tests/drop_ref
    (element (row, column) at row * D + column). Elements either branch drops get EXACTLY zero in dPa and in dPb (both carry ka * kb)."""
    c = _Case(cuda, d, l, t, n)
    ma, mb = c.masks(R.DROP_P)
    fw = c.fwd(R.DROP_P)
    dropped = (ma == 0) | (mb == 0)
    share = dropped.float().mean().item()
    assert 0.3 <= share <= 0.55, share                           # 7/16 expected
    for ext in (False, True):
        ref, ref32 = c.ref(ext, R.DROP_P), c.ref(ext, R.DROP_P, dtype=torch.float32)
        if not ext:
            assert (fw[0].cpu().double() - ref["a_raw"]).abs().max().item() <= 1e-5 and (fw[1].cpu().double() - ref["m"]).abs().max().item() <= 1e-5
        out = c.bwd(fw, True if ext else None, R.DROP_P)
        _check_values(f"dropout {(d, l, t)} n={n} da_ext={ext}", out, ref, ref32, n, ext)
        dp = out[0].cpu()
        assert (dp[:, :d][dropped] == 0).all() and (dp[:, d:][dropped] == 0).all()
        assert (ref["dpa"][dropped] == 0).all() and (ref["dpb"][dropped] == 0).all()
        kept_nonzero = (dp[:, :d][~dropped] != 0).float().mean().item()
        assert kept_nonzero > 0.99, kept_nonzero                 # ... and only those
    # the masks are the seeds': other seeds, other zeros
    from toad_amd import ops
    v = c.dev
    other = ops.gated_pool_bwd(v["p"], d, v["h"], v["wc"], fw[0], fw[2], fw[1], v["dm"], v["da"], drop_p=R.DROP_P, seed_a=c.sa + 1, seed_b=c.sb + 1)[0].cpu()
    assert ((other[:, :d] == 0) != dropped).float().mean().item() > 0.3          # two independent patterns differ on 2 * 7/16 * 9/16 of the elements


def _saturated_inputs(which):
    """The two inputs of test_gpu_kernels.py::test_gated_pool_softmax_saturation_and_rescale."""
    d, l, t, n = 384, 512, 2, 4099
    p, h, wc, bc = R.pool_inputs(n, d, l, t, 11)
    wc = wc.abs() * 3.0
    if which == "ramp":
        ramp = torch.linspace(-6, 6, n)[:, None]
        p = torch.cat([ramp.expand(n, d) + 0.1 * p[:, :d], 4.0 + 0.0 * p[:, d:]], 1).contiguous()
        p[n - 7, :d] = 15.0
        return p, h, wc, bc
    p2 = torch.cat([torch.full((64, d), 90.0), torch.full((64, d), -95.0)], 1)
    p2[::2] *= -1
    return p2, h[:64].contiguous(), wc, bc


@pytest.mark.parametrize("which", ["ramp", "gates"])
def test_saturated_softmax_and_gates_through_the_backward(cuda, which):
    inputs = _saturated_inputs(which)
    n = inputs[0].shape[0]
    c = _Case(cuda, 384, 512, 2, n, inputs=inputs)
    fw = c.fwd()
    for ext in (False, True):
        ref, ref32 = c.ref(ext), c.ref(ext, dtype=torch.float32)
        if which == "ramp":
            assert (ref["a_raw"].max(0).values - ref["a_raw"].min(0).values).min().item() > 50
        _check_values(f"saturated {which} da_ext={ext}", c.bwd(fw, True if ext else None), ref, ref32, n, ext)


@pytest.mark.parametrize("n", [1, 9, 257])
@pytest.mark.parametrize("d,l,t", [(384, 512, 2), (100, 200, 1), (260, 520, 2)])
def test_rows_past_n_stay_unwritten(cuda, d, l, t, n):
    """dP and dH handed in as the first n rows of buffers with 8 more: a wave step covers 8 rows, so the rows a partly valid step would
    reach past N must keep their sentinel (columns past D / L of a row are the next row's, or dPb's: the value tests hold those)."""
    c = _Case(cuda, d, l, t, n)
    sentinel = -7777.0
    for drop in (0.0, R.DROP_P):
        fw = c.fwd(drop)
        plain = c.bwd(fw, True, drop)
        dp = torch.full((n + 8, 2 * d), sentinel, device=cuda); dh = torch.full((n + 8, l), sentinel, device=cuda)
        out = c.bwd(fw, True, drop, dp=dp[:n], dh=dh[:n])
        assert out[0].data_ptr() == dp.data_ptr() and out[1].data_ptr() == dh.data_ptr()
        assert torch.equal(dp[:n], plain[0]) and torch.equal(dh[:n], plain[1])
        assert (dp[n:] == sentinel).all() and (dh[n:] == sentinel).all()


# ---- C. the batched launch ------------------------------------------------------------------------------------------------------------------
LENS = [3, 250, 9, 515, 1, 300]             # boundaries inside 8-row steps and inside 256-row blocks of the concatenation
WEIGHT_EXP = (-4, 3, -2, 2, 0, -4)          # the loss term on slide b's scores weighs 10^k_b: neighbours' dP differ by up to 10^7 inside one block
TRUNK = ("w1", "b1", "w2", "b2")


@pytest.mark.parametrize("half", [False, True])
def test_ragged_batch_with_score_gradients_seven_decades_apart(cuda, half):
    """A per-row bound shifted by one slide puts a 10^7 times too small scale under a neighbour's dP (fp16 overflow: non-finite gradients), or a
    10^7 times too large one (its pieces vanish). All 14 gradients are finite, equal the per-slide one-slide route, and the six attention
    gradients equal the float64 oracle backward on the device's activations with each slide's own da_ext."""
    from tests.test_gpu_forward_batch import _dev, _grads, _model, _slides
    from toad_amd import ops
    cls = 18
    model, params = _model(cuda, c=cls, seed=57)
    slides = _slides(LENS, cls, seed=29)
    if half:
        slides = [(s[0].half(),) + s[1:] for s in slides]
    dev = _dev(slides, cuda)
    B, ntot, d = len(LENS), sum(LENS), model._weights()["wc"].shape[1]
    g = torch.Generator().manual_seed(77)
    coef = [torch.randn(2, n, generator=g) for n in LENS]
    coef_dev = [c.to(cuda) for c in coef]
    sex = torch.cat([s[1] for s in dev])

    def loss_of(o, b):
        s = dev[b]
        return (0.75 * F.cross_entropy(o["logits"], s[2]) + 0.25 * F.cross_entropy(o["site_logits"], s[3])) / B + 10.0 ** WEIGHT_EXP[b] * (o["A"] * coef_dev[b]).sum()

    outs = model.forward_batch([s[0] for s in dev], sex)
    sum(loss_of(o, b) for b, o in enumerate(outs)).backward()
    got = _grads(model)
    for slot in SLOT2KEY:
        assert torch.isfinite(got[slot]).all(), slot
    model.zero_grad(set_to_none=True)
    for b, s in enumerate(dev):
        loss_of(model(s[0], s[1]), b).backward()
    ref = _grads(model)
    for slot in SLOT2KEY:
        sc = max(grad_scale(ref, slot), grad_scale(ref, {"ba": "wa", "bb": "wb"}.get(slot, slot)))
        chk = assert_grad_close_or_few_flips if slot in TRUNK else assert_grad_close
        chk(got[slot], ref[slot], 5e-5, sc, what=f"batch vs per-slide ({'fp16' if half else 'fp32'} bags): {slot}")
    # the six attention gradients against the oracle in float64 on the device's activations (the same forward again through ops: bitwise)
    w = {k: v.detach() for k, v in model._weights().items()}
    arena, o = ops.mil_multi_fwd(w, [s[0] for s in dev], sex)
    assert torch.equal(o["logits"], torch.cat([r["logits"].detach() for r in outs]))
    v = arena.view
    act = dict(h1=v("h1", (ntot, 512)).cpu(), h=v("h", (ntot, 512)).cpu(), p=v("p", (ntot, 2 * d)).cpu(), a_raw=o["a_raw"].cpu())
    p64 = {k: t.double() for k, t in params.items()}
    tot = {torch.float64: {k: 0.0 for k in params}, torch.float32: {k: 0.0 for k in params}}
    r0 = 0
    for b, (x, sx, lb, st) in enumerate(slides):
        r1 = r0 + LENS[b]
        for dt, pp in ((torch.float64, p64), (torch.float32, params)):
            s_ = orc.Saved(x=x.to(dt), h1=act["h1"][r0:r1].to(dt), h=act["h"][r0:r1].to(dt), p=act["p"][r0:r1].to(dt), a_raw=act["a_raw"][r0:r1].to(dt),
                           m=None, mcat=None, sex=sx.to(dt))
            s_.m = orc.softmax_pool(s_.a_raw, s_.h)
            s_.mcat, lg, _, _, sl, _, _ = orc.heads_fwd(s_.m, s_.sex, pp["classifier.weight"], pp["classifier.bias"], pp["site_classifier.weight"],
                                                         pp["site_classifier.bias"])
            dl, ds = orc.loss_grad(lg, lb, sl, st)
            gb = orc.backward(pp, s_, dl / B, ds / B, da_ext=(10.0 ** WEIGHT_EXP[b] * coef[b].t()).to(dt))
            for k in gb:
                tot[dt][k] = tot[dt][k] + gb[k].double()
        r0 = r1
    t64, t32 = tot[torch.float64], tot[torch.float32]
    for slot in ("wc", "bc", "wa", "wb", "ba", "bb"):
        key = SLOT2KEY[slot]
        noise = (t32[key] - t64[key]).abs().max().item()
        assert_grad_close(got[slot], t64[key], 2e-5, grad_scale(t64, key), what=f"batch vs fp64 oracle ({'fp16' if half else 'fp32'} bags): {key}",
                          floor=(32.0 if slot in ("ba", "bb", "bc") else 10.0) * noise)
