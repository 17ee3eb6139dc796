"""GPU: the per-slide step tail (csrc/heads.hip) away from the model's one shape - the fused heads + CE + heads-backward launch on all three of its
staging paths, the standalone kernels, the optimisers past one grid-stride trip - against the fp64 host statement tests/tail_ref.py.

Bounds. Dot products (logits, dM): the kernels' own rounding model, tail_ref.dot_bound. Copies and outer products (Mcat, dW, db): one rounding,
2^-23 |value|, plus the same for the beta term. Softmax / CE at ordinary scales (weights 0.1 randn, M randn): 1e-5 on probabilities and loss, 1e-6
on dlogits / dsite (tests/test_gpu_kernels.py). Large logits and underflow: 8 x the deviation of the oracle's fp32 CPU functions from tail_ref on
the same case, floor 4 ulp of the result. Optimisers: 4 x the deviation of torch's fp32 CPU optimiser from tail_ref, floor 2 ulp. The fused launch
against the three-call chain, run against run and guard elements: torch.equal.
"""

import math

import numpy as np
import pytest
import torch

from oracle import toad_oracle as orc
from tests import tail_ref as tr

pytestmark = pytest.mark.gpu

W_CLS, W_SITE = 0.75, 0.25
OUT_NAMES = ("mcat", "logits", "y_prob", "y_hat", "site_logits", "site_prob", "site_hat")


def _inputs(L, C, seed=None):
    g = torch.Generator().manual_seed(1000 * L + C if seed is None else seed)
    return dict(m=torch.randn(2, L, generator=g), sex=torch.tensor([1.0 if (L + C) % 2 else -0.5]),      # never 0: a zero would hide the weights' last column
                wcls=torch.randn(C, L + 1, generator=g) * 0.1, bcls=torch.randn(C, generator=g) * 0.1,
                wsite=torch.randn(2, L + 1, generator=g) * 0.1, bsite=torch.randn(2, generator=g) * 0.1,
                ext=torch.randn(2, L + 1, generator=g),
                prev=(torch.randn(C, L + 1, generator=g), torch.randn(C, generator=g), torch.randn(2, L + 1, generator=g), torch.randn(2, generator=g)))


def _off4(t, dev):
    """``t`` on the device, 4 bytes into a larger allocation: off the 16-byte boundary the vector path wants."""
    big = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    v = big[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _n(t):
    return t.detach().cpu().double().numpy()


def _labels(C):
    return sorted({0, C - 1, C // 2})


def _fused(lib, d, label, site, beta, export, grads):
    """toad_heads_ce_fused_f32 through the C ABI on the device tensors of ``d``; ``grads`` are overwritten / accumulated into."""
    L, C = d["m"].shape[1], d["wcls"].shape[0]
    dev = d["m"].device
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int64, device=dev)
    o = dict(mcat=f(2, L + 1), logits=f(1, C), y_prob=f(1, C), y_hat=i(1, 1), site_logits=f(1, 2), site_prob=f(1, 2), site_hat=i(1, 1), loss=f(3),
             dlogits=f(1, C) if export else None, dsite=f(1, 2) if export else None, dm=f(2, L))
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.toad_heads_ce_fused_f32(p(d["m"]), p(d["sex"]), p(d["wcls"]), p(d["bcls"]), p(d["wsite"]), p(d["bsite"]), p(label), p(site), W_CLS, W_SITE,
                                     p(o["mcat"]), p(o["logits"]), p(o["y_prob"]), p(o["y_hat"]), p(o["site_logits"]), p(o["site_prob"]), p(o["site_hat"]),
                                     p(o["loss"]), p(o["dlogits"]), p(o["dsite"]), p(grads[0]), p(grads[1]), p(grads[2]), p(grads[3]), p(o["dm"]),
                                     float(beta), L, C, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib.toad_last_error().decode())
    return o


def _chain(ops, d, label, site, beta, grads, ext=None, want_dsex=False):
    outs = ops.heads_fwd(d["m"], d["sex"], d["wcls"], d["bcls"], d["wsite"], d["bsite"])
    o = dict(zip(OUT_NAMES, outs))
    o["loss"], o["dlogits"], o["dsite"] = ops.mtl_ce_fwd_bwd(o["logits"], o["site_logits"], label, site, W_CLS, W_SITE)
    r = ops.heads_bwd(o["mcat"], o["dlogits"], o["dsite"], d["wcls"], d["wsite"], ext, grads=grads, beta=beta, want_dsex=want_dsex)
    o["dm"] = r[4]
    if want_dsex:
        o["dsex"] = r[5]
    return o


class _Ref:
    """tail_ref on one set of inputs: the forward once, the loss per (label, site)."""

    def __init__(self, c):
        self.c = {k: (_n(v) if torch.is_tensor(v) else v) for k, v in c.items()}
        self.fwd = tr.heads_fwd(*(self.c[k] for k in ("m", "sex", "wcls", "bcls", "wsite", "bsite")))
        mcat = self.fwd[0]
        # what the dot-product bound scales with: sum_k |w_k x_k| + |bias|
        self.abs_lg = np.abs(self.c["wcls"]) @ np.abs(mcat[0]) + np.abs(self.c["bcls"])
        self.abs_sl = np.abs(self.c["wsite"]) @ np.abs(mcat[1]) + np.abs(self.c["bsite"])
        self._ce = {}

    def ce(self, label, site):
        if (label, site) not in self._ce:
            self._ce[(label, site)] = tr.ce(self.fwd[1], label, self.fwd[4], site, W_CLS, W_SITE)
        return self._ce[(label, site)]


def _within(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    bad = err > tol
    assert not bad.any(), f"{what}: err {err.max():.3e} over the bound at {np.argwhere(bad)[:3].tolist()} (bound there {np.broadcast_to(tol, err.shape)[bad][:3]})"
    return float(err.max())


def _check_forward(o, ref, what, scales="ordinary"):
    """Forward outputs and the loss triple against tail_ref computed from the inputs."""
    L = ref.c["m"].shape[1]
    mcat, lg, prob, hat, sl, sprob, shat = ref.fwd
    _within(_n(o["mcat"]), mcat, 2.0 ** -23 * np.abs(mcat), what + " Mcat")
    e_lg = _within(_n(o["logits"]), lg, tr.dot_bound(ref.abs_lg, lg, tr.row_depth(L)), what + " logits")
    e_sl = _within(_n(o["site_logits"]), sl, tr.dot_bound(ref.abs_sl, sl, tr.row_depth(L)), what + " site_logits")
    if scales == "ordinary":
        _within(_n(o["y_prob"]), prob, 1e-5, what + " Y_prob")
        _within(_n(o["site_prob"]), sprob, 1e-5, what + " site_prob")
        # the arg-max is decided where the reference's two largest logits are further apart than twice the error the logits show
        for z, e, got, want, nm in ((lg, e_lg, o["y_hat"], hat, "Y_hat"), (sl, e_sl, o["site_hat"], shat, "site_hat")):
            top = np.sort(z)[::-1]
            assert len(top) == 1 or top[0] - top[1] > 2 * e, f"{what}: the test's own {nm} is not decided"
            assert int(got.item()) == want, f"{what} {nm}"


def _check_loss(o, ref, label, site, what):
    loss, dl, ds = ref.ce(label, site)
    _within(_n(o["loss"]), loss, 1e-5, what + " loss")
    if o.get("dlogits") is not None:
        _within(_n(o["dlogits"]), dl, 1e-6, what + " dlogits")
        _within(_n(o["dsite"]), ds, 1e-6, what + " dsite")


def _check_backward(got_grads, dm, dsex, ref, dl_dev, ds_dev, prev, beta, ext, what):
    """The heads backward against tail_ref.heads_bwd on the DEVICE's own Mcat (a copy of the inputs), dlogits and dsite: outer products are one
    rounding (+ one for the beta term), dM a C-term serial sum."""
    c = ref.c
    C = c["wcls"].shape[0]
    dl, ds = _n(dl_dev).reshape(-1), _n(ds_dev).reshape(-1)
    mcat = ref.fwd[0]
    r = tr.heads_bwd(mcat, dl, ds, c["wcls"], c["wsite"], ext, prev=prev, beta=beta)
    new = (np.outer(dl, mcat[0]), dl, np.outer(ds, mcat[1]), ds)
    for g, want, nw, pv, nm in zip(got_grads, r[:4], new, prev, ("dWcls", "dbcls", "dWsite", "dbsite")):
        _within(_n(g), want, 2.0 ** -23 * (np.abs(nw) + abs(beta) * np.abs(pv)), f"{what} {nm}")
    L = mcat.shape[1] - 1
    e = np.zeros((2, L + 1)) if ext is None else np.abs(ext)
    a0 = np.abs(dl) @ np.abs(c["wcls"]) + e[0]
    a1 = np.abs(ds) @ np.abs(c["wsite"]) + e[1]
    _within(_n(dm)[0], r[4][0], tr.dot_bound(a0[:L], r[4][0], C), what + " dM[0]")
    _within(_n(dm)[1], r[4][1], tr.dot_bound(a1[:L], r[4][1], 2), what + " dM[1]")
    if dsex is not None:
        _within(_n(dsex), r[5], tr.dot_bound(a0[L] + a1[L], r[5], C + 4), what + " dsex")


FUSED_CASES = [(L, C, None) for L, C in tr.FUSED_SHAPES] + [(L, C, mis) for L, C in tr.MISALIGNED_SHAPES for mis in ("m", "wcls")]


@pytest.mark.parametrize("L,C,mis", FUSED_CASES, ids=[f"L{L}-C{C}" + (f"-{mis}+4B" if mis else "") for L, C, mis in FUSED_CASES])
def test_fused_entry_matches_the_statement_and_the_three_call_chain(cuda, L, C, mis):
    """toad_heads_ce_fused_f32 through the C ABI, every label in {0, interior, C - 1} x site x beta in {0, 1 onto pre-filled gradients} x dlogits /
    dsite exported or NULL: every output inside the bounds of the module docstring against tail_ref, and torch.equal to ops.heads_fwd ->
    ops.mtl_ce_fwd_bwd -> ops.heads_bwd on the same values (the header's "bitwise the results of the three calls"), on the vector, cached and
    uncached staging paths (tests/test_step_tail_host.py::test_shape_table_reaches_every_staging_path)."""
    from toad_amd import _lib, ops
    lib = _lib.load()
    c = _inputs(L, C)
    d = {k: v.to(cuda) for k, v in c.items() if k not in ("prev", "ext")}
    aligned = {k: v for k, v in d.items()}                    # the chain runs on ordinary allocations of the same values
    if mis:
        d[mis] = _off4(c[mis], cuda)
    assert tr.fused_path(L, C, aligned=not mis) == ("cached" if mis else tr.fused_path(L, C))
    assert d["m"].data_ptr() % 16 == (4 if mis == "m" else 0) and d["wcls"].data_ptr() % 16 == (4 if mis == "wcls" else 0)
    ref = _Ref({k: c[k] for k in ("m", "sex", "wcls", "bcls", "wsite", "bsite")})
    prev = [_n(t) for t in c["prev"]]
    first = True
    for label in _labels(C):
        for site in (0, 1):
            lab, sit = torch.tensor([label], device=cuda), torch.tensor([site], device=cuda)
            for beta in (0.0, 1.0):
                for export in (True, False):
                    what = f"L={L} C={C} {mis or ''} label={label} site={site} beta={beta} export={export}:"
                    gf = [t.to(cuda) for t in c["prev"]]
                    gc = [t.to(cuda) for t in c["prev"]]
                    o = _fused(lib, d, lab, sit, beta, export, gf)
                    ch = _chain(ops, aligned, lab, sit, beta, gc)
                    for k in OUT_NAMES + ("loss", "dm") + (("dlogits", "dsite") if export else ()):
                        assert torch.equal(o[k], ch[k]), f"{what} fused {k} != the three-call chain"
                    for a, b, nm in zip(gf, gc, ("dWcls", "dbcls", "dWsite", "dbsite")):
                        assert torch.equal(a, b), f"{what} fused {nm} != the three-call chain"
                    if first:
                        _check_forward(o, ref, what)
                    _check_loss(o, ref, label, site, what)
                    _check_backward(gf, o["dm"], None, ref, ch["dlogits"], ch["dsite"], prev, beta, None, what)
                    first = False


@pytest.mark.parametrize("L,C", tr.FUSED_SHAPES, ids=[f"L{L}-C{C}" for L, C in tr.FUSED_SHAPES])
def test_standalone_kernels_match_the_statement(cuda, L, C):
    """heads_fwd_kernel, mtl_ce_kernel and heads_bwd_kernel one by one over the fused entry's shapes; the backward with the caller's dMcat_ext and
    the gradient of ``sex``, beta = 0 and beta = 1."""
    from toad_amd import ops
    c = _inputs(L, C, seed=7 * L + C)
    d = {k: v.to(cuda) for k, v in c.items() if k != "prev"}
    ref = _Ref({k: c[k] for k in ("m", "sex", "wcls", "bcls", "wsite", "bsite")})
    prev, ext = [_n(t) for t in c["prev"]], _n(c["ext"])
    for i, label in enumerate(_labels(C)):
        site, beta = i % 2, float(i % 2)
        what = f"L={L} C={C} label={label} site={site} beta={beta}:"
        g = [t.to(cuda) for t in c["prev"]]
        o = _chain(ops, d, torch.tensor([label], device=cuda), torch.tensor([site], device=cuda), beta, g, ext=d["ext"], want_dsex=True)
        _check_forward(o, ref, what)
        _check_loss(o, ref, label, site, what)
        _check_backward(g, o["dm"], o["dsex"], ref, o["dlogits"], o["dsite"], prev, beta, ext, what)
    # without an external gradient, and beta = 1 where the loop above had beta = 0 only (C == 1)
    g = [t.to(cuda) for t in c["prev"]]
    o = _chain(ops, d, torch.tensor([C - 1], device=cuda), torch.tensor([1], device=cuda), 1.0, g, want_dsex=True)
    _check_backward(g, o["dm"], o["dsex"], ref, o["dlogits"], o["dsite"], prev, 1.0, None, f"L={L} C={C} no ext:")


def _both_entries(cuda, c, label, site):
    """The standalone chain and the fused entry on the CPU inputs ``c`` -> [(name, outputs)]."""
    from toad_amd import _lib, ops
    C, L = c["wcls"].shape[0], c["m"].shape[1]
    d = {k: v.to(cuda) for k, v in c.items() if torch.is_tensor(v)}
    lab, sit = torch.tensor([label], device=cuda), torch.tensor([site], device=cuda)
    z = lambda: [torch.zeros(C, L + 1, device=cuda), torch.zeros(C, device=cuda), torch.zeros(2, L + 1, device=cuda), torch.zeros(2, device=cuda)]
    return [("standalone", _chain(ops, d, lab, sit, 0.0, z())), ("fused", _fused(_lib.load(), d, lab, sit, 0.0, True, z()))]


@pytest.mark.parametrize("L,C,tied", [(512, 100, (5, 40)), (512, 100, (70, 90, 99)), (512, 100, (10, 70)), (128, 99, (3, 64, 98)), (512, 18, (2, 17)),
                                      (64, 64, (62, 63)), (512, 100, (6, 70)), (128, 99, (3, 67)), (512, 512, (1, 65, 449))])
def test_tied_maximal_logits_give_the_smallest_index(cuda, L, C, tied):
    """Two and three exactly equal maximal logits (duplicate weight rows, equal biases), below and above the 64 lanes of the arg-max wave: Y_hat is
    the smallest tied index (torch.topk) and the tied probabilities are equal. (6, 70), (3, 67) and (1, 65, 449) tie WITHIN one lane of the
    lane-strided loop (indices 64 apart), the others across lanes: the two halves of the arg-max reduction."""
    c = _inputs(L, C, seed=L + C + sum(tied))
    c["wcls"] *= 0.1                                            # the other rows: logits of std ~0.2
    row = c["m"][0] * (3.0 / float((c["m"][0] ** 2).sum()))     # logit ~3 on this bag
    for t in tied:
        c["wcls"][t, :L] = row; c["wcls"][t, L] = 0.0; c["bcls"][t] = 0.25
    ref = _Ref(c)
    lg = ref.fwd[1]
    assert lg[list(tied)].min() > np.delete(lg, list(tied)).max() + 1.0 and ref.fwd[3] == min(tied)       # the test's own construction
    for name, o in _both_entries(cuda, c, tied[-1], 0):
        lgd, pr = o["logits"].cpu()[0], o["y_prob"].cpu()[0]
        assert all(lgd[t] == lgd[tied[0]] for t in tied), f"{name}: duplicate rows gave different logits"
        assert int(o["y_hat"].item()) == min(tied), f"{name}: Y_hat {int(o['y_hat'].item())}, tied {tied}"
        assert all(pr[t] == pr[tied[0]] for t in tied), f"{name}: tied probabilities differ"
        _check_forward(o, ref, f"{name} ties {tied}", scales="ties")
        _within(_n(o["y_prob"]), ref.fwd[2], 1e-5, f"{name} ties Y_prob")
        _check_loss(o, ref, tied[-1], 0, f"{name} ties")


def _oracle_fp32(c, label, site):
    """The oracle's fp32 CPU functions on the same case -> the outputs the yardstick is taken from."""
    mcat, lg, prob, hat, sl, sprob, shat = orc.heads_fwd(c["m"], c["sex"], c["wcls"], c["bcls"], c["wsite"], c["bsite"])
    lb, st = torch.tensor([label]), torch.tensor([site])
    cef = torch.nn.functional.cross_entropy
    lc, ls = cef(lg, lb), cef(sl, st)
    dl, ds = orc.loss_grad(lg, lb, sl, st)
    return dict(y_prob=prob, site_prob=sprob, loss=torch.stack([orc.loss_fn(lg, lb, sl, st), lc, ls]), dlogits=dl, dsite=ds, y_hat=hat, site_hat=shat)


LARGE_CASES = [("plus_1e4_labelled", 1e4, "same"), ("plus_1e4_other_label", 1e4, "other"), ("minus_1e4_labelled_underflow", -1e4, "same"),
               ("plus_120_other_label_underflow", 120.0, "other")]
_RATIOS = {}


@pytest.mark.parametrize("name,target,which", LARGE_CASES, ids=[c[0] for c in LARGE_CASES])
@pytest.mark.parametrize("L,C", [(512, 18), (512, 100)])
def test_large_logits_and_underflowing_label(cuda, L, C, name, target, which):
    """One classifier row and one site row scaled so that their logits are about +-1e4 (and +120: the label's probability underflows fp32 but not
    its logarithm): the maximum is subtracted, so probabilities, loss and gradients are finite, and the loss of a label whose probability is 0 in
    fp32 is the fp64 lse - logit, not inf. Bound: 8 x the deviation of the oracle's fp32 CPU functions from tail_ref, floor 4 ulp of the result.
    Measured on an MI355X (printed per case, both entries): the device's deviation is at most 1.24 x the oracle's (Y_prob 1.24, loss 1.18, dlogits
    1.09, site outputs 1.00) and at most 0.16 of what the bound allows."""
    c = _inputs(L, C, seed=31 * L + C)
    r = 3
    for wkey, t in (("wcls", 0), ("wsite", 1)):
        row = c[wkey][r if wkey == "wcls" else 1]
        row[:L] = c["m"][t] * (target / float((c["m"][t] ** 2).sum())); row[L] = 0.0
    label = r if which == "same" else C - 1
    site = 1 if which == "same" else 0
    ref = _Ref({k: c[k] for k in ("m", "sex", "wcls", "bcls", "wsite", "bsite")})
    want = dict(zip(("loss", "dlogits", "dsite"), ref.ce(label, site)), y_prob=ref.fwd[2], site_prob=ref.fwd[5])
    assert abs(ref.fwd[1][r] - target) < 1.0 + 1e-3 * abs(target)
    if which == "other" or target < 0:
        assert want["loss"][1] > 100.0                                               # the label's probability is below fp32's smallest normal
    orc32 = _oracle_fp32(c, label, site)
    for ename, o in _both_entries(cuda, c, label, site):
        _check_forward(o, ref, f"{ename} {name}", scales="large")                    # logits: the dot-product bound holds at any scale
        for z, got, hat in ((ref.fwd[1], o["y_hat"], ref.fwd[3]), (ref.fwd[4], o["site_hat"], ref.fwd[6])):
            top = np.sort(z)[::-1]
            if len(top) == 1 or top[0] - top[1] > 1e-3 * max(1.0, abs(top[0])):          # decided beyond the logits' own rounding
                assert int(got.item()) == hat, f"{ename} {name} arg-max"
        for k in ("y_prob", "site_prob", "loss", "dlogits", "dsite"):
            w = np.asarray(want[k], dtype=np.float64).reshape(-1)
            yard = float(np.abs(_n(orc32[k]).reshape(-1) - w).max())
            tol = np.maximum(8.0 * yard, 4.0 * tr.ulp32(w))
            err = _within(_n(o[k]).reshape(-1), w, tol, f"{ename} {name} {k}")
            allowed = float(np.max(tol))
            print(f"large-logit {name} L={L} C={C} {ename} {k}: device {err:.3e} oracle-fp32 {yard:.3e} allowed {allowed:.3e} device/allowed {err / allowed:.3f}")


# ---- optimisers ---------------------------------------------------------------------------------------------------------------------------
F32 = lambda x: float(np.float32(x))          # the C ABI takes floats: every implementation is given the SAME real numbers, the fp32 values
GRID_FLOATS = 2048 * 256 * 4                  # one trip of the capped grid: 2,097,152 elements
OPT_LENGTHS = [4, 1020, GRID_FLOATS, GRID_FLOATS + 4, 3 * GRID_FLOATS + 8]
GUARD = 64
ADAM_RUNS = [("default_wd1e-5", dict(lr=F32(2e-4), betas=(F32(0.9), F32(0.999)), eps=F32(1e-8), weight_decay=F32(1e-5)), (1, 2, 3), False),
             ("default_wd0", dict(lr=F32(2e-4), betas=(F32(0.9), F32(0.999)), eps=F32(1e-8), weight_decay=0.0), (1, 2, 3), False),
             ("betas_.5_.9_eps1e-3", dict(lr=F32(1e-3), betas=(0.5, F32(0.9)), eps=F32(1e-3), weight_decay=F32(1e-5)), (1, 2, 3), False),
             ("resume_step1000", dict(lr=F32(2e-4), betas=(F32(0.9), F32(0.999)), eps=F32(1e-8), weight_decay=F32(1e-5)), (1000, 1001), True)]


def _grad(n, gen):
    """N(0, 1e-2) with exact zeros in a quarter of the entries and one block of 1e-12 magnitudes."""
    g = torch.randn(n, generator=gen) * 1e-2
    g[torch.rand(n, generator=gen) < 0.25] = 0.0
    lo = n // 3 - (n // 3) % 4
    hi = min(n, lo + max(4, min(n // 8, 4096)))
    g[lo:hi] *= 1e-10
    return g


def _guarded(t, dev, fill):
    buf = torch.full((t.numel() + GUARD,), fill, dtype=torch.float32, device=dev)
    buf[:t.numel()].copy_(t)
    return buf


def _opt_check(name, dev_t, ref64, yard32, scale, n):
    """device within max(4 x torch-fp32's deviation, 2 ulp) of tail_ref; deviations in ulps of ``scale`` - the largest magnitude the element's
    update passes through (its old and new value, the increment), since a result that cancels carries the round-off of its operands."""
    u = tr.ulp32(scale)
    yard = np.abs(yard32.double().numpy() - ref64) / u
    err = np.abs(dev_t[:n].cpu().double().numpy() - ref64) / u
    y, e = float(yard.max()), float(err.max())
    print(f"optimiser {name}: device {e:.2f} ulp, torch-fp32 {y:.2f} ulp, ratio {e / max(y, 0.5):.2f}")
    assert e <= max(4.0 * y, 2.0), f"{name}: device {e:.2f} ulp of the operand scale, torch fp32 {y:.2f}"


@pytest.mark.parametrize("n", OPT_LENGTHS)
def test_adam_state_matches_torch(cuda, n):
    """toad_adam_step_f32 through the C ABI: p, m AND v after every step against tail_ref.adam_step, within 4 x what torch.optim.Adam in fp32 on the
    CPU deviates from it (floor 2 ulp); the guard elements behind each buffer untouched. Lengths around one trip of the capped grid (2,097,152).
    Every step starts all three implementations from the device's state, so one step's rounding is compared; the hyper-parameters are the fp32
    values the C ABI carries (a float beta2 of 0.999 is 0.99900001287: fed to torch as a double 0.999, v would differ by 1.3e-5 of itself).
    Measured on an MI355X, worst over all lengths, runs and steps, in ulp of the operand scale: p 3.68 (torch fp32 3.86), m 1.79 (2.09), v 3.18
    (2.77); worst device / torch ratio within one step 1.32."""
    from toad_amd import _lib
    lib = _lib.load()
    for rname, hp, steps, preload in ADAM_RUNS:
        gen = torch.Generator().manual_seed(n % 1000 + len(rname))
        p0 = torch.randn(n, generator=gen) * 0.05
        m0 = torch.randn(n, generator=gen) * 1e-3 if preload else torch.zeros(n)
        v0 = torch.rand(n, generator=gen) * 1e-4 if preload else torch.zeros(n)
        dp, dm, dv = _guarded(p0, cuda, 11.0), _guarded(m0, cuda, 12.0), _guarded(v0, cuda, 13.0)
        rp, rm, rv = p0.double().numpy(), m0.double().numpy(), v0.double().numpy()
        # torch's fp32 CPU optimiser, its state pre-loaded for the resume
        tp = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([tp], **hp)
        if preload:
            opt.state[tp] = dict(step=torch.tensor(float(steps[0] - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
        for step in (steps if n <= GRID_FLOATS + 4 or rname == ADAM_RUNS[0][0] else steps[:1]):     # (the longest buffer: the first run whole, one step of the others)
            g = _grad(n, gen)
            dg = _guarded(g, cuda, 14.0)
            # every implementation starts this step from the DEVICE's state, so one step's rounding is what is compared
            cur = [t[:n].cpu() for t in (dp, dm, dv)]
            with torch.no_grad():
                tp.copy_(cur[0])
            if step > 1 or preload:
                opt.state[tp]["exp_avg"].copy_(cur[1]); opt.state[tp]["exp_avg_sq"].copy_(cur[2])
            tp.grad = g.clone()
            opt.step()
            assert int(opt.state[tp]["step"]) == step
            old = [t.double().numpy() for t in cur]
            rp, rm, rv = tr.adam_step(old[0], g.double().numpy(), old[1], old[2], hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], step)
            rc = lib.toad_adam_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"],
                                        hp["weight_decay"], step, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.toad_last_error().decode()
            gd = g.double().numpy() + hp["weight_decay"] * old[0]
            st = opt.state[tp]
            what = f"adam n={n} {rname} step {step}"
            sc_m = np.maximum.reduce([np.abs(old[1]), np.abs(rm), np.abs(gd) * (1 - hp["betas"][0])])
            # p: its own magnitude, or - where the parameter is tiny - the step, whose round-off is that of m carried through lr / bc1 / denom
            b1, b2 = hp["betas"]
            sc_p = np.maximum.reduce([np.abs(old[0]), np.abs(rp), hp["lr"] / (1 - b1 ** step) * sc_m / (np.sqrt(rv) / math.sqrt(1 - b2 ** step) + hp["eps"])])
            _opt_check(what + " p", dp, rp, tp.detach(), sc_p, n)
            _opt_check(what + " m", dm, rm, st["exp_avg"], sc_m, n)
            _opt_check(what + " v", dv, rv, st["exp_avg_sq"], np.maximum.reduce([old[2], rv, gd * gd * (1 - hp["betas"][1])]), n)
            for buf, fill in ((dp, 11.0), (dm, 12.0), (dv, 13.0), (dg, 14.0)):
                assert torch.equal(buf[n:], torch.full((GUARD,), fill, device=cuda)), f"{what}: guard elements written"
            assert torch.equal(dg[:n].cpu(), g), f"{what}: the gradient was modified"


SGD_RUNS = [("momentum_.9", F32(0.9), (1, 2, 3, 4), False), ("momentum_0_null_buffer", 0.0, (1, 2), False), ("resume_step5", F32(0.9), (5, 6), True)]


@pytest.mark.parametrize("n", OPT_LENGTHS)
def test_sgd_state_matches_torch(cuda, n):
    """toad_sgd_step_f32: p AND the momentum buffer against tail_ref.sgd_step, bound as for Adam. Momentum 0 runs with a NULL buffer; a resume at
    step 5 from a pre-loaded buffer must use it (the first-step flag is off: buf = momentum buf + g', not g'). Measured on an MI355X, worst in ulp
    of the operand scale: p 1.69 (torch fp32 1.69), buf 1.00 (1.25); worst device / torch ratio within one step 1.14."""
    from toad_amd import _lib
    lib = _lib.load()
    lr, wd = F32(1e-2), F32(1e-5)
    for rname, mom, steps, preload in SGD_RUNS:
        gen = torch.Generator().manual_seed(n % 1000 + 7 * len(rname))
        p0 = torch.randn(n, generator=gen) * 0.05
        b0 = torch.randn(n, generator=gen) * 1e-2 if preload else torch.zeros(n)
        dp = _guarded(p0, cuda, 21.0)
        db = _guarded(b0, cuda, 22.0) if mom else None
        tp = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([tp], lr=lr, momentum=mom, weight_decay=wd)
        if preload:
            opt.state[tp] = dict(momentum_buffer=b0.clone())
        for step in steps:
            g = _grad(n, gen)
            dg = _guarded(g, cuda, 23.0)
            cur_p = dp[:n].cpu()
            cur_b = db[:n].cpu() if mom else None
            with torch.no_grad():
                tp.copy_(cur_p)
            if mom and (step > 1):
                opt.state[tp]["momentum_buffer"].copy_(cur_b)
            tp.grad = g.clone()
            opt.step()
            rp, rb = tr.sgd_step(cur_p.double().numpy(), g.double().numpy(), None if not mom else cur_b.double().numpy(), lr, mom, wd, step)
            rc = lib.toad_sgd_step_f32(dp.data_ptr(), dg.data_ptr(), None if db is None else db.data_ptr(), n, lr, mom, wd, step,
                                       torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.toad_last_error().decode()
            gd = g.double().numpy() + wd * cur_p.double().numpy()
            what = f"sgd n={n} {rname} step {step}"
            sc_b = np.maximum.reduce([np.abs(cur_b.double().numpy()), np.abs(rb), np.abs(gd)]) if mom else np.abs(g.double().numpy()) + wd * np.abs(cur_p.double().numpy())
            _opt_check(what + " p", dp, rp, tp.detach(), np.maximum.reduce([np.abs(cur_p.double().numpy()), np.abs(rp), lr * sc_b]), n)
            if mom:
                if step > 1:          # the resume: the buffer it was given entered the update
                    assert np.abs(rb - gd).max() > 0
                _opt_check(what + " buf", db, rb, opt.state[tp]["momentum_buffer"], sc_b, n)
                assert torch.equal(db[n:], torch.full((GUARD,), 22.0, device=cuda)), f"{what}: guard elements written"
            assert torch.equal(dp[n:], torch.full((GUARD,), 21.0, device=cuda)) and torch.equal(dg[n:], torch.full((GUARD,), 23.0, device=cuda)), what
            assert torch.equal(dg[:n].cpu(), g), f"{what}: the gradient was modified"


# ---- the public routes with other class counts ------------------------------------------------------------------------------------------------
def _model(cuda, c, size_arg="big", seed=1):
    """(module on the device, its state dict on the CPU, the STEP_SLOTS weight views): xavier weights, N(0, 0.05) biases (tests/fuzz_mil.py)."""
    from toad_amd import TOAD_fc_mtl_concat
    params = orc.xavier_params(c, seed=seed, size_arg=size_arg)
    gen = torch.Generator().manual_seed(7 + seed)
    for v in params.values():
        if v.dim() == 1:
            v.normal_(0, 0.05, generator=gen)
    model = TOAD_fc_mtl_concat(n_classes=c, size_arg=size_arg)
    model.load_state_dict(params); model.relocate()
    return model, params, {k: v.detach() for k, v in model._weights().items()}


def _split_ab(g, d):
    o = dict(g)
    o["wa"], o["wb"], o["ba"], o["bb"] = g["wab"][:d], g["wab"][d:], g["bab"][:d], g["bab"][d:]
    return o


def _oracle_backward_on_device_activations(params, x, sex, label, site, arena, n, c, d):
    """tests/fuzz_mil.py's yardstick: the oracle's backward in fp64 (and in fp32, for the round-off of the same computation) on the activations
    the device saved, so that the ReLU masks are identical. -> (fp64 gradients, {key: fp32 noise})."""
    L = 512
    sv = orc.Saved(x=x, h1=arena.view("h1", (n, L)).cpu(), h=arena.view("h", (n, L)).cpu(), p=arena.view("p", (n, 2 * d)).cpu(),
                   a_raw=arena.view("a_raw", (n, 2)).cpu(), m=arena.view("m", (2, L)).cpu(), mcat=arena.view("mcat", (2, L + 1)).cpu(), sex=sex)
    dl, ds = orc.loss_grad(arena.view("logits", (1, c)).cpu(), label, arena.view("site_logits", (1, 2)).cpu(), site)
    o32 = orc.backward(params, sv, dl, ds)
    sv64 = orc.Saved(**{k: (v.double() if (v is not None and v.is_floating_point()) else v) for k, v in sv.__dict__.items()})
    og = orc.backward({k: v.double() for k, v in params.items()}, sv64, dl.double(), ds.double())
    return og, {k: (o32[k].double() - og[k]).abs().max().item() for k in og}


def _assert_grads_like_fuzz_mil(got, og, noise, what):
    """{oracle key: gradient} against the fp64 oracle backward: 2e-5 of the gradient's own scale + 32 x the fp32 noise (tests/fuzz_mil.py)."""
    for k, ref in og.items():
        scale = ref.abs().max().item()
        if k.endswith("attention_c.bias"):
            scale = max(scale, og["attention_net.4.attention_c.weight"].abs().max().item())
        if scale == 0.0:                      # one-patch bags: the attention branch has no gradient
            scale = max(v.abs().max().item() for v in og.values())
        err = (got[k].detach().cpu().double() - ref).abs().max().item()
        assert err <= 2e-5 * scale + 32.0 * noise[k], f"{what}: {k} err {err:.2e} scale {scale:.2e} noise {noise[k]:.2e}"


ROUTE_CASES = [(1, 3, "big"), (2, 1, "big"), (25, 64, "big"), (26, 300, "big"), (26, 64, "small"), (100, 3, "big"), (100, 300, "big"), (512, 64, "big"),
               (2, 300, "big"), (512, 1, "big")]


@pytest.mark.parametrize("c,n,size_arg", ROUTE_CASES)
def test_other_class_counts_through_the_step_and_the_forward_backward_pair(cuda, c, n, size_arg):
    """n_classes on both sides of the fused tail's cache threshold (25 | 26) and at the limits (1, 512) through ops.mil_step and through ops.mil_fwd
    + ops.mtl_ce_fwd_bwd + ops.mil_bwd on tiny bags, against the oracle as tests/fuzz_mil.py does; the two routes against each other per
    helpers.assert_step_grad_matches_per_op."""
    from toad_amd import ops
    from tests.helpers import SLOT2KEY, assert_step_grad_matches_per_op
    model, params, w = _model(cuda, c, size_arg, seed=c)
    d = w["wc"].shape[1]
    assert d == (384 if size_arg == "big" else 256)
    gen = torch.Generator().manual_seed(100 * c + n)
    x = torch.randn(n, 1024, generator=gen)
    sex, label, site = torch.tensor([float(n % 2)]), torch.tensor([c - 1 if n % 2 else c // 2]), torch.tensor([(c + n) % 2])
    bag, sexd, labd, sited = x.to(cuda), sex.to(cuda), label.to(cuda), site.to(cuda)
    g_step = {k: torch.full_like(w[k], 7.0) for k in ops.STEP_SLOTS}
    loss, logits, slog = ops.mil_step(w, g_step, 0.0, bag, sexd, labd, sited, 0.75, 0.25, want_logits=True)
    arena = ops.mil_fwd(w, bag, sexd)
    v = arena.view
    loss2, dl, ds = ops.mtl_ce_fwd_bwd(v("logits", (1, c)), v("site_logits", (1, 2)), labd, sited, 0.75, 0.25)
    g_pair = {k: torch.full_like(w[k], -3.0) for k in ops.STEP_SLOTS}
    ops.mil_bwd(w, g_pair, 0.0, bag, arena, dl, ds)
    # outputs: 1e-4 against the oracle's fp32 forward
    o_out, o_loss, _ = orc.fwd_bwd(params, x, sex, label, site)
    for got, key in ((logits, "logits"), (v("logits", (1, c)), "logits"), (v("y_prob", (1, c)), "Y_prob"), (slog, "site_logits"),
                     (v("site_logits", (1, 2)), "site_logits"), (v("site_prob", (1, 2)), "site_prob"), (v("a_raw", (n, 2)).t(), "A")):
        err = (got.cpu() - o_out[key]).abs().max().item()
        assert err <= 1e-4, (key, err)
    assert abs(loss[0].item() - o_loss.item()) <= 1e-4 and abs(loss2[0].item() - o_loss.item()) <= 1e-4
    assert torch.equal(loss, loss2) and torch.equal(logits, v("logits", (1, c))) and torch.equal(slog, v("site_logits", (1, 2)))
    # gradients of both routes against the fp64 backward on the device's saved activations
    og, noise = _oracle_backward_on_device_activations(params, x, sex, label, site, arena, n, c, d)
    for name, g in (("mil_step", g_step), ("mil_fwd + mil_bwd", g_pair)):
        full = _split_ab(g, d)
        _assert_grads_like_fuzz_mil({key: full[slot] for slot, key in SLOT2KEY.items()}, og, noise, f"C={c} N={n} {name}")
    for k in ops.STEP_SLOTS:
        assert_step_grad_matches_per_op(g_step[k], g_pair[k], k, n)


@pytest.mark.parametrize("c,n", [(2, 64), (26, 3), (100, 300)])
def test_other_class_counts_through_the_module_with_autograd(cuda, c, n):
    """model(bag, sex), torch's CrossEntropyLoss on its logits, loss.backward(): outputs and parameter gradients as tests/fuzz_mil.py checks them."""
    from toad_amd import ops
    model, params, w = _model(cuda, c, seed=c + 1)
    gen = torch.Generator().manual_seed(10 * c + n)
    x = torch.randn(n, 1024, generator=gen)
    sex, label, site = torch.tensor([1.0]), torch.tensor([c - 1]), torch.tensor([n % 2])
    model.zero_grad(set_to_none=True)
    res = model(x.to(cuda), sex.to(cuda))
    ce = torch.nn.CrossEntropyLoss()
    loss = ce(res["logits"], label.to(cuda)) * 0.75 + ce(res["site_logits"], site.to(cuda)) * 0.25
    loss.backward()
    o_out, o_loss, _ = orc.fwd_bwd(params, x, sex, label, site)
    for k in ("logits", "Y_prob", "site_logits", "site_prob", "A"):
        assert (res[k].detach().cpu() - o_out[k]).abs().max().item() <= 1e-4, k
    assert int(res["Y_hat"].item()) == int(o_out["Y_hat"].item()) or c > 2       # (decided for two classes; a near-tie among many is not this test's matter)
    assert abs(loss.item() - o_loss.item()) <= 1e-4
    arena = ops.mil_fwd(w, x.to(cuda), sex.to(cuda))
    assert torch.equal(arena.view("logits", (1, c)), res["logits"].detach())
    og, noise = _oracle_backward_on_device_activations(params, x, sex, label, site, arena, n, c, w["wc"].shape[1])
    _assert_grads_like_fuzz_mil({k: p.grad for k, p in model.named_parameters()}, og, noise, f"module C={c} N={n}")


# ---- the ragged routes ----------------------------------------------------------------------------------------------------------------------------
def _ragged(B, seed):
    """B slides of 1 to 3 rows each plus one of 257 rows -> (slides [(x, sex, label-less...)], lens)."""
    lens = [1 + (3 * i + seed) % 3 for i in range(B)] + [257]
    return lens


def _head_grad_sum(mcat, dl, ds, wcls, wsite, prev, beta):
    """Sum over slides, in fp64, of tail_ref.heads_bwd's head gradients, and the magnitude sum the rounding bound scales with."""
    tot, mag = None, None
    for b in range(mcat.shape[0]):
        r = tr.heads_bwd(mcat[b], dl[b], ds[b], wcls, wsite)[:4]
        tot = list(r) if tot is None else [a + x for a, x in zip(tot, r)]
        mag = [np.abs(x) for x in r] if mag is None else [a + np.abs(x) for a, x in zip(mag, r)]
    if beta:
        tot = [t + beta * p for t, p in zip(tot, prev)]
        mag = [m + abs(beta) * np.abs(p) for m, p in zip(mag, prev)]
    return tot, mag


RAGGED_CASES = [(1, 2, torch.float32), (2, 26, torch.float32), (17, 100, torch.float32), (300, 26, torch.float32), (300, 2, torch.float32),
                (17, 26, torch.float16), (2, 100, torch.float32)]


@pytest.mark.parametrize("B,c,dtype", RAGGED_CASES, ids=[f"B{B}+1-C{c}-{str(dt).split('.')[-1]}" for B, c, dt in RAGGED_CASES])
def test_ragged_routes_with_other_class_counts(cuda, B, c, dtype):
    """ops.mil_multi_step and ops.mil_multi_fwd + ops.mil_multi_bwd on B slides of 1 to 3 rows plus one of 257 rows: the batched heads forward
    (heads_fwd_kernel with m_stride), the batched fused tail (rec != 0), heads_bwd_batch_kernel and heads_wgrad_batch_kernel at class counts on
    both sides of the cache threshold. Everything against helpers.check_batch_against_oracle (fp32 bags); the head-weight gradients and biases
    against the SUM over slides of tail_ref.heads_bwd on the device's own per-slide Mcat, dlogits and dsite - one rounding per product and B + 1
    per sum; beta = 1 accumulates onto pre-filled gradients; two runs are bitwise equal (the slide sum is in index order)."""
    from toad_amd import ops
    from tests.helpers import SLOT2KEY, check_batch_against_oracle
    from tests.test_gpu_multi_step import _step_workspace_activations
    model, params, w = _model(cuda, c, seed=B + c)
    d = w["wc"].shape[1]
    lens = _ragged(B, c)
    nb, ntot = len(lens), sum(lens)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    gen = torch.Generator().manual_seed(B * 1000 + c)
    xcat32 = torch.randn(ntot, 1024, generator=gen)
    if dtype == torch.float16:
        xcat32 = xcat32.half().float()                     # the values the fp16 bag holds: the oracle sees the same
    sex = (torch.arange(nb) % 2).float(); label = (torch.arange(nb) * 7) % c; site = (torch.arange(nb) // 2) % 2
    label[-1] = c - 1; label[0] = 0
    slides = [(xcat32[offs[b]:offs[b + 1]], sex[b:b + 1], label[b:b + 1], site[b:b + 1]) for b in range(nb)]
    xd = xcat32.to(cuda).to(dtype)
    sexd, labd, sited = sex.to(cuda), label.to(cuda), site.to(cuda)
    wc_, ws_ = 0.75 / nb, 0.25 / nb
    head_slots = ("wcls", "bcls", "wsite", "bsite")
    wcls64, wsite64 = _n(w["wcls"]), _n(w["wsite"])

    def full(g):
        return {s: _split_ab(g, d)[s].cpu() for s in SLOT2KEY}

    # ---- forward + backward pair: the caller's gradients are tail_ref's own, from the device's logits
    arena, outs = ops.mil_multi_fwd(w, xd, sexd, offsets=offs)
    lg, sl, mcat = _n(outs["logits"]), _n(outs["site_logits"]), _n(outs["features"])
    dl64 = np.zeros((nb, c)); ds64 = np.zeros((nb, 2)); loss64 = np.zeros((nb, 3))
    for b in range(nb):
        loss64[b], dl64[b], ds64[b] = tr.ce(lg[b], int(label[b]), sl[b], int(site[b]), wc_, ws_)
    dl32, ds32 = torch.from_numpy(dl64).float(), torch.from_numpy(ds64).float()
    g_pair = {k: torch.full_like(w[k], 5.0) for k in ops.STEP_SLOTS}
    ops.mil_multi_bwd(w, g_pair, 0.0, None, None, arena, dl32.to(cuda), ds32.to(cuda))
    v = arena.view
    dev = dict(h1=v("h1", (ntot, 512)).cpu(), h=v("h", (ntot, 512)).cpu(), p=v("p", (ntot, 2 * d)).cpu(), a_raw=outs["a_raw"].cpu(),
               logits=outs["logits"].cpu(), site_logits=outs["site_logits"].cpu(), loss=torch.from_numpy(loss64).float())
    for b in range(nb):                                    # per-slide forward outputs of the batched heads kernel against the statement on ITS Mcat
        r = tr.heads_fwd(mcat[b][:, :512], mcat[b][0, 512], wcls64, _n(w["bcls"]), wsite64, _n(w["bsite"]))
        assert mcat[b][0, 512] == mcat[b][1, 512] == float(sex[b])
        a_lg = np.abs(wcls64) @ np.abs(r[0][0]) + np.abs(_n(w["bcls"]))
        _within(lg[b], r[1], tr.dot_bound(a_lg, r[1], tr.row_depth(512)), f"slide {b} logits")
        _within(_n(outs["y_prob"])[b], r[2], 1e-5, f"slide {b} Y_prob")
        _within(_n(outs["site_prob"])[b], r[5], 1e-5, f"slide {b} site_prob")
        top = np.sort(r[1])[::-1]
        if c == 1 or top[0] - top[1] > 1e-4:
            assert int(outs["y_hat"][b].item()) == r[3], f"slide {b} Y_hat"
    if dtype == torch.float32:
        check_batch_against_oracle(f"multi_fwd+bwd B={nb} C={c}", params, slides, offs, dev, full(g_pair))
    prev0 = [np.zeros_like(x) for x in (wcls64, _n(w["bcls"]), wsite64, _n(w["bsite"]))]
    want, mag = _head_grad_sum(mcat, dl32.double().numpy(), ds32.double().numpy(), wcls64, wsite64, prev0, 0.0)
    for s, wnt, mg in zip(head_slots, want, mag):
        _within(_n(g_pair[s]), wnt, (nb + 2) * 2.0 ** -24 * mg, f"multi_bwd B={nb} C={c} {s} against the slide sum")
    # beta = 1 onto the gradients just formed, and run to run
    g_acc = {k: g_pair[k].clone() for k in ops.STEP_SLOTS}
    ops.mil_multi_bwd(w, g_acc, 1.0, None, None, arena, dl32.to(cuda), ds32.to(cuda))
    prev = [_n(g_pair[s]) for s in head_slots]
    want1, mag1 = _head_grad_sum(mcat, dl32.double().numpy(), ds32.double().numpy(), wcls64, wsite64, prev, 1.0)
    for s, wnt, mg in zip(head_slots, want1, mag1):
        _within(_n(g_acc[s]), wnt, (nb + 3) * 2.0 ** -24 * mg, f"multi_bwd beta=1 B={nb} C={c} {s}")
    g_again = {k: torch.full_like(w[k], -1.0) for k in ops.STEP_SLOTS}
    ops.mil_multi_bwd(w, g_again, 0.0, None, None, arena, dl32.to(cuda), ds32.to(cuda))
    assert all(torch.equal(g_again[k], g_pair[k]) for k in ops.STEP_SLOTS)

    # ---- the fused multi-slide step
    g_step = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
    loss, logits, slog = ops.mil_multi_step(w, g_step, 0.0, xd, sexd, labd, sited, wc_, ws_, want_logits=True, offsets=offs)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        h1_d, h_d, p_d, a_d = (t.cpu() for t in _step_workspace_activations(ntot, nb, c, d, cuda))
        check_batch_against_oracle(f"multi_step B={nb} C={c}", params, slides, offs,
                                   dict(h1=h1_d, h=h_d, p=p_d, a_raw=a_d, logits=logits.cpu(), site_logits=slog.cpu(), loss=loss.cpu()), full(g_step))
    # its loss triple per slide against the statement on the step's own logits; its head gradients against the slide sum with the statement's
    # dlogits of those logits: the rounding of the sum plus what 1e-6-accurate (at weights 0.75 / 0.25) dlogits can move it
    lgs, sls = _n(logits), _n(slog)
    dls, dss = np.zeros((nb, c)), np.zeros((nb, 2))
    for b in range(nb):
        l3, dls[b], dss[b] = tr.ce(lgs[b], int(label[b]), sls[b], int(site[b]), wc_, ws_)
        _within(_n(loss)[b], l3, np.array([1e-5 / nb, 1e-5, 1e-5]), f"multi_step slide {b} loss")        # (the total carries the 1 / B of its weights)
    want_s, mag_s = _head_grad_sum(mcat, dls, dss, wcls64, wsite64, prev0, 0.0)
    amc = np.abs(mcat).sum(0)                                                   # [2, 513]: sum_b |Mcat_b|
    slack = (1e-6 / nb) * np.stack([amc[0]] * c), np.full(c, 1e-6), (1e-6 / nb) * np.stack([amc[1]] * 2), np.full(2, 1e-6)
    if dtype == torch.float32:
        assert torch.equal(logits, outs["logits"]) and torch.equal(slog, outs["site_logits"])          # same forward kernels on the same rows
        for s, wnt, mg, sk in zip(head_slots, want_s, mag_s, slack):
            _within(_n(g_step[s]), wnt, (nb + 2) * 2.0 ** -24 * mg + sk, f"multi_step B={nb} C={c} {s} against the slide sum")
    g_step1 = {k: g_step[k].clone() for k in ops.STEP_SLOTS}
    ops.mil_multi_step(w, g_step1, 1.0, xd, sexd, labd, sited, wc_, ws_, offsets=offs)
    for s in head_slots:                                                        # beta = 1: exactly one more rounding on top of twice the gradient
        _within(_n(g_step1[s]), 2 * _n(g_step[s]), 2.0 ** -23 * 2 * np.abs(_n(g_step[s])) + 1e-30, f"multi_step beta=1 {s}")
    g_step2 = {k: torch.full_like(w[k], 9.0) for k in ops.STEP_SLOTS}
    loss_b, _, _ = ops.mil_multi_step(w, g_step2, 0.0, xd, sexd, labd, sited, wc_, ws_, offsets=offs)
    assert torch.equal(loss_b, loss) and all(torch.equal(g_step2[k], g_step[k]) for k in ops.STEP_SLOTS)
