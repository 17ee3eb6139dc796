"""GPU: TOAD_fc_mtl_concat.forward_batch - the ragged multi-slide forward with autograd (toad_mil_multi_fwd_f32 / toad_mil_multi_bwd_f32).
Values against model(data, sex) slide by slide; gradients of the reference's loss against the fused multi-slide step (same kernels) and against
the CPU oracle; a custom loss reaching the attention scores and the features against per-slide autograd; dropout masks, autograd accumulation,
retain_graph and the no-grad route."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import SLOT2KEY, assert_grad_close, assert_grad_close_or_few_flips, check_batch_against_oracle, grad_scale

pytestmark = pytest.mark.gpu

TRUNK = ("w1", "b1", "w2", "b2")


def _model(cuda, c=18, size_arg="big", seed=0, dropout=False):
    from toad_amd import TOAD_fc_mtl_concat
    torch.manual_seed(seed)
    m = TOAD_fc_mtl_concat(n_classes=c, size_arg=size_arg, dropout=dropout)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.relocate()
    return m, params


def _slides(lens, c, seed=0):
    out = []
    for i, n in enumerate(lens):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        out.append((torch.randn(n, 1024, generator=g), torch.tensor([float(i % 2)]), torch.tensor([(7 * i) % c]), torch.tensor([(i // 2) % 2])))
    return out


def _dev(slides, cuda):
    return [tuple(t.to(cuda) for t in s) for s in slides]


def _grads(model):
    """{slot: .grad} of the 14 parameter slots (functional.SLOTS names)."""
    from toad_amd import functional as F_
    sp = model._slot_params()
    return {k: sp[k].grad.detach().clone() for k in F_.SLOTS}


def _step_grads(g, d):
    o = dict(g)
    o["wa"], o["wb"], o["ba"], o["bb"] = g["wab"][:d], g["wab"][d:], g["bab"][:d], g["bab"][d:]
    return o


def _mtl_loss(outs, dev_slides):
    B = len(outs)
    return sum(0.75 * F.cross_entropy(o["logits"], s[2]) + 0.25 * F.cross_entropy(o["site_logits"], s[3]) for o, s in zip(outs, dev_slides)) / B


VALUE_CASES = [([1, 2, 63, 300, 1000, 257, 64], 18, "big"), ([1, 2, 63, 300, 1000, 257, 64], 2, "small"), ([10000] * 4, 2, "big"),
               ([10000] * 4, 18, "small"), ([40], 18, "small"), ([40], 2, "big")]


@pytest.mark.parametrize("lens,c,size_arg", VALUE_CASES)
def test_values_equal_per_slide_forward(cuda, lens, c, size_arg):
    """forward_batch (autograd route) == model(data, sex, return_features=True) slide by slide: fp32 round-off (operand scales per 256-row block of
    the concatenation), 2e-5 of each tensor's own magnitude - the bound of test_forward_many_equals_per_slide_forward; the hats exactly."""
    model, _ = _model(cuda, c=c, size_arg=size_arg, seed=len(lens) + c)
    model.eval()
    slides = _dev(_slides(lens, c, seed=3), cuda)
    outs = model.forward_batch([s[0] for s in slides], torch.cat([s[1] for s in slides]), return_features=True)
    assert len(outs) == len(lens)
    assert outs[0]["logits"].requires_grad and outs[0]["A"].requires_grad and not outs[0]["Y_prob"].requires_grad
    for s, r in zip(slides, outs):
        with torch.no_grad():
            one = model(s[0], s[1], return_features=True)
        assert set(r) == set(one)
        for k in ("logits", "Y_prob", "site_logits", "site_prob", "features", "A"):
            assert r[k].shape == one[k].shape, k
            tol = 2e-5 * max(one[k].abs().max().item(), 1e-6)
            assert (r[k].detach() - one[k]).abs().max().item() <= tol, (k, s[0].shape[0])
        assert r["Y_hat"].shape == one["Y_hat"].shape and torch.equal(r["Y_hat"], one["Y_hat"]) and torch.equal(r["site_hat"], one["site_hat"])


@pytest.mark.parametrize("lens", [[1, 2, 63, 300, 1000, 257, 64], [256] * 8, [3000, 5000, 777]])
def test_reference_loss_gradients_equal_the_fused_step(cuda, lens):
    """loss = sum_b (0.75 CE(logits_b) + 0.25 CE(site_b)) / B through torch's cross_entropy and loss.backward() == ops.mil_multi_step with
    w_cls = 0.75 / B, w_site = 0.25 / B on the same weights: the forward activations are bitwise the fused step's (same kernels, same operands), so the
    14 gradients differ only through the rounding of dlogits (torch's softmax vs the kernel's)."""
    from toad_amd import ops
    c = 18
    model, _ = _model(cuda, c=c, seed=len(lens))
    slides = _dev(_slides(lens, c, seed=5), cuda)
    B = len(lens)
    sex = torch.cat([s[1] for s in slides]); label = torch.cat([s[2] for s in slides]); site = torch.cat([s[3] for s in slides])
    outs = model.forward_batch([s[0] for s in slides], sex)
    _mtl_loss(outs, slides).backward()
    got = _grads(model)
    w = {k: v.detach() for k, v in model._weights().items()}
    g = {k: torch.zeros_like(w[k]) for k in ops.STEP_SLOTS}
    ops.mil_multi_step(w, g, 0.0, [s[0] for s in slides], sex, label, site, 0.75 / B, 0.25 / B)
    ref = _step_grads(g, w["wc"].shape[1])
    for slot in SLOT2KEY:
        assert_grad_close(got[slot], ref[slot], 2e-5, grad_scale(ref, slot), what=f"forward_batch vs fused step: {slot}")


@pytest.mark.parametrize("name,lens", [("ragged7", [1, 2, 63, 300, 1000, 257, 64]), ("three", [3000, 5000, 777])])
def test_reference_loss_gradients_match_the_oracle(cuda, name, lens):
    """The same loss against the CPU oracle (tests/helpers.check_batch_against_oracle, as tests/test_gpu_multi_step.py does for the fused step): per-slide
    outputs and losses, H1 / H of the concatenation against the exact forward, all 14 gradients against the oracle's fp64 backward summed over slides."""
    from toad_amd import ops
    c = 18
    model, params = _model(cuda, c=c, seed=len(lens) + 11)
    slides = _slides(lens, c, seed=9)
    dev = _dev(slides, cuda)
    B, ntot, d = len(lens), sum(lens), model._weights()["wc"].shape[1]
    sex = torch.cat([s[1] for s in dev])
    outs = model.forward_batch([s[0] for s in dev], sex)
    losses = [(0.75 * F.cross_entropy(o["logits"], s[2]) + 0.25 * F.cross_entropy(o["site_logits"], s[3])) / B for o, s in zip(outs, dev)]
    sum(losses).backward()
    got = _grads(model)
    # the activations of the concatenation: the same forward again (bitwise the one above) through ops, whose arena is readable
    w = {k: v.detach() for k, v in model._weights().items()}
    arena, o = ops.mil_multi_fwd(w, [s[0] for s in dev], sex)
    v = arena.view
    devd = dict(h1=v("h1", (ntot, 512)).cpu(), h=v("h", (ntot, 512)).cpu(), p=v("p", (ntot, 2 * d)).cpu(), a_raw=o["a_raw"].cpu(),
                logits=torch.cat([r["logits"].detach() for r in outs]).cpu(), site_logits=torch.cat([r["site_logits"].detach() for r in outs]).cpu(),
                loss=torch.stack([l.detach() for l in losses]).reshape(B, 1).expand(B, 3).cpu())
    assert torch.equal(devd["logits"], o["logits"].cpu())
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    check_batch_against_oracle(name, params, slides, offs, devd, {k: got[k].cpu() for k in SLOT2KEY})


def _custom_terms(o, s, cw):
    """class-weighted CE + site CE + entropy of the task-0 attention + L2 of the features: reaches dlogits, dsite, dA and dMcat."""
    a0 = torch.softmax(o["A"][0], 0)
    ent = -(a0 * torch.log(a0 + 1e-12)).sum()
    return F.cross_entropy(o["logits"], s[2], weight=cw) + 0.25 * F.cross_entropy(o["site_logits"], s[3]) + 1.0 * ent + 1e-2 * (o["features"] ** 2).sum()


def test_custom_loss_through_scores_and_features_equals_per_slide_autograd(cuda):
    """A loss with terms on A and on the features (the dA / dMcat inputs of toad_mil_multi_bwd_f32, the batched pool backward's dA_ext) against the
    sum of per-slide autograd through model(data, sex, return_features=True) with the same loss. The two routes scale GEMM operands per 256-row block
    of different row ranges: fp32 round-off (and, on the trunk, at most a few legitimate ReLU-mask flips)."""
    c = 18
    lens = [1, 2, 63, 300, 1000, 257, 64]
    model, _ = _model(cuda, c=c, seed=23)
    slides = _dev(_slides(lens, c, seed=13), cuda)
    B = len(lens)
    cw = torch.linspace(0.5, 2.0, c, device=cuda)
    outs = model.forward_batch([s[0] for s in slides], torch.cat([s[1] for s in slides]), return_features=True)
    (sum(_custom_terms(o, s, cw) for o, s in zip(outs, slides)) / B).backward()
    got = _grads(model)
    model.zero_grad(set_to_none=True)
    for s in slides:
        (_custom_terms(model(s[0], s[1], return_features=True), s, cw) / B).backward()
    ref = _grads(model)
    # the same batch without the A / feature terms: they must move the attention and head gradients far beyond the tolerance below
    model.zero_grad(set_to_none=True)
    outs = model.forward_batch([s[0] for s in slides], torch.cat([s[1] for s in slides]), return_features=True)
    (sum(F.cross_entropy(o["logits"], s[2], weight=cw) + 0.25 * F.cross_entropy(o["site_logits"], s[3]) for o, s in zip(outs, slides)) / B).backward()
    plain = _grads(model)
    for slot in ("wc", "wa", "wb"):                   # (dWcls depends on dlogits and the features only: these terms do not reach it)
        sc = grad_scale(ref, slot)
        assert (plain[slot] - ref[slot]).abs().max().item() > 1e-2 * sc, slot
    for slot in SLOT2KEY:
        sc = max(grad_scale(ref, slot), grad_scale(ref, {"ba": "wa", "bb": "wb"}.get(slot, slot)))
        chk = assert_grad_close_or_few_flips if slot in TRUNK else assert_grad_close
        chk(got[slot], ref[slot], 5e-5, sc, what=f"custom loss, batch vs per-slide: {slot}")


def test_dropout_masks_are_the_fused_steps(cuda):
    """Train mode with dropout=True: forward_batch draws ONE seed with _draw_dropout; replaying the draw and running ops.mil_multi_step at the same
    (drop_p, seed) gives the same gradients as in the no-dropout comparison - the masks are the fused step's (streams over the concatenated rows)."""
    from toad_amd import ops
    from toad_amd.model_toad import _draw_dropout
    c = 18
    lens = [300, 64, 777, 300, 1]
    model, _ = _model(cuda, c=c, seed=31, dropout=True)
    model.train()
    slides = _dev(_slides(lens, c, seed=17), cuda)
    B = len(lens)
    sex = torch.cat([s[1] for s in slides]); label = torch.cat([s[2] for s in slides]); site = torch.cat([s[3] for s in slides])
    torch.manual_seed(4242)
    outs = model.forward_batch([s[0] for s in slides], sex)
    _mtl_loss(outs, slides).backward()
    got = _grads(model)
    torch.manual_seed(4242)
    drop_p, seed = _draw_dropout(True)
    assert drop_p == 0.25
    w = {k: v.detach() for k, v in model._weights().items()}
    g = {k: torch.zeros_like(w[k]) for k in ops.STEP_SLOTS}
    loss, logits, _ = ops.mil_multi_step(w, g, 0.0, [s[0] for s in slides], sex, label, site, 0.75 / B, 0.25 / B, drop_p=drop_p, seed=seed, want_logits=True)
    assert torch.equal(torch.cat([o["logits"].detach() for o in outs]), logits)          # same masks, same kernels: bitwise the same logits
    ref = _step_grads(g, w["wc"].shape[1])
    for slot in SLOT2KEY:
        assert_grad_close(got[slot], ref[slot], 2e-5, grad_scale(ref, slot), what=f"dropout: forward_batch vs fused step: {slot}")
    # a different seed draws different masks
    g2 = {k: torch.zeros_like(w[k]) for k in ops.STEP_SLOTS}
    ops.mil_multi_step(w, g2, 0.0, [s[0] for s in slides], sex, label, site, 0.75 / B, 0.25 / B, drop_p=drop_p, seed=seed + 1)
    assert (g2["w1"] - g["w1"]).abs().max().item() > 1e-3 * g["w1"].abs().max().item()


def test_autograd_accumulation_retain_graph_and_zero_grad(cuda):
    c = 5
    lens = [300, 64, 1000]
    model, _ = _model(cuda, c=c, seed=41)
    slides = _dev(_slides(lens, c, seed=19), cuda)
    sex = torch.cat([s[1] for s in slides])

    def run(retain=False):
        outs = model.forward_batch([s[0] for s in slides], sex, return_features=True)
        loss = _mtl_loss(outs, slides) + 1e-3 * sum((o["features"] ** 2).sum() + o["A"].sum() for o in outs)
        loss.backward(retain_graph=retain)
        return loss
    run()
    g1 = _grads(model)

    def same(a, b, k=1.0):
        for slot in a:
            sc = max(b[slot].abs().max().item(), 1e-30)
            assert (a[slot] - k * b[slot]).abs().max().item() <= 1e-6 * sc, slot
    run()                                                     # two backwards without zero_grad: twice the gradient
    same(_grads(model), g1, 2.0)
    model.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in model.parameters())
    loss = run(retain=True)
    same(_grads(model), g1)
    loss.backward()                                           # the arena lives with the graph: a second backward of the same forward
    same(_grads(model), g1, 2.0)
    model.zero_grad(set_to_none=False)
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in model.parameters())
    run()
    same(_grads(model), g1)


def test_no_grad_forward_equals_forward_many(cuda):
    """Under torch.no_grad() forward_batch is a one-call multi-slide forward: equal to forward_many within its tolerance, outputs are copies that
    a later forward does not overwrite."""
    c = 18
    lens = [1, 255, 256, 257, 700, 3, 2049, 64]
    model, _ = _model(cuda, c=c, seed=7)
    model.eval()
    slides = _dev(_slides(lens, c, seed=21), cuda)
    bags, sexes = [s[0] for s in slides], [s[1] for s in slides]
    with torch.no_grad():
        got = model.forward_batch(bags, sexes, return_features=True)
        many = model.forward_many(bags, sexes, return_features=True)
        keep = {k: got[3][k].clone() for k in got[3]}
        model.forward_batch([b * 2.0 for b in bags], sexes, return_features=True)         # reuses the cached arena
    assert torch.equal(keep["logits"], got[3]["logits"]) and torch.equal(keep["A"], got[3]["A"])
    for r, m in zip(got, many):
        assert set(r) == set(m)
        for k in ("logits", "Y_prob", "site_logits", "site_prob", "features", "A"):
            assert r[k].shape == m[k].shape and not r[k].requires_grad, k
            tol = 2e-5 * max(m[k].abs().max().item(), 1e-6)
            assert (r[k] - m[k]).abs().max().item() <= tol, k
        assert torch.equal(r["Y_hat"], m["Y_hat"]) and torch.equal(r["site_hat"], m["site_hat"])
    # fp16 bags are up-cast (the same values as the fp32 bags they round to)
    with torch.no_grad():
        h16 = model.forward_batch([b.half() for b in bags[:3]], sexes[:3])
        h32 = model.forward_batch([b.half().float() for b in bags[:3]], sexes[:3])
    assert all(torch.equal(a["logits"], b["logits"]) for a, b in zip(h16, h32))
