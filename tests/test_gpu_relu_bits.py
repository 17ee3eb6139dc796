"""GPU: the one-bit ReLU image over POISONED buffers. A dgrad launch that reads a tile of the image the forward launch never wrote gets whatever
the buffer held before - so every buffer the library may read before writing is given known contents here: the image itself (0x00, then 0xFF),
the cached workspaces of the whole-slide calls (arena, slabs, abs-max arrays, both images) and the caching allocator's free blocks. Results must
not depend on them, bit for bit, and the per-op dgrads are held to an fp64 product as well. tests/test_relu_bits_plan.py proves the same
inclusion on the host from the launch plan; this file would see a kernel that does not follow that plan."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 255, 256, 257, 2000, 2048, 4097, 10000, 16500, 20000, 33000, 70001)      # 10,000: half-height tiles; 16,500: one XCD two tiles ahead
NS = (256, 384, 512, 768, 1024)
KFS = (64, 512, 1024)                                    # forward reductions
KBS = (32, 64, 512, 768)                                 # reader reductions (32: one stage, cannot be K-split)
READERS = ("plain", "addend", "pool")


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _pool_inputs(m, n, g, dev, t=2):
    a_raw = torch.randn(m, t, generator=g, device=dev) * 2.0
    dm = torch.randn(t, n, generator=g, device=dev) * 0.05
    mx = a_raw.max(0).values
    ssum = (a_raw - mx).exp().sum(0)
    stats = torch.stack([mx, ssum], 1).contiguous()
    p64 = (a_raw.double() - mx.double()).exp() / ssum.double()
    return (a_raw, stats, dm), p64 @ dm.double()


def _three_way_dgrad(ops, dy, w2, y, images, mscale, reader, g, what):
    """The dgrad with the image of a forward over a zero-filled buffer, with that of a forward over a 0xFF-filled buffer, and with the fp32 mask
    alone: bitwise one result; and that result against fp64."""
    m, n = y.shape
    dev = y.device
    kw = {}
    extra = 0.0
    if reader == "addend":
        add = torch.randn(m, n, generator=g, device=dev) * 0.5
        kw["addend"] = add
        extra = add.double()
    elif reader == "pool":
        kw["pool"], extra = _pool_inputs(m, n, g, dev)
    wt = ops.transpose(w2)                                 # [N, K_b]
    outs = [ops.linear_dgrad(dy, wt, relu_src=y, mask_scale=mscale, relu_bits=b, **kw) for b in (*images, None)]
    assert torch.equal(outs[0], outs[2]), f"{what}: image over a zeroed buffer != fp32 mask ({(outs[0] != outs[2]).sum().item()} elements)"
    assert torch.equal(outs[1], outs[2]), f"{what}: image over a 0xFF buffer != fp32 mask ({(outs[1] != outs[2]).sum().item()} elements)"
    ref = (dy.double() @ w2.double() + extra) * (y > 0) * mscale
    e = _rel(outs[2], ref)
    assert e <= 2e-5, f"{what}: {e:.2e} against fp64"


def _forward_pair(ops, x, w, b, drop, seed, what):
    """The forward twice, its image landing in a zero-filled and in a 0xFF-filled buffer -> (y, (image0, imageF))."""
    m, n = x.shape[0], w.shape[0]
    nb = ops.relu_bits_bytes(m, n)
    imgs, ys = [], []
    for fill in (0x00, 0xFF):
        buf = torch.full((nb,), fill, dtype=torch.uint8, device=x.device)
        y, _, bits = ops.linear_act_fwd(x, w, b, 1, drop_p=drop, drop_seed=seed, bits_out=buf)
        assert bits is not None and bits.data_ptr() == buf.data_ptr() and bits.numel() == nb, what
        imgs.append(bits); ys.append(y)
    assert torch.equal(ys[0], ys[1]), what
    zf = (ys[0] == 0).float().mean().item()
    assert 0.2 < zf < 0.8, f"{what}: zero fraction {zf:.3f} - the mask must be non-trivial"
    return ys[0], imgs


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_per_op_dgrad_does_not_depend_on_what_the_image_buffer_held(cuda, m, n):
    """Every forward reduction against every reader reduction, readers plain / with an addend buffer / with the recomputed pooling addend,
    forward with and without dropout (mask_scale 1 and 4/3)."""
    from toad_amd import ops
    g = torch.Generator(device=cuda).manual_seed(m * 131 + n)
    cases = 0
    for kf in KFS:
        x = torch.randn(m, kf, generator=g, device=cuda)
        w = torch.randn(n, kf, generator=g, device=cuda) / kf ** 0.5
        b = torch.randn(n, generator=g, device=cuda) * 0.1
        for drop in (0.0, 0.25):
            y, imgs = _forward_pair(ops, x, w, b, drop, 1234 + kf, f"M{m} N{n} Kf{kf} drop{drop}")
            mscale = 1.0 / (1.0 - drop)
            for kb in KBS:
                dy = torch.randn(m, kb, generator=g, device=cuda)
                w2 = torch.randn(kb, n, generator=g, device=cuda) / kb ** 0.5
                for reader in READERS:
                    _three_way_dgrad(ops, dy, w2, y, imgs, mscale, reader, g, f"M{m} N{n} Kf{kf} Kb{kb} drop{drop} {reader}")
                    cases += 1
    assert cases == len(KFS) * 2 * len(KBS) * len(READERS)


def _poison_free_blocks(dev, nbytes, fill=0xFF):
    """Leave `fill` in the caching allocator's free blocks: what the next torch.empty of up to nbytes bytes will hand out."""
    torch.cuda.synchronize()
    t = torch.full((int(nbytes),), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    del t


def _weights(cuda, size_arg, c=18, seed=0):
    from toad_amd import TOAD_fc_mtl_concat
    torch.manual_seed(seed)
    model = TOAD_fc_mtl_concat(n_classes=c, size_arg=size_arg)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    model.relocate()
    return model, {k: v.detach() for k, v in model._weights().items()}


def test_above_the_chunk_size_per_op_and_functional_routes(cuda):
    """1,049,600 rows: two launches of 1,047,552 + 2,048 rows for EVERY operand width (ops._row_chunks). Cut by operand bytes, as the wrappers
    once did, the 1024-wide forward made two launches and the 512- or 768-wide dgrad one, whose plan took rows 1,047,552.. as whole tiles and
    read bit words no launch had written. Part 1: the three-way image check of this file on the trunk's three shape pairs. Part 2:
    functional.mil_forward + mil_backward (per-op route) and ops.mil_step (whole-slide route, row chunks made in C) on a 1,025-row bag repeated
    1,024 times, both against the small bag itself by the duplication property (bounds of test_million_patch_bag_duplication_property: logits
    1e-5, gradients 1e-4 absolute), after 0xFF was left in the allocator's free blocks. Those bounds belong to that test's parameters (the
    reference's initialisation, xavier weights and zero biases) and bag, which are therefore used here: the two sizes run on different kernels,
    and with other parameters ONE legitimate ReLU-boundary flip in H was measured to move dW2 by 2.4e-4 on both routes alike. What no flip can
    explain is asserted bitwise at the end: image against fp32 mask, whole-slide call against per-op route."""
    from toad_amd import functional as F_, ops
    m = 1_049_600
    assert m > ops._CHUNK_ROWS and len(ops._row_chunks(m, 4096)) == 2 and ops._row_chunks(m, 4096) == ops._row_chunks(m, 2048) == ops._row_chunks(m, 3072)
    g = torch.Generator(device=cuda).manual_seed(11)
    small = torch.randn(1025, 1024, generator=torch.Generator().manual_seed(3)).to(cuda)     # (the bag and, below, the parameters of the test the bounds come from)
    big = small.repeat(1024, 1)                              # 4.3 GB, built once for the whole test
    assert big.shape[0] == m
    # ---- part 1
    for kf, n, kb in ((1024, 512, 512), (1024, 512, 768), (512, 512, 768)):
        x = big[:, :kf].contiguous() if kf != 1024 else big
        w = torch.randn(n, kf, generator=g, device=cuda) / kf ** 0.5
        b = torch.randn(n, generator=g, device=cuda) * 0.1
        y, imgs = _forward_pair(ops, x, w, b, 0.0, 5, f"M{m} N{n} Kf{kf}")
        del x
        dy = torch.randn(m, kb, generator=g, device=cuda)
        w2 = torch.randn(kb, n, generator=g, device=cuda) / kb ** 0.5
        for reader in ("plain", "pool"):
            _three_way_dgrad(ops, dy, w2, y, imgs, 1.0, reader, g, f"M{m} N{n} Kf{kf} Kb{kb} {reader}")
        del y, imgs, dy
    # ---- part 2
    sex, label, site = torch.ones(1, device=cuda), torch.tensor([3], device=cuda), torch.tensor([1], device=cuda)
    from oracle import toad_oracle as orc
    from tests.helpers import assert_step_grad_matches_per_op
    from toad_amd import TOAD_fc_mtl_concat
    for size_arg in ("big", "small"):
        model = TOAD_fc_mtl_concat(n_classes=18, size_arg=size_arg)
        model.load_state_dict(orc.xavier_params(18, seed=2, size_arg=size_arg)); model.relocate()
        w = {k: v.detach() for k, v in model._weights().items()}
        d = w["wa"].shape[0]

        def step(bag):
            gr = {k: torch.full_like(w[k], 7.0) for k in ops.STEP_SLOTS}
            loss, logits, slog = ops.mil_step(w, gr, 0.0, bag, sex, label, site, 0.75, 0.25, want_logits=True)
            return loss.clone(), logits.clone(), gr

        def per_op(bag, images=True):
            outs, sv = F_.mil_forward(w, bag, sex)
            assert sv.h1_bits is not None and sv.h_bits is not None          # the images are in play on this route
            if not images:
                sv.h1_bits = sv.h_bits = None                                # ... unless the fp32 masks are asked for
            _, dl, ds = ops.mtl_ce_fwd_bwd(outs["logits"], outs["site_logits"], label, site, 0.75, 0.25)
            gd, _ = F_.mil_backward(w, sv, dl, ds)
            gd = dict(gd)
            gd["wab"] = torch.cat([gd["wa"], gd["wb"]], 0); gd["bab"] = torch.cat([gd["ba"], gd["bb"]], 0)
            return outs["logits"].clone(), {k: gd[k].clone() for k in ops.STEP_SLOTS}

        _, logits_s, g_s = step(small)
        logits_sp, g_sp = per_op(small)
        ops.release_workspaces()
        torch.cuda.empty_cache()
        _poison_free_blocks(cuda, 4 * ops.relu_bits_bytes(m, 512) + (1 << 30))
        logits_p, g_p = per_op(big)
        _poison_free_blocks(cuda, 4 * ops.relu_bits_bytes(m, 512) + (1 << 30))
        ops.release_workspaces()
        _, logits_w, g_w = step(big)
        for name, lg, gg, ref_l, ref_g in (("per-op", logits_p, g_p, logits_sp, g_sp), ("whole-slide", logits_w, g_w, logits_s, g_s)):
            el = (lg - ref_l).abs().max().item()
            assert el <= 1e-5, f"{size_arg} {name}: logits {el:.2e}"
            for k in ops.STEP_SLOTS:
                eg = (gg[k] - ref_g[k]).abs().max().item()
                assert eg <= 1e-4, f"{size_arg} {name}: gradient {k} {eg:.2e}"
        # and, free of any ReLU-boundary effect: the per-op route gives bitwise the same gradients from the images as from the fp32 masks,
        # and the whole-slide call - the same launches over the same row chunks - gives the per-op route's
        _, g_m = per_op(big, images=False)
        for k in ops.STEP_SLOTS:
            assert torch.equal(g_p[k], g_m[k]), f"{size_arg}: gradient {k} from the bit images != from the fp32 masks"
            assert_step_grad_matches_per_op(g_w[k], g_p[k], k, m)
        assert torch.equal(logits_p, logits_w)
        assert d == (384 if size_arg == "big" else 256)
        del g_p, g_w, g_m


# ---- whole-slide and batched calls over a poisoned workspace ----------------------------------------------------------------------------

def _fill_workspaces(ops, dev, fill):
    """Every cached workspace (the step's arena, slabs, abs-max arrays and both bit images live in them) and the allocator's free blocks."""
    torch.cuda.synchronize()
    total = 0
    for t in ops._WS_CACHE.values():
        t.fill_(fill)
        total += t.numel()
    _poison_free_blocks(dev, max(total, 1 << 26), fill)
    return total


@pytest.mark.parametrize("n", (64, 300, 2000, 4097, 10000, 16500, 40000))
@pytest.mark.parametrize("bag_kind", ("fp32", "fp16", "prepared"))
def test_whole_slide_step_does_not_depend_on_what_its_workspace_held(cuda, bag_kind, n):
    """ops.mil_step on one slide, dropout off and on: run, fill every cached workspace with 0xFF, run, fill with 0x00, run - loss, logits and all
    gradient slots bitwise equal. The sizes straddle the switch to half-height tiles and the fp16 / prepared bag's layer-1 rule
    (csrc/step.hip step_dgrad1_reads_bits)."""
    from toad_amd import ops
    _, w = _weights(cuda, "big", seed=n)
    g = torch.Generator(device=cuda).manual_seed(n)
    x = torch.randn(n, 1024, generator=g, device=cuda)
    bag = x if bag_kind == "fp32" else (x.half() if bag_kind == "fp16" else ops.prepare_bag(x))
    sex, label, site = torch.ones(1, device=cuda), torch.tensor([5], device=cuda), torch.tensor([0], device=cuda)
    for drop in (0.0, 0.25):
        runs = []
        for fill in (None, 0xFF, 0x00):
            if fill is not None:
                assert _fill_workspaces(ops, cuda, fill) > 0
            gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
            loss, logits, slog = ops.mil_step(w, gr, 0.0, bag, sex, label, site, 0.75, 0.25, drop, 99, want_logits=True)
            runs.append((loss.clone(), logits.clone(), slog.clone(), gr))
        assert torch.isfinite(runs[0][0]).all()
        for i, name in ((1, "0xFF"), (2, "0x00")):
            for a, b, what in zip(runs[i][:3], runs[0][:3], ("loss", "logits", "site_logits")):
                assert torch.equal(a, b), f"{bag_kind} n={n} drop={drop}: {what} changed over a workspace of {name}"
            for k in ops.STEP_SLOTS:
                assert torch.equal(runs[i][3][k], runs[0][3][k]), f"{bag_kind} n={n} drop={drop}: gradient {k} changed over a workspace of {name}"


@pytest.mark.parametrize("lens", ([1, 2, 63, 300, 1000, 257, 64], [3000, 5000, 777]))
def test_batched_calls_do_not_depend_on_what_their_workspace_held(cuda, lens):
    """ops.mil_multi_step and forward_batch + backward on a ragged batch, dropout off and on, over workspaces (and allocator free blocks, where
    forward_batch takes its arena from) of as-is / 0xFF / 0x00 contents."""
    import torch.nn.functional as F
    from toad_amd import functional as F_, ops
    nb = len(lens)
    for dropout in (False, True):
        from toad_amd import TOAD_fc_mtl_concat
        torch.manual_seed(len(lens))
        model = TOAD_fc_mtl_concat(n_classes=18, dropout=dropout)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.05)
        model.relocate(); model.train()
        w = {k: v.detach() for k, v in model._weights().items()}
        g = torch.Generator(device=cuda).manual_seed(sum(lens))
        bags = [torch.randn(m, 1024, generator=g, device=cuda) for m in lens]
        sex = torch.tensor([float(i % 2) for i in range(nb)], device=cuda)
        label = torch.tensor([(7 * i) % 18 for i in range(nb)], device=cuda)
        site = torch.tensor([i % 2 for i in range(nb)], device=cuda)
        drop = 0.25 if dropout else 0.0
        runs = []
        for fill in (None, 0xFF, 0x00):
            if fill is not None:
                assert _fill_workspaces(ops, cuda, fill) > 0
            gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
            loss, logits, slog = ops.mil_multi_step(w, gr, 0.0, bags, sex, label, site, 0.75 / nb, 0.25 / nb, drop, 4321, want_logits=True)
            res = [loss.clone(), logits.clone(), slog.clone()] + [gr[k] for k in ops.STEP_SLOTS]
            if fill is not None:
                _fill_workspaces(ops, cuda, fill)
            model.zero_grad(set_to_none=True)
            torch.manual_seed(77)                              # forward_batch draws its dropout seed from torch's generator
            outs = model.forward_batch(bags, sex)
            total = sum(0.75 * F.cross_entropy(o["logits"], label[i:i + 1]) + 0.25 * F.cross_entropy(o["site_logits"], site[i:i + 1])
                        for i, o in enumerate(outs)) / nb
            total.backward()
            sp = model._slot_params()
            res += [total.detach().clone()] + [o["logits"].detach().clone() for o in outs] + [sp[k].grad.detach().clone() for k in F_.SLOTS]
            runs.append(res)
        assert all(torch.isfinite(t).all() for t in runs[0])
        for i, name in ((1, "0xFF"), (2, "0x00")):
            assert len(runs[i]) == len(runs[0])
            for j, (a, b) in enumerate(zip(runs[i], runs[0])):
                assert torch.equal(a, b), f"lens={lens} dropout={dropout}: result {j} changed over workspaces of {name}"
