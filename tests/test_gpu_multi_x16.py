"""GPU: fp16 bags through the ragged multi-slide calls as they are stored (toad_mil_multi_{step,fwd,bwd}_x16_f32): the A16 first Linear on the
concatenated halves, the layer-1 weight gradient as a B16 product - inside the ONE weight-gradient launch for calls of at most 262,144 rows,
gemm_tn_h2_batch_kernel<true> - no up-cast pass and no fp32 copy, from the kernels up to forward_batch, SlideShardedDP and the ingest's fp16
landing buffers. Reference semantics: the reference up-casts whatever the .pt file holds (datasets/dataset_mtl_concat.py:358-373) and steps
slide by slide (utils/core_utils_mtl_concat.py:200-234); the batch gradient is the sum of the slide gradients."""
import pytest
import torch

from oracle import toad_oracle as orc
from tests.helpers import SLOT2KEY, assert_grad_close_or_few_flips, check_batch_against_oracle

pytestmark = pytest.mark.gpu

C = 18
TRUNK_SLOTS = ("w1", "b1", "w2", "b2")          # the gradients a ReLU mask reaches (tests/helpers.py MASK_FREE_KEYS is the complement)


def _model(cuda, seed=0, dropout=False):
    from toad_amd import TOAD_fc_mtl_concat
    torch.manual_seed(seed)
    m = TOAD_fc_mtl_concat(n_classes=C, dropout=dropout)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.relocate()
    return m, params


def _batch(lens, cuda, seed):
    """One fp16 buffer holding the bags back to back, its row offsets, per-slide sex / label / site on the device."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    buf = (torch.randn(sum(lens), 1024, generator=g, device=cuda) * 0.7).half()
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    nb = len(lens)
    sex = torch.tensor([float(i % 2) for i in range(nb)], device=cuda)
    label = torch.tensor([(7 * i) % C for i in range(nb)], device=cuda)
    site = torch.tensor([(i // 2) % 2 for i in range(nb)], device=cuda)
    return buf, offs, sex, label, site


def _close(got, ref, what, report=None, failures=None):
    """1e-6 of the tensor's magnitude: the bound of tests/test_gpu_h2.py::test_fp16_bag_equals_the_upcast_bag for this statement. With
    `failures`, a miss is collected (the caller asserts the list is empty at its end, so one run shows every figure)."""
    s = ref.abs().max().item()
    tol = 1e-6 * max(s, 1e-12)
    err = (got - ref).abs().max().item()
    if report is not None:
        report.append(f"{what}: err {err:.3e} = {err / max(s, 1e-300):.2e} of magnitude {s:.3e}")
    msg = f"{what}: {err:.3e} > {tol:.3e} ({err / max(s, 1e-300):.2e} of the tensor's magnitude {s:.3e})"
    if failures is not None:
        if err > tol:
            failures.append(msg)
        return
    assert err <= tol, msg


def _mask_differences(h16, h32, what):
    """ReLU masks of the two routes. fp16-valued inputs are exact under either route's power-of-two scale, so the routes sum the SAME products,
    and on the same tile plan in the same order: no difference is expected. Should the sums ever round differently, a pre-activation within
    round-off of zero may land on either side; such a difference is legitimate only if the activation is round-off itself on the side where
    it is positive: 1e-6 of the tensor's magnitude, the value bound."""
    diff = (h16 > 0) != (h32 > 0)
    n = int(diff.sum())
    if n:
        worst = torch.maximum(h16, h32)[diff].max().item()
        assert worst <= 1e-6 * h32.abs().max().item(), f"{what}: a ReLU mask differs at an activation of {worst:.3e}: not round-off of zero"
    return n


BATCHES = [[256] * 8, [1, 2, 63, 300, 1000, 257, 64], [3000, 5000, 777], [10000] * 4, [50000, 50000],
           [100000, 50000, 50000, 100000, 100000, 100000, 24288]]         # 524,288 rows: the default call size, above kTnBatchMaxRows


@pytest.mark.parametrize("drop_p", [0.0, 0.25])
@pytest.mark.parametrize("lens", BATCHES, ids=["8x256", "ragged_1_to_1000", "8777_rows", "4x10000", "2x50000", "524288_rows"])
def test_fp16_multi_equals_fp32_multi_on_the_upcast_bags(cuda, lens, drop_p):
    """ops.mil_multi_step and mil_multi_fwd + mil_multi_bwd (with dA_ext and dMcat_ext) on fp16 bags against the same calls on the up-cast
    bags, same (drop_p, seed): losses, logits, A, features and all 12 gradient slots within 1e-6 of each tensor's magnitude. The ReLU masks are
    compared element by element first (H1, H of both routes from the arenas): the trunk gradients get a flip allowance only for a mask
    difference that was shown to be legitimate (_mask_differences), never otherwise."""
    from toad_amd import ops
    model, _ = _model(cuda, seed=len(lens), dropout=drop_p > 0)
    w = {k: v.detach() for k, v in model._weights().items()}
    x16, offs, sex, label, site = _batch(lens, cuda, seed=sum(lens))
    B, n = len(lens), sum(lens)
    seed = 20261016
    report = []
    # ---- the split pair first: its arenas show the activations of both routes
    g = torch.Generator(device=cuda).manual_seed(3)
    dl = torch.randn(B, C, generator=g, device=cuda) / B
    ds = torch.randn(B, 2, generator=g, device=cuda) / B
    da = torch.randn(n, 2, generator=g, device=cuda) * 1e-3
    dm = torch.randn(B, 2, 513, generator=g, device=cuda) * 1e-2
    res = {}
    for kind in ("fp32", "fp16"):
        x = x16 if kind == "fp16" else x16.float()
        arena, o = ops.mil_multi_fwd(w, x, sex, drop_p, seed, offsets=offs)
        assert arena.xcat.dtype == x.dtype
        gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
        ops.mil_multi_bwd(w, gr, 0.0, None, None, arena, dl, ds, da, dm, drop_p, seed)
        res[kind] = dict(out={k: o[k].clone() for k in ("logits", "site_logits", "a_raw", "features", "y_prob", "site_prob", "y_hat")},
                         h1=arena.view("h1", (n, 512)), h=arena.view("h", (n, 512)), grads=gr, arena=arena)
        del x
    flips = _mask_differences(res["fp16"]["h1"], res["fp32"]["h1"], "H1") + _mask_differences(res["fp16"]["h"], res["fp32"]["h"], "H")
    report.append(f"rows {n}: {flips} ReLU-mask differences between the routes")
    _close(res["fp16"]["h1"], res["fp32"]["h1"], "H1", report=report)
    _close(res["fp16"]["h"], res["fp32"]["h"], "H", report=report)
    for k in ("logits", "site_logits", "a_raw", "features", "y_prob", "site_prob"):
        _close(res["fp16"]["out"][k], res["fp32"]["out"][k], f"fwd {k}", report=report)
    assert torch.equal(res["fp16"]["out"]["y_hat"], res["fp32"]["out"]["y_hat"])

    failures = []

    def grads_close(g16, g32, what):
        for k in ops.STEP_SLOTS:
            if flips and k in TRUNK_SLOTS:
                # a mask difference shown above to sit at round-off of zero moves one dZ element, i.e. a rank-one term of these gradients
                # (tests/helpers.py assert_grad_close_or_few_flips); everything outside those terms is held to the same 1e-6
                s = max(g32[k].abs().max().item(), 1e-12)
                try:
                    assert_grad_close_or_few_flips(g16[k], g32[k], 1e-6, s, what=f"{what} {k} ({flips} legitimate mask differences)")
                except AssertionError as e:
                    failures.append(str(e))
            else:
                _close(g16[k], g32[k], f"{what} {k}", report=report, failures=failures)

    try:
        grads_close(res["fp16"]["grads"], res["fp32"]["grads"], "fwd+bwd grad")
        del res
        # ---- the fused step
        out = {}
        for kind in ("fp32", "fp16"):
            x = x16 if kind == "fp16" else x16.float()
            gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
            loss, logits, slog = ops.mil_multi_step(w, gr, 0.0, x, sex, label, site, 0.75 / B, 0.25 / B, drop_p, seed, want_logits=True, offsets=offs)
            out[kind] = (loss.clone(), logits.clone(), slog.clone(), gr)
            del x
        for a, b, what in zip(out["fp16"][:3], out["fp32"][:3], ("step loss", "step logits", "step site_logits")):
            _close(a, b, what, report=report)
        grads_close(out["fp16"][3], out["fp32"][3], "step grad")
        # a list of fp16 views of the buffer is the same call (no copy), and so is beta = 1 on top
        g2 = {k: out["fp16"][3][k].clone() for k in ops.STEP_SLOTS}
        ops.mil_multi_step(w, g2, 1.0, [x16[offs[i]:offs[i + 1]] for i in range(B)], sex, label, site, 0.75 / B, 0.25 / B, drop_p, seed)
        for k in ops.STEP_SLOTS:
            assert (g2[k] - 2 * out["fp16"][3][k]).abs().max().item() <= 1e-6 * max(out["fp16"][3][k].abs().max().item(), 1e-30) + 1e-12, k
        assert not failures, "\n".join(failures)
    finally:
        print("\n".join(report))


def _step_workspace_activations(n, nb, c, d, dev):
    """What the fused multi-slide step left in the cached step workspace (the forward arena sits at its aligned base, csrc/step.hip): H1, H, P
    and A_raw of the concatenation, as in tests/test_gpu_multi_step.py."""
    import ctypes
    from toad_amd import _lib, ops
    lib = _lib.load()
    ws = ops._ws(int(lib.toad_mil_multi_ws_bytes(n, nb, c, d)), dev, "step")
    base = (-ws.data_ptr()) % int(lib.toad_mil_buffer_align(n))
    offs = (ctypes.c_int64 * len(ops.ARENA_SLOTS))()
    _lib.check(lib.toad_mil_arena_layout(n, c, d, offs), "toad_mil_arena_layout")
    off = dict(zip(ops.ARENA_SLOTS, (base + int(o) for o in offs)))

    def view(name, cols):
        return ws[off[name]:off[name] + n * cols * 4].view(torch.float32).view(n, cols)
    return view("h1", 512), view("h", 512), view("p", 2 * d), view("a_raw", 2)


@pytest.mark.parametrize("name,lens,drop_p", [("x16_ragged", [300, 1000, 257, 64, 2049], 0.0), ("x16_dropout_10k", [6000, 4000, 1500], 0.25)])
def test_fp16_multi_step_against_the_oracle(cuda, name, lens, drop_p):
    """The fp16 route answers to the reference, not only to its fp32 sibling: tests/helpers.py::check_batch_against_oracle with the bags' fp16
    values as the oracle's input, at that helper's bounds (1e-4 outputs, 2e-5 of each gradient's scale)."""
    from toad_amd import functional as F_, ops
    model, params = _model(cuda, seed=len(lens) + 7, dropout=drop_p > 0)
    if drop_p > 0:                                            # dropout=True shifts the state-dict indices; the oracle uses the dropout=False names
        rename = {"attention_net.3.": "attention_net.2.", "attention_net.6.": "attention_net.4."}
        params = {next((b + k[len(a):] for a, b in rename.items() if k.startswith(a)), k): v for k, v in params.items()}
    w = {k: v.detach() for k, v in model._weights().items()}
    x16, offs, sex, label, site = _batch(lens, cuda, seed=11)
    B, ntot, d = len(lens), sum(lens), w["wc"].shape[1]
    seed = 20261017
    g = {k: torch.zeros_like(w[k]) for k in ops.STEP_SLOTS}
    loss, logits, slog = ops.mil_multi_step(w, g, 0.0, x16, sex, label, site, 0.75 / B, 0.25 / B, drop_p=drop_p, seed=seed, want_logits=True, offsets=offs)
    torch.cuda.synchronize()
    h1_d, h_d, p_d, a_d = (t.cpu() for t in _step_workspace_activations(ntot, B, C, d, cuda))
    xc = x16.float().cpu()
    slides = [(xc[offs[b]:offs[b + 1]], sex[b:b + 1].cpu(), label[b:b + 1].cpu(), site[b:b + 1].cpu()) for b in range(B)]
    G, mask64 = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF
    masks = None
    if drop_p > 0:
        s1, s2, sa, sb = F_.drop_seeds(seed)
        mk_h1 = ops.dropout_mask(ntot * 512, drop_p, s1, cuda).reshape(ntot, 512).cpu()
        mk_h = ops.dropout_mask(ntot * 512, drop_p, s2, cuda).reshape(ntot, 512).cpu()
        masks = [{"h1": mk_h1[offs[b]:offs[b + 1]], "h": mk_h[offs[b]:offs[b + 1]],
                  "a": ops.dropout_mask(lens[b] * d, drop_p, (sa + 2 * b * G) & mask64, cuda).reshape(lens[b], d).cpu(),
                  "b": ops.dropout_mask(lens[b] * d, drop_p, (sb + 2 * b * G) & mask64, cuda).reshape(lens[b], d).cpu()} for b in range(B)]
    got = dict(g)
    got["wa"], got["wb"], got["ba"], got["bb"] = g["wab"][:d], g["wab"][d:], g["bab"][:d], g["bab"][d:]
    check_batch_against_oracle(name, params, slides, offs, dict(h1=h1_d, h=h_d, p=p_d, a_raw=a_d, logits=logits.cpu(), site_logits=slog.cpu(), loss=loss.cpu()),
                               {s_: got[s_].cpu() for s_ in SLOT2KEY}, masks)
    assert orc.PARAM_KEYS                                     # (the oracle module is the reference restatement the helper runs)


def test_fp16_views_of_one_buffer_run_without_a_copy_or_an_up_cast(cuda):
    """fp16 views cut from one buffer: the arena keeps an fp16 xcat at the buffer's address; forward_batch + backward() and SlideShardedDP on bags
    landed by BagPrefetcher(arena_rows=..., arena_dtype=torch.float16) give the gradients of the same bags up-cast in separate allocations."""
    import torch.nn.functional as F
    from toad_amd import functional as F_, ops
    from toad_amd.dp import SlideShardedDP
    from toad_amd.ingest import BagPrefetcher
    lens = [700, 64, 1300, 500]
    g = torch.Generator().manual_seed(9)
    recs = [((torch.randn(n, 1024, generator=g) * 0.7).half(), (3 * i) % C, i % 2, float(i % 2)) for i, n in enumerate(lens)]
    landed = [(b, sx, lb, st) for (b, lb, st, sx) in BagPrefetcher(recs, cuda, depth=3, dtype=torch.float16, arena_rows=4096, arena_dtype=torch.float16)]
    torch.cuda.synchronize()
    for (b, _, _, _), r in zip(landed, recs):
        assert b.dtype == torch.float16 and torch.equal(b.cpu(), r[0])
    bags = [s[0] for s in landed]
    view = ops._adjacent_rows(bags)
    assert view is not None and view.dtype == torch.float16 and view.data_ptr() == bags[0].data_ptr()
    model, _ = _model(cuda, seed=2)
    model.train()
    w = {k: v.detach() for k, v in model._weights().items()}
    sex = torch.cat([s[1] for s in landed])
    arena, _ = ops.mil_multi_fwd(w, bags, sex)
    assert arena.xcat.dtype == torch.float16 and arena.xcat.data_ptr() == bags[0].data_ptr() and arena.xcat.shape == (sum(lens), 1024)
    del arena
    apart32 = [b.float().clone() for b in bags]
    assert ops._adjacent_rows(apart32) is None
    label = torch.cat([s[2] for s in landed]); site = torch.cat([s[3] for s in landed])
    # ---- forward_batch + backward()
    grads = []
    for bb in (bags, apart32):
        model.zero_grad(set_to_none=True)
        ops.enable_timing(True)
        outs = model.forward_batch(bb, sex)
        total = sum(0.75 * F.cross_entropy(o["logits"], label[i:i + 1]) + 0.25 * F.cross_entropy(o["site_logits"], site[i:i + 1])
                    for i, o in enumerate(outs)) / len(lens)
        total.backward()
        names = ops.collect_timing()
        ops.enable_timing(False)
        half = bb is bags
        assert names.get("mil_multi_fwd_x16" if half else "mil_multi_fwd", (0,))[0] == 1 and names.get("mil_multi_bwd_x16" if half else "mil_multi_bwd", (0,))[0] == 1
        assert ("mil_multi_fwd" in names) != half
        sp = model._slot_params()
        grads.append([("loss", total.detach().clone())] + [(f"logits {i}", o["logits"].detach().clone()) for i, o in enumerate(outs)] +
                     [(k, sp[k].grad.detach().clone()) for k in F_.SLOTS])
    report, failures = [], []
    for (name, a), (_, b) in zip(*grads):
        _close(a, b, f"forward_batch {name}", report=report, failures=failures)
    print("\n".join(report))
    assert not failures, "\n".join(failures)
    # ---- SlideShardedDP.step on the landed bags against the same bags up-cast in separate allocations
    flat = []
    for slides in (landed, [(x, sx, lb, st) for x, (_, sx, lb, st) in zip(apart32, landed)]):
        m2, _ = _model(cuda, seed=2)
        m2.train()
        dp = SlideShardedDP(m2, {"lr": 1e-3, "weight_decay": 1e-5})
        ops.enable_timing(True)
        dp.accumulate(slides, len(slides))
        names = ops.collect_timing()
        assert ops.timing_call_count() == 1                    # the whole shard is ONE library call on either route
        ops.enable_timing(False)
        assert ("mil_multi_step_x16" in names) == (slides is landed) and ("mil_multi_step" in names) == (slides is not landed)
        flat.append(dp.flat_grad.clone())
        losses = dp.step(slides, len(slides))
        assert len(losses) == len(lens) and torch.isfinite(torch.stack([l[0] for l in losses])).all()
    assert (flat[0] - flat[1]).abs().max().item() <= 1e-6 * flat[1].abs().max().item()


def test_a_mixed_shard_is_cut_where_the_dtype_changes(cuda):
    """[fp16, fp16, fp32, fp32, fp16]: one x16 multi-slide call, one fp32 multi-slide call, one one-slide x16 step - three library calls, no up-cast -
    and the gradient of the five slides."""
    from toad_amd import ops
    from toad_amd.dp import SlideShardedDP
    lens = [300, 512, 1000, 257, 640]
    kinds = [torch.float16, torch.float16, torch.float32, torch.float32, torch.float16]
    g = torch.Generator().manual_seed(21)
    slides = [((torch.randn(n, 1024, generator=g) * 0.7).half().to(dt).to(cuda), torch.tensor([float(i % 2)], device=cuda),
               torch.tensor([(5 * i) % C], device=cuda), torch.tensor([i % 2], device=cuda)) for i, (n, dt) in enumerate(zip(lens, kinds))]
    out = []
    for shard in (slides, [(s[0].float(),) + s[1:] for s in slides]):
        model, _ = _model(cuda, seed=6)
        model.train()
        dp = SlideShardedDP(model, {"lr": 1e-3, "weight_decay": 1e-5})
        ops.enable_timing(True)
        dp.accumulate(shard, len(shard))
        names = ops.collect_timing()
        calls = ops.timing_call_count()
        ops.enable_timing(False)
        if shard is slides:
            assert calls == 3 and names["mil_multi_step_x16"][0] == 1 and names["mil_multi_step"][0] == 1, (calls, {k: v[0] for k, v in names.items()})
        else:
            assert calls == 1 and names["mil_multi_step"][0] == 1 and "mil_multi_step_x16" not in names
        out.append(dp.flat_grad.clone())
    # (different batching: operand scales and tile plans per call, the bound of tests/test_gpu_multi_step.py::test_dp_step_batches_small_slides)
    assert (out[0] - out[1]).abs().max().item() <= 5e-5 * out[1].abs().max().item()


def _fill_workspaces(ops, dev, fill):
    """Every cached workspace and the allocator's free blocks (tests/test_gpu_relu_bits.py)."""
    torch.cuda.synchronize()
    total = 0
    for t in ops._WS_CACHE.values():
        t.fill_(fill)
        total += t.numel()
    torch.cuda.synchronize()
    t = torch.full((max(total, 1 << 26),), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    del t
    return total


@pytest.mark.parametrize("lens", ([1, 2, 63, 300, 1000, 257, 64], [3000, 5000, 777], [10000, 6500], [6000, 4000]),
                         ids=["ragged_1_to_1000", "8777_rows", "16500_rows", "10000_rows_half_height_dgrad"])
def test_fp16_batched_calls_do_not_depend_on_what_their_workspace_held(cuda, lens):
    """The device-side half of the bit-image contract of the fp16 multi route (tests/test_multi_x16_host.py): ops.mil_multi_step and
    forward_batch + backward on fp16 bags, dropout off and on, over workspaces and allocator free blocks of as-is / 0xFF / 0x00 contents -
    losses, logits and every gradient bitwise equal. 8,777 and 10,000 rows: the layer-1 dgrad runs on half-height tiles, which read the
    image for every tile - the A16 forward must have run on half-height tiles as well (on 256-row tiles its K-split tiles write no bits)."""
    import torch.nn.functional as F
    from toad_amd import TOAD_fc_mtl_concat, functional as F_, ops
    nb = len(lens)
    for dropout in (False, True):
        torch.manual_seed(len(lens))
        model = TOAD_fc_mtl_concat(n_classes=C, dropout=dropout)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.05)
        model.relocate(); model.train()
        w = {k: v.detach() for k, v in model._weights().items()}
        g = torch.Generator(device=cuda).manual_seed(sum(lens))
        bags = [(torch.randn(m, 1024, generator=g, device=cuda) * 0.7).half() for m in lens]
        sex = torch.tensor([float(i % 2) for i in range(nb)], device=cuda)
        label = torch.tensor([(7 * i) % C for i in range(nb)], device=cuda)
        site = torch.tensor([i % 2 for i in range(nb)], device=cuda)
        drop = 0.25 if dropout else 0.0
        runs = []
        for fill in (None, 0xFF, 0x00):
            if fill is not None:
                assert _fill_workspaces(ops, cuda, fill) > 0
            gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
            ops.enable_timing(True)
            loss, logits, slog = ops.mil_multi_step(w, gr, 0.0, bags, sex, label, site, 0.75 / nb, 0.25 / nb, drop, 4321, want_logits=True)
            assert "mil_multi_step_x16" in ops.collect_timing()
            ops.enable_timing(False)
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
                assert torch.equal(a, b), f"lens={lens} dropout={dropout}: result {j} changed over workspaces of {name} ({(a != b).sum().item()} elements)"


@pytest.mark.parametrize("n", [2000, 20000])
def test_one_slide_x16_step_on_the_batched_weight_gradient_launch(cuda, n):
    """The one-slide x16 step now takes the one-launch weight gradient too (csrc/step.hip backward_body: bags of 64 ... 262,144 rows): still within
    the bound of tests/test_gpu_h2.py::test_fp16_bag_equals_the_upcast_bag against the fp32 step on the up-cast bag, and bitwise run to run."""
    from toad_amd import ops
    model, _ = _model(cuda, seed=n)
    model.train()
    w = {k: v.detach() for k, v in model._weights().items()}
    g = torch.Generator().manual_seed(40 + n)
    x16 = (torch.randn(n, 1024, generator=g) * 0.7).half().to(cuda)
    sex = torch.tensor([1.0], device=cuda); label = torch.tensor([3], device=cuda); site = torch.tensor([1], device=cuda)
    runs = []
    for x in (x16.float(), x16, x16):
        gr = {k: torch.full_like(w[k], 3.0) for k in ops.STEP_SLOTS}
        loss, logits, slog = ops.mil_step(w, gr, 0.0, x, sex, label, site, want_logits=True)
        runs.append((loss.clone(), logits.clone(), slog.clone(), gr))
    for a, b in zip(runs[1][:3], runs[0][:3]):
        assert (a - b).abs().max().item() <= 1e-6 * max(b.abs().max().item(), 1e-6)
    for k in ops.STEP_SLOTS:
        ref = runs[0][3][k]
        s = ref.abs().max().item()
        err = (runs[1][3][k] - ref).abs().max().item()
        assert err <= 1e-6 * max(s, 1e-12), (k, err, s)
        assert torch.equal(runs[1][3][k], runs[2][3][k]), k
