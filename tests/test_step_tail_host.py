"""CPU: the host statement of the step tail (tests/tail_ref.py) against torch in float64, the reach of the device tests' shape table over the
three staging paths of heads_ce_fused_kernel, and the argument refusals of the heads entry points that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tail_ref as tr


def _case(L, C, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return dict(M=rng.standard_normal((2, L)), sex=float(seed % 2), Wcls=0.1 * rng.standard_normal((C, L + 1)), bcls=0.1 * rng.standard_normal(C),
                Wsite=0.1 * rng.standard_normal((2, L + 1)), bsite=0.1 * rng.standard_normal(2), ext=rng.standard_normal((2, L + 1)),
                label=int(rng.integers(C)), site=int(rng.integers(2)))


@pytest.mark.parametrize("L,C", [(512, 18), (512, 100), (128, 99), (8, 3), (4, 1), (513, 5)])
def test_heads_and_loss_statement_matches_autograd_in_float64(L, C):
    """models/model_toad.py:99-107 as nn.Linear on the concatenated rows, utils/core_utils_mtl_concat.py:213-215 as two CrossEntropyLoss; an extra
    loss term <ext, Mcat> plays the caller's dMcat_ext."""
    c = _case(L, C, 100 * L + C)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    cls, sitecls = torch.nn.Linear(L + 1, C).double(), torch.nn.Linear(L + 1, 2).double()
    with torch.no_grad():
        cls.weight.copy_(t(c["Wcls"])); cls.bias.copy_(t(c["bcls"])); sitecls.weight.copy_(t(c["Wsite"])); sitecls.bias.copy_(t(c["bsite"]))
    M = t(c["M"]).requires_grad_(True)
    sex = torch.tensor([c["sex"]], dtype=torch.float64, requires_grad=True)
    mcat = torch.cat([M, sex.repeat(2, 1)], dim=1)
    logits, slog = cls(mcat[0].unsqueeze(0)), sitecls(mcat[1].unsqueeze(0))
    ce = torch.nn.CrossEntropyLoss()
    lc, ls = ce(logits, torch.tensor([c["label"]])), ce(slog, torch.tensor([c["site"]]))
    loss = 0.75 * lc + 0.25 * ls
    logits.retain_grad(); slog.retain_grad()
    (loss + (t(c["ext"]) * mcat).sum()).backward()

    r_mcat, r_lg, r_p, r_hat, r_sl, r_sp, r_shat = tr.heads_fwd(c["M"], c["sex"], c["Wcls"], c["bcls"], c["Wsite"], c["bsite"])
    r_loss, r_dl, r_ds = tr.ce(r_lg, c["label"], r_sl, c["site"], 0.75, 0.25)
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a), b.detach().numpy().reshape(np.asarray(a).shape), rtol=1e-12, atol=1e-13)
    close(r_mcat, mcat); close(r_lg, logits); close(r_sl, slog)
    close(r_p, torch.softmax(logits, 1)); close(r_sp, torch.softmax(slog, 1))
    assert r_hat == int(torch.topk(logits, 1, dim=1)[1]) and r_shat == int(torch.topk(slog, 1, dim=1)[1])
    close(r_loss, torch.stack([loss, lc, ls]))
    close(r_dl, logits.grad); close(r_ds, slog.grad)
    dW, db, dWs, dbs, dM, dsex = tr.heads_bwd(r_mcat, r_dl, r_ds, c["Wcls"], c["Wsite"], c["ext"])
    close(dW, cls.weight.grad); close(db, cls.bias.grad); close(dWs, sitecls.weight.grad); close(dbs, sitecls.bias.grad)
    close(dM, M.grad); close(dsex, sex.grad)
    # beta: the previous gradients are scaled and added to
    prev = [np.ones_like(dW), np.ones_like(db), 2 * np.ones_like(dWs), 3 * np.ones_like(dbs)]
    acc = tr.heads_bwd(r_mcat, r_dl, r_ds, c["Wcls"], c["Wsite"], c["ext"], prev=prev, beta=0.5)
    for got, new, old in zip(acc[:4], (dW, db, dWs, dbs), prev):
        np.testing.assert_allclose(got, 0.5 * old + new, rtol=0, atol=1e-15)
    # no external gradient
    plain = tr.heads_bwd(r_mcat, r_dl, r_ds, c["Wcls"], c["Wsite"])
    np.testing.assert_allclose(plain[4], dM - c["ext"][:, :L], rtol=1e-12, atol=1e-13)


def test_first_maximal_index_and_large_logits():
    lg = np.array([1.0, 7.0, 7.0, -3.0, 7.0])
    W = np.zeros((5, 3)); sl = np.zeros((2, 3))
    out = tr.heads_fwd(np.zeros((2, 2)), 0.0, W, lg, sl, np.array([2.0, 2.0]))
    assert out[3] == 1 and out[6] == 0 and out[2][1] == out[2][2] == out[2][4]
    loss, dl, _ = tr.ce(np.array([1e4, -1e4, 0.0]), 1, np.zeros(2), 0)
    assert np.isfinite(loss).all() and loss[1] == 2e4 and dl[1] == -0.75


ADAM_SETTINGS = [dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5), dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
                 dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-3, weight_decay=1e-5)]


@pytest.mark.parametrize("hp", ADAM_SETTINGS)
def test_adam_statement_matches_torch_in_float64(hp):
    g_ = torch.Generator().manual_seed(3)
    n = 1020
    p = torch.nn.Parameter(torch.randn(n, dtype=torch.float64, generator=g_) * 0.05)
    opt = torch.optim.Adam([p], **hp)
    rp, rm, rv = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 5):
        g = torch.randn(n, dtype=torch.float64, generator=g_) * 1e-2
        g[::4] = 0.0
        p.grad = g.clone()
        opt.step()
        rp, rm, rv = tr.adam_step(rp, g.numpy(), rm, rv, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], step)
        st = opt.state[p]
        for got, ref in ((rp, p.detach()), (rm, st["exp_avg"]), (rv, st["exp_avg_sq"])):
            np.testing.assert_allclose(got, ref.numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_statement_matches_torch_in_float64(momentum):
    g_ = torch.Generator().manual_seed(4)
    n = 1020
    p = torch.nn.Parameter(torch.randn(n, dtype=torch.float64, generator=g_) * 0.05)
    opt = torch.optim.SGD([p], lr=1e-2, momentum=momentum, weight_decay=1e-5)
    rp, rb = p.detach().numpy().copy(), None
    for step in range(1, 5):
        g = torch.randn(n, dtype=torch.float64, generator=g_) * 1e-2
        p.grad = g.clone()
        opt.step()
        rp, rb = tr.sgd_step(rp, g.numpy(), rb, 1e-2, momentum, 1e-5, step)
        np.testing.assert_allclose(rp, p.detach().numpy(), rtol=1e-12, atol=1e-300)
        if momentum:
            np.testing.assert_allclose(rb, opt.state[p]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-300)
        else:
            assert rb is None and "momentum_buffer" not in opt.state[p] or opt.state[p].get("momentum_buffer") is None


def test_shape_table_reaches_every_staging_path():
    """The (L, C) table the device tests run reaches the vector copy, the uncached arm and the generic cached copy - the last for each of its three
    reasons: L % 4 != 0, L >= 1024, and M / Wcls off a 16-byte boundary."""
    paths = {s: tr.fused_path(*s) for s in tr.FUSED_SHAPES}
    assert set(paths.values()) == {"vector", "cached", "uncached"}
    assert paths[(512, 25)] == "vector" and paths[(512, 26)] == "uncached"          # the last cached C at the model's L, and the first uncached
    assert all(tr.fused_path(512, c) != "uncached" for c in range(1, 26)) and all(tr.fused_path(512, c) == "uncached" for c in range(26, 513))
    assert paths[(128, 99)] == "vector" and (99 * 129) % 4 == 3                     # three weights behind the last whole 16-byte vector
    for s in ((512, 2), (512, 18), (64, 64), (8, 3), (4, 1), (1020, 2)):
        assert paths[s] == "vector", s
    for s in ((512, 33), (512, 100), (512, 512), (8192, 1), (8186, 1)):
        assert paths[s] == "uncached", s
    assert paths[(510, 18)] == "cached" and 510 % 4 == 2                            # reason 1: L no multiple of 4
    assert paths[(513, 5)] == "cached" and 513 % 4 == 1
    assert paths[(1024, 2)] == "cached" and tr.fused_path(1020, 2) == "vector"      # reason 2: 2 (L + 1) floats of Mcat past the 2048 the copy covers
    for s in tr.MISALIGNED_SHAPES:                                                  # reason 3: an operand 4 bytes off
        assert s in tr.FUSED_SHAPES and tr.fused_path(*s, aligned=True) == "vector" and tr.fused_path(*s, aligned=False) == "cached"
    # the LDS the fused launch asks for: 41 KB at the model's shape, exactly 64 KiB at L = 8186, the most at the largest admitted L
    assert tr.fused_lds_bytes(512, 18) == 4352 + 20 * 513 * 4
    assert tr.fused_lds_bytes(8186, 1) == 65536 and tr.fused_lds_bytes(8192, 1) == 65584
    assert max(tr.fused_lds_bytes(L, 1) for L in range(1, 8193)) == 65584


def test_heads_entry_points_refuse_bad_shapes_without_a_gpu():
    from toad_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 21)
    err = lambda: lib.toad_last_error().decode()
    ESHAPE = -2
    fwd = lambda L, C: lib.toad_heads_fwd_f32(*([one] * 13), L, C, None)
    bwd = lambda L, C: lib.toad_heads_bwd_f32(*([one] * 12), 0.0, L, C, None)
    fused = lambda L, C: lib.toad_heads_ce_fused_f32(*([one] * 8), 0.75, 0.25, *([one] * 15), 0.0, L, C, None)
    ce = lambda C: lib.toad_mtl_ce_fwd_bwd_f32(*([one] * 4), 0.75, 0.25, *([one] * 3), C, None)
    for call, name in ((fwd, "toad_heads_fwd_f32"), (bwd, "toad_heads_bwd_f32"), (fused, "toad_heads_ce_fused_f32")):
        for L, C in ((512, 0), (0, 1), (8193, 1), (512, 1025), (512, -1)):
            assert call(L, C) == ESHAPE and name in err() and f"L={L}" in err(), (name, L, C)
    for call in (bwd, fused):                                   # dM is formed by L threads looping over C; the entries want C <= L
        assert call(4, 5) == ESHAPE and call(512, 513) == ESHAPE and call(17, 18) == ESHAPE
    assert ce(0) == ESHAPE and ce(1025) == ESHAPE and "C=1025" in err()
