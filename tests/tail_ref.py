"""TEST INFRASTRUCTURE ONLY - host statement of the per-slide step tail: the two classifier heads, the weighted two-task cross entropy, the heads
backward and the two flat optimisers. numpy, float64 throughout; it does not import the product package. Written from include/toad_hip.h
("Classifier heads", toad_adam_step_f32, toad_sgd_step_f32) and from the reference lines that header cites:

    models/model_toad.py:99-107            Mcat[t] = [M[t], sex];  logits = Mcat[0] Wcls^T + bcls;  site_logits = Mcat[1] Wsite^T + bsite;
                                           softmax, and topk(1) = the FIRST maximal index
    utils/core_utils_mtl_concat.py:213-215 loss = w_cls CE(logits, label) + w_site CE(site_logits, site)
    utils/utils.py:63-70                   torch.optim.Adam(lr, weight_decay) / torch.optim.SGD(lr, momentum=0.9, weight_decay)

Every function takes array-likes and returns float64 (int64 for the arg-max) arrays.
"""
import math

import numpy as np

F64 = np.float64
EPS32 = 2.0 ** -24          # unit round-off of fp32 (half an ulp of 1)


def _a(x):
    return np.asarray(x, dtype=F64)


def softmax(z):
    """softmax of a 1-D array and its log-sum-exp, shifted by the maximum (exact to fp64 round-off at any logit scale)."""
    z = _a(z).reshape(-1)
    mx = z.max()
    e = np.exp(z - mx)
    s = e.sum()
    return e / s, math.log(s) + mx


def heads_fwd(M, sex, Wcls, bcls, Wsite, bsite):
    """M [2, L], sex scalar, Wcls [C, L+1], bcls [C], Wsite [2, L+1], bsite [2] ->
    (Mcat [2, L+1], logits [C], Y_prob [C], Y_hat, site_logits [2], site_prob [2], site_hat); the arg-max is the first maximal index."""
    M, Wcls, bcls, Wsite, bsite = _a(M), _a(Wcls), _a(bcls).reshape(-1), _a(Wsite), _a(bsite).reshape(-1)
    sx = float(_a(sex).reshape(-1)[0])
    mcat = np.concatenate([M, np.full((2, 1), sx)], axis=1)
    logits = Wcls @ mcat[0] + bcls
    site_logits = Wsite @ mcat[1] + bsite
    return (mcat, logits, softmax(logits)[0], int(np.argmax(logits)), site_logits, softmax(site_logits)[0], int(np.argmax(site_logits)))


def ce(logits, label, site_logits, site, w_cls=0.75, w_site=0.25):
    """-> (loss [3] = (w_cls cls + w_site site, cls, site), dlogits [C], dsite [2]): CE = logsumexp - logit[label], d = w (softmax - onehot)."""
    out, grads = [], []
    for z, y, w in ((logits, label, w_cls), (site_logits, site, w_site)):
        z = _a(z).reshape(-1)
        p, lse = softmax(z)
        y = int(y)
        out.append(lse - z[y])
        g = p.copy()
        g[y] -= 1.0
        grads.append(w * g)
    return np.array([w_cls * out[0] + w_site * out[1], out[0], out[1]]), grads[0], grads[1]


def heads_bwd(Mcat, dlogits, dsite, Wcls, Wsite, dMcat_ext=None, prev=None, beta=0.0):
    """toad_heads_bwd_f32: dWcls = beta dWcls + dlogits^T Mcat[0] (dbcls, dWsite, dbsite likewise; ``prev`` = the four arrays beta scales),
    dM[t] = (d{logits, site} W{cls, site})[:L] + dMcat_ext[t, :L], dsex = the column L of both products + dMcat_ext[0, L] + dMcat_ext[1, L].
    -> (dWcls, dbcls, dWsite, dbsite, dM [2, L], dsex)."""
    Mcat, dl, ds, Wcls, Wsite = _a(Mcat), _a(dlogits).reshape(-1), _a(dsite).reshape(-1), _a(Wcls), _a(Wsite)
    L = Mcat.shape[1] - 1
    g = [np.outer(dl, Mcat[0]), dl.copy(), np.outer(ds, Mcat[1]), ds.copy()]
    if prev is not None and beta != 0.0:
        g = [beta * _a(o).reshape(n.shape) + n for o, n in zip(prev, g)]
    full = np.stack([dl @ Wcls, ds @ Wsite])                     # [2, L+1]
    if dMcat_ext is not None:
        full = full + _a(dMcat_ext)
    return g[0], g[1], g[2], g[3], full[:, :L].copy(), float(full[0, L] + full[1, L])


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """One torch.optim.Adam step (L2 weight decay folded into the gradient, no amsgrad); ``step`` counts from 1. -> (p, m, v)."""
    p, g, m, v = _a(p), _a(g), _a(m), _a(v)
    g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def sgd_step(p, g, buf, lr, momentum, weight_decay, step):
    """One torch.optim.SGD step (dampening 0, no nesterov): g' = g + wd p; buf = momentum buf + g' (buf = g' at step 1); p -= lr buf.
    momentum == 0: no buffer (``buf`` may be None and is returned as given), p -= lr g'. -> (p, buf)."""
    p, g = _a(p), _a(g)
    g = g + weight_decay * p
    if momentum == 0.0:
        return p - lr * g, buf
    buf = g if step == 1 else momentum * _a(buf) + g
    return p - lr * buf, buf


def fused_path(L, C, aligned=True):
    """Which staging path heads_ce_fused_kernel takes for [C, L+1] head weights: "vector" | "cached" | "uncached".
    WRITTEN FROM THE SOURCE and must follow it: the ``cache_w`` arithmetic of toad_heads_ce_fused_f32 / launch_heads_batch and the fast-path
    condition at the top of the kernel (toad_amd/csrc/heads.hip). ``aligned``: M and Wcls both on a 16-byte boundary."""
    lp = L + 1
    smem = ((2 * lp + 3 * C + 6 + 3) & ~3) * 4
    wbytes = (C + 2) * lp * 4
    if smem + wbytes > 60 * 1024:
        return "uncached"
    if aligned and L % 4 == 0 and 2 * L <= 4096 and C + 2 <= 1024 and C * lp <= 16 * 1024 and 2 * lp <= 2048:
        return "vector"
    return "cached"


def fused_lds_bytes(L, C):
    """Dynamic LDS the fused launch asks for (same arithmetic as fused_path)."""
    smem = ((2 * (L + 1) + 3 * C + 6 + 3) & ~3) * 4
    wbytes = (C + 2) * (L + 1) * 4
    return smem + (wbytes if smem + wbytes <= 60 * 1024 else 0)


# ---- rounding models of the kernels (the bounds the device tests hold them to) -------------------------------------------------------------
def ulp32(x):
    """Spacing of fp32 at |x| (array), never below the smallest normal's spacing."""
    return np.spacing(np.maximum(np.abs(_a(x)), 2.0 ** -126).astype(np.float32)).astype(F64)


def dot_bound(terms_abs_sum, result, depth):
    """|error| of an fp32 dot product whose longest chain of dependent roundings is ``depth`` fused multiply-adds, followed by at most 8 more
    additions (the 6-step wave butterfly and the bias, or the external addend) and one final rounding of the result:
        (depth + 8) 2^-24 sum |w_k x_k| + 2^-24 |result|.
    Row dot products (logits): 64 lanes stride the L + 1 columns, depth = ceil((L + 1) / 64). dM: one thread sums the C classes, depth = C."""
    return (depth + 8) * EPS32 * _a(terms_abs_sum) + EPS32 * np.abs(_a(result))


def row_depth(L):
    return math.ceil((L + 1) / 64)


# ---- the shape table of the device tests (tests/test_gpu_step_tail.py; tests/test_step_tail_host.py shows what it reaches) --------------------
FUSED_SHAPES = ((512, 2), (512, 18), (512, 25), (512, 26), (512, 33), (512, 100), (512, 512),
                (128, 99), (64, 64), (8, 3), (4, 1),
                (510, 18), (513, 5), (1020, 2), (1024, 2),
                (8192, 1), (8186, 1))               # the largest L the argument checks admit, and the L whose fused launch asks for exactly 64 KiB
MISALIGNED_SHAPES = ((512, 18), (128, 99))          # run again with M, then Wcls, 4 bytes into a larger allocation
