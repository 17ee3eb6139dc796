"""Host reference for the extractor's numerical contract (csrc/conv.hip, gemm_narrow.inc, gemm_stream.inc, stem_halo.inc): operand families that span
the fp32 range, the error bound of the fp16 two-piece arithmetic with the extractor's scale groups, and that arithmetic restated on the host.

The extractor's GEMMs compute act(X' W^T + bias + residual) with X' scaled by ONE power of two per tensor (per tile of two conv rows in
stem_halo_pool_kernel) and every weight row by its own. With x s = h + m (two fp16 pieces) an element keeps 22 bits relative to itself while m is a
normal fp16 number, i.e. down to 2^-17 of the abs-max its scale came from; below that the representation error is absolute, <= 2^-39 of that abs-max.
Hence, as tests/test_gpu_h2.py::_nt_bound states for the MIL GEMMs,

    |y - ref| <= c 2^-24 (|x| @ |w|^T)  +  2^-38 (amax_a sum_k |w|  +  sum_k |x| rowmax |w|)  +  3 2^-24 (|x w^T| + |bias| + |res|)

The last term is the epilogue: (acc f1) iv + bias + residual is three fp32 roundings of values no larger than the sum of the magnitudes. The middle term
is the absolute regime. c has two parts, c = c_rep + c_acc:
  c_rep = 6 (with exact accumulation: max(6, 0.75 sqrt(K)), the constant of _nt_bound) - the representation of both operands (2^-22 each) and the dropped
      m.m term (2^-22), which do not all reach their worst case at once;
  c_acc = 6 sqrt(K) - the fp32 ACCUMULATION. The 3 K products (h.h, h.m, m.h) reach the accumulator through 3 K additions, in whatever grouping the
      matrix core uses; each addition rounds once, by at most half a unit in the last place of a value no larger than sum_k |x w|, i.e. uniformly within
      +-2^-24 sum|x w|: standard deviation <= 2^-24 sum|x w| / sqrt(3) each, sqrt(3 K) / sqrt(3) = sqrt(K) of them in a walk, held at six standard
      deviations (2e-9 per element; the tests look at some 1e7 elements).
  _nt_bound's 0.75 sqrt(K) is three standard deviations of a walk of one rounding per 16-deep MFMA, with sum|x w| standing in for the running sum. That holds
  where the running sum stays far below sum|x w| (terms of random sign and similar size), and it cannot hold for a sum that ONE product dominates (the
  `heavy` family, a ReLU layer's rare huge activation): there the running sum IS sum|x w| from that product on, and among 1e4 .. 1e5 such elements
  some walk four standard deviations. `emulate(..., acc32=True)` shows it on the host, with no kernel involved: at (300, 64, 128) the fp32 chain sits at
  1.48 of the bound with c = max(6, 0.75 sqrt(K)) (tests/test_extractor_range_host.py), and the kernels at up to 1.17 (profiles/extractor_range_bound.md).
`emulate` restates the arithmetic on the host - with exact accumulation (the representation alone) or with an fp32 chain of one rounding per product - and
tests/test_extractor_range_host.py holds both to the bound; tests/test_gpu_extractor_range.py holds the kernels to it.
Used by tests only; plain torch on the CPU, float64 throughout."""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
FAMILIES = ("unit", "tiny", "huge", "heavy", "relu_sparse", "giant_last")
MAGNITUDE = {"unit": 1.0, "tiny": 1e-30, "huge": 1e30, "heavy": 1.0, "relu_sparse": 1.0, "giant_last": 1.0}    # what bias / residual are scaled by


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def make_a(family, shape, seed=0):
    """The A operand (any shape: [M, K], NHWC or NCHW) of one family, fp32."""
    g = torch.Generator().manual_seed(_seed(family, tuple(shape), seed))
    x = torch.randn(*shape, generator=g)
    if family == "unit":
        return x
    if family == "tiny":
        return x * 1e-30
    if family == "huge":
        return x * 1e30
    if family == "heavy":                      # log-normal magnitudes per element: about eight decades inside one scale group
        return x.sign() * torch.exp(4.0 * torch.randn(*shape, generator=g)).clamp(max=1e12)
    if family == "relu_sparse":                # what a ReLU layer hands on: mostly zeros, one rare huge activation
        x = (x - 1.5).relu()
        x.view(-1)[x.numel() // 3] = 3e4
        return x
    if family == "giant_last":                 # the maximum is negative and sits where only the end of a grid-stride loop reads it
        x.view(-1)[-1] = -2.0 ** 20
        return x
    raise ValueError(family)


def zero_row(n):
    return (2 * n) // 3 + 1 if n > 2 else n - 1           # never a multiple of 7 for the widths used here; checked by the host test


def make_w(n, k, seed=0):
    """Weights [n, k]: randn / sqrt(k), rows [::7] times 1e-5 (a weight row carries its own scale), row zero_row(n) exactly zero."""
    g = torch.Generator().manual_seed(_seed("w", n, k, seed))
    w = torch.randn(n, k, generator=g) / k ** 0.5
    w[::7] *= 1e-5
    w[zero_row(n)] = 0.0
    return w


def make_bias_res(family, m, n, bias, res, seed=0):
    """randn times the magnitude of the product (1e-30 / 1e30 along with A), or None."""
    g = torch.Generator().manual_seed(_seed("br", family, m, n, seed))
    mag = MAGNITUDE[family]
    b = torch.randn(n, generator=g) * mag if bias else None
    r = torch.randn(m, n, generator=g) * mag if res else None
    return b, r


def c_exact(k):
    """c for the arithmetic with EXACT accumulation (the representation alone): the constant of tests/test_gpu_h2.py::_nt_bound."""
    return max(6.0, 0.75 * k ** 0.5)


def c_fp32(k):
    """c with fp32 accumulation: c_rep + c_acc (module docstring)."""
    return 6.0 + 6.0 * k ** 0.5


def nt_bound(x, w, amax_a, bias=None, res=None, c=None):
    """Elementwise bound [M, N] on |y - (x w^T + bias + res)| (module docstring). x [M, K], w [N, K]; amax_a: the abs-max of A's scale group, a scalar
    or one value per row of x; bias [N] / res [M, N] or None; c: c_fp32(K) unless given."""
    x, w = x.double(), w.double()
    c = c_fp32(x.shape[1]) if c is None else c
    ax, aw = x.abs(), w.abs()
    amax_a = torch.as_tensor(amax_a, dtype=torch.float64).reshape(-1, 1)
    out = c * EPS * (ax @ aw.t())
    out += 2.0 ** -38 * (amax_a * aw.sum(1).view(1, -1) + ax.sum(1).view(-1, 1) * aw.max(1).values.view(1, -1))
    mag = (x @ w.t()).abs()
    if bias is not None:
        mag = mag + bias.double().abs().view(1, -1)
    if res is not None:
        mag = mag + res.double().abs()
    return out + 3.0 * EPS * mag


def exp_from_amax(amax):
    """k with amax 2^k in [2^13, 2^14), clamped to +-120 (h2_exp_from_amax; 0 -> 14). amax: float64 tensor of any shape."""
    _, e = torch.frexp(torch.as_tensor(amax, dtype=torch.float64))
    return (14 - e).clamp(-120, 120).to(torch.float64)


def split2(x, k):
    """The two fp16 pieces of x 2^k as float64: h = rn16(x s), m = rn16(x s - h). x s is a float (a power-of-two multiple), so it is rounded once."""
    xs = x.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), k)
    h = xs.float().half().double()
    m = (xs - h).float().half().double()
    return h, m


def emulate(x, w, amax_a, acc32=False):
    """x w^T in the two-piece arithmetic: A scaled by its group's power of two, every weight row by its own, the products h.h + h.m + m.h, descaled.
    acc32 = False: summed exactly (float64). acc32 = True: summed into an fp32 accumulator, one rounding per product, in the kernels' order (per 16-deep
    step m.h, h.m, h.h: gemm_stream.inc `mma`) - the finest grouping an accumulation can have; the matrix core's own grouping is coarser."""
    ka = exp_from_amax(torch.as_tensor(amax_a, dtype=torch.float64).reshape(-1, 1))
    kw = exp_from_amax(w.double().abs().max(1).values).view(-1, 1)
    ha, ma = split2(x, ka)
    hw, mw = split2(w, kw)
    if acc32:
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64)
        for k0 in range(0, x.shape[1], 16):
            for a, b in ((ma, hw), (ha, mw), (ha, hw)):
                for k in range(k0, min(k0 + 16, x.shape[1])):
                    acc = (acc + a[:, k:k + 1] * b[:, k].view(1, -1)).float().double()      # fp16 x fp16 is exact; the sum is rounded to fp32
    else:
        acc = ha @ hw.t() + ha @ mw.t() + ma @ hw.t()
    two = torch.tensor(2.0, dtype=torch.float64)
    return acc * torch.pow(two, -ka) * torch.pow(two, -kw.view(1, -1))


# ---- convolutions as the same product --------------------------------------------------------------------------------------------------------------
def unfold_nhwc(x, k, s, p):
    """float64 rows of the implicit GEMM: x [B, H, W, C] -> [B Ho Wo, k k C] in (ky, kx, c) order, zeros outside."""
    b, h, w, c = x.shape
    u = F.unfold(x.double().permute(0, 3, 1, 2), k, padding=p, stride=s)               # [B, C k k, L], rows (c, ky, kx)
    return u.view(b, c, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * c)


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def stem_weights(seed=0):
    """7x7 weights [64, 147] in the reference's (c, ky, kx) order with the weight rules of make_w, and their embedding in [64, 192] (the space-to-depth
    (qy, qx, ry, rx, c) order of the stem kernels, slot 2q + r holding tap 2q + r - 1)."""
    wt = make_w(64, 147, seed)
    return wt, embed_stem(wt)


def embed_stem(wt):
    w8 = torch.zeros(64, 3, 8, 8)
    w8[:, :, 1:, 1:] = wt.view(64, 3, 7, 7)
    return w8.view(64, 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(64, 192).contiguous()


def unfold_stem(x):
    """float64 rows of the 7x7 / 2 / pad 3 stem: x [B, 3, H, W] -> [B Ho Wo, 147] in (c, ky, kx) order."""
    return F.unfold(x.double(), 7, padding=3, stride=2).permute(0, 2, 1).reshape(-1, 147)


def stem_tile_amax(x):
    """Abs-max of the window stem_halo_pool_kernel scales a tile by, one value per CONV ROW: [B, Ho]. Tile t of an image is conv rows 2t, 2t + 1; its
    window is the five space-to-depth rows 2t .. 2t + 4 = image rows 4t - 4 .. 4t + 5 (stem_halo.inc: raw[k] holds image row 4t - 4 + 2 Yl + ry), every
    column and channel. Row 4t - 4 only meets zero weights but is measured with the rest, so this is the set the kernel takes, not a looser one."""
    b, _, h, _ = x.shape
    rowmax = x.double().abs().amax(dim=(1, 3))                                          # [B, H]
    out = torch.zeros(b, h // 2, dtype=torch.float64)
    for oy in range(h // 2):
        t = oy // 2
        out[:, oy] = rowmax[:, max(4 * t - 4, 0):min(4 * t + 6, h)].amax(1)
    return out


def pool_max(t_nhwc):
    """3x3 / 2 / pad 1 max-pool of an NHWC float64 tensor: outputs, and bounds (an output's bound is the largest bound of the values it is taken over)."""
    return F.max_pool2d(t_nhwc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def ratio(err, bound):
    """Largest err / bound; 0 / 0 (exact zeros under a zero bound) counts as 0, a nonzero error under a zero bound as inf."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max())


@functools.lru_cache(maxsize=None)
def host_ratio(family, acc32=True, m=512, k=576, n=64):
    """err / bound of `emulate` at the host test's shape - the figure profiles/extractor_range_bound.md prints next to the device's. acc32 = False: exact
    accumulation against the bound with c_exact."""
    x, w = make_a(family, (m, k)), make_w(n, k)
    amax = x.abs().max().double()
    ref = x.double() @ w.double().t()
    return ratio((emulate(x, w, amax, acc32) - ref).abs(), nt_bound(x, w, amax, c=None if acc32 else c_exact(k)))
