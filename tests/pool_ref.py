"""TEST INFRASTRUCTURE ONLY - float64 statement of what the fused gated-attention pool backward (toad_amd/csrc/gated_pool.hip) adds to the
oracle's backward: the analytic per-row bound of |dP| behind its abs-max array, and that bound's fold to one value per 256 rows. The backward
values themselves are oracle.toad_oracle.gated_pool_bwd called on float64 inputs. It does not import the product package.

    dS[i,t]  = softmax_i(A_raw)[i,t] * (dM[t].H[i] - dM[t].M[t]) + dA_ext[i,t]
    bound[i] = sum_t |dS[i,t]| * max_e |Wc[t,e]|          (times (1/(1-p))^2 when the two gate branches drop with probability p)
    amax[rb] = max over rows 256 rb ... 256 rb + 255 of bound

|dPa|, |dPb| <= |dg| ka kb with dg = dS Wc, because |tanh|, sigmoid, 1 - tanh^2 <= 1 and the dropout multipliers are <= 1/(1-p): the bound holds for
every input. How far above the measured maximum it lies depends on the data (how much of max|Wc| the gates let through, how far the tasks
cancel in dg); the input families below are the ones on which tests/test_pool_ref_host.py shows the float64 ratio to stay within CAP.
"""
import numpy as np
import torch

from oracle import toad_oracle as orc
from tests import drop_ref

ROWBLK = 256                    # rows per abs-max slot (csrc/h2_arith.h H2_ROWBLK)
CAP = 8.0                       # bound / measured maximum on the ordinary families: three operand bits of the fp16 two-piece GEMMs
DROP_P = 0.25                   # nn.Dropout(0.25) after tanh and after sigmoid (models/model_toad.py:27-29)

EXACT_SHAPES = [(384, 512, 2), (256, 512, 2)]                                            # (D, L, T) with an instantiation of their own
COVER_SHAPES = [(100, 200, 1), (260, 520, 2), (384, 512, 3), (512, 1024, 4), (4, 8, 1)]  # served by the covering instantiation
AMAX_NS = [1, 7, 8, 9, 255, 256, 257, 511, 513, 4097, 12289]
# the ordinary families: pool_inputs at every shape above except (4, 8, 1), every n above (and n = 513 with P scaled by 4), with and without
# da_ext = 0.1 randn, with and without dropout: float64 ratios 1.1 ... 6.3 (tests/test_pool_ref_host.py). At D = 4 a block's maximum is taken
# over as few as four gate products (a one-row block: n = 1, or the last block of n = 257, 513, ...), each of which may let through a small
# part of max|Wc| only, and dropout can leave a single survivor: the ratio is a property of four random numbers there (17 at n = 513 in
# float64), not of the kernel. That shape keeps the lower bound (which holds for every input) and leaves the cap to the others.
ORDINARY_SHAPES = EXACT_SHAPES + COVER_SHAPES[:-1]


def pool_inputs(n, d, l, t, seed, scale=1.0):
    """(P [n,2D], H [n,L], Wc [T,D], bc [T]) fp32 - the family tests/test_gpu_kernels.py::_pool_inputs draws."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, 2 * d, generator=g) * scale
    h = torch.randn(n, l, generator=g).relu()
    wc = torch.randn(t, d, generator=g) * 0.1
    bc = torch.randn(t, generator=g) * 0.1
    return p, h, wc, bc


def grad_inputs(n, l, t, seed):
    """(dM [T,L], dA_ext [n,T]) fp32 of the same family (test_gated_pool_bwd)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t, l, generator=g), torch.randn(n, t, generator=g) * 0.1


def seeds(n, d):
    """The two branch seeds a test uses at (n, D): 64-bit, distinct, with both halves set."""
    sa = (0x9E3779B97F4A7C15 * (2 * n + 1) + d) & drop_ref.M64
    return sa, (sa ^ 0xD1B54A32D192ED03) & drop_ref.M64


def drop_masks(n, d, p, seed_a, seed_b):
    """Multipliers (0 or 1/(1-p), fp32 values) of the tanh and the sigmoid branch, [n, D] each, element (row, column) at row * D + column."""
    return tuple(torch.from_numpy(drop_ref.keep(n * d, p, s).reshape(n, d).copy()) for s in (seed_a, seed_b))


def forward_plain(pa, pb, h, wc, bc, ma=None, mb=None):
    """models/model_toad.py:36-41,92,97-98 written out: (A_raw [n,T], M [T,L])."""
    a, b = torch.tanh(pa), torch.sigmoid(pb)
    if ma is not None:
        a, b = a * ma, b * mb
    a_raw = (a * b) @ wc.t() + bc
    return a_raw, torch.softmax(a_raw.t(), 1) @ h


def d_scores(h, a_raw, m, dm, da_ext=None):
    """dS [n,T]: the gradient of the raw scores (oracle.toad_oracle.gated_pool_bwd's ds)."""
    p = torch.softmax(a_raw.t(), 1).t()
    ds = p * (h @ dm.t() - (dm * m).sum(1)[None, :])
    return ds if da_ext is None else ds + da_ext


def row_bound(ds, wc, drop_p=0.0):
    """bound [n] of max(|dPa[i,:]|, |dPb[i,:]|)."""
    b = ds.abs().double() @ wc.abs().double().max(1).values
    if drop_p > 0:
        keep = 1.0 / (1.0 - float(np.float32(drop_p)))
        b = b * keep * keep
    return b


def fold256(v):
    """max over each block of 256 rows of v [n] or of |v| [n, k] -> [ceil(n / 256)]."""
    v = v.abs().double()
    if v.dim() == 2:
        v = v.max(1).values
    n = v.shape[0]
    nb = (n + ROWBLK - 1) // ROWBLK
    pad = torch.zeros(nb * ROWBLK, dtype=torch.float64)
    pad[:n] = v
    return pad.view(nb, ROWBLK).max(1).values


def reference(p, h, wc, bc, dm, da_ext=None, ma=None, mb=None, dtype=torch.float64):
    """Forward and backward of the pool in ``dtype``: dict(a_raw, m, dpa, dpb, dh, dwc, dbc, ds)."""
    d = wc.shape[1]
    c = lambda x: None if x is None else x.to(dtype)
    pa, pb = c(p[:, :d]), c(p[:, d:])
    a_raw, m = orc.gated_pool_fwd(pa, pb, c(h), c(wc), c(bc), c(ma), c(mb))
    dpa, dpb, dh, dwc, dbc = orc.gated_pool_bwd(pa, pb, c(h), c(wc), a_raw, m, c(dm), c(da_ext), c(ma), c(mb))
    return dict(a_raw=a_raw, m=m, dpa=dpa, dpb=dpb, dp=torch.cat([dpa, dpb], 1), dh=dh, dwc=dwc, dbc=dbc, ds=d_scores(c(h), a_raw, m, c(dm), c(da_ext)))


def bound_ratios(ref, wc, drop_p=0.0):
    """(bound per block, measured max |dP| per block) of a reference() result."""
    return fold256(row_bound(ref["ds"], wc, drop_p)), fold256(ref["dp"])
