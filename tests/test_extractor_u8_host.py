"""CPU: the extractor's uint8 front end (toad_tiles_u8_nhwc_to_nchw_f32, toad_stem_pool_nhwc_u8, toad_resnet50_trunc_u8_ws_bytes,
toad_resnet50_trunc_fwd_u8: an additive extension of ABI 15). The entry points exist in the header, the library and the ctypes table and check their
arguments before any device access; the workspace query adds the staging image only where it is needed; forward_u8 refuses what forward refuses;
and the normalisation formula x = fmaf(u, a_c, b_c) is the fp64 expression the GPU tests build their expected tensors with."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

U8_SYMBOLS = ("toad_tiles_u8_nhwc_to_nchw_f32", "toad_stem_pool_nhwc_u8", "toad_resnet50_trunc_u8_ws_bytes", "toad_resnet50_trunc_fwd_u8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NORM_SETS = (((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),            # ImageNet, the default
             ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
             ((0.0, 0.0, 0.0), (1.0 / 255.0,) * 3),                     # identity: x = u
             ((0.9, 0.01, 0.3333), (0.03, 1.7, 0.111)))                 # skewed


def _lib():
    from toad_amd import _lib as L
    return L.load()


def test_u8_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in U8_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert "resnet_custom.py:121-124" in header                # the entries say whose constants the default is


def _norm(vals=None):
    from toad_amd import ops
    return ops.norm_constants_u8() if vals is None else (ctypes.c_float * 6)(*vals)


def test_u8_entries_report_argument_errors_without_a_gpu():
    lib = _lib()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)
    off4 = ctypes.c_void_p((1 << 21) + 4)
    big = 1 << 40
    good = _norm()
    inf_a = _norm([math.inf, 0.01, 0.01, -1.0, -1.0, -1.0])   # std_R = 0
    nan_b = _norm([0.01, 0.01, 0.01, -1.0, math.nan, -1.0])
    w43 = (ctypes.c_void_p * 43)(*([1 << 21] * 43))

    conv = lambda t=one, n=good, o=one, b=2, h=7, w=9: lib.toad_tiles_u8_nhwc_to_nchw_f32(t, n, o, b, h, w, None)                   # noqa: E731
    stem = lambda t=one, n=good, y=one, b=2, h=8, w=256, ws=one, wsb=big: lib.toad_stem_pool_nhwc_u8(t, n, one, one, y, b, h, w, ws, wsb, None)   # noqa: E731
    net = lambda t=one, n=good, f=one, f16=None, b=2, h=8, w=256, wsb=big, wp=w43: lib.toad_resnet50_trunc_fwd_u8(            # noqa: E731
        t, n, wp, w43, f, f16, b, h, w, one, wsb, None)
    cases = [
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(t=None), -1, "null pointer"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(n=None), -1, "null pointer"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(o=None), -1, "null pointer"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(b=0), -2, "bad shape"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(h=0), -2, "bad shape"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(n=inf_a), -1, "norm[0] is not finite"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(n=nan_b), -1, "norm[4] is not finite"),
        ("toad_tiles_u8_nhwc_to_nchw_f32", lambda: conv(o=off4), -4, "16-byte aligned"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(t=None), -1, "null pointer"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(n=None), -1, "null pointer"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(b=0), -2, "W = 256"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(w=128), -2, "W = 256"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(h=6), -2, "H % 4 == 0"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(n=inf_a), -1, "norm[0] is not finite"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(n=nan_b), -1, "norm[4] is not finite"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(wsb=16), -3, "workspace too small"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(t=odd), -4, "2-byte aligned"),
        ("toad_stem_pool_nhwc_u8", lambda: stem(y=off4), -4, "16-byte aligned"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(t=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(n=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(f=None, f16=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(wp=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(b=0), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(h=0), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(n=inf_a), -1, "norm[0] is not finite"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(n=nan_b), -1, "norm[4] is not finite"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(wsb=16), -3, "workspace too small"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(h=7, w=9, wsb=lib.toad_resnet50_trunc_ws_bytes(2, 7, 9)), -3, "workspace too small"),   # no room for the staging image
        ("toad_resnet50_trunc_fwd_u8", lambda: net(t=odd), -4, "2-byte aligned"),
        ("toad_resnet50_trunc_fwd_u8", lambda: net(f=None, f16=off4), -4, "16-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)
    # the shapes make_plan refuses are refused by both network calls and both queries
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 256, 256)):
        assert lib.toad_resnet50_trunc_ws_bytes(*shape) == 0 and lib.toad_resnet50_trunc_u8_ws_bytes(*shape) == 0, shape


def test_u8_workspace_is_the_fp32_one_plus_the_staging_image_where_needed():
    lib = _lib()
    for shape in ((64, 256, 256), (1, 4, 256), (512, 256, 256), (3, 64, 256)):           # the stem reads the bytes: nothing is added
        assert lib.toad_resnet50_trunc_u8_ws_bytes(*shape) == lib.toad_resnet50_trunc_ws_bytes(*shape) > 0, shape
    for b, h, w in ((2, 7, 9), (3, 6, 256), (1, 40, 300), (1, 1, 1), (2, 256, 128)):     # staged
        extra = lib.toad_resnet50_trunc_u8_ws_bytes(b, h, w) - lib.toad_resnet50_trunc_ws_bytes(b, h, w)
        assert b * 3 * h * w * 4 <= extra <= b * 3 * h * w * 4 + (1 << 21), (b, h, w, extra)
    assert lib.toad_resnet50_trunc_u8_ws_bytes(2, 7, 9) - lib.toad_resnet50_trunc_ws_bytes(2, 7, 9) >= 2 * 3 * 7 * 9 * 4


def test_forward_u8_refusals_cpu():
    from toad_amd.resnet_custom import resnet50_baseline
    m = resnet50_baseline().eval()
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_u8(u8)
    with pytest.raises(RuntimeError, match=r"\[B,H,W,3\]"):
        m.forward_u8(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"\[B,H,W,3\]"):
        m.forward_u8(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="uint8"):
        m.forward_u8(torch.zeros(2, 8, 8, 3))
    with pytest.raises(RuntimeError, match="out_dtype"):
        m.forward_u8(u8, out_dtype=torch.bfloat16)
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.forward_u8(u8)
    m.eval()
    with pytest.raises(RuntimeError, match="HIP device"):     # forward itself is as it was
        m(torch.zeros(2, 3, 8, 8))


def test_norm_constants_are_rounded_once_from_double_and_refuse_bad_statistics():
    from toad_amd import ops
    for mean, std in NORM_SETS:
        got = np.array(list(ops.norm_constants_u8(mean, std)), dtype=np.float32)
        want = np.array([1.0 / (255.0 * s) for s in std] + [-m / s for m, s in zip(mean, std)], dtype=np.float64).astype(np.float32)
        assert np.array_equal(got, want), (mean, std)
    assert list(ops.norm_constants_u8((0, 0, 0), (1 / 255,) * 3)) == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    for mean, std in (((0.5,) * 3, (0.5, 0.0, 0.5)), ((0.5, math.nan, 0.5), (0.5,) * 3), ((0.5,) * 3, (math.inf, 1, 1)), ((0.5,) * 2, (0.5,) * 3),
                      ((0.5,) * 3, (1e-45,) * 3)):
        with pytest.raises(ValueError):
            ops.norm_constants_u8(mean, std)


def _fma_f32_exact(u, a, b):
    """Single-rounded fp32 fma(u, a, b) for an integer u in [0, 255] and fp32 a, b, by exact integer arithmetic (numpy has no fma): the exact value as a
    Python fraction of two integers, rounded to nearest even onto the fp32 grid."""
    from fractions import Fraction
    exact = Fraction(int(u)) * Fraction(float(a)) + Fraction(float(b))
    if exact == 0:
        return np.float32(0.0)
    sign = -1 if exact < 0 else 1
    mag = abs(exact)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()       # 2^(e-1) < mag < 2^(e+1)
    if Fraction(2) ** e > mag:
        e -= 1
    e = max(e, -126)                                                    # subnormal grid below 2^-126
    ulp = Fraction(2) ** (e - 23)
    q, r = divmod(mag, ulp)
    q = int(q)
    if r * 2 > ulp or (r * 2 == ulp and q % 2 == 1):
        q += 1
    return np.float32(sign * float(q * ulp))


def test_fp64_expression_is_the_single_rounded_fma():
    """What the GPU tests compare against: (u.double() * a.double() + b.double()).float(). The exact sum needs about 40 bits, so the fp64 product and sum
    are exact and the one rounding is the cast - the same value as fmaf((float)u, a, b)."""
    from toad_amd import ops
    u = torch.arange(256, dtype=torch.float64)
    bad = 0
    for mean, std in NORM_SETS[:3]:
        n = list(ops.norm_constants_u8(mean, std))
        for c in range(3):
            a, b = np.float32(n[c]), np.float32(n[3 + c])
            expr = (u * float(a) + float(b)).float().numpy()
            emu = np.array([_fma_f32_exact(i, a, b) for i in range(256)], dtype=np.float32)
            bad += int((expr.view(np.uint32) != emu.view(np.uint32)).sum())
    assert bad == 0
