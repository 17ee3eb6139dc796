"""CPU: tiles read by origin from one decoded uint8 region (toad_tiles_u8_region_to_nchw_f32, toad_stem_pool_region_u8, toad_resnet50_trunc_fwd_u8_region:
an additive extension of ABI 15). The entry points exist in the header, the library and the ctypes table and refuse what the host can see before any device
access; the Python layer checks every origin on the host - an origin out of range would be an out-of-bounds read - and refuses origins it cannot check."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

REGION_SYMBOLS = ("toad_tiles_u8_region_to_nchw_f32", "toad_stem_pool_region_u8", "toad_resnet50_trunc_fwd_u8_region")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from toad_amd import _lib as L
    return L.load()


def test_region_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in REGION_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert "CALLER'S DUTY" in header and "Python layer" in header          # the header says whose job the bounds of the origins are


def test_region_entries_report_argument_errors_without_a_gpu():
    from toad_amd import ops
    lib = _lib()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # a region at an odd address is fine; it is refused for origins (int32)
    off4 = ctypes.c_void_p((1 << 21) + 4)
    big = 1 << 40
    good = ops.norm_constants_u8()
    inf_a = (ctypes.c_float * 6)(math.inf, 0.01, 0.01, -1.0, -1.0, -1.0)
    nan_b = (ctypes.c_float * 6)(0.01, 0.01, 0.01, -1.0, math.nan, -1.0)
    w43 = (ctypes.c_void_p * 43)(*([1 << 21] * 43))

    def conv(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, o=one, n=good, out=one, b=2, h=7, w=9):
        return lib.toad_tiles_u8_region_to_nchw_f32(r, pitch, hr, wr, o, n, out, b, h, w, None)

    def stem(r=odd, pitch=1593, hr=23, wr=531, o=one, n=good, y=one, b=2, h=8, w=256, ws=one, wsb=big):
        return lib.toad_stem_pool_region_u8(r, pitch, hr, wr, o, n, one, one, y, b, h, w, ws, wsb, None)

    def net(r=odd, pitch=1593, hr=23, wr=531, o=one, n=good, f=one, f16=None, b=2, h=8, w=256, wsb=big, wp=w43):
        return lib.toad_resnet50_trunc_fwd_u8_region(r, pitch, hr, wr, o, n, wp, w43, f, f16, b, h, w, one, wsb, None)

    cases = []
    for name, fn in (("toad_tiles_u8_region_to_nchw_f32", conv), ("toad_stem_pool_region_u8", stem), ("toad_resnet50_trunc_fwd_u8_region", net)):
        wr = 31 if fn is conv else 531
        cases += [
            (name, lambda fn=fn: fn(r=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(o=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(n=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(n=inf_a), -1, "norm[0] is not finite"),
            (name, lambda fn=fn: fn(n=nan_b), -1, "norm[4] is not finite"),
            (name, lambda fn=fn, wr=wr: fn(pitch=3 * wr - 1), -2, "pitch"),
            (name, lambda fn=fn: fn(pitch=0), -2, "pitch"),
            (name, lambda fn=fn: fn(pitch=-1593), -2, "pitch"),
            (name, lambda fn=fn: fn(hr=4), -2, "does not fit"),           # H > Hr
            (name, lambda fn=fn: fn(wr=8 if fn is conv else 255, pitch=2000), -2, "does not fit"),                         # W > Wr
            (name, lambda fn=fn: fn(hr=0), -2, None),
            (name, lambda fn=fn: fn(pitch=(1 << 31) // (7 if fn is conv else 8) + 1, hr=1 << 20), -2, "pitch too large"),   # H * pitch reaches 2^31
            (name, lambda fn=fn: fn(o=odd), -4, "4-byte aligned"),
        ]
    cases += [
        ("toad_tiles_u8_region_to_nchw_f32", lambda: conv(out=None), -1, "null pointer"),
        ("toad_tiles_u8_region_to_nchw_f32", lambda: conv(b=0), -2, "bad shape"),
        ("toad_tiles_u8_region_to_nchw_f32", lambda: conv(out=off4), -4, "16-byte aligned"),
        ("toad_stem_pool_region_u8", lambda: stem(b=0), -2, "W = 256"),
        ("toad_stem_pool_region_u8", lambda: stem(w=128), -2, "W = 256"),
        ("toad_stem_pool_region_u8", lambda: stem(h=6), -2, "H % 4 == 0"),
        ("toad_stem_pool_region_u8", lambda: stem(wsb=16), -3, "workspace too small"),
        ("toad_stem_pool_region_u8", lambda: stem(y=off4), -4, "16-byte aligned"),
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(f=None, f16=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(wp=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(b=0), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(wsb=16), -3, "workspace too small"),
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(h=7, w=9, wsb=lib.toad_resnet50_trunc_ws_bytes(2, 7, 9)), -3, "workspace too small"),   # the staging image
        ("toad_resnet50_trunc_fwd_u8_region", lambda: net(f=None, f16=off4), -4, "16-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and (text is None or text in msg) and msg.startswith(name + ":"), (name, text, got, msg)
    # the largest pitch that is taken is the one just below the bound (H * pitch = 2^31 - 8 for H = 8): only the later workspace check stops this call
    assert stem(pitch=(1 << 31) // 8 - 1, hr=1 << 20, wsb=16) == -3 and "workspace too small" in err()


def test_origins_are_checked_on_the_host():
    from toad_amd import ops
    hr, wr, h, w = 23, 531, 8, 256
    ok = [(0, 0), (275, 15), (2, 3), (2, 3)]
    for form in (ok, np.array(ok), np.array(ok, dtype=np.int16), torch.tensor(ok), torch.tensor(ok, dtype=torch.int32)):
        o = ops.check_origins(form, hr, wr, h, w)
        assert o.dtype == torch.int32 and o.device.type == "cpu" and o.is_contiguous() and o.tolist() == [list(t) for t in ok]
    with pytest.raises(ValueError, match=r"origins\[2\]"):                    # x + W == Wr + 1; the first offender is named, not the later one
        ops.check_origins([(0, 0), (275, 15), (276, 0), (400, 0)], hr, wr, h, w)
    with pytest.raises(ValueError, match=r"origins\[1\]"):                    # a negative y
        ops.check_origins([(0, 0), (5, -1)], hr, wr, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\]"):                    # y + H == Hr + 1
        ops.check_origins([(0, 16)], hr, wr, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\]"):                    # a negative x
        ops.check_origins(np.array([(-1, 0)]), hr, wr, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\]"):                    # no wrap-around through int32
        ops.check_origins(torch.tensor([(2 ** 32, 0)]), hr, wr, h, w)
    with pytest.raises(TypeError, match="integers"):
        ops.check_origins(np.array(ok, dtype=np.float32), hr, wr, h, w)
    with pytest.raises(TypeError, match="integers"):
        ops.check_origins([(0.0, 0.0)], hr, wr, h, w)
    with pytest.raises(ValueError, match=r"\[B,2\]"):
        ops.check_origins([0, 0], hr, wr, h, w)
    with pytest.raises(ValueError, match=r"\[B,2\]"):
        ops.check_origins(torch.zeros(2, 3, dtype=torch.int64), hr, wr, h, w)
    with pytest.raises(ValueError, match="on the host"):                     # a device tensor cannot be checked without a synchronisation
        ops.check_origins(torch.zeros(2, 2, dtype=torch.int32, device="meta"), hr, wr, h, w)
    assert ops.tile_shape(256) == (256, 256) and ops.tile_shape((8, 256)) == (8, 256)
    for bad in (0, (8, 0), (8.0, 256), (1, 2, 3)):
        with pytest.raises(ValueError):
            ops.tile_shape(bad)


def test_region_layout_rule():
    from toad_amd import ops
    wide = torch.zeros(25, 540, 3, dtype=torch.uint8)
    assert ops.region_layout_ok(wide) and ops.region_layout_ok(wide[1:24, 3:534]) and ops.region_layout_ok(wide[::2])       # any pitch >= 3 Wr
    assert not ops.region_layout_ok(wide[:, ::2])                          # stride(1) == 6
    assert not ops.region_layout_ok(wide.permute(1, 0, 2))                 # stride(1) == 1620
    assert not ops.region_layout_ok(torch.zeros(3, 25, 540, dtype=torch.uint8).permute(1, 2, 0))      # planar: stride(2) != 1
    assert not ops.region_layout_ok(torch.zeros(25, 540, 4, dtype=torch.uint8)) and not ops.region_layout_ok(torch.zeros(2, 25, 540, 3, dtype=torch.uint8))
    assert not ops.region_layout_ok(torch.zeros(1, 540, 3, dtype=torch.uint8).expand(25, 540, 3))                         # pitch 0


def test_forward_u8_region_refusals_cpu(monkeypatch):
    """Each refusal comes with the expected exception and before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.resnet_custom import resnet50_baseline
    m = resnet50_baseline().eval()

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    region = torch.zeros(23, 531, 3, dtype=torch.uint8)
    org = [(0, 0), (275, 15)]
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_u8_region(region, org, tile=(8, 256))
    with pytest.raises(RuntimeError, match=r"\[Hr,Wr,3\]"):
        m.forward_u8_region(torch.zeros(3, 23, 531, dtype=torch.uint8), org, tile=(8, 256))
    with pytest.raises(RuntimeError, match=r"\[Hr,Wr,3\]"):
        m.forward_u8_region(torch.zeros(2, 23, 531, 3, dtype=torch.uint8), org, tile=(8, 256))
    with pytest.raises(RuntimeError, match="uint8"):
        m.forward_u8_region(region.float(), org, tile=(8, 256))
    with pytest.raises(RuntimeError, match="out_dtype"):
        m.forward_u8_region(region, org, tile=(8, 256), out_dtype=torch.bfloat16)
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.forward_u8_region(region, org, tile=(8, 256))
    m.eval()
    # what comes after the device test, on a stand-in that claims to be on the device: layout, then the origins
    meta = torch.zeros(23, 1062, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(RuntimeError, match=r"stride\(1\) == 3"):
        m.forward_u8_region(meta[:, ::2], org, tile=(8, 256))
    with pytest.raises(ValueError, match=r"stride\(1\) == 3"):
        ops.tiles_u8_region_to_f32(meta[:, ::2], org, tile=(8, 256))
    with pytest.raises(ValueError, match=r"stride\(1\) == 3"):
        ops.stem_pool_region_u8(meta[:, ::2], org, None, None, tile=(8, 256))
    m = m.to("meta")
    reg = meta[:, :531]
    assert ops.region_layout_ok(reg)
    for call in (lambda o: m.forward_u8_region(reg, o, tile=(8, 256)), lambda o: ops.tiles_u8_region_to_f32(reg, o, tile=(8, 256)),
                 lambda o: ops.stem_pool_region_u8(reg, o, None, None, tile=(8, 256))):
        with pytest.raises(ValueError, match=r"origins\[1\]"):
            call([(0, 0), (276, 0)])                                          # x + W == Wr + 1
        with pytest.raises(ValueError, match=r"origins\[0\]"):
            call([(0, -1)])
        with pytest.raises(ValueError, match="on the host"):
            call(torch.zeros(2, 2, dtype=torch.int32, device="meta"))
        with pytest.raises(TypeError, match="integers"):
            call(np.zeros((2, 2), dtype=np.float64))
