"""CPU: the extractor's region calls with a 2 x 2 box filter in front of the tile (toad_tiles_u8_region_box_to_nchw_f32, toad_stem_pool_region_box_u8,
toad_resnet50_trunc_fwd_u8_region_box: an additive extension of ABI 15). A tile is a (shrink H, shrink W) footprint of the region and

    t[iy, ix, c] = (sum of region[y + s iy + dy, x + s ix + dx, c] over dy, dx in 0 .. s-1, + s*s/2) // (s*s)

The entry points exist in the header, the library and the ctypes table and refuse what the host can see before any device access, in a fixed order;
ops.box_tiles_u8, the materialised reference of every bitwise GPU test, is itself checked against the formula; the Python layer refuses a bad shrink
before it looks at anything else."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

BOX_SYMBOLS = ("toad_tiles_u8_region_box_to_nchw_f32", "toad_stem_pool_region_box_u8", "toad_resnet50_trunc_fwd_u8_region_box")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 2 x 2 boxes (a b / c d) whose sums are 0, 1, 2, 3 (all four residues mod 4 at the bottom of the range), 509, 510 (residues 1, 2 in the middle),
# 1018 (residue 2 near the top) and 1020 (the top): (sum + 2) // 4 must be 0, 0, 1, 1, 127, 128, 255, 255
BOXES = [((0, 0, 0, 0), 0), ((1, 0, 0, 0), 0), ((0, 1, 1, 0), 1), ((1, 1, 0, 1), 1), ((255, 254, 0, 0), 127), ((255, 0, 255, 0), 128),
         ((255, 255, 254, 254), 255), ((255, 255, 255, 255), 255)]


def box_region():
    """uint8 [2, 2 * len(BOXES), 3]: box i at columns 2 i, 2 i + 1; channel c holds box (i + c) % len(BOXES), so the channels differ."""
    n = len(BOXES)
    r = torch.zeros(2, 2 * n, 3, dtype=torch.uint8)
    for i in range(n):
        for c in range(3):
            a, b, cc, d = BOXES[(i + c) % n][0]
            r[0, 2 * i, c], r[0, 2 * i + 1, c], r[1, 2 * i, c], r[1, 2 * i + 1, c] = a, b, cc, d
    return r


def box_formula(region, origins, fh, fw, s):
    """The definition, restated with numpy loops over dy, dx (no reshape: another way to the same numbers than ops.box_tiles_u8)."""
    r = region.numpy().astype(np.int64)
    out = np.zeros((len(origins), fh // s, fw // s, 3), dtype=np.int64)
    for b, (x, y) in enumerate(origins):
        acc = np.zeros((fh // s, fw // s, 3), dtype=np.int64)
        for dy in range(s):
            for dx in range(s):
                acc += r[y + dy:y + fh:s, x + dx:x + fw:s]
        out[b] = (acc + s * s // 2) // (s * s)
    assert out.min() >= 0 and out.max() <= 255
    return torch.from_numpy(out.astype(np.uint8))


def test_box_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in BOX_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
        twin = name.replace("_box", "")
        ret, args = L.SIGNATURES[name]
        tret, targs = L.SIGNATURES[twin]
        assert ret == tret and len(args) == len(targs) + 1          # the twin's arguments plus `int shrink`


def test_box_entries_report_argument_errors_without_a_gpu():
    """Every refusal of each new entry through fake pointers: nothing below reaches a device. The ORDER is checked too - each call breaks one thing more
    than the previous one of its chain and must report the earlier check."""
    from toad_amd import ops
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)
    odd = ctypes.c_void_p((1 << 21) + 1)
    off4 = ctypes.c_void_p((1 << 21) + 4)
    big = 1 << 40
    good = ops.norm_constants_u8()
    inf_a = (ctypes.c_float * 6)(math.inf, 0.01, 0.01, -1.0, -1.0, -1.0)
    nan_b = (ctypes.c_float * 6)(0.01, 0.01, 0.01, -1.0, math.nan, -1.0)
    w43 = (ctypes.c_void_p * 43)(*([1 << 21] * 43))

    # network tiles (7, 9) / (8, 256): footprints (14, 18) in a 20 x 31 region, (16, 512) in a 23 x 531 region
    def conv(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, o=one, n=good, out=one, b=2, h=7, w=9, s=2):
        return lib.toad_tiles_u8_region_box_to_nchw_f32(r, pitch, hr, wr, o, n, out, b, h, w, s, None)

    def stem(r=odd, pitch=1593, hr=23, wr=531, o=one, n=good, y=one, b=2, h=8, w=256, s=2, ws=one, wsb=big):
        return lib.toad_stem_pool_region_box_u8(r, pitch, hr, wr, o, n, one, one, y, b, h, w, s, ws, wsb, None)

    def net(r=odd, pitch=1593, hr=23, wr=531, o=one, n=good, f=one, f16=None, b=2, h=8, w=256, s=2, wsb=big, wp=w43):
        return lib.toad_resnet50_trunc_fwd_u8_region_box(r, pitch, hr, wr, o, n, wp, w43, f, f16, b, h, w, s, one, wsb, None)

    cases = []
    for name, fn in (("toad_tiles_u8_region_box_to_nchw_f32", conv), ("toad_stem_pool_region_box_u8", stem), ("toad_resnet50_trunc_fwd_u8_region_box", net)):
        hr, wr, fh, fw = (20, 31, 14, 18) if fn is conv else (23, 531, 16, 512)
        cases += [
            (name, lambda fn=fn: fn(r=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(o=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(n=None), -1, "null pointer"),
            (name, lambda fn=fn: fn(n=None, s=3), -1, "null pointer"),                      # a null pointer is reported before a bad shrink
            (name, lambda fn=fn: fn(n=inf_a), -1, "norm[0] is not finite"),
            (name, lambda fn=fn: fn(n=nan_b), -1, "norm[4] is not finite"),
            (name, lambda fn=fn: fn(s=0), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn: fn(s=3), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn: fn(s=4), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn: fn(s=-2), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn: fn(s=3, pitch=0), -2, "shrink must be 1 or 2"),            # ... and a bad shrink before the region's shape
            (name, lambda fn=fn: fn(s=3, hr=0), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn, wr=wr: fn(pitch=3 * wr - 1), -2, "pitch"),
            (name, lambda fn=fn: fn(pitch=0), -2, "pitch"),
            (name, lambda fn=fn: fn(pitch=0, hr=4), -2, "pitch"),                           # the pitch before the fit
            (name, lambda fn=fn, fh=fh: fn(hr=fh - 1), -2, "footprint"),                    # the footprint one pixel over the bottom edge
            (name, lambda fn=fn, fw=fw: fn(wr=fw - 1, pitch=2000), -2, "footprint"),        # ... and over the right edge
            (name, lambda fn=fn, fh=fh: fn(hr=fh - 1, n=inf_a), -2, "footprint"),           # the region before the constants
            (name, lambda fn=fn: fn(hr=0), -2, None),
            (name, lambda fn=fn, fh=fh: fn(pitch=(1 << 31) // fh + 1, hr=1 << 20), -2, "pitch too large"),     # 2 H * pitch reaches 2^31 (H * pitch does not)
            (name, lambda fn=fn, fh=fh: fn(pitch=(1 << 31) // fh + 1, hr=1 << 20, o=odd), -2, "pitch too large"),
            (name, lambda fn=fn: fn(o=odd), -4, "4-byte aligned"),
        ]
        # the footprint that fits exactly is taken: the call gets as far as a later check of its own
        cases += [(name, lambda fn=fn, fh=fh, fw=fw: fn(hr=fh, wr=fw, pitch=3 * fw, **({"out": off4} if fn is conv else {"wsb": 16})),
                   -4 if fn is conv else -3, "16-byte aligned" if fn is conv else "workspace too small")]
    cases += [
        ("toad_tiles_u8_region_box_to_nchw_f32", lambda: conv(out=None), -1, "null pointer"),
        ("toad_tiles_u8_region_box_to_nchw_f32", lambda: conv(b=0), -2, "bad shape"),
        ("toad_tiles_u8_region_box_to_nchw_f32", lambda: conv(out=off4), -4, "16-byte aligned"),
        ("toad_stem_pool_region_box_u8", lambda: stem(b=0), -2, "W = 256"),
        ("toad_stem_pool_region_box_u8", lambda: stem(w=128), -2, "W = 256"),
        ("toad_stem_pool_region_box_u8", lambda: stem(w=512, s=1), -2, "W = 256"),         # W is the network tile's, never the footprint's
        ("toad_stem_pool_region_box_u8", lambda: stem(h=6), -2, "H % 4 == 0"),
        ("toad_stem_pool_region_box_u8", lambda: stem(h=6, s=3), -2, "H % 4 == 0"),        # the twin's tile shape before the region's checks
        ("toad_stem_pool_region_box_u8", lambda: stem(wsb=16), -3, "workspace too small"),
        ("toad_stem_pool_region_box_u8", lambda: stem(y=off4), -4, "16-byte aligned"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(f=None, f16=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(wp=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(b=0), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(b=0, s=3), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(wsb=16), -3, "workspace too small"),
        # the workspace is the NETWORK tile's: the fp32 figure of a staged (7, 9) tile lacks the staging image, whatever the footprint
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(h=7, w=9, wsb=lib.toad_resnet50_trunc_ws_bytes(2, 7, 9)), -3, "workspace too small"),
        ("toad_resnet50_trunc_fwd_u8_region_box", lambda: net(f=None, f16=off4), -4, "16-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and (text is None or text in msg) and msg.startswith(name + ":"), (name, text, got, msg)
    # the largest pitch the box form takes is the one just below ITS bound, 2 H * pitch = 2^31 - 16 for H = 8: only the later workspace check stops the call.
    # The same pitch with twice the tile height is refused; shrink = 1 at that pitch is the twin's bound, H * pitch < 2^31, and passes it
    p = (1 << 31) // 16 - 1
    assert stem(pitch=p, hr=1 << 20, wsb=16) == -3 and "workspace too small" in err()
    assert stem(pitch=p + 1, hr=1 << 20, wsb=16) == -2 and "pitch too large" in err()
    assert stem(pitch=p + 1, hr=1 << 20, wsb=16, s=1) == -3 and "workspace too small" in err()
    assert lib.toad_resnet50_trunc_u8_ws_bytes(2, 8, 256) == lib.toad_resnet50_trunc_ws_bytes(2, 8, 256)          # no staging image on the 256-wide route


def test_box_tiles_u8_is_the_formula():
    from toad_amd import ops
    # rounding: every box of the table, on every channel
    r = box_region()
    n = len(BOXES)
    got = ops.box_tiles_u8(r, [(0, 0)], (2, 2 * n), 2)
    assert got.shape == (1, 1, n, 3) and got.dtype == torch.uint8
    for i in range(n):
        for c in range(3):
            box, want = BOXES[(i + c) % n]
            assert sum(box) in (0, 1, 2, 3, 509, 510, 1018, 1020) and want == (sum(box) + 2) // 4
            assert int(got[0, 0, i, c]) == want, (i, c, box)
    assert sorted({sum(b) % 4 for b, _ in BOXES[:4]}) == [0, 1, 2, 3]
    assert torch.equal(got, box_formula(r, [(0, 0)], 2, 2 * n, 2))
    # one box alone, at an odd origin of a larger region
    wide = torch.full((5, 9, 3), 9, dtype=torch.uint8)
    wide[1:3, 3:5] = r[:, 10:12]
    assert torch.equal(ops.box_tiles_u8(wide, [(3, 1)], 2, 2), r[:, 10:12].to(torch.int64).sum(dim=(0, 1)).add(2).div(4, rounding_mode="floor").to(torch.uint8).view(1, 1, 1, 3))
    # random bytes: odd origins, a duplicate, overlaps, the far corner; rectangular footprints
    g = torch.Generator().manual_seed(11)
    region = torch.randint(0, 256, (29, 41, 3), generator=g, dtype=torch.uint8)
    for (fh, fw), origins in (((14, 18), [(0, 0), (23, 15), (1, 2), (1, 2), (7, 3), (22, 0)]), ((2, 40), [(1, 27), (0, 0)]), ((28, 2), [(39, 1)])):
        got = ops.box_tiles_u8(region, origins, (fh, fw), 2)
        assert got.shape == (len(origins), fh // 2, fw // 2, 3) and torch.equal(got, box_formula(region, origins, fh, fw, 2))
        same = ops.box_tiles_u8(region, np.array(origins), (fh, fw), 1)
        assert torch.equal(same, torch.stack([region[y:y + fh, x:x + fw] for x, y in origins])) and torch.equal(same, box_formula(region, origins, fh, fw, 1))
    # a strided view gives what its copy gives
    view = torch.randint(0, 256, (31, 50, 3), generator=g, dtype=torch.uint8)[1:30, 4:45]
    assert not view.is_contiguous() and torch.equal(ops.box_tiles_u8(view, [(3, 5)], (8, 6), 2), ops.box_tiles_u8(view.clone(), [(3, 5)], (8, 6), 2))
    assert ops.box_tiles_u8(region, np.zeros((0, 2), dtype=np.int64), (14, 18), 2).shape == (0, 7, 9, 3)
    # refusals
    with pytest.raises(ValueError, match=r"origins\[0\]"):                    # the FOOTPRINT is what has to fit: x + 18 == Wr + 1
        ops.box_tiles_u8(region, [(24, 0)], (14, 18), 2)
    with pytest.raises(ValueError, match="does not divide"):
        ops.box_tiles_u8(region, [(0, 0)], (14, 17), 2)
    for bad in (0, 3, 4, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="shrink must be"):
            ops.box_tiles_u8(region, [(0, 0)], (14, 18), bad)
    assert ops.shrunk_tile(512, 2) == ((512, 512), (256, 256)) and ops.shrunk_tile((16, 512), 2) == ((16, 512), (8, 256))
    assert ops.shrunk_tile((7, 9), 1) == ((7, 9), (7, 9))


def test_shrink_refusals_come_before_the_library(monkeypatch):
    """A bad shrink, or a footprint it does not divide, is a ValueError before anything else is looked at: on a CPU region, with the library out of reach."""
    from toad_amd import _lib as L, eval as E, ops
    from toad_amd.resnet_custom import resnet50_baseline
    m = resnet50_baseline().eval()

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    region = torch.zeros(40, 531, 3, dtype=torch.uint8)
    org = [(0, 0), (3, 5)]
    with pytest.raises(ValueError, match="does not divide"):
        m.forward_u8_region(region, org, tile=(8, 255), shrink=2)
    with pytest.raises(ValueError, match="shrink must be"):
        m.forward_u8_region(region, org, tile=(16, 512), shrink=3)
    with pytest.raises(ValueError, match="shrink must be"):
        m.forward_u8_region(region, org, tile=(16, 512), shrink=True)
    for bad in (0, 4, 2.0, None):
        with pytest.raises(ValueError, match="shrink must be"):
            m.forward_u8_region(region, org, tile=(16, 512), shrink=bad)
    # the ops and the pipeline calls say the same, as early
    for call in (lambda **kw: ops.tiles_u8_region_to_f32(region, org, **kw), lambda **kw: ops.stem_pool_region_u8(region, org, None, None, **kw),
                 lambda **kw: E.region_attention_scores(m, None, region, org, **kw), lambda **kw: E.region_tissue_attention_heatmap(m, None, region, **kw)):
        with pytest.raises(ValueError, match="shrink must be"):
            call(tile=(16, 512), shrink=3)
    for call in (lambda **kw: E.region_attention_scores(m, None, region, org, **kw), lambda **kw: E.region_tissue_attention_heatmap(m, None, region, **kw)):
        with pytest.raises(ValueError, match="does not divide"):
            call(tile=(8, 255), shrink=2)
    # a good shrink gets as far as the calls without it: the device test
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_u8_region(region, org, tile=(16, 512), shrink=2)
    # ... and, on a stand-in that claims to be on the device, to the origins, which are checked for the FOOTPRINT: x + 512 == Wr + 1
    meta = torch.zeros(40, 531, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    m = m.to("meta")
    for call in (lambda o: m.forward_u8_region(meta, o, tile=(16, 512), shrink=2), lambda o: ops.tiles_u8_region_to_f32(meta, o, tile=(16, 512), shrink=2),
                 lambda o: ops.stem_pool_region_u8(meta, o, None, None, tile=(16, 512), shrink=2)):
        with pytest.raises(ValueError, match=r"origins\[1\]"):
            call([(19, 24), (20, 0)])
        with pytest.raises(ValueError, match=r"origins\[0\]"):                # y + 16 == Hr + 1
            call([(0, 25)])
