"""CPU: the extractor's region-LIST calls (toad_stem_pool_regions_u8, toad_tiles_u8_regions_to_nchw_f32, toad_resnet50_trunc_fwd_u8_regions: an additive
extension of ABI 15). The entry points and the descriptor exist in the header, the library and the ctypes table; they refuse what the host can see, in the
order the header states, before any device access; the Python layer checks every triple (x, y, k) on the host, and slide_attention_heatmap refuses a bad
batch_extract before anything is launched."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

LIST_SYMBOLS = ("toad_stem_pool_regions_u8", "toad_tiles_u8_regions_to_nchw_f32", "toad_resnet50_trunc_fwd_u8_regions")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_symbols_and_the_descriptor_are_declared_exported_and_bound():
    from toad_amd import _lib as L, ops
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in LIST_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert re.search(r"typedef struct \{ const unsigned char \*region; int64_t pitch; int Hr, Wr; \} ToadTileRegion;", header)
    t = L.ToadTileRegion
    assert ctypes.sizeof(t) == 24 and (t.region.offset, t.pitch.offset, t.Hr.offset, t.Wr.offset) == (0, 8, 16, 20)
    assert ops.TILE_REGIONS_MAX == 128 and re.search(r"#define\s+TOAD_TILE_REGIONS_MAX\s+128\b", header)
    assert "THE CALLER'S DUTY" in header and "check_region_origins" in header        # whose job the triples' bounds are


def test_list_entries_report_argument_errors_in_their_order_without_a_gpu():
    from toad_amd import _lib as L, ops
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = (1 << 21) + 1                                       # a region at an odd address is fine; the triples (int32) are refused there
    off4 = ctypes.c_void_p((1 << 21) + 4)
    big = 1 << 40
    good = ops.norm_constants_u8()
    inf_a = (ctypes.c_float * 6)(math.inf, 0.01, 0.01, -1.0, -1.0, -1.0)
    nan_b = (ctypes.c_float * 6)(0.01, 0.01, 0.01, -1.0, math.nan, -1.0)
    w43 = (ctypes.c_void_p * 43)(*([1 << 21] * 43))

    def regs(wide, *over, count=3):
        """`count` regions of 23 x 531 (pitch 1593) - or 20 x 31 (pitch 94) for the converter - with region k's fields replaced by over[k] (a dict)."""
        arr = (L.ToadTileRegion * max(count, 1))()
        for k in range(count):
            f = dict(region=odd, pitch=1593, Hr=23, Wr=531) if wide else dict(region=odd, pitch=94, Hr=20, Wr=31)
            f.update(over[k] if k < len(over) and over[k] else {})
            arr[k].region, arr[k].pitch, arr[k].Hr, arr[k].Wr = f["region"], f["pitch"], f["Hr"], f["Wr"]
        return arr

    def conv(r=None, n=3, t=one, nm=good, out=one, b=2, h=7, w=9, s=1):
        return lib.toad_tiles_u8_regions_to_nchw_f32(regs(False) if r is None else r, n, t, nm, out, b, h, w, s, None)

    def stem(r=None, n=3, t=one, nm=good, y=one, b=2, h=8, w=256, s=1, ws=one, wsb=big):
        return lib.toad_stem_pool_regions_u8(regs(True) if r is None else r, n, t, nm, one, one, y, b, h, w, s, ws, wsb, None)

    def net(r=None, n=3, t=one, nm=good, f=one, f16=None, b=2, h=8, w=256, s=1, wsb=big, wp=w43):
        return lib.toad_resnet50_trunc_fwd_u8_regions(regs(True) if r is None else r, n, t, nm, wp, w43, f, f16, b, h, w, s, one, wsb, None)

    cases = []
    for name, fn in (("toad_tiles_u8_regions_to_nchw_f32", conv), ("toad_stem_pool_regions_u8", stem), ("toad_resnet50_trunc_fwd_u8_regions", net)):
        wide = fn is not conv
        wr, h = (531, 8) if wide else (31, 7)
        R = lambda *over, wide=wide, **kw: regs(wide, *over, **kw)             # noqa: E731
        null_list = ctypes.cast(None, ctypes.POINTER(L.ToadTileRegion))
        cases += [
            # 1. null pointers - in front of everything, a bad n, a bad shrink and a bad region included
            (name, lambda fn=fn: fn(r=null_list, n=0), -1, "null pointer"),
            (name, lambda fn=fn: fn(t=None, n=0, s=3), -1, "null pointer"),
            (name, lambda fn=fn, R=R: fn(nm=None, r=R({}, dict(pitch=1))), -1, "null pointer"),
            # 2. n - in front of shrink and the regions
            (name, lambda fn=fn: fn(n=0, s=3), -2, "TOAD_TILE_REGIONS_MAX"),
            (name, lambda fn=fn, R=R: fn(r=R(count=129), n=129), -2, "1 .. 128"),
            (name, lambda fn=fn, R=R: fn(n=-1), -2, "TOAD_TILE_REGIONS_MAX"),
            # 3. shrink - in front of the regions
            (name, lambda fn=fn, R=R: fn(s=3, r=R({}, dict(pitch=1))), -2, "shrink must be 1 or 2"),
            (name, lambda fn=fn: fn(s=0), -2, "shrink must be 1 or 2"),
            # 4. region by region; the first failing region wins and is named
            (name, lambda fn=fn, R=R, wr=wr: fn(r=R({}, dict(pitch=3 * wr - 1))), -2, "region 1: pitch"),
            (name, lambda fn=fn, R=R: fn(r=R({}, {}, dict(Hr=4))), -2, "region 2: a"),                                  # H > Hr: "a 8 x 256 tile does not fit"
            (name, lambda fn=fn, R=R: fn(r=R({}, {}, dict(Hr=4))), -2, "does not fit"),
            (name, lambda fn=fn, R=R, wr=wr: fn(r=R({}, dict(pitch=3 * wr - 1), dict(Hr=4))), -2, "region 1: pitch"),
            (name, lambda fn=fn, R=R: fn(r=R({}, {}, dict(Hr=2 * (8 if fn is not conv else 7) - 1)), s=2, h=8 if fn is not conv else 7), -2, "region 2: the"),   # the footprint
            (name, lambda fn=fn, R=R: fn(r=R(dict(Hr=0))), -2, "region 0: bad shape"),
            (name, lambda fn=fn, R=R: fn(r=R({}, dict(region=None))), -1, "region 1: null pointer"),
            (name, lambda fn=fn, R=R, h=h: fn(r=R({}, {}, dict(pitch=(1 << 31) // h + 1, Hr=1 << 20))), -2, "region 2: pitch too large"),       # H * pitch reaches 2^31
            # ... in front of the triples' alignment
            (name, lambda fn=fn, R=R: fn(r=R(dict(pitch=5)), t=ctypes.c_void_p(odd)), -2, "region 0: pitch"),
            # 5. the triples - in front of norm
            (name, lambda fn=fn: fn(t=ctypes.c_void_p(odd), nm=inf_a), -4, "tiles (int32 [B][3]) must be 4-byte aligned"),
            # 6. what the twin checks after its region
            (name, lambda fn=fn: fn(nm=inf_a), -1, "norm[0] is not finite"),
            (name, lambda fn=fn: fn(nm=nan_b), -1, "norm[4] is not finite"),
        ]
    cases += [
        ("toad_tiles_u8_regions_to_nchw_f32", lambda: conv(out=None), -1, "null pointer"),
        ("toad_tiles_u8_regions_to_nchw_f32", lambda: conv(b=0), -2, "bad shape"),
        ("toad_tiles_u8_regions_to_nchw_f32", lambda: conv(out=off4), -4, "16-byte aligned"),
        ("toad_stem_pool_regions_u8", lambda: stem(b=0), -2, "W = 256"),
        ("toad_stem_pool_regions_u8", lambda: stem(h=4, w=128), -2, "W = 256"),
        ("toad_stem_pool_regions_u8", lambda: stem(h=6), -2, "H % 4 == 0"),
        ("toad_stem_pool_regions_u8", lambda: stem(wsb=16), -3, "workspace too small"),
        ("toad_stem_pool_regions_u8", lambda: stem(y=off4), -4, "16-byte aligned"),
        ("toad_resnet50_trunc_fwd_u8_regions", lambda: net(f=None, f16=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_regions", lambda: net(wp=None), -1, "null pointer"),
        ("toad_resnet50_trunc_fwd_u8_regions", lambda: net(b=0), -2, "bad shape"),
        ("toad_resnet50_trunc_fwd_u8_regions", lambda: net(wsb=16), -3, "workspace too small"),
        ("toad_resnet50_trunc_fwd_u8_regions", lambda: net(f=None, f16=off4), -4, "16-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)
    # the largest pitch that is taken is the one just below the bound (H * pitch = 2^31 - 8 for H = 8), in the last of 128 regions: only the workspace stops it
    full = regs(True, *([{}] * 127 + [dict(pitch=(1 << 31) // 8 - 1, Hr=1 << 20)]), count=128)
    assert stem(r=full, n=128, wsb=16) == -3 and "workspace too small" in err()


def test_region_origins_are_checked_on_the_host():
    from toad_amd import ops
    shapes = [(23, 531), (16, 512), (23, 531)]
    h, w = 8, 256
    ok = [(0, 0, 0), (275, 15, 2), (256, 8, 1), (2, 3, 0), (2, 3, 0)]
    for form in (ok, np.array(ok), np.array(ok, dtype=np.int16), torch.tensor(ok), torch.tensor(ok, dtype=torch.int32)):
        o = ops.check_region_origins(form, shapes, h, w)
        assert o.dtype == torch.int32 and o.device.type == "cpu" and o.is_contiguous() and o.tolist() == [list(t) for t in ok]
    empty = ops.check_region_origins(np.zeros((0, 3), dtype=np.int64), shapes, h, w)
    assert empty.dtype == torch.int32 and tuple(empty.shape) == (0, 3)
    with pytest.raises(ValueError, match=r"origins\[1\].*region 1, which is 16 x 512"):        # fits regions 0 and 2, not ITS region; the first offender is named
        ops.check_region_origins([(0, 0, 0), (275, 15, 1), (276, 0, 0)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[2\].*region 0, which is 23 x 531"):        # x + W == Wr + 1
        ops.check_region_origins([(0, 0, 0), (275, 15, 2), (276, 0, 0)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\].*region 1"):                           # y + H == Hr + 1
        ops.check_region_origins([(0, 9, 1)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[1\]"):                                     # a negative y
        ops.check_region_origins([(0, 0, 0), (5, -1, 2)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\]"):                                     # a negative x
        ops.check_region_origins(np.array([(-1, 0, 0)]), shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[1\].*k=3.*3 regions \(0 \.\. 2\)"):        # k == n
        ops.check_region_origins([(0, 0, 0), (0, 0, 3)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\].*k=-1"):                               # no wrap-around to the last region
        ops.check_region_origins([(0, 0, -1)], shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\]"):                                     # no wrap-around through int32
        ops.check_region_origins(torch.tensor([(2 ** 32, 0, 0)]), shapes, h, w)
    with pytest.raises(ValueError, match=r"origins\[0\].*k="):
        ops.check_region_origins(torch.tensor([(0, 0, 2 ** 32)]), shapes, h, w)
    with pytest.raises(TypeError, match="integers"):
        ops.check_region_origins(np.array(ok, dtype=np.float32), shapes, h, w)
    with pytest.raises(TypeError, match="integers"):
        ops.check_region_origins([(0.0, 0.0, 0.0)], shapes, h, w)
    with pytest.raises(ValueError, match=r"\[B,3\]"):
        ops.check_region_origins([(0, 0)], shapes, h, w)
    with pytest.raises(ValueError, match=r"\[B,3\]"):
        ops.check_region_origins([0, 0, 0], shapes, h, w)
    with pytest.raises(ValueError, match="on the host"):                                      # a device tensor cannot be checked without a synchronisation
        ops.check_region_origins(torch.zeros(2, 3, dtype=torch.int32, device="meta"), shapes, h, w)


def test_forward_u8_regions_refusals_cpu(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.resnet_custom import resnet50_baseline
    m = resnet50_baseline().eval()

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    region = torch.zeros(23, 531, 3, dtype=torch.uint8)
    org = [(0, 0, 0), (275, 15, 1)]
    with pytest.raises(ValueError, match="shrink"):                                           # shrink first, as in forward_u8_region
        m.forward_u8_regions([region.float()], [(0, 0, 7)], tile=(8, 256), shrink=3)
    with pytest.raises(TypeError, match="list or tuple"):
        m.forward_u8_regions(region, org, tile=(8, 256))
    with pytest.raises(ValueError, match="129 regions"):
        m.forward_u8_regions([region] * 129, org, tile=(8, 256))
    with pytest.raises(ValueError, match="0 regions"):
        m.forward_u8_regions([], org, tile=(8, 256))
    with pytest.raises(RuntimeError, match=r"HIP device.*regions\[0\]"):
        m.forward_u8_regions([region, region], org, tile=(8, 256))
    with pytest.raises(RuntimeError, match=r"float32 as regions\[0\]"):
        m.forward_u8_regions([region.float(), region], org, tile=(8, 256))
    with pytest.raises(RuntimeError, match=r"\[Hr,Wr,3\].*regions\[0\]"):
        m.forward_u8_regions([torch.zeros(3, 23, 531, dtype=torch.uint8), region], org, tile=(8, 256))
    with pytest.raises(RuntimeError, match="out_dtype"):
        m.forward_u8_regions([region], org, tile=(8, 256), out_dtype=torch.bfloat16)
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m.forward_u8_regions([region], org, tile=(8, 256))
    m.eval()
    # what comes after the device test, on stand-ins that claim to be on the device: layout, then the triples
    meta = torch.zeros(23, 1062, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    reg = meta[:, :531]
    with pytest.raises(RuntimeError, match=r"stride\(1\) == 3.*regions\[1\]"):
        m.forward_u8_regions([reg, meta[:, ::2]], org, tile=(8, 256))
    with pytest.raises(ValueError, match=r"regions\[1\].*stride\(1\) == 3"):
        ops.tiles_u8_regions_to_f32([reg, meta[:, ::2]], org, tile=(8, 256))
    with pytest.raises(ValueError, match=r"regions\[1\].*stride\(1\) == 3"):
        ops.stem_pool_regions_u8([reg, meta[:, ::2]], org, None, None, tile=(8, 256))
    with pytest.raises(ValueError, match=r"regions\[1\] is on cpu.*one device"):
        ops.stem_pool_regions_u8([reg, region], org, None, None, tile=(8, 256))
    with pytest.raises(ValueError, match="129 regions"):
        ops.tiles_u8_regions_to_f32([reg] * 129, org, tile=(8, 256))
    m = m.to("meta")
    small = meta[:16, :512]
    for call in (lambda o: m.forward_u8_regions([reg, small], o, tile=(8, 256)), lambda o: ops.tiles_u8_regions_to_f32([reg, small], o, tile=(8, 256)),
                 lambda o: ops.stem_pool_regions_u8([reg, small], o, None, None, tile=(8, 256))):
        with pytest.raises(ValueError, match=r"origins\[1\].*region 1, which is 16 x 512"):
            call([(0, 0, 0), (275, 15, 1)])                                   # inside region 0, outside ITS region
        with pytest.raises(ValueError, match=r"origins\[0\].*k=2"):
            call([(0, 0, 2)])
        with pytest.raises(ValueError, match=r"origins\[0\].*k=-1"):
            call([(0, 0, -1)])
        with pytest.raises(ValueError, match=r"\[B,3\]"):
            call([(0, 0)])
        with pytest.raises(ValueError, match="on the host"):
            call(torch.zeros(2, 3, dtype=torch.int32, device="meta"))
        with pytest.raises(TypeError, match="integers"):
            call(np.zeros((2, 3), dtype=np.float64))
    assert tuple(m.forward_u8_regions([reg, small], np.zeros((0, 3), dtype=np.int64), tile=(8, 256)).shape) == (0, 1024)       # B == 0: no library call


def test_slide_attention_heatmap_refuses_a_bad_batch_extract_before_anything_is_launched(monkeypatch):
    from toad_amd import _lib as L, ops
    from toad_amd.eval import slide_attention_heatmap

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    hs, ws = 256, 1100
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    strips = [(slide[y:y + n], y) for y, n in [(0, 112), (64, 144), (176, 80)]]
    kw = dict(tile=(64, 256), stride=(64, 256))
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="batch_extract must be a bool"):
            slide_attention_heatmap(None, None, strips, (hs, ws), batch_extract=bad, **kw)
    many = [(slide[y:y + 1], y) for y in range(ops.TILE_REGIONS_MAX + 1)]                    # 129 strips: refused whatever else is wrong with them
    with pytest.raises(ValueError, match=r"batch_extract=True takes at most 128 strips .*got 129"):
        slide_attention_heatmap(None, None, many, (hs, ws), batch_extract=True, **kw)
    with pytest.raises(ValueError, match=r"batch_extract=True takes at most 128 strips"):    # independent of batch_render
        slide_attention_heatmap(None, None, many, (hs, ws), batch_extract=True, batch_render=True, **kw)


def test_batch_extract_lists_only_the_strips_that_own_tiles(monkeypatch):
    """A remainder strip shorter than the tile owns no lattice row and only renders the slide's last rows; the list call wants a tile to fit every region it
    is given. So the one call gets the strips that own tiles, renumbered - never a strip the per-strip walk would skip. Nothing is launched here: a stand-in
    extractor records its arguments and stops the walk."""
    from toad_amd import _lib as L
    from toad_amd.eval import slide_attention_heatmap, strip_triples
    from toad_amd.heatmap import strip_plan

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)

    class Captured(Exception):
        pass

    class Recorder:
        def forward_u8_regions(self, regions, origins, **kw):
            self.regions, self.origins, self.kw = regions, np.asarray(origins), kw
            raise Captured

        def forward_u8_region(self, *a, **kw):
            raise AssertionError("batch_extract=True makes no per-strip call")
    kw = dict(tile=(64, 256), stride=(64, 256), batch_extract=True)
    # a 300-row slide as 256 + 44 rows: the last strip is shorter than the tile
    hs, ws = 300, 1100
    spans = [(0, 256), (256, 44)]
    plan = strip_plan((hs, ws), spans, (64, 256), (64, 256), (0, 0), 1)
    assert [p["rows"] for p in plan] == [(0, 4), (4, 4)]
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    strips = [(slide[y:y + n], y) for y, n in spans]
    given = np.array([(0, 0), (256, 64), (512, 192)], dtype=np.int64)
    rec = Recorder()
    with pytest.raises(Captured):
        slide_attention_heatmap(rec, None, strips, (hs, ws), origins=given, **kw)
    assert len(rec.regions) == 1 and rec.regions[0] is strips[0][0] and rec.origins.tolist() == [[0, 0, 0], [256, 64, 0], [512, 192, 0]]
    assert rec.kw["tile"] == (64, 256) and all(r.shape[0] >= 64 for r in rec.regions)
    # three overlapping strips, the middle one without a tile: the third strip becomes region 1, its tile at its local row
    hs = 256
    spans = [(0, 112), (64, 144), (176, 80)]
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    strips = [(slide[y:y + n], y) for y, n in spans]
    rec = Recorder()
    with pytest.raises(Captured):
        slide_attention_heatmap(rec, None, strips, (hs, ws), origins=np.array([(256, 0), (0, 192), (768, 192)]), **kw)
    assert len(rec.regions) == 2 and rec.regions[0] is strips[0][0] and rec.regions[1] is strips[2][0]
    assert rec.origins.tolist() == [[256, 0, 0], [0, 16, 1], [768, 16, 1]]
    # the helper itself
    a, b = object(), object()
    regions, triples = strip_triples([(a, [(1, 2)]), (b, np.array([(3, 4), (5, 6)]))])
    assert regions == [a, b] and triples.dtype == np.int64 and triples.tolist() == [[1, 2, 0], [3, 4, 1], [5, 6, 1]]
    assert strip_triples([])[1].shape == (0, 3)
    with pytest.raises(ValueError, match="part 1"):
        strip_triples([(a, [(1, 2)]), (b, np.zeros((0, 2), dtype=np.int64))])
