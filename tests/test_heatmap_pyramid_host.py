"""CPU: several levels of the heat-map pyramid in one call (toad_region_heat_pyramid_u8: an additive extension of ABI 15; ops.region_heat_pyramid,
heatmap.window_pyramid / attention_pyramid, a sequence as ``down`` of heatmap.strip_plan and of the two eval heat-map calls). The entry point exists in
the header, the library and the ctypes table and refuses what the host can see before any device access, in the window entry's order; the Python layers
refuse before the library is loaded; and with an int ``down`` everything calls what it called before."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NAME = "toad_region_heat_pyramid_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOWNS = (1, 2, 4, 8, 16, 32)


def test_pyramid_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header), f"{NAME} is not declared in include/toad_hip.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 23
    wn = L.SIGNATURES["toad_region_heat_window_u8"][1]
    sig = L.SIGNATURES[NAME][1]
    assert sig[:12] == wn[:12] and sig[12] == ctypes.c_uint and sig[13:20] == wn[13:20] and sig[20:] == [ctypes.c_void_p] * 3      # levels for down; outs, out_pitches
    block = header[header.index("toad_region_heat_window_u8("):header.index(NAME + "(")]
    for text in ("bit k asks for down = 2^k", "HOST arrays of 6 entries", "byte for byte what toad_region_heat_window_u8", "Each level keeps its own Ho = Hr / down",
                 "levels == 0 or a bit above 5", "multiples of max(4, D)", "mask_down is a multiple of D", "smooth = 1 at cell == 4 is refused",
                 "A set of one level IS toad_region_heat_window_u8"):
        assert text in block, text


def test_pyramid_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = 1 << 21                                             # non-null fake pointers: every check below comes before a device access
    odd, two = one + 1, one + 2                               # the region, the mask and the canvases may lie at an odd address; int32 cells may not

    # a 40 x 61 window at (32, 64) of an image of 7 x 8 cells of 16 pixels (112 x 128), levels 1, 4 and 16, the image's 16-box mask plane (7 x 8)
    def py(r=odd, pitch=3 * 61 + 1, hr=40, wr=61, wx=32, wy=64, c=one, gy=7, gx=8, cell=16, lut=odd, alpha=102, levels=0b10101, smooth=1, mask=odd, mpitch=9, hm=7,
           wm=8, md=16, mt=8, outs=(odd,) * 6, pitches=(183, 90, 45, 21, 9, 3), stream=None):
        o = None if outs is None else (ctypes.c_void_p * 6)(*outs)
        p = None if pitches is None else (ctypes.c_int64 * 6)(*pitches)
        return lib.toad_region_heat_pyramid_u8(r, pitch, hr, wr, wx, wy, c, gy, gx, cell, lut, alpha, levels, smooth, mask, mpitch, hm, wm, md, mt, o, p, stream)

    def outs_without(k):
        return tuple(None if j == k else odd for j in range(6))

    cases = [
        # the window entry's refusals, in its order
        (lambda: py(r=None), -1, "null pointer"), (lambda: py(c=None), -1, "null pointer"), (lambda: py(lut=None), -1, "null pointer"),
        (lambda: py(outs=None), -1, "null pointer"), (lambda: py(pitches=None), -1, "null pointer"),
        (lambda: py(cell=12), -2, "cell"), (lambda: py(cell=2, levels=0), -2, "cell"), (lambda: py(hr=0), -2, "bad shape"), (lambda: py(wr=-1, levels=0), -2, "bad shape"),
        (lambda: py(alpha=-1), -2, "alpha"), (lambda: py(alpha=257, levels=64), -2, "alpha"),
        # the set, where the down check sits: empty, a bit above 5, the largest level above the cell, a canvas that is asked for and missing
        (lambda: py(levels=0), -2, "levels = 0x0"), (lambda: py(levels=64), -2, "levels = 0x40"), (lambda: py(levels=0b1000001), -2, "bits 0 .. 5"),
        (lambda: py(levels=0xFFFFFFFF), -2, "bits 0 .. 5"), (lambda: py(levels=0, wx=3), -2, "levels"),
        (lambda: py(levels=0b100001), -2, "down = 32, the largest level, exceeds cell = 16"), (lambda: py(levels=0b11000, cell=8), -2, "exceeds cell = 8"),
        (lambda: py(levels=0b1001, cell=4), -2, "exceeds cell = 4"), (lambda: py(levels=0b100001, wx=3, smooth=2), -2, "exceeds cell"),
        (lambda: py(outs=outs_without(0)), -1, "outs[0], the canvas of down = 1"), (lambda: py(outs=outs_without(4), wx=3), -1, "outs[4], the canvas of down = 16"),
        (lambda: py(outs=outs_without(2), levels=0b100, wx=3), -1, "outs[2]"),
        # the window: negative, or not a multiple of max(4, D)
        (lambda: py(wx=-16), -2, "window"), (lambda: py(wy=-16, smooth=2), -2, "window"), (lambda: py(wx=8), -2, "multiple of max(4, down) = 16"),
        (lambda: py(wy=24), -2, "max(4, down) = 16"), (lambda: py(levels=0b011, wx=2, md=2), -2, "max(4, down) = 4"), (lambda: py(levels=0b1100, wx=4), -2, "max(4, down) = 8"),
        (lambda: py(smooth=2), -1, "smooth"), (lambda: py(smooth=-1), -1, "smooth"),
        (lambda: py(cell=4, levels=0b011, gy=28, gx=32), -2, "smooth at cell = 4"), (lambda: py(cell=4, levels=0b110, gy=28, gx=32, pitch=1), -2, "smooth at cell = 4"),
        (lambda: py(pitch=3 * 61 - 1), -2, "pitch"), (lambda: py(pitch=-184), -2, "pitch"),
        (lambda: py(md=0), -2, "mask_down"), (lambda: py(md=3), -2, "mask_down"), (lambda: py(md=64), -2, "mask_down"),
        (lambda: py(md=8), -2, "multiple of down = 16, the largest level"), (lambda: py(md=4, pitches=(0,) * 6), -2, "multiple of down = 16"),
        (lambda: py(levels=0b110, md=2), -2, "multiple of down = 4"),
        (lambda: py(hm=-1), -2, "Hm x Wm"), (lambda: py(wm=-1), -2, "Hm x Wm"),
        (lambda: py(mpitch=7), -2, "mask_pitch"), (lambda: py(mt=-1), -1, "mask_thresh"), (lambda: py(mt=256), -1, "mask_thresh"),
        # every canvas asked for has a row's worth of pitch; the ones not asked for are not looked at
        (lambda: py(pitches=(182, 90, 45, 21, 9, 3)), -2, "out_pitches[0] = 182"), (lambda: py(pitches=(183, 0, 44, 0, 9, 0)), -2, "out_pitches[2] = 44"),
        (lambda: py(pitches=(183, 90, 45, 21, 8, 3)), -2, "canvas of down = 16 (3 Wo = 9 bytes)"), (lambda: py(pitches=(183, 0, 45, 0, -9, 0), gy=5), -2, "out_pitches[4]"),
        # the window beyond the table: rows 64 .. 104 need 7 cell rows, columns 32 .. 93 need 6 cell columns
        (lambda: py(gy=6), -2, "beyond the table"), (lambda: py(gx=5), -2, "beyond the table"), (lambda: py(wy=80), -2, "beyond the table"),
        (lambda: py(wx=80, c=odd), -2, "beyond the table"),
        (lambda: py(hr=1 << 30, wr=16385, wx=0, wy=0, pitch=1 << 20, gy=1 << 26, gx=1025, pitches=(1 << 20,) * 6, mask=None), -2, "workgroups"),
        (lambda: py(c=odd), -4, "4-byte aligned"), (lambda: py(c=two), -4, "4-byte aligned"),
    ]
    big = dict(wr=64, pitch=192, mask=None, pitches=(192,) * 6, levels=0b11, wy=0)
    cases += [(lambda: py(wx=(1 << 30) - 64, gx=1 << 26, **big), -2, "2^30"), (lambda: py(wx=(1 << 30) - 128, gx=(1 << 26) - 5, **big), -2, "beyond the table")]
    for call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # what is taken: only the later alignment check stops these calls
    for ok in (dict(), dict(wx=0, wy=0), dict(gy=100, gx=100), dict(smooth=0), dict(hm=0, wm=0, mpitch=0), dict(md=32), dict(levels=0b111111, cell=64, gy=2, gx=2, md=32, wx=32),
               dict(levels=0b011, md=2, wx=4, wy=12), dict(levels=0b110, cell=4, smooth=0, gy=28, gx=32, wx=4, wy=4), dict(levels=0b11000, wx=48), dict(alpha=0), dict(alpha=256),
               dict(outs=(odd, None, odd, None, odd, None), pitches=(183, -1, 45, -1, 9, -1)), dict(mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999)):
        assert py(c=odd, **ok) == -4, ok
    # one level is the window entry: its checks, its messages under this entry's name - smooth at cell 4 among what it takes
    assert py(levels=0b100, cell=4, gy=28, gx=32, c=odd) == -4 and py(levels=0b10000, md=8) == -2 and "multiple of down = 16" in err() and err().startswith(NAME + ":")
    assert py(levels=0b1000, wx=8, wy=8, pitches=(0, 0, 0, 20, 0, 0)) == -2 and "out_pitch" in err()
    # levels that are empty write nothing and the call returns 0 where all are: everything is checked, nothing is launched (no device is present here)
    assert py(hr=3, levels=0b10100) == 0 and py(hr=3, levels=0b10100, gy=3) == -2 and py(hr=3, levels=0b10100, c=odd) == -4
    assert py(wr=3, pitch=9, levels=0b1100, pitches=(0,) * 6) == 0 and py(hr=15, wr=15, pitch=45, levels=0b110000, md=32, wx=32, cell=64, gy=2, gx=2) == 0


# ---- strip_plan -----------------------------------------------------------------------------------------------------------------------------------------
def test_strip_plan_takes_a_set_of_levels():
    from toad_amd.heatmap import strip_plan
    rng = np.random.default_rng(5)
    seen = 0
    for trial in range(200):
        hs = int(rng.integers(3, 12)) * 32
        cut = int(rng.integers(1, hs // 32)) * 32
        strips = [(0, cut), (cut - 32, hs - cut + 32)]
        ds = tuple(int(d) for d in rng.permutation(DOWNS)[:int(rng.integers(1, 7))])
        for args in (((hs, 640), strips, (32, 32), (32, 32), (0, 0)), ((hs, 640), strips, 64, 32, (0, 0))):
            try:
                want = strip_plan(*args, max(ds))
            except ValueError as e:
                with pytest.raises(ValueError, match=re.escape(str(e))):
                    strip_plan(*args, ds)
                continue
            assert strip_plan(*args, ds) == want == strip_plan(*args, list(ds))
            seen += 1
    assert seen > 100
    # an int is today's: the cases of test_heatmap_window_host.test_strip_plan_refuses
    plan = lambda strips, down=1, hs=256, tile=64, stride=32: strip_plan((hs, 512), strips, tile, stride, (0, 0), down)      # noqa: E731
    assert [p["render"] for p in plan([(0, 128), (96, 160)])] == [(0, 128), (128, 256)] and [p["rows"] for p in plan([(0, 128), (96, 160)])] == [(0, 3), (3, 7)]
    assert plan([(0, 128), (120, 48), (128, 128)], stride=64)[1] == dict(rows=(2, 2), origin=None, render=(128, 168))
    for strips, k, text in (([(0, 130), (96, 160)], {}, r"multiple of max\(4, down\) = 4"), ([(0, 132), (96, 160)], dict(down=8), r"max\(4, down\) = 8"),
                            ([(0, 144), (96, 160)], dict(down=32), r"max\(4, down\) = 32"), ([(0, 128), (96, 160)], dict(down=3), "down must be one of"),
                            ([(0, 144), (96, 160)], dict(down=(1, 32)), r"max\(4, down\) = 32"), ([(0, 132), (96, 160)], dict(down=(8, 2)), r"max\(4, down\) = 8"),
                            ([(0, 128), (96, 160)], dict(down=(1, 3)), "distinct values"), ([(0, 128), (96, 160)], dict(down=()), "non-empty"),
                            ([(0, 128), (96, 160)], dict(down=(4, 4)), "distinct")):
        with pytest.raises(ValueError, match=text):
            plan(strips, **k)
    assert len(plan([(0, 132), (96, 160)], down=(1, 4))) == 2


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pyramid_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.heatmap import window_pyramid

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_pyramid(cpu, (0, 0), torch.zeros(8, 8, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, (1, 4))
    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells, lut = torch.zeros(8, 8, dtype=torch.int32, device="meta"), torch.zeros(256, 3, dtype=torch.uint8, device="meta")
    m8 = torch.zeros(8, 8, dtype=torch.uint8, device="meta")
    canv = lambda h, w: torch.zeros(h, w, 3, dtype=torch.uint8, device="meta")      # noqa: E731
    base = dict(region=meta, window=(16, 16), cells=cells, cell=16, lut=lut, alpha=102, downs=(1, 4, 16))
    for k, text in ((dict(downs=()), "non-empty"), (dict(downs=4), "downs must be"), (dict(downs=(1, 3)), "distinct values from"), (dict(downs=(1, 64)), "distinct values from"),
                    (dict(downs=(4, 4)), "distinct"), (dict(downs=(True, 4)), "downs must be"), (dict(downs=(1.0, 4)), "downs must be"), (dict(downs="14"), "downs must be"),
                    (dict(downs=(1, 32)), "exceeds cell = 16"), (dict(downs=(8,), cell=4), "exceeds cell = 4"), (dict(cell=12), "cell"), (dict(alpha=257), "alpha"),
                    (dict(window=(0,)), "window must be"), (dict(window=(8, 16)), r"multiples of max\(4, down\) = 16"), (dict(window=(16, 4)), r"max\(4, down\) = 16"),
                    (dict(window=(2, 0), downs=(1, 2)), r"max\(4, down\) = 4"), (dict(window=(4, 8), downs=(8, 2)), r"max\(4, down\) = 8"),
                    (dict(window=((1 << 30) - 64, 0)), "below 2\\^30"), (dict(window=(80, 16)), "beyond the int32"), (dict(cells=cells[:4]), "beyond the int32"),
                    (dict(lut=lut[:255]), "lut"), (dict(smooth=2), "smooth"), (dict(smooth=True, cell=4, downs=(1, 2), cells=torch.zeros(32, 32, dtype=torch.int32, device="meta")), "smooth at cell = 4"),
                    (dict(mask_down=16), "without a mask"), (dict(mask=m8), "mask_down"), (dict(mask=m8, mask_down=3), "mask_down"),
                    (dict(mask=m8, mask_down=8), "multiple of down = 16"), (dict(mask=m8, mask_down=4, downs=(8, 1)), "multiple of down = 8"),
                    (dict(mask=m8, mask_down=16, mask_thresh=256), "mask_thresh"),
                    (dict(outs=[canv(64, 64), canv(16, 16)]), "sequence of 3 canvases"), (dict(outs=canv(64, 64)), "sequence of 3 canvases"),
                    (dict(outs=[canv(64, 64), canv(16, 16), canv(4, 5)]), r"outs\[2\] \(down = 16\) must be a uint8 \[4,4,3\]"),
                    (dict(outs=[canv(64, 64), canv(16, 32)[:, ::2], canv(4, 4)]), r"outs\[1\] \(down = 4\) must have strides"),
                    (dict(outs=[canv(64, 64).float(), canv(16, 16), canv(4, 4)]), r"outs\[0\]")):
        args = dict(base)
        args.update(k)
        with pytest.raises(ValueError, match=text):
            ops.region_heat_pyramid(**args)
    # storage: real (host) tensors, which have addresses; is_cuda is patched, so the checks run as they do on the device
    region = torch.zeros(64, 64, 3, dtype=torch.uint8)
    rc, rl = torch.zeros(8, 8, dtype=torch.int32), torch.zeros(256, 3, dtype=torch.uint8)
    atlas = torch.zeros(80, 64, 3, dtype=torch.uint8)
    fresh = lambda: [torch.zeros(64 // d, 64 // d, 3, dtype=torch.uint8) for d in (1, 4, 16)]      # noqa: E731
    shared = fresh()
    shared[2] = shared[1][:4, :4]
    with pytest.raises(ValueError, match=r"outs\[1\] and outs\[2\] must not share storage"):
        ops.region_heat_pyramid(region, (16, 16), rc, 16, rl, 102, (1, 4, 16), outs=shared)
    with pytest.raises(ValueError, match=r"outs\[0\] and outs\[1\] must not share storage"):
        ops.region_heat_pyramid(region, (16, 16), rc, 16, rl, 102, (1, 4, 16), outs=[atlas[:64], atlas[64:, :16], fresh()[2]])
    inside = fresh()
    inside[1] = region[:16, :16]
    with pytest.raises(ValueError, match=r"outs\[1\] \(down = 4\) must not share storage with region"):
        ops.region_heat_pyramid(region, (16, 16), rc, 16, rl, 102, (1, 4, 16), outs=inside)
    for outs in (None, fresh()):                                     # canvases of their own are taken: only now is the library reached
        with pytest.raises(AssertionError, match="library was reached"):
            ops.region_heat_pyramid(region, (16, 16), rc, 16, rl, 102, (1, 4, 16), outs=outs)
    # a call in which every level is empty launches nothing; an empty plane is no plane
    got = ops.region_heat_pyramid(meta[:3], (16, 16), cells, 16, lut, 102, (4, 16, 8))
    assert [tuple(g.shape) for g in got] == [(0, 16, 3), (0, 4, 3), (0, 8, 3)]
    got = ops.region_heat_pyramid(meta[:, :1], (16, 16), cells, 16, lut, 102, (2, 4), mask=m8[:0], mask_down=16)
    assert [tuple(g.shape) for g in got] == [(32, 0, 3), (16, 0, 3)]
    for m in (m8, m8[:2, :3], torch.zeros(100, 100, dtype=torch.uint8, device="meta")):
        with pytest.raises(AssertionError, match="library was reached"):
            ops.region_heat_pyramid(meta, (16, 16), cells, 16, lut, 102, (16, 1), mask=m, mask_down=32)
    for k, text in ((dict(alpha=1.5), "alpha"), (dict(smooth=1), "bool"), (dict(mask=(m8, 8)), "triple"), (dict(window=(8, 16)), r"max\(4, down\)"),
                    (dict(downs=(1, 32)), "exceeds cell"), (dict(downs=(2, 2)), "distinct"), (dict(mask=(m8, 8, 8)), "multiple of down = 16")):
        with pytest.raises(ValueError, match=text):
            window_pyramid(meta, k.pop("window", (16, 16)), cells, 16, lut=lut, **k)


def _logger(log, name, result):
    def f(*a, **k):
        log.append((name, a, k))
        return result(*a, **k)
    return f


def test_attention_pyramid_builds_the_table_once(monkeypatch):
    from toad_amd import heatmap, ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    log = []
    monkeypatch.setattr(heatmap, "tile_table", _logger(log, "tile_table", lambda *a, **k: torch.zeros(4, 8, dtype=torch.int32, device="meta")))
    monkeypatch.setattr(ops, "heat_cells", _logger(log, "heat_cells", lambda *a, **k: torch.zeros(5, 9, dtype=torch.int32, device="meta")))
    monkeypatch.setattr(ops, "heat_cells_blur", _logger(log, "heat_cells_blur", lambda c, t: torch.ones_like(c)))
    monkeypatch.setattr(ops, "region_heat_pyramid", _logger(log, "region_heat_pyramid", lambda *a, **k: "canvases"))
    for n in ("region_heat_window", "region_heat_blend_px", "region_heat_thumb"):
        monkeypatch.setattr(ops, n, _logger(log, n, lambda *a, **k: None))
    meta = torch.zeros(300, 520, 3, dtype=torch.uint8, device="meta")
    origins, scores = np.array([[0, 0], [64, 128]]), torch.zeros(2, device="meta")
    mask = (torch.zeros(18, 32, dtype=torch.uint8, device="meta"), 9, 16)
    assert heatmap.attention_pyramid(meta, origins, scores, 128, 64, downs=[1, 16, 4], blur=True, smooth=True, mask=mask, alpha=0.5) == "canvases"
    assert [n for n, _, _ in log] == ["tile_table", "heat_cells", "heat_cells_blur", "region_heat_pyramid"]
    _, a, k = log[-1]
    assert a[1] == (0, 0) and a[3] == 64 and a[5] == 128 and a[6] == (1, 16, 4)
    assert k["smooth"] is True and k["mask"] is mask[0] and k["mask_down"] == 16 and k["mask_thresh"] == 9 and k["outs"] is None
    del log[:]
    for kw, text in ((dict(downs=(1, 64)), "distinct values"), (dict(downs=(8, 16), tile=8, stride=8), "exceeds the lattice's cell"), (dict(smooth=1), "bool"),
                     (dict(alpha=2.5), "alpha")):
        with pytest.raises(ValueError, match=text):
            heatmap.attention_pyramid(meta, origins, scores, kw.pop("tile", 128), kw.pop("stride", 64), **kw)
    assert not log


def test_eval_heatmaps_with_an_int_down_call_what_they_called(monkeypatch):
    """slide_attention_heatmap and region_tissue_attention_heatmap: an int down goes through window_canvas / attention_canvas with the arguments it went
    with; a sequence goes through window_pyramid / attention_pyramid, once per strip / once, with the same table."""
    from toad_amd import eval as E, heatmap, ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    log = []
    monkeypatch.setattr(ops, "region_heat_window", _logger(log, "region_heat_window", lambda *a, **k: k["out"]))
    monkeypatch.setattr(ops, "region_heat_pyramid", _logger(log, "region_heat_pyramid", lambda *a, **k: tuple(k["outs"])))
    hs, ws = 256, 512
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    spans = [(0, 112), (64, 144), (176, 80)]
    strips = [(slide[y:y + n], y) for y, n in spans]
    none = np.zeros((0, 2), dtype=np.int64)
    kw = dict(tile=64, stride=64, origins=none, smooth=True, alpha=0.5)
    for down in DOWNS[:5]:                                           # (seams at 112 and 208: 32 is refused, below)
        del log[:]
        o, s, canvas = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=down, **kw)
        assert o.shape == (0, 2) and s.shape == (0,) and isinstance(canvas, torch.Tensor) and tuple(canvas.shape) == (hs // down, ws // down, 3)
        assert [n for n, _, _ in log] == ["region_heat_window"] * 3
        for (_, a, k), (r0, r1) in zip(log, ((0, 112), (112, 208), (208, 256))):
            assert tuple(a[0].shape) == (r1 - r0, ws, 3) and a[1] == (0, r0) and tuple(a[2].shape) == (4, 8) and a[3] == 64 and a[5] == 128 and a[6] == down
            assert k["smooth"] is True and k["mask"] is None and tuple(k["out"].shape) == ((r1 - r0) // down, ws // down, 3)
    with pytest.raises(ValueError, match=r"multiple of max\(4, down\) = 32"):
        E.slide_attention_heatmap(None, None, strips, (hs, ws), down=32, **dict(kw, tile=64))
    for ds in ((1, 4, 16), [16, 2]):
        del log[:]
        o, s, canvas = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=ds, **kw)
        assert isinstance(canvas, dict) and list(canvas) == list(ds) and all(tuple(canvas[d].shape) == (hs // d, ws // d, 3) for d in ds)
        assert [n for n, _, _ in log] == ["region_heat_pyramid"] * 3                  # ONE walk over the strips
        for (_, a, k), (r0, r1) in zip(log, ((0, 112), (112, 208), (208, 256))):
            assert a[1] == (0, r0) and a[6] == tuple(ds) and [tuple(v.shape) for v in k["outs"]] == [((r1 - r0) // d, ws // d, 3) for d in ds]
    del log[:]
    for bad, text in ((dict(down=(1, 3)), "distinct values"), (dict(down=(1, 32), tile=16, stride=16), "exceeds the lattice's cell = 16"), (dict(down=(1, 32)), r"max\(4, down\) = 32"),
                      (dict(down=(1, 4), out=slide), "out must be None or a dict"), (dict(down=(1, 4), out={1: slide}), "out must be None or a dict"),
                      (dict(down=(1, 4), out={1: slide, 4: slide}), r"out\[4\] must be")):
        with pytest.raises(ValueError, match=text):
            E.slide_attention_heatmap(None, None, strips, (hs, ws), **dict(kw, **bad))
    assert not log
    # region_tissue_attention_heatmap: the selection and the scoring faked
    calls = []
    plane = (torch.zeros(16, 32, dtype=torch.uint8, device="meta"), 9, 16)

    def scores(*a, **k):
        calls.append(("scores", k.get("return_mask")))
        return none, torch.zeros(0, device="meta"), plane if k.get("return_mask") else None
    monkeypatch.setattr(E, "_tissue_scores", scores)
    monkeypatch.setattr(heatmap, "attention_canvas", _logger(calls, "attention_canvas", lambda *a, **k: "canvas"))
    monkeypatch.setattr(heatmap, "attention_pyramid", _logger(calls, "attention_pyramid", lambda *a, **k: tuple(f"canvas{d}" for d in k["downs"])))
    for down in (1, 16):
        del calls[:]
        assert E.region_tissue_attention_heatmap(None, None, slide, tile=64, down=down, smooth=True, blur=(2, 1), thresh=0.5)[2] == "canvas"
        assert [c[0] for c in calls] == ["scores", "attention_canvas"]
        assert calls[1][2] == dict(tile=64, stride=None, alpha=102, down=down, lut=None, out=None, smooth=True, mask=None, thresh=0.5, binarize=False, blur=(2, 1))
    del calls[:]
    got = E.region_tissue_attention_heatmap(None, None, slide, tile=64, down=(16, 1), smooth=True, tissue_mask=True, segment=dict(down=16))[2]
    assert got == {16: "canvas16", 1: "canvas1"} and [c[0] for c in calls] == ["scores", "attention_pyramid"]
    assert calls[1][2] == dict(tile=64, stride=None, alpha=102, downs=(16, 1), lut=None, outs=None, smooth=True, mask=plane, thresh=None, binarize=False, blur=False)
    del calls[:]
    for bad, text in ((dict(down=(1, 32), tissue_mask=True, segment=dict(down=16)), "multiple of the largest canvas down = 32"), (dict(down=(4, 4)), "distinct"),
                      (dict(down=(1, 32), tile=16), "exceeds the lattice's cell = 16"), (dict(down=(1, 4), out=[slide, slide]), "out must be None or a dict"),
                      (dict(down=8, tissue_mask=True, segment=dict(down=4)), "multiple of the canvas down = 8")):
        with pytest.raises(ValueError, match=text):
            E.region_tissue_attention_heatmap(None, None, slide, **dict(dict(tile=64), **bad))
    assert not calls
