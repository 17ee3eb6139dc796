"""CPU: a list of windows of one slide in one call (toad_region_heat_windows_u8: an additive extension of ABI 15; ops.region_heat_windows,
heatmap.windows_canvas, eval.slide_attention_heatmap(batch_render=True)). The entry point exists in the header, the library and the ctypes table and
refuses what the host can see before any device access - the shared arguments first, in the window entry's order and with its messages, then window by
window under "window k:"; the Python layers refuse before the library is loaded; and slide_attention_heatmap without batch_render calls what it called."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NAME = "toad_region_heat_windows_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_windows_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L, ops
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+ToadHeatWindow\s*\*", header), f"{NAME} is not declared in include/toad_hip.h"
    assert re.search(r"typedef\s+struct\s*\{\s*const unsigned char \*region; int64_t pitch; int Hr, Wr, wx, wy; unsigned char \*out; int64_t out_pitch;\s*\}\s*ToadHeatWindow;",
                     header)
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES
    sig, wn = L.SIGNATURES[NAME][1], L.SIGNATURES["toad_region_heat_window_u8"][1]
    # the window entry's arguments without its region (6 in front) and its canvas (2 before the stream), behind the host array and its length
    assert sig[0] == ctypes.POINTER(L.ToadHeatWindow) and sig[1] == ctypes.c_int and sig[2:] == wn[6:20] + wn[22:] and len(sig) == 17
    assert [f[0] for f in L.ToadHeatWindow._fields_] == ["region", "pitch", "Hr", "Wr", "wx", "wy", "out", "out_pitch"] and ctypes.sizeof(L.ToadHeatWindow) == 48
    assert ops.HEAT_LIST_MAX == 32
    block = header[header.index("A LIST of windows"):header.index(NAME + "(")]
    for text in ("HOST array of n descriptors", "exactly as\n * toad_region_heat_window_u8 renders it", 'begins "window k:"', "Nothing is launched unless every",
                 "n == 0 launches nothing", "Canvases that overlap each other", "are the caller's business", "no allocation, no host synchronisation, no copy",
                 "ceil(n / 32) launches", "n < 0 (TOAD_EINVAL)"):
        assert text in block, text


def test_windows_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = 1 << 21                                             # non-null fake pointers: every check below comes before a device access
    odd, two = one + 1, one + 2                               # regions, mask and canvases may lie at an odd address; int32 cells may not

    # windows of a 200 x 600 image: 4 x 10 cells of 64 pixels, its 32-box mask plane (6 x 18). A 40 x 61 window at (32, 64) ends in cell row 1, column 1.
    def win(r=odd, pitch=3 * 61 + 1, hr=40, wr=61, wx=32, wy=64, out=odd, opitch=183):
        return L.ToadHeatWindow(r, pitch, hr, wr, wx, wy, out, opitch)

    def ls(*wins, n=None, c=one, gy=4, gx=10, cell=64, lut=odd, alpha=102, down=1, smooth=1, mask=odd, mpitch=19, hm=6, wm=18, md=32, mt=8, null=False):
        arr = None if null else (L.ToadHeatWindow * max(len(wins), 1))(*wins)
        return lib.toad_region_heat_windows_u8(arr, len(wins) if n is None else n, c, gy, gx, cell, lut, alpha, down, smooth, mask, mpitch, hm, wm, md, mt, None)

    good = win()
    shared = [
        (lambda: ls(good, n=-1), -1, "n = -1"), (lambda: ls(n=-5, null=True), -1, "n = -5"),
        (lambda: ls(n=1, null=True), -1, "null pointer"), (lambda: ls(n=3, null=True, cell=5), -1, "null pointer"),
        (lambda: ls(good, c=None), -1, "null pointer"), (lambda: ls(good, lut=None), -1, "null pointer"), (lambda: ls(c=None), -1, "null pointer"),
        # each shared-argument error, with the window entry's message, also in front of a bad window and with no window at all
        (lambda: ls(good, cell=12), -2, "cell = 12 is not one of 4, 8, 16, 32, 64"), (lambda: ls(cell=2), -2, "cell"),
        (lambda: ls(good, alpha=-1), -2, "alpha = -1 must lie in [0, 256]"), (lambda: ls(win(wx=3), alpha=257), -2, "alpha"),
        (lambda: ls(good, down=3), -2, "down = 3 is not one of 1, 2, 4, 8, 16, 32"), (lambda: ls(good, down=0), -2, "down"), (lambda: ls(down=64), -2, "down"),
        (lambda: ls(good, down=16, cell=8, gy=32, gx=80), -2, "down = 16 exceeds cell = 8"), (lambda: ls(win(pitch=1), down=32, cell=16, gy=16, gx=40), -2, "exceeds cell = 16"),
        (lambda: ls(good, smooth=2), -1, "smooth = 2 must be 0 or 1"), (lambda: ls(win(hr=0), smooth=-1), -1, "smooth"),
        (lambda: ls(good, md=0), -2, "mask_down = 0 is not one of"), (lambda: ls(good, md=3), -2, "mask_down"), (lambda: ls(md=64), -2, "mask_down"),
        (lambda: ls(good, down=16, md=8), -2, "mask_down = 8 is not a multiple of down = 16"), (lambda: ls(win(wx=8), down=32, md=16), -2, "multiple of down = 32"),
        (lambda: ls(good, hm=-1), -2, "Hm x Wm"), (lambda: ls(good, wm=-1), -2, "Hm x Wm"), (lambda: ls(good, mpitch=17), -2, "mask_pitch"),
        (lambda: ls(good, mt=-1), -1, "mask_thresh"), (lambda: ls(win(out=None), mt=256), -1, "mask_thresh"),
    ]
    for call, rc, text in shared:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # a bad second window: the window entry's per-window checks in its order, under "window 1:"
    second = [
        (win(r=None), -1, "null pointer"), (win(out=None), -1, "null pointer"), (win(hr=0), -2, "bad shape (Hr = 0, Wr = 61)"), (win(wr=-1, wx=3), -2, "bad shape"),
        (win(wx=30), -2, "(wx, wy) = (30, 64) is negative or not a multiple of max(4, down) = 4"), (win(wy=-4), -2, "window (wx, wy)"), (win(wx=2, pitch=1), -2, "window (wx, wy)"),
        (win(wx=(1 << 30) - 64, wr=64, pitch=192, opitch=192), -2, "2^30"),
        (win(pitch=3 * 61 - 1), -2, "pitch 182 is less than a row of the region"), (win(pitch=-184, opitch=0), -2, "pitch"),
        (win(opitch=182), -2, "out_pitch 182 is less than a row of the canvas (3 Wo = 183 bytes)"), (win(opitch=-1, wy=220), -2, "out_pitch"),
        (win(wy=220), -2, "beyond the table"), (win(wx=580), -2, "beyond the table"), (win(hr=200, wy=60), -2, "ends at cell row 5"),
    ]
    for bad, rc, text in second:
        got = ls(good, bad, good)
        msg = err()
        assert got == rc and text in msg and msg.startswith("window 1: ") and NAME in msg, (text, got, msg)
        assert ls(bad, bad) == rc and err().startswith("window 0: ")                       # the first failing window wins
        assert ls(good, bad, c=odd) == rc and err().startswith("window 1: ")               # ... and comes before the alignment of cells
    assert ls(good, win(wx=40), down=16, md=16) == -2 and "window 1: " in err() and "max(4, down) = 16" in err()
    assert ls(good, win(opitch=90), down=2, c=odd) == -4 and ls(good, win(opitch=89), down=2) == -2 and "3 Wo = 90 bytes" in err()
    # the workgroups of the whole list: two windows that pass alone do not pass together
    tall = win(hr=1 << 28, wr=16385, wx=0, wy=0, pitch=1 << 20, opitch=1 << 20)
    big = dict(gy=1 << 22, gx=257, mask=None, c=odd)
    assert ls(tall, **big) == -4 and ls(good, tall, **big) == -4
    assert ls(tall, good, tall, **big) == -2 and "workgroups" in err() and err().startswith(NAME + ":")
    # cells: 4-byte aligned, the last check
    for c in (odd, two):
        assert ls(good, good, c=c) == -4 and "4-byte aligned" in err() and err().startswith(NAME + ":")
    # what is taken: only the alignment check stops these calls
    for wins, ok in (((good,), {}), ((good, win(wx=0, wy=0), win(hr=200, wr=600, wx=0, wy=0, pitch=1800, opitch=1800)), {}), ((good,), dict(smooth=0)),
                     ((good,), dict(hm=0, wm=0, mpitch=0)), ((good,), dict(mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999)), ((good,), dict(alpha=0)), ((good,), dict(alpha=256)),
                     ((win(wx=64), win(wx=32, wy=32)), dict(down=32, opitch=None)), ((good,) * 40, {}), ((good,), dict(cell=4, gy=50, gx=150)),
                     ((good,), dict(down=8, cell=8, gy=25, gx=75))):
        ok.pop("opitch", None)
        assert ls(*wins, c=odd, **ok) == -4, ok
    # n == 0 launches nothing, and neither does a list whose windows are all empty: everything is checked, TOAD_OK (no device is present here)
    assert ls() == 0 and ls(n=0, null=True) == 0 and ls(good, n=0) == 0
    assert ls(win(hr=15), win(wr=15, pitch=45), win(hr=1, wr=1, pitch=3), down=16) == 0
    assert ls(win(hr=15), win(hr=15, wx=8), down=16) == -2 and err().startswith("window 1: ")      # an empty window is checked like any other
    assert ls(win(hr=15), down=16, c=odd) == -4


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------------------
def test_windows_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded. The messages name the window."""
    from toad_amd import _lib as L, ops
    from toad_amd.heatmap import windows_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_windows([cpu], [(0, 0)], torch.zeros(8, 8, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, 1)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    # real (host) tensors, which have addresses; is_cuda is patched, so the checks run as they do on the device. A slide tensor is "another device".
    slide = torch.zeros(128, 128, 3, dtype=torch.uint8)
    other = torch.zeros(80, 112, 3, dtype=torch.uint8, device="meta")
    cells, lut = torch.zeros(8, 8, dtype=torch.int32), torch.zeros(256, 3, dtype=torch.uint8)
    m8 = torch.zeros(8, 8, dtype=torch.uint8)
    canv = lambda h, w: torch.zeros(h, w, 3, dtype=torch.uint8)      # noqa: E731
    a, b = slide[:48, :80], slide[48:, 16:]                           # 48 x 80 at (0, 0) and 80 x 112 at (16, 48)
    base = dict(regions=[a, b], windows=[(0, 0), (16, 48)], cells=cells, cell=16, lut=lut, alpha=102, down=1)
    for k, text in ((dict(windows=[(0, 0)]), "2 regions but 1 windows"), (dict(regions=[a]), "1 regions but 2 windows"), (dict(regions=slide), "regions must be a sequence"),
                    (dict(windows=5), "windows must be a sequence"), (dict(outs=[canv(48, 80)]), "sequence of 2 canvases"), (dict(outs=canv(48, 80)), "sequence of 2 canvases"),
                    (dict(regions=[a, other]), "window 1: every region must be on one device"), (dict(lut=torch.zeros(256, 3, dtype=torch.uint8, device="meta")), "lut"),
                    (dict(smooth=2), "smooth must be False or True"), (dict(smooth="yes"), "smooth"), (dict(cell=12), "cell"), (dict(alpha=257), "alpha"), (dict(down=3), "down must be one of"),
                    (dict(down=32), "exceeds cell = 16"),
                    (dict(windows=[(0, 0), (18, 48)]), r"window 1: window \(wx, wy\) = \(18, 48\)"), (dict(windows=[(0,), (16, 48)]), "window 0: window must be"),
                    (dict(windows=[(0, 0), (16, 56)], down=16), r"window 1: .*max\(4, down\) = 16"), (dict(windows=[(0, 0), (32, 48)]), "window 1: the window ends at cell row 8 and cell column 9"),
                    (dict(regions=[a, slide[:, ::2]]), "window 1: expected a uint8"), (dict(regions=[a.float(), b]), "window 0"),
                    (dict(outs=[canv(48, 80), canv(80, 111)]), r"window 1: outs\[1\] must be a uint8 \[80,112,3\]"),
                    (dict(outs=[canv(24, 40), canv(40, 56)]), r"window 0: outs\[0\] must be a uint8 \[48,80,3\]"),
                    (dict(outs=[canv(24, 40), canv(40, 112)[:, ::2]], down=2), r"window 1: outs\[1\] must have strides"),
                    (dict(mask_down=16), "without a mask"), (dict(mask=m8), "mask_down"), (dict(mask=m8, mask_down=8, down=16), "multiple of down = 16"),
                    (dict(mask=m8, mask_down=16, mask_thresh=256), "mask_thresh")):
        args = dict(base)
        args.update(k)
        with pytest.raises((ValueError, TypeError), match=text):
            ops.region_heat_windows(**args)
    rc, rl = cells, lut
    with pytest.raises(ValueError, match=r"window 1: outs\[1\] must not share storage with region"):
        ops.region_heat_windows([slide[:48], slide[48:]], [(0, 0), (0, 48)], rc, 16, rl, 102, 1, outs=[torch.zeros(48, 128, 3, dtype=torch.uint8), slide[:80]])
    canvas = torch.zeros(128, 128, 3, dtype=torch.uint8)             # views of ONE canvas are taken: only now is the library reached
    for outs in (None, [canvas[:48], canvas[48:]]):
        with pytest.raises(AssertionError, match="library was reached"):
            ops.region_heat_windows([slide[:48], slide[48:]], [(0, 0), (0, 48)], rc, 16, rl, 102, 1, outs=outs)
    # an empty list and a list of empty canvases launch nothing; an empty plane is no plane
    assert ops.region_heat_windows([], [], cells, 16, lut, 102, 4) == ()
    got = ops.region_heat_windows([slide[:3], slide[:7, 16:]], [(0, 0), (16, 0)], cells, 16, lut, 102, 8, mask=m8[:0], mask_down=16)
    assert [tuple(g.shape) for g in got] == [(0, 16, 3), (0, 14, 3)]
    with pytest.raises(AssertionError, match="library was reached"):
        ops.region_heat_windows([slide[:3], b], [(0, 0), (16, 48)], cells, 16, lut, 102, 8, mask=m8, mask_down=32)
    for k, text in ((dict(alpha=1.5), "alpha"), (dict(smooth=1), "bool"), (dict(mask=(m8, 8)), "triple"), (dict(windows=[(0, 0), (18, 48)]), "window 1"),
                    (dict(windows=[(0, 0)]), "2 regions but 1 windows"), (dict(down=32), "exceeds cell"), (dict(mask=(m8, 8, 8), down=16), "multiple of down = 16"),
                    (dict(outs=[canv(48, 80)]), "sequence of 2 canvases")):
        with pytest.raises(ValueError, match=text):
            windows_canvas([a, b], k.pop("windows", [(0, 0), (16, 48)]), cells, 16, lut=lut, **k)


def _logger(log, name, result):
    def f(*a, **k):
        log.append((name, a, k))
        return result(*a, **k)
    return f


def test_slide_attention_heatmap_batch_render_makes_one_windows_call(monkeypatch):
    from toad_amd import eval as E, ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    log = []
    monkeypatch.setattr(ops, "region_heat_window", _logger(log, "region_heat_window", lambda *a, **k: k["out"]))
    monkeypatch.setattr(ops, "region_heat_windows", _logger(log, "region_heat_windows", lambda *a, **k: tuple(k["outs"])))
    monkeypatch.setattr(ops, "region_heat_pyramid", _logger(log, "region_heat_pyramid", lambda *a, **k: tuple(k["outs"])))
    hs, ws = 256, 512
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    spans = [(0, 112), (64, 144), (176, 80)]
    renders = ((0, 112), (112, 208), (208, 256))
    strips = [(slide[y:y + n], y) for y, n in spans]
    none = np.zeros((0, 2), dtype=np.int64)
    kw = dict(tile=64, stride=64, origins=none, smooth=True, alpha=0.5)
    for down in (1, 2, 4, 8, 16):                                     # (seams at 112 and 208: 32 is refused by strip_plan either way)
        del log[:]
        o, s, canvas = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=down, batch_render=True, **kw)
        assert o.shape == (0, 2) and s.shape == (0,) and isinstance(canvas, torch.Tensor) and tuple(canvas.shape) == (hs // down, ws // down, 3)
        assert [n for n, _, _ in log] == ["region_heat_windows"]     # exactly one call
        _, a, k = log[0]
        assert [tuple(r.shape) for r in a[0]] == [(r1 - r0, ws, 3) for r0, r1 in renders] and list(a[1]) == [(0, r0) for r0, _ in renders]
        assert tuple(a[2].shape) == (4, 8) and a[3] == 64 and a[5] == 128 and a[6] == down and k["smooth"] is True and k["mask"] is None
        assert [tuple(v.shape) for v in k["outs"]] == [((r1 - r0) // down, ws // down, 3) for r0, r1 in renders]
        assert all(v.untyped_storage()._cdata == canvas.untyped_storage()._cdata for v in k["outs"])      # views of the one canvas
        # without it: the window_canvas calls it made before, argument for argument
        del log[:]
        for extra in ({}, dict(batch_render=False)):
            o, s, canvas = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=down, **kw, **extra)
            assert tuple(canvas.shape) == (hs // down, ws // down, 3)
        assert [n for n, _, _ in log] == ["region_heat_window"] * 6
        for (_, a, k), (r0, r1) in zip(log, renders * 2):
            assert tuple(a[0].shape) == (r1 - r0, ws, 3) and a[1] == (0, r0) and tuple(a[2].shape) == (4, 8) and a[3] == 64 and a[5] == 128 and a[6] == down
            assert k["smooth"] is True and k["mask"] is None and tuple(k["out"].shape) == ((r1 - r0) // down, ws // down, 3)
    # the caller's canvas is the one that is filled
    out = torch.zeros(hs // 4, ws // 4, 3, dtype=torch.uint8, device="meta")
    assert E.slide_attention_heatmap(None, None, strips, (hs, ws), down=4, out=out, batch_render=True, **kw)[2] is out
    del log[:]
    for bad, text in ((dict(down=(1, 4), batch_render=True), "batch_render=True takes one down"), (dict(down=[16], batch_render=True), "batch_render=True takes one down"),
                      (dict(batch_render=1), "batch_render must be a bool"), (dict(down=32, batch_render=True), r"max\(4, down\) = 32"),
                      (dict(down=4, batch_render=True, out=slide), "out must be a uint8")):
        with pytest.raises(ValueError, match=text):
            E.slide_attention_heatmap(None, None, strips, (hs, ws), **dict(kw, **bad))
    assert not log
    # a sequence of levels without batch_render is the pyramid walk it was
    E.slide_attention_heatmap(None, None, strips, (hs, ws), down=(1, 16), **kw)
    assert [n for n, _, _ in log] == ["region_heat_pyramid"] * 3
