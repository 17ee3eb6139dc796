"""CPU: several pyramid levels for a list of windows of one slide in one call (toad_region_heat_pyramid_windows_u8: an additive extension of ABI 15;
ops.region_heat_pyramid_windows, heatmap.windows_pyramid, eval.slide_attention_heatmap(batch_levels=True)). The entry point exists in the header, the
library and the ctypes table and refuses what the host can see before any device access - the shared arguments first, in the pyramid entry's order and
with its messages, then window by window under "window k:"; a level that is empty for a window needs no canvas there; the Python layers refuse before
the library is loaded; and slide_attention_heatmap without batch_levels calls what it called."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NAME = "toad_region_heat_pyramid_windows_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pyramid_windows_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L, ops
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+ToadHeatPyramidWindow\s*\*", header), f"{NAME} is not declared in include/toad_hip.h"
    assert re.search(r"typedef\s+struct\s*\{\s*const unsigned char \*region; int64_t pitch; int Hr, Wr, wx, wy;\s*unsigned char \*outs\[6\]; "
                     r"int64_t out_pitches\[6\];\s*\}\s*ToadHeatPyramidWindow;", header)
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES
    sig, ws, py = L.SIGNATURES[NAME][1], L.SIGNATURES["toad_region_heat_windows_u8"][1], L.SIGNATURES["toad_region_heat_pyramid_u8"][1]
    # the windows entry's arguments with the pyramid entry's `levels` where `down` stood
    assert sig[0] == ctypes.POINTER(L.ToadHeatPyramidWindow) and sig[1:8] == ws[1:8] and sig[8] == py[12] == ctypes.c_uint and sig[9:] == ws[9:] and len(sig) == 17
    assert [f[0] for f in L.ToadHeatPyramidWindow._fields_] == ["region", "pitch", "Hr", "Wr", "wx", "wy", "outs", "out_pitches"]
    assert ctypes.sizeof(L.ToadHeatPyramidWindow) == 8 + 8 + 4 * 4 + 6 * 8 + 6 * 8 == 128
    assert ops.HEAT_PYR_LIST_MAX == 16
    block = header[header.index("Several levels for a LIST of windows"):header.index(NAME + "(")]
    for text in ("HOST array of n descriptors", "byte for byte what the\n * pyramid call writes", 'begins "window k:"', "Nothing is launched unless every",
                 "n == 0 launches nothing", "outs[k] may be NULL", "are the caller's business", "no allocation, no host synchronisation, no copy",
                 "ceil(n / 16) launches", "n < 0 (TOAD_EINVAL)", "With ONE level this\n * is the list call above"):
        assert text in block, text
    # the gap is no longer named as not done
    assert "Not done: several levels for a list" not in header


def test_pyramid_windows_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = 1 << 21                                             # non-null fake pointers: every check below comes before a device access
    odd, two = one + 1, one + 2                               # regions, mask and canvases may lie at an odd address; int32 cells may not

    # windows of a 200 x 600 image: 4 x 10 cells of 64 pixels, its 32-box mask plane (6 x 18), levels 1, 4 and 16. A 40 x 61 window at (32, 64) ends in
    # cell row 1, column 1; its canvases are 61, 30, 15, 7, 3 and 1 pixels wide.
    def win(r=odd, pitch=3 * 61 + 1, hr=40, wr=61, wx=32, wy=64, outs=(odd,) * 6, pitches=(183, 90, 45, 21, 9, 3), **one_level):
        w = L.ToadHeatPyramidWindow(r, pitch, hr, wr, wx, wy)
        for j in range(6):
            w.outs[j], w.out_pitches[j] = outs[j], pitches[j]
        for key, v in one_level.items():                      # o2=None, p2=44: level 2's canvas and pitch
            if key[0] == "o":
                w.outs[int(key[1])] = v
            else:
                w.out_pitches[int(key[1])] = v
        return w

    def ls(*wins, n=None, c=one, gy=4, gx=10, cell=64, lut=odd, alpha=102, levels=0b10101, smooth=1, mask=odd, mpitch=19, hm=6, wm=18, md=32, mt=8, null=False):
        arr = None if null else (L.ToadHeatPyramidWindow * max(len(wins), 1))(*wins)
        return lib.toad_region_heat_pyramid_windows_u8(arr, len(wins) if n is None else n, c, gy, gx, cell, lut, alpha, levels, smooth, mask, mpitch, hm, wm, md, mt, None)

    good = win()
    c4 = dict(cell=4, gy=50, gx=150)
    shared = [
        (lambda: ls(good, n=-1), -1, "n = -1"), (lambda: ls(n=-5, null=True), -1, "n = -5"),
        (lambda: ls(n=1, null=True), -1, "null pointer"), (lambda: ls(n=3, null=True, cell=5), -1, "null pointer"),
        (lambda: ls(good, c=None), -1, "null pointer"), (lambda: ls(good, lut=None), -1, "null pointer"), (lambda: ls(c=None), -1, "null pointer"),
        # each shared-argument error, with the pyramid entry's message, also in front of a bad window and with no window at all
        (lambda: ls(good, cell=12), -2, "cell = 12 is not one of 4, 8, 16, 32, 64"), (lambda: ls(cell=2), -2, "cell"), (lambda: ls(win(r=None), cell=3), -2, "cell"),
        (lambda: ls(good, alpha=-1), -2, "alpha = -1 must lie in [0, 256]"), (lambda: ls(win(wx=3), alpha=257), -2, "alpha"), (lambda: ls(alpha=300), -2, "alpha"),
        (lambda: ls(good, levels=0), -2, "levels = 0x0 is not a non-empty set of bits 0 .. 5"), (lambda: ls(win(hr=0), levels=64), -2, "levels = 0x40"),
        (lambda: ls(levels=0), -2, "levels"), (lambda: ls(levels=1 << 6 | 1), -2, "levels"),
        (lambda: ls(good, levels=0b10001, cell=8, gy=32, gx=80), -2, "down = 16, the largest level, exceeds cell = 8"),
        (lambda: ls(win(pitch=1), levels=0b100001, cell=16, gy=16, gx=40), -2, "down = 32, the largest level, exceeds cell = 16"), (lambda: ls(levels=0b11000, cell=8), -2, "exceeds cell = 8"),
        (lambda: ls(good, smooth=2), -1, "smooth = 2 must be 0 or 1"), (lambda: ls(win(hr=0), smooth=-1), -1, "smooth"), (lambda: ls(smooth=7), -1, "smooth"),
        (lambda: ls(good, levels=0b101, **c4), -2, "smooth at cell = 4 is not done for more than one level"), (lambda: ls(win(wx=3), levels=0b11, **c4), -2, "smooth at cell = 4"),
        (lambda: ls(levels=0b110, **c4), -2, "smooth at cell = 4"),
        (lambda: ls(good, md=0), -2, "mask_down = 0 is not one of"), (lambda: ls(good, md=3), -2, "mask_down"), (lambda: ls(md=64), -2, "mask_down"),
        (lambda: ls(good, md=8), -2, "mask_down = 8 is not a multiple of down = 16, the largest level"), (lambda: ls(win(wx=8), levels=0b100001, md=16), -2, "multiple of down = 32"),
        (lambda: ls(levels=0b1100, md=4), -2, "multiple of down = 8"),
        (lambda: ls(good, hm=-1), -2, "Hm x Wm"), (lambda: ls(good, wm=-1), -2, "Hm x Wm"), (lambda: ls(good, mpitch=17), -2, "mask_pitch"), (lambda: ls(mpitch=17), -2, "mask_pitch"),
        (lambda: ls(good, mt=-1), -1, "mask_thresh"), (lambda: ls(win(o0=None), mt=256), -1, "mask_thresh"), (lambda: ls(mt=256), -1, "mask_thresh"),
    ]
    for call, rc, text in shared:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # a bad second window: the pyramid entry's per-window checks in its order, under "window 1:"
    second = [
        (win(r=None), -1, "null pointer"), (win(o2=None), -1, "null pointer (outs[2], the canvas of down = 4)"), (win(o0=None, pitch=1), -1, "outs[0], the canvas of down = 1"),
        (win(o4=None, wx=3), -1, "outs[4], the canvas of down = 16"),
        (win(hr=0), -2, "bad shape (Hr = 0, Wr = 61)"), (win(wr=-1, wx=3), -2, "bad shape"), (win(hr=0, o0=None, o2=None, o4=None), -2, "bad shape"),
        (win(wx=40), -2, "(wx, wy) = (40, 64) is negative or not a multiple of max(4, down) = 16, down the largest level"), (win(wy=-16), -2, "window (wx, wy)"),
        (win(wy=72, pitch=1), -2, "window (wx, wy)"),
        (win(wx=(1 << 30) - 64, wr=64, pitch=192, pitches=(192,) * 6), -2, "2^30"),
        (win(pitch=3 * 61 - 1), -2, "pitch 182 is less than a row of the region"), (win(pitch=-184, p0=0), -2, "pitch"),
        (win(p2=44), -2, "out_pitches[2] = 44 is less than a row of the canvas of down = 4 (3 Wo = 45 bytes)"), (win(p0=182), -2, "out_pitches[0] = 182"),
        (win(p4=8, wy=224), -2, "out_pitches[4] = 8 is less than a row of the canvas of down = 16 (3 Wo = 9 bytes)"),
        (win(wy=224), -2, "beyond the table"), (win(wx=592), -2, "beyond the table"), (win(hr=200, wy=64), -2, "ends at cell row 5"),
    ]
    for bad, rc, text in second:
        got = ls(good, bad, good)
        msg = err()
        assert got == rc and text in msg and msg.startswith("window 1: ") and NAME in msg, (text, got, msg)
        assert ls(bad, bad) == rc and err().startswith("window 0: ")                       # the first failing window wins
        assert ls(good, bad, c=odd) == rc and err().startswith("window 1: ")               # ... and comes before the alignment of cells
    # levels that were not asked for have no canvas: nothing of theirs is looked at
    assert ls(good, win(o1=None, o3=None, o5=None, p1=-1, p3=0, p5=-9), c=odd) == -4
    # a null outs[j] is accepted exactly where level j is empty for THIS window: 12 rows have no level 16, 3 rows no level 4 either; their pitches are not looked at
    assert ls(good, win(hr=12, o4=None, p4=-5), c=odd) == -4
    assert ls(good, win(hr=12, o2=None), c=odd) == -1 and "window 1: " in err() and "outs[2]" in err()
    assert ls(good, win(hr=3, o2=None, o4=None, p2=0, p4=0), c=odd) == -4 and ls(good, win(hr=3, o0=None, o2=None, o4=None), c=odd) == -1 and "outs[0]" in err()
    assert ls(win(wr=15, pitch=45, o4=None, p4=-1), good, c=odd) == -4 and ls(win(wr=16, pitch=48, o4=None), good, c=odd) == -1 and err().startswith("window 0: ")
    assert ls(good, win(hr=12, o4=None, p2=8), c=odd) == -2 and "out_pitches[2] = 8" in err()      # the levels that are not empty are still checked
    # ONE level is the windows entry for that down: its messages, and a canvas only where the window has one
    assert ls(good, win(wx=30), levels=0b100, md=4) == -2 and "window 1: " in err() and "max(4, down) = 4" in err() and NAME in err()
    assert ls(good, win(p2=44), levels=0b100) == -2 and "out_pitch 44 is less than a row of the canvas (3 Wo = 45 bytes)" in err() and err().startswith("window 1: ")
    assert ls(good, win(o2=None), levels=0b100) == -1 and "window 1: " in err() and "null pointer" in err()
    assert ls(good, win(hr=3, o2=None, p2=-1), levels=0b100, c=odd) == -4 and ls(good, win(hr=3, o2=None, wx=30), levels=0b100) == -2 and "window 1: " in err()
    assert ls(good, levels=0b100, md=2) == -2 and "mask_down = 2 is not a multiple of down = 4" in err() and err().startswith(NAME + ":")
    assert ls(good, levels=0b100, c=odd, **c4) == -4                                       # smooth at cell 4 is done for one level
    # the workgroups of the whole list: two windows that pass alone do not pass together
    tall = win(hr=1 << 28, wr=16385, wx=0, wy=0, pitch=1 << 20, pitches=(1 << 20,) * 6)
    big = dict(gy=1 << 22, gx=257, mask=None, c=odd, levels=0b101)
    assert ls(tall, **big) == -4 and ls(good, tall, **big) == -4
    assert ls(tall, good, tall, **big) == -2 and "workgroups" in err() and err().startswith(NAME + ":")
    # cells: 4-byte aligned, the last check
    for c in (odd, two):
        assert ls(good, good, c=c) == -4 and "4-byte aligned" in err() and err().startswith(NAME + ":")
    # what is taken: only the alignment check stops these calls
    for wins, ok in (((good,), {}), ((good, win(wx=0, wy=0), win(hr=200, wr=600, wx=0, wy=0, pitch=1800, pitches=(1800, 900, 450, 225, 111, 54))), {}), ((good,), dict(smooth=0)),
                     ((good,), dict(hm=0, wm=0, mpitch=0)), ((good,), dict(mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999)), ((good,), dict(alpha=0)), ((good,), dict(alpha=256)),
                     ((win(wx=64), win(wx=32, wy=32)), dict(levels=0b111111)), ((good,) * 40, {}), ((good,), dict(levels=0b111, smooth=0, **c4)),
                     ((good,), dict(levels=0b1001, cell=8, gy=25, gx=75))):
        assert ls(*wins, c=odd, **ok) == -4, ok
    # n == 0 launches nothing, and neither does a list whose canvases are all empty: everything is checked, TOAD_OK (no device is present here)
    assert ls() == 0 and ls(n=0, null=True) == 0 and ls(good, n=0) == 0
    none = dict(o2=None, o4=None, p2=-1, p4=-1)
    assert ls(win(hr=3, **none), win(wr=3, pitch=9, **none), win(hr=1, wr=1, pitch=3, **none), levels=0b10100) == 0
    assert ls(win(hr=3, **none), win(hr=3, wx=8, **none), levels=0b10100) == -2 and err().startswith("window 1: ")      # an empty window is checked like any other
    assert ls(win(hr=3, **none), levels=0b10100, c=odd) == -4
    assert ls(win(hr=3, o2=None), levels=0b100) == 0 and ls(win(hr=3, o2=None), levels=0b100, c=odd) == -4      # ... and with one level


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pyramid_windows_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded. The messages name the window."""
    from toad_amd import _lib as L, ops
    from toad_amd.heatmap import windows_pyramid

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_pyramid_windows([cpu], [(0, 0)], torch.zeros(8, 8, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, (1, 4))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    # real (host) tensors, which have addresses; is_cuda is patched, so the checks run as they do on the device. A meta tensor is "another device".
    slide = torch.zeros(128, 128, 3, dtype=torch.uint8)
    other = torch.zeros(80, 112, 3, dtype=torch.uint8, device="meta")
    cells, lut = torch.zeros(8, 8, dtype=torch.int32), torch.zeros(256, 3, dtype=torch.uint8)
    m8 = torch.zeros(8, 8, dtype=torch.uint8)
    canv = lambda h, w: torch.zeros(h, w, 3, dtype=torch.uint8)      # noqa: E731
    a, b = slide[:48, :80], slide[48:, 16:]                           # 48 x 80 at (0, 0) and 80 x 112 at (16, 48)
    base = dict(regions=[a, b], windows=[(0, 0), (16, 48)], cells=cells, cell=16, lut=lut, alpha=102, downs=(1, 4))
    ok_a, ok_b = [canv(48, 80), canv(12, 20)], [canv(80, 112), canv(20, 28)]
    both = canv(48, 80)
    for k, text in ((dict(windows=[(0, 0)]), "2 regions but 1 windows"), (dict(regions=[a]), "1 regions but 2 windows"), (dict(regions=slide), "regions must be a sequence"),
                    (dict(windows=5), "windows must be a sequence"), (dict(outs=[ok_a]), "sequence of 2 sequences of 2 canvases"), (dict(outs=canv(48, 80)), "sequence of 2 sequences"),
                    (dict(outs=[ok_a, ok_b[:1]]), r"window 1: outs\[1\] must be a sequence of 2 canvases"), (dict(outs=[ok_a[0], ok_b]), r"window 0: outs\[0\] must be a sequence"),
                    (dict(downs=()), "downs must be a non-empty sequence"), (dict(downs=(1, 1)), "distinct"), (dict(downs=(1, 3)), "downs"), (dict(downs=4), "downs"),
                    (dict(regions=[a, other]), "window 1: every region must be on one device"), (dict(lut=torch.zeros(256, 3, dtype=torch.uint8, device="meta")), "lut"),
                    (dict(smooth=2), "smooth must be False or True"), (dict(smooth="yes"), "smooth"), (dict(cell=12), "cell"), (dict(alpha=257), "alpha"),
                    (dict(downs=(1, 32)), "down = 32, the largest level, exceeds cell = 16"),
                    (dict(smooth=True, cell=4, cells=torch.zeros(32, 32, dtype=torch.int32)), "smooth at cell = 4 is not done for more than one level"),
                    (dict(windows=[(0, 0), (18, 48)]), r"window 1: window \(wx, wy\) = \(18, 48\)"), (dict(windows=[(0,), (16, 48)]), "window 0: window must be"),
                    (dict(windows=[(0, 0), (16, 56)], downs=(2, 16)), r"window 1: .*max\(4, down\) = 16"),
                    (dict(windows=[(0, 0), (32, 48)]), "window 1: the window ends at cell row 8 and cell column 9"),
                    (dict(regions=[a, slide[:, ::2]]), "window 1: expected a uint8"), (dict(regions=[a.float(), b]), "window 0"),
                    (dict(outs=[ok_a, [canv(80, 112), canv(20, 27)]]), r"window 1: outs\[1\]\[1\] \(down = 4\) must be a uint8 \[20,28,3\]"),
                    (dict(outs=[[canv(24, 40), canv(12, 20)], ok_b]), r"window 0: outs\[0\]\[0\] \(down = 1\) must be a uint8 \[48,80,3\]"),
                    (dict(outs=[ok_a, [canv(80, 112), canv(20, 56)[:, ::2]]]), r"window 1: outs\[1\]\[1\] \(down = 4\) must have strides"),
                    (dict(outs=[[both, both[:12, :20]], ok_b]), r"window 0: outs\[0\]\[0\] and outs\[0\]\[1\] must not share storage"),
                    (dict(mask_down=16), "without a mask"), (dict(mask=m8), "mask_down"), (dict(mask=m8, mask_down=8, downs=(1, 16)), "multiple of down = 16"),
                    (dict(mask=m8, mask_down=16, mask_thresh=256), "mask_thresh")):
        args = dict(base)
        args.update(k)
        with pytest.raises((ValueError, TypeError), match=text):
            ops.region_heat_pyramid_windows(**args)
    with pytest.raises(ValueError, match=r"window 1: outs\[1\]\[1\] \(down = 4\) must not share storage with region"):
        ops.region_heat_pyramid_windows([slide[:48], slide[48:]], [(0, 0), (0, 48)], cells, 16, lut, 102, (1, 4), outs=[[canv(48, 128), canv(12, 32)], [canv(80, 128), slide[:20, :32]]])
    c1, c4 = torch.zeros(128, 128, 3, dtype=torch.uint8), torch.zeros(32, 32, 3, dtype=torch.uint8)
    # across windows the canvases are views of ONE canvas per level: taken, and only now is the library reached
    for outs in (None, [[c1[:48], c4[:12]], [c1[48:], c4[12:]]]):
        with pytest.raises(AssertionError, match="library was reached"):
            ops.region_heat_pyramid_windows([slide[:48], slide[48:]], [(0, 0), (0, 48)], cells, 16, lut, 102, (1, 4), outs=outs)
    # an empty list and a list of empty canvases launch nothing; an empty plane is no plane; the tuples have the order of downs
    assert ops.region_heat_pyramid_windows([], [], cells, 16, lut, 102, (4, 1)) == ()
    got = ops.region_heat_pyramid_windows([slide[:3], slide[:7, 16:]], [(0, 0), (16, 0)], cells, 16, lut, 102, (16, 8), mask=m8[:0], mask_down=16)
    assert [[tuple(g.shape) for g in w] for w in got] == [[(0, 8, 3), (0, 16, 3)], [(0, 7, 3), (0, 14, 3)]]
    with pytest.raises(AssertionError, match="library was reached"):                      # one window empty at level 8, the other not: the call is made
        ops.region_heat_pyramid_windows([slide[:3], b], [(0, 0), (16, 48)], cells, 16, lut, 102, (16, 8), mask=m8, mask_down=32)
    for k, text in ((dict(alpha=1.5), "alpha"), (dict(smooth=1), "bool"), (dict(mask=(m8, 8)), "triple"), (dict(windows=[(0, 0), (18, 48)]), "window 1"),
                    (dict(windows=[(0, 0)]), "2 regions but 1 windows"), (dict(downs=(1, 32)), "exceeds cell"), (dict(mask=(m8, 8, 8), downs=(4, 16)), "multiple of down = 16"),
                    (dict(outs=[ok_a]), "sequence of 2 sequences")):
        with pytest.raises(ValueError, match=text):
            windows_pyramid([a, b], k.pop("windows", [(0, 0), (16, 48)]), cells, 16, lut=lut, **dict(dict(downs=(1, 4)), **k))


def _logger(log, name, result):
    def f(*a, **k):
        log.append((name, a, k))
        return result(*a, **k)
    return f


def test_slide_attention_heatmap_batch_levels_makes_one_pyramid_windows_call(monkeypatch):
    from toad_amd import eval as E, ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    log = []
    monkeypatch.setattr(ops, "region_heat_window", _logger(log, "region_heat_window", lambda *a, **k: k["out"]))
    monkeypatch.setattr(ops, "region_heat_windows", _logger(log, "region_heat_windows", lambda *a, **k: tuple(k["outs"])))
    monkeypatch.setattr(ops, "region_heat_pyramid", _logger(log, "region_heat_pyramid", lambda *a, **k: tuple(k["outs"])))
    monkeypatch.setattr(ops, "region_heat_pyramid_windows", _logger(log, "region_heat_pyramid_windows", lambda *a, **k: tuple(tuple(o) for o in k["outs"])))
    hs, ws = 256, 512
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    spans = [(0, 112), (64, 144), (176, 80)]
    renders = ((0, 112), (112, 208), (208, 256))
    strips = [(slide[y:y + n], y) for y, n in spans]
    none = np.zeros((0, 2), dtype=np.int64)
    kw = dict(tile=64, stride=64, origins=none, smooth=True, alpha=0.5)
    for downs in ((1, 4, 16), [16, 2], (8,)):                         # (seams at 112 and 208: 32 is refused by strip_plan either way)
        del log[:]
        o, s, canvases = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=downs, batch_levels=True, **kw)
        assert o.shape == (0, 2) and s.shape == (0,) and isinstance(canvases, dict) and list(canvases) == list(downs)
        assert all(tuple(canvases[d].shape) == (hs // d, ws // d, 3) for d in downs)
        assert [n for n, _, _ in log] == ["region_heat_pyramid_windows"]      # exactly one call
        _, a, k = log[0]
        assert [tuple(r.shape) for r in a[0]] == [(r1 - r0, ws, 3) for r0, r1 in renders] and list(a[1]) == [(0, r0) for r0, _ in renders]
        assert tuple(a[2].shape) == (4, 8) and a[3] == 64 and a[5] == 128 and tuple(a[6]) == tuple(downs) and k["smooth"] is True and k["mask"] is None
        assert len(k["outs"]) == 3
        for views, (r0, r1) in zip(k["outs"], renders):
            assert [tuple(v.shape) for v in views] == [((r1 - r0) // d, ws // d, 3) for d in downs]
            assert all(v.untyped_storage()._cdata == canvases[d].untyped_storage()._cdata for v, d in zip(views, downs))      # views of the per-level canvases
            assert all(v.storage_offset() == (r0 // d) * canvases[d].stride(0) for v, d in zip(views, downs))               # ... at the strip's own rows
        # without it: the three region_heat_pyramid calls it made before, argument for argument
        del log[:]
        for extra in ({}, dict(batch_levels=False)):
            o, s, canvases = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=downs, **kw, **extra)
            assert list(canvases) == list(downs)
        assert [n for n, _, _ in log] == ["region_heat_pyramid"] * 6
        for (_, a, k), (r0, r1) in zip(log, renders * 2):
            assert tuple(a[0].shape) == (r1 - r0, ws, 3) and a[1] == (0, r0) and tuple(a[2].shape) == (4, 8) and a[3] == 64 and a[5] == 128 and tuple(a[6]) == tuple(downs)
            assert k["smooth"] is True and k["mask"] is None and [tuple(v.shape) for v in k["outs"]] == [((r1 - r0) // d, ws // d, 3) for d in downs]
    # the caller's canvases are the ones that are filled
    out = {d: torch.zeros(hs // d, ws // d, 3, dtype=torch.uint8, device="meta") for d in (4, 16)}
    got = E.slide_attention_heatmap(None, None, strips, (hs, ws), down=(4, 16), out=out, batch_levels=True, **kw)[2]
    assert all(got[d] is out[d] for d in (4, 16))
    del log[:]
    for bad, text in ((dict(down=4, batch_levels=True), "batch_levels=True takes a sequence of levels.*batch_render"), (dict(batch_levels=True), "batch_levels=True takes a sequence"),
                      (dict(down=(1, 4), batch_levels=1), "batch_levels must be a bool"), (dict(batch_levels=None), "batch_levels must be a bool"),
                      (dict(down=(1, 4), batch_render=True), "batch_render=True takes one down.*batch_levels"),
                      (dict(down=(1, 4), batch_render=True, batch_levels=True), "batch_render=True takes one down"),
                      (dict(down=(1, 32), batch_levels=True), r"max\(4, down\) = 32"), (dict(down=(4, 16), batch_levels=True, out=slide), "out must be None or a dict"),
                      (dict(down=(4, 16), batch_levels=True, out={4: slide, 16: slide}), r"out\[4\] must be a uint8")):
        with pytest.raises(ValueError, match=text):
            E.slide_attention_heatmap(None, None, strips, (hs, ws), **dict(kw, **bad))
    assert not log
    # one down without either switch is the window walk it was
    E.slide_attention_heatmap(None, None, strips, (hs, ws), down=4, **kw)
    assert [n for n, _, _ in log] == ["region_heat_window"] * 3
