"""CPU: heat maps rendered window by window (toad_region_heat_window_u8: an additive extension of ABI 15; ops.region_heat_window, heatmap.slide_cells,
heatmap.window_canvas, heatmap.strip_plan, eval.slide_attention_heatmap). The entry point exists in the header, the library and the ctypes table and
refuses what the host can see before any device access, while the three older entries refuse what they refused; the windowed reference the GPU tests
compare against (tests/heat_window_ref.py) equals the matching slice of tests/heat_px_ref.py's whole-image canvas; strip_plan against a brute-force
statement of what it promises; and attention_canvas is still slide_cells plus the blend."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import heat_px_ref as ref, heat_window_ref as wref

NAME = "toad_region_heat_window_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOWNS = (1, 2, 4, 8, 16, 32)


def test_window_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header), f"{NAME} is not declared in include/toad_hip.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 23
    px = L.SIGNATURES["toad_region_heat_blend_px_u8"][1]
    assert L.SIGNATURES[NAME][1] == px[:4] + [ctypes.c_int, ctypes.c_int] + px[4:]              # wx, wy after Hr, Wr; the rest in the same order
    block = header[header.index("toad_region_heat_thumb_u8("):header.index(NAME + "(")]
    for text in ("(wx, wy)", "X = down * ox + wx and Y = down * oy + wy", "own = cells[Y / cell][X / cell]", "p = 2 * X + down - cell",
                 "outside the table or without a value counts as `own`", "mx = X / mask_down < Wm, my = Y / mask_down < Hm", "multiple of max(4, down)",
                 "wx + Wr >= 2^30", "ceil((wy + Hr) / cell) > Gy or ceil((wx + Wr) / cell) > Gx", "down not in {1, 2, 4, 8, 16, 32}"):
        assert text in block, text


def test_window_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # the region, the mask and the canvas may lie at an odd address; int32 cells may not
    two = ctypes.c_void_p((1 << 21) + 2)

    # a 40 x 61 window at (32, 48) of an image of 7 x 8 cells of 16 pixels (112 x 128), canvas down 8 (5 x 7), the image's 16-box mask plane (7 x 8)
    def wn(r=odd, pitch=3 * 61 + 1, hr=40, wr=61, wx=32, wy=48, c=one, gy=7, gx=8, cell=16, lut=odd, alpha=102, down=8, smooth=1, mask=odd, mpitch=9, hm=7,
           wm=8, md=16, mt=8, out=odd, opitch=3 * 7 + 2):
        return lib.toad_region_heat_window_u8(r, pitch, hr, wr, wx, wy, c, gy, gx, cell, lut, alpha, down, smooth, mask, mpitch, hm, wm, md, mt, out, opitch, None)

    cases = [
        # the old refusals, in the old order
        (lambda: wn(r=None), -1, "null pointer"), (lambda: wn(c=None), -1, "null pointer"), (lambda: wn(lut=None), -1, "null pointer"),
        (lambda: wn(out=None), -1, "null pointer"),
        (lambda: wn(cell=12), -2, "cell"), (lambda: wn(cell=2), -2, "cell"), (lambda: wn(hr=0), -2, "bad shape"), (lambda: wn(wr=-1), -2, "bad shape"),
        (lambda: wn(alpha=-1), -2, "alpha"), (lambda: wn(alpha=257), -2, "alpha"),
        (lambda: wn(down=0), -2, "not one of 1, 2, 4, 8, 16, 32"), (lambda: wn(down=3), -2, "not one of"), (lambda: wn(down=64, cell=64), -2, "not one of"),
        (lambda: wn(down=-8), -2, "not one of"),
        (lambda: wn(down=16, cell=8), -2, "exceeds cell = 8"), (lambda: wn(cell=4), -2, "cell = 4"), (lambda: wn(down=32, wx=32, wy=64), -2, "cell = 16"),
        (lambda: wn(down=16, cell=8, alpha=300), -2, "alpha"), (lambda: wn(down=16, cell=8, smooth=2, wx=3), -2, "exceeds cell"),
        # the window: negative, or not a multiple of max(4, down) - for every down, one step of 4 off where down is above 4
        (lambda: wn(wx=-8), -2, "window"), (lambda: wn(wy=-8), -2, "window"), (lambda: wn(wx=-8, smooth=2), -2, "window"),
        (lambda: wn(smooth=2), -1, "smooth"), (lambda: wn(smooth=-1), -1, "smooth"),
        (lambda: wn(pitch=3 * 61 - 1), -2, "pitch"), (lambda: wn(pitch=-184), -2, "pitch"),
        (lambda: wn(md=0), -2, "mask_down"), (lambda: wn(md=3), -2, "mask_down"), (lambda: wn(md=64), -2, "mask_down"),
        (lambda: wn(md=4), -2, "multiple of down"), (lambda: wn(down=16, wx=32, md=8, opitch=9), -2, "multiple of down"),
        (lambda: wn(hm=-1), -2, "Hm x Wm"), (lambda: wn(wm=-1), -2, "Hm x Wm"),
        (lambda: wn(mpitch=7), -2, "mask_pitch"), (lambda: wn(mpitch=-9), -2, "mask_pitch"),
        (lambda: wn(mt=-1), -1, "mask_thresh"), (lambda: wn(mt=256), -1, "mask_thresh"),
        (lambda: wn(opitch=3 * 7 - 1), -2, "out_pitch"), (lambda: wn(down=16, wx=32, opitch=3 * 3 - 1), -2, "out_pitch"),
        (lambda: wn(wr=715827883, wx=0, pitch=1 << 32, opitch=1 << 32, gx=44739243, mask=None), -2, "2^31"),
        # the window beyond the table: rows 48 .. 88 need 6 cell rows, columns 32 .. 93 need 6 cell columns
        (lambda: wn(gy=5), -2, "beyond the table"), (lambda: wn(gx=5), -2, "beyond the table"), (lambda: wn(wy=80), -2, "beyond the table"),
        (lambda: wn(wx=72), -2, "beyond the table"), (lambda: wn(cell=8), -2, "beyond the table"), (lambda: wn(wy=1 << 30), -2, "beyond the table"),
        (lambda: wn(hr=1 << 30, wr=16385, wx=0, wy=0, pitch=1 << 20, gy=1 << 26, gx=1025, opitch=1 << 20, mask=None), -2, "workgroups"),
        (lambda: wn(c=odd), -4, "4-byte aligned"), (lambda: wn(c=two), -4, "4-byte aligned"),
    ]
    for down in DOWNS:
        step = max(4, down)
        k = dict(down=down, cell=32, gy=4, gx=4, md=32, hm=1, wm=1, mpitch=1, opitch=3 * 61)
        cases += [(lambda k=k, v=v: wn(wx=v, wy=0, **k), -2, f"multiple of max(4, down) = {step}") for v in (step - 4 or 2, step + 4 if step > 4 else 6, 1, 2 * step + step // 2)]
        cases += [(lambda k=k, v=v: wn(wx=0, wy=v, **k), -2, f"multiple of max(4, down) = {step}") for v in (step - 4 or 2, step + 4 if step > 4 else 6, 3, 2 * step + step // 2)]
    # wx + Wr must stay below 2^30: the last legal one passes on to the table check
    big = dict(wr=64, pitch=192, mask=None, opitch=192, down=1, wy=0)
    cases += [(lambda: wn(wx=(1 << 30) - 64, gx=1 << 26, **big), -2, "2^30"), (lambda: wn(wx=(1 << 30), gx=1 << 27, **big), -2, "2^30"),
              (lambda: wn(wx=(1 << 30) - 128, gx=(1 << 26) - 5, **big), -2, "beyond the table")]
    for call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # what is taken: only the later alignment check stops these calls
    for ok in (dict(), dict(wx=0, wy=0), dict(wx=64, wy=64), dict(gy=6, gx=6), dict(gy=100, gx=100), dict(smooth=0), dict(hm=0, wm=0, mpitch=0),
               dict(hm=2, wm=3, mpitch=3), dict(hm=1000, wm=1000, mpitch=1000), dict(md=8), dict(md=32), dict(down=16, wx=16, wy=16, opitch=9),
               dict(down=1, wx=4, wy=4, md=1, opitch=183), dict(down=2, wx=4, wy=12, md=2, opitch=90), dict(down=4, wx=60, wy=68, md=4, opitch=45),
               dict(cell=4, down=4, gy=28, gx=32, wx=4, wy=4, opitch=45), dict(cell=64, gy=2, gx=2), dict(alpha=0), dict(alpha=256),
               dict(wx=(1 << 30) - 128, gx=(1 << 26) - 4, **big)):
        assert wn(c=odd, **ok) == -4, ok
    assert wn(c=odd, mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999) == -4      # mask == NULL means no mask: its other arguments are not looked at
    # an empty canvas: everything is checked, nothing is launched, 0 is returned (no device is present here, so a launch would fail)
    assert wn(hr=7) == 0 and wn(wr=7, pitch=21, opitch=0) == 0 and wn(hr=7, mask=None) == 0 and wn(hr=7, gy=3) == -2 and wn(hr=7, c=odd) == -4
    assert wn(hr=3, down=1, md=1, wx=4, wy=4, opitch=183, c=odd) == -4 and wn(hr=3, down=4, md=4, wx=4, wy=4, opitch=45) == 0


def test_the_older_entries_refuse_what_they_refused():
    """The three older calls pass wx = wy = 0 into the shared launcher: their table and plane checks are the equalities, in their own names."""
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one, odd = ctypes.c_void_p(1 << 21), ctypes.c_void_p((1 << 21) + 1)

    def px(name, hr=40, wr=61, gy=3, gx=4, cell=16, down=4, hm=10, wm=15, md=4, mask=odd, c=one):
        return getattr(lib, name)(odd, 3 * 61 + 1, hr, wr, c, gy, gx, cell, odd, 102, down, 1, mask, 16, hm, wm, md, 8, odd, 3 * 61, None)
    for name, down in (("toad_region_heat_blend_px_u8", 4), ("toad_region_heat_thumb_u8", 8)):
        md, hm, wm = (4, 10, 15) if down == 4 else (8, 5, 7)
        for k, text in ((dict(gy=4), "Gy x Gx"), (dict(gx=5), "Gy x Gx"), (dict(gy=7, gx=8), "is not ceil(Hr / cell) x ceil(Wr / cell)"), (dict(hm=hm + 1), "Hm x Wm"),
                        (dict(wm=wm - 1), "Hm x Wm"), (dict(hm=100, wm=100), "is not (Hr / mask_down) x (Wr / mask_down)"),
                        (dict(down=1 if down == 8 else 8), "down")):
            a = dict(down=down, md=md, hm=hm, wm=wm)
            a.update(k)
            assert px(name, **a) == -2 and text in err() and err().startswith(name + ":"), (name, k, err())
        assert px(name, down=down, md=md, hm=hm, wm=wm, c=odd) == -4
    flat = lambda **k: lib.toad_region_heat_blend_u8(odd, 184, 40, 61, k.get("c", one), k.get("gy", 3), k.get("gx", 4), 16, odd, 102, k.get("down", 2), odd, 90, None)      # noqa: E731
    assert flat(gy=7, gx=8) == -2 and "Gy x Gx" in err() and flat(down=8) == -2 and "not one of 1, 2, 4" in err() and flat(c=odd) == -4


# ---- the windowed reference against slices of the whole-image reference ---------------------------------------------------------------------------------
def _slide(hs, ws, cell, seed):
    rng = np.random.default_rng(seed)
    slide = rng.integers(0, 256, size=(hs, ws, 3), dtype=np.uint8)
    cells = rng.integers(-1, 300, size=(-(-hs // cell), -(-ws // cell)))
    cells[rng.random(cells.shape) < 0.2] = -1
    lut = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    return rng, slide, cells, lut


@pytest.mark.parametrize("down", DOWNS)
def test_windowed_reference_equals_the_slice_of_the_whole_canvas(down):
    """Random slides, tables and masks; windows whose edges are off the cell grid, windows that end at the slide's edge (where the table's last cell and
    the plane's dropped boxes lie) and the whole slide; smooth on and off, with and without a mask."""
    step = max(4, down)
    for seed, (hs, ws), cell in ((1, (75, 99), 4), (2, (75, 99), 8), (3, (131, 167), 16), (4, (131, 203), 32), (5, (150, 203), 64)):
        if down > 4 and down > cell:
            continue
        rng, slide, cells, lut = _slide(hs, ws, cell, 10 * seed + down)
        for md in sorted({m for m in (down, 2 * down, 32) if m <= 32}):
            mask = rng.integers(0, 256, size=(hs // md, ws // md), dtype=np.uint8)
            t = int(rng.integers(0, 255))
            windows = [(0, 0, ws, hs), (step, 2 * step, ws - step, hs - 2 * step), (3 * step, step, step + 3, step + 1)]
            windows += [(step, step, 2 * step + 1, 3 * step + 2)] if md == down else []
            for smooth in (False, True):
                for m in (None, mask):
                    whole = ref.canvas(slide, cells, cell, lut, 102, down, smooth=smooth, mask=m, mask_down=md, mask_thresh=t)
                    for wx, wy, w, h in windows:
                        if wx + w > ws or wy + h > hs or w < 1 or h < 1:
                            continue
                        got = wref.canvas(slide[wy:wy + h, wx:wx + w], (wx, wy), cells, cell, lut, 102, down, smooth=smooth, mask=m, mask_down=md, mask_thresh=t)
                        want = whole[wy // down:wy // down + h // down, wx // down:wx // down + w // down]
                        assert got.shape == want.shape and np.array_equal(got, want), (down, cell, md, smooth, m is not None, (wx, wy, w, h))


def test_windowed_reference_sees_the_neighbour_outside_the_window():
    """The point of the window: under the tent a strip's canvas differs from the canvas of the strip rendered as a region of its own."""
    _, slide, cells, lut = _slide(64, 64, 16, 7)
    cells = np.arange(16).reshape(4, 4) * 17
    strip = slide[32:64]
    alone = ref.canvas(strip, cells[2:], 16, lut, 256, 1, smooth=True)
    window = wref.canvas(strip, (0, 32), cells, 16, lut, 256, 1, smooth=True)
    assert np.array_equal(window, ref.canvas(slide, cells, 16, lut, 256, 1, smooth=True)[32:])
    assert not np.array_equal(window[:8], alone[:8]) and np.array_equal(window[8:], alone[8:])      # the half cell below the seam leans on the row above it


# ---- strip_plan -----------------------------------------------------------------------------------------------------------------------------------------
def _brute_plan(hs, strips, h, sy, y0):
    """What strip_plan promises, stated row by row: the owner of lattice row j is the first strip that holds rows y0 + j sy .. + h whole; slide row r is
    rendered by the first strip that holds it."""
    ny = (hs - y0 - h) // sy + 1 if hs - y0 >= h else 0
    owner = []
    for j in range(ny):
        top = y0 + j * sy
        owner.append(next((k for k, (y, n) in enumerate(strips) if y <= top and top + h <= y + n), None))
    render = [next((k for k, (y, n) in enumerate(strips) if y <= r < y + n), None) for r in range(hs)]
    return owner, render


def test_strip_plan_against_a_brute_force_statement():
    from toad_amd.heatmap import strip_plan
    rng = np.random.default_rng(3)
    seen = 0
    for trial in range(300):
        h = int(rng.choice([16, 32, 64]))
        sy = int(rng.choice([s for s in (8, 16, 32, 64) if s <= h]))
        y0 = int(rng.choice([0, 4, 8]))
        down = int(rng.choice([1, 2, 4, 8]))
        hs = int(rng.integers(h + y0, 400))
        cuts = sorted(set((rng.integers(1, max(hs // 8, 2), size=int(rng.integers(0, 4))) * 8).tolist()))      # render starts: multiples of 8
        cuts = [c for c in cuts if c < hs]
        starts, ends = [0] + cuts, cuts + [hs]
        over = int(rng.choice([0, h - sy, h - sy + 5, h]))
        strips = [(max(0, s - (over if k else 0)), 0) for k, s in enumerate(starts)]
        strips = [(y, e - y) for (y, _), e in zip(strips, ends)]
        if any(b[0] <= a[0] for a, b in zip(strips, strips[1:])):
            continue
        owner, render = _brute_plan(hs, strips, h, sy, y0)
        if None in owner:
            with pytest.raises(ValueError, match="lies whole in no strip"):
                strip_plan((hs, 640), strips, (h, 32), (sy, 32), (0, y0), down)
            continue
        plan = strip_plan((hs, 640), strips, (h, 32), (sy, 32), (0, y0), down)
        seen += 1
        assert len(plan) == len(strips)
        owned = [k for k, p in enumerate(plan) for _ in range(*p["rows"])]
        assert owned == owner                                        # every lattice row once, by the first strip that holds it whole
        assert [k for k, p in enumerate(plan) for _ in range(*p["render"])] == render and plan[0]["render"][0] == 0 and plan[-1]["render"][1] == hs
        for (y, n), p, r in zip(strips, plan, starts):
            assert p["render"] == (r, y + n)
            j0, j1 = p["rows"]
            assert p["origin"] == ((0, y0 + j0 * sy - y) if j1 > j0 else None)
            if j1 > j0:                                              # the strip's own lattice from that origin is exactly the rows it owns
                assert p["origin"][1] >= 0 and (n - p["origin"][1] - h) // sy + 1 == j1 - j0
    assert seen > 100


def test_strip_plan_refuses():
    from toad_amd.heatmap import strip_plan
    plan = lambda strips, down=1, hs=256, tile=64, stride=32: strip_plan((hs, 512), strips, tile, stride, (0, 0), down)      # noqa: E731
    assert [p["render"] for p in plan([(0, 128), (96, 160)])] == [(0, 128), (128, 256)]
    assert [p["rows"] for p in plan([(0, 128), (96, 160)])] == [(0, 3), (3, 7)] and plan([(0, 128), (96, 160)])[1]["origin"] == (0, 0)
    for strips, k, text in (([(0, 128), (100, 156)], {}, "lies whole in no strip"),                  # overlap 28 < tile - stride = 32
                            ([(0, 128), (128, 128)], {}, "lies whole in no strip"),                  # abutting strips under an overlapping lattice
                            ([(0, 120), (128, 128)], {}, "gap"), ([(0, 128), (96, 100)], {}, "cover rows 0 .. Hs"), ([(8, 120), (96, 160)], {}, "cover rows 0"),
                            ([(0, 128), (96, 200)], {}, "cover rows 0 .. Hs"), ([], {}, "cover rows"),
                            ([(0, 128), (0, 256)], {}, "not sorted"), ([(0, 200), (96, 64), (160, 96)], {}, "not sorted"), ([(0, 128), (64, 64), (96, 160)], {}, "not sorted"),
                            ([(0, 130), (96, 160)], {}, r"multiple of max\(4, down\) = 4"), ([(0, 132), (96, 160)], dict(down=8), r"max\(4, down\) = 8"),
                            ([(0, 144), (96, 160)], dict(down=32), r"max\(4, down\) = 32"), ([(0, 128), (96, 160)], dict(down=3), "down must be one of")):
        with pytest.raises(ValueError, match=text):
            plan(strips, **k)
    assert len(plan([(0, 132), (96, 160)], down=4)) == 2 and len(plan([(0, 128), (128, 128)], stride=64)) == 2      # abutting is fine where tiles do not overlap
    short = plan([(0, 128), (120, 48), (128, 128)], stride=64)      # a strip that holds no tile whole owns nothing and still renders its rows
    assert short[1] == dict(rows=(2, 2), origin=None, render=(128, 168)) and short[2] == dict(rows=(2, 4), origin=(0, 0), render=(168, 256))


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------------------
def test_window_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.heatmap import window_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_window(cpu, (0, 0), torch.zeros(8, 8, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, 8)
    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells, lut = torch.zeros(8, 8, dtype=torch.int32, device="meta"), torch.zeros(256, 3, dtype=torch.uint8, device="meta")
    m8 = torch.zeros(8, 8, dtype=torch.uint8, device="meta")
    for k, text in ((dict(cell=12), "cell"), (dict(down=3), "down must be one of"), (dict(down=64), "down must be one of"), (dict(down=32), "exceeds cell = 16"),
                    (dict(alpha=257), "alpha"), (dict(lut=lut[:255]), "lut"), (dict(window=(0,)), "window must be"), (dict(window=None), "window must be"),
                    (dict(window=(8.0, 8)), "window must be"), (dict(window=(True, 8)), "window must be"),
                    (dict(window=(-8, 8)), r"multiples of max\(4, down\) = 8"), (dict(window=(8, 4)), r"multiples of max\(4, down\) = 8"),
                    (dict(window=(4, 8)), r"max\(4, down\) = 8"), (dict(window=(2, 0), down=1), r"max\(4, down\) = 4"), (dict(window=(0, 6), down=2), r"max\(4, down\) = 4"),
                    (dict(window=(16, 8), down=16), r"max\(4, down\) = 16"),
                    (dict(window=((1 << 30) - 64, 0)), "below 2\\^30"), (dict(window=(72, 8)), "beyond the int32"), (dict(window=(8, 72)), "beyond the int32"),
                    (dict(cells=cells[:4]), "beyond the int32"), (dict(cells=cells.view(-1)), "beyond the int32"),
                    (dict(out=torch.zeros(16, 16, 3, dtype=torch.uint8, device="meta")), "out must be"),
                    (dict(smooth=2), "smooth"), (dict(mask_down=16), "without a mask"), (dict(mask=m8), "mask_down"), (dict(mask=m8, mask_down=3), "mask_down"),
                    (dict(mask=m8, mask_down=4), "multiple of down"), (dict(mask=m8, mask_down=16, mask_thresh=256), "mask_thresh"),
                    (dict(mask=torch.zeros(8, 16, dtype=torch.uint8, device="meta")[:, ::2], mask_down=16), "stride")):
        args = dict(region=meta, window=(8, 8), cells=cells, cell=16, lut=lut, alpha=102, down=8)
        args.update(k)
        with pytest.raises(ValueError, match=text):
            ops.region_heat_window(**args)
    with pytest.raises(TypeError, match="uint8"):
        ops.region_heat_window(meta, (8, 8), cells, 16, lut, 102, 8, mask=m8.float(), mask_down=16)
    # the slide's plane may have any extent; a canvas with no rows or no columns launches nothing, and neither does an empty plane... until the library
    for k in (dict(region=meta[:7]), dict(region=meta[:, :7]), dict(region=meta[:7], mask=m8[:1, :1], mask_down=16)):
        args = dict(region=meta, window=(8, 8), cells=cells, cell=16, lut=lut, alpha=102, down=8)
        args.update(k)
        assert 0 in ops.region_heat_window(**args).shape
    for m in (m8, m8[:2, :3], torch.zeros(100, 100, dtype=torch.uint8, device="meta")):
        with pytest.raises(AssertionError, match="library was reached"):
            ops.region_heat_window(meta, (8, 8), cells, 16, lut, 102, 8, mask=m, mask_down=16)
    for k, text in ((dict(alpha=1.5), "alpha"), (dict(smooth=1), "bool"), (dict(mask=(m8, 8)), "triple"), (dict(window=(4, 8), down=8), r"max\(4, down\)")):
        with pytest.raises(ValueError, match=text):
            window_canvas(meta, k.pop("window", (8, 8)), cells, 16, lut=lut, **k)


def test_attention_canvas_is_slide_cells_plus_the_blend(monkeypatch):
    """With the library faked: attention_canvas makes the calls it made - tile_table, heat_cells, heat_cells_blur where asked, then region_heat_blend_px or
    region_heat_thumb with the same arguments - and slide_cells makes the first three of them with the same arguments."""
    from toad_amd import heatmap, ops
    from toad_amd.heatmap import attention_canvas, slide_cells
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    log = []

    def fake(name, result):
        def f(*a, **k):
            log.append((name, [x if not isinstance(x, torch.Tensor) else ("T", tuple(x.shape), x.dtype) for x in a],
                        {n: v if not isinstance(v, torch.Tensor) else ("T", tuple(v.shape), v.dtype) for n, v in k.items()}))
            return result(*a, **k)
        return f
    table = torch.zeros(4, 8, dtype=torch.int32, device="meta")
    monkeypatch.setattr(heatmap, "tile_table", fake("tile_table", lambda *a, **k: table))
    monkeypatch.setattr(ops, "heat_cells", fake("heat_cells", lambda *a, **k: torch.zeros(5, 9, dtype=torch.int32, device="meta")))
    monkeypatch.setattr(ops, "heat_cells_blur", fake("heat_cells_blur", lambda c, t: torch.ones_like(c)))
    for blend in ("region_heat_blend_px", "region_heat_thumb"):
        monkeypatch.setattr(ops, blend, fake(blend, lambda region, cells, *a, **k: ("canvas", cells)))
    monkeypatch.setattr(ops, "region_heat_window", fake("region_heat_window", lambda *a, **k: None))
    meta = torch.zeros(300, 520, 3, dtype=torch.uint8, device="meta")
    origins, scores = np.array([[0, 0], [64, 128]]), torch.zeros(2, device="meta")
    mask = (torch.zeros(18, 32, dtype=torch.uint8, device="meta"), 9, 16)
    for down, blend in ((1, "region_heat_blend_px"), (4, "region_heat_blend_px"), (8, "region_heat_thumb"), (16, "region_heat_thumb")):
        for kw in (dict(), dict(blur=True), dict(blur=(4, 2, 1), thresh=0.5, binarize=True, smooth=True, mask=mask, alpha=0.5), dict(score_range=(-1, 3), origin=(64, 0))):
            del log[:]
            tag, cells = attention_canvas(meta, origins, scores, 128, 64, down=down, **kw)
            whole = list(log)
            names = [n for n, _, _ in whole]
            assert tag == "canvas" and names == ["tile_table", "heat_cells"] + (["heat_cells_blur"] if "blur" in kw else []) + [blend]
            args = whole[-1][1]
            assert args[2] == 64 and args[4] == (128 if kw.get("alpha") == 0.5 else 102) and args[5] == down
            assert whole[-1][2] == dict(smooth=kw.get("smooth", False), mask=("T", (18, 32), torch.uint8) if "mask" in kw else None,
                                        mask_down=16 if "mask" in kw else None, mask_thresh=9 if "mask" in kw else 0, out=None)
            del log[:]
            sk = {k: v for k, v in kw.items() if k in ("blur", "thresh", "binarize", "score_range", "origin")}
            got, cell = slide_cells((300, 520), origins, scores, 128, 64, **sk)
            assert cell == 64 and log == whole[:-1] and got.shape == cells.shape
    # no tile: a table of -1 over the slide's extent, nothing launched
    del log[:]
    got, cell = slide_cells((300, 520), np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"), 128, 64, blur=True)
    assert cell == 64 and tuple(got.shape) == (5, 9) and [n for n, _, _ in log] == ["tile_table"]
    for k, text in ((dict(thresh="x"), "thresh"), (dict(binarize=1), "binarize"), (dict(blur=-1.0), "positive and finite"), (dict(score_range=(1, 1)), "score_range")):
        with pytest.raises(ValueError, match=text):
            slide_cells((300, 520), origins, scores, 128, 64, **k)
