"""CPU: the saturation plane of a slide that arrives in strips (toad_regions_saturation_u8: an additive extension of ABI 15; toad_amd/tissue.py
plane_strip_plan, slide_saturation, segment_tissue_strips, segmented_slide_origins; the segment= and tissue_mask= keywords of
eval.slide_attention_heatmap). The plan is host arithmetic, the assembly is checked in numpy against tests/tissue_seg_ref.py, and every refusal comes
before a device is touched. Integers throughout: every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tissue_seg_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "toad_regions_saturation_u8"
DOWNS = (1, 2, 4, 8, 16, 32)
WALK_SPANS = [(0, 112), (64, 144), (176, 80)]                        # the spans of the walk test: rows 0 .. 112, 64 .. 208, 176 .. 256 of a 256-row slide
CASE_SPANS = [(0, 96), (64, 96), (160, 40)]                          # the spans of the GPU cases: rows 0 .. 96, 64 .. 160, 160 .. 200 of a 200-row slide


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------------
def test_list_entry_is_declared_exported_and_bound():
    from toad_amd import _lib as L, ops
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert re.search(r"typedef\s+struct\s*\{\s*const unsigned char \*region; int64_t pitch; int Hr, Wr; unsigned char \*plane; int64_t plane_pitch;\s*\}\s*"
                     r"ToadSatWindow;", header)
    assert re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header) and L.ABI_VERSION == 15
    lib = L.load()
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES
    assert L.SIGNATURES[NAME][1] == [ctypes.POINTER(L.ToadSatWindow), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert ctypes.sizeof(L.ToadSatWindow) == 40 and L.ToadSatWindow.plane.offset == 24 and L.ToadSatWindow.plane_pitch.offset == 32
    assert ops.SAT_LIST_MAX == 32


def test_list_entry_reports_argument_errors_in_order_without_a_gpu():
    """Every check comes before a device access, in the order the header gives: the array and n, val_min and down with the single entry's messages, then
    window by window the single entry's checks under "window k:", then the workgroups of the whole list."""
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    base = 1 << 21

    def win(region=base + 1, pitch=3 * 31 + 1, hr=20, wr=31, plane=base + (1 << 20), pp=15):
        return L.ToadSatWindow(region, pitch, hr, wr, plane, pp)

    def call(wins, n=None, down=2, vmin=0):
        arr = (L.ToadSatWindow * max(len(wins), 1))(*wins) if wins is not None else None
        return lib.toad_regions_saturation_u8(arr, len(wins) if n is None else n, down, vmin, None)

    def single(down=2, vmin=0):
        return lib.toad_region_saturation_u8(ctypes.c_void_p(base + 1), 3 * 31 + 1, 20, 31, down, vmin, ctypes.c_void_p(base + (1 << 20)), 15, None)

    good = win()
    huge = win(hr=1 << 30, wr=1 << 28, pitch=1 << 32, pp=1 << 28)     # 2^20 chunks x 2^26 row blocks = 2^46 workgroups at down = 1
    cases = [
        (lambda: call(None, n=3), -1, NAME + ": null pointer"),
        (lambda: call(None, n=3, down=3, vmin=-1), -1, NAME + ": null pointer"),          # the array comes first
        (lambda: call([good], n=-1), -1, NAME + ": n = -1 windows"),
        (lambda: call([good], n=-1, vmin=256), -1, NAME + ": n = -1 windows"),            # n before val_min
        (lambda: call([good], vmin=256, down=3), -1, NAME + ": val_min"),                 # val_min before down
        (lambda: call([good], vmin=-1), -1, NAME + ": val_min"),
        (lambda: call([win(region=None)], down=3), -2, NAME + ": down = 3"),              # down before the windows
        (lambda: call([good], down=64), -2, NAME + ": down = 64"),
        (lambda: call([], n=0, down=5), -2, NAME + ": down = 5"),                         # an empty list is still checked for what the windows share
        (lambda: call([good, win(region=None)]), -1, "window 1: " + NAME + ": null pointer"),
        (lambda: call([good, good, win(plane=None)]), -1, "window 2: " + NAME + ": null pointer"),
        (lambda: call([win(hr=0), win(region=None)]), -2, "window 0: " + NAME + ": bad shape"),      # the first failing window wins
        (lambda: call([good, win(wr=-1)]), -2, "window 1: " + NAME + ": bad shape"),
        (lambda: call([win(region=None, hr=0)]), -1, "window 0: " + NAME + ": null pointer"),        # inside a window: pointers before the shape
        (lambda: call([win(hr=0, pitch=1)]), -2, "window 0: " + NAME + ": bad shape"),               # ... the shape before the region pitch
        (lambda: call([good, win(pitch=3 * 31 - 1, pp=1)]), -2, "window 1: " + NAME + ": pitch 92"),  # ... the region pitch before the plane pitch
        (lambda: call([good, win(pp=14)]), -2, "window 1: " + NAME + ": plane_pitch 14"),
        (lambda: call([win(wr=715827883, pitch=1 << 32, pp=1 << 30)]), -2, "window 0: " + NAME + ": region too wide"),
        (lambda: call([huge, win(pp=14)], down=1), -2, "window 1: " + NAME + ": plane_pitch"),       # every window before the workgroup count
        (lambda: call([win(pp=31), huge], down=1), -2, NAME + ": list of regions too large"),
        (lambda: call([huge] * 40, down=1), -2, NAME + ": list of regions too large"),
    ]
    for k, (fn, rc, text) in enumerate(cases):
        got = fn()
        msg = err()
        assert got == rc and msg.startswith(text), (k, got, msg)
    # val_min and down carry the single entry's messages
    for kw in (dict(vmin=256), dict(vmin=-1), dict(down=3), dict(down=0)):
        assert call([good], **kw) == single(**kw) != 0
        m_list = err()
        single(**kw)
        assert m_list.replace(NAME, "toad_region_saturation_u8") == err()
    # nothing to launch: TOAD_OK without a device. An empty list (with or without an array), and windows smaller than one box.
    assert call([], n=0) == 0 and call(None, n=0) == 0
    assert call([win(hr=1, wr=31, pp=15), win(hr=20, wr=1, pitch=3, pp=0)], down=2) == 0
    assert call([win(hr=31, wr=31, pp=0)], down=32) == 0


# ---- plane_strip_plan ----------------------------------------------------------------------------------------------------------------------------------------
def test_plane_strip_plan_on_the_spans_of_the_walk():
    from toad_amd.tissue import plane_strip_plan
    hw = (256, 1100)
    assert plane_strip_plan(hw, WALK_SPANS, 16) == [(0, 7), (7, 13), (13, 16)]
    assert plane_strip_plan(hw, WALK_SPANS, 1) == [(0, 112), (112, 208), (208, 256)]
    # down = 32: the seam at 112 falls inside box row 3 (rows 96 .. 128), which lies whole in strip 1 (rows 64 .. 208); the seam at 208 inside box row 6
    # (rows 192 .. 224), which lies whole in strip 2 (rows 176 .. 256)
    assert plane_strip_plan(hw, WALK_SPANS, 32) == [(0, 3), (3, 6), (6, 8)]
    for down, want in ((2, [(0, 56), (56, 104), (104, 128)]), (4, [(0, 28), (28, 52), (52, 64)]), (8, [(0, 14), (14, 26), (26, 32)])):
        assert plane_strip_plan(hw, WALK_SPANS, down) == want
    # the sub-region of every strip lies inside the strip, and the rows partition 0 .. Hp
    for down in DOWNS:
        for hs, spans in ((256, WALK_SPANS), (200, CASE_SPANS), (200, [(0, 200)]), (37, [(0, 33), (5, 32)])):
            plan = plane_strip_plan((hs, 600), spans, down)
            assert len(plan) == len(spans) and plan[0][0] == 0 and plan[-1][1] == hs // down
            for k, ((y, n), (p0, p1)) in enumerate(zip(spans, plan)):
                assert p0 <= p1 and (k == 0 or p0 == plan[k - 1][1])
                assert 0 <= p0 * down - y and p1 * down - y <= n
    # box rows below Hp * down are dropped: 200 rows at down = 32 are 6 plane rows, the last strip gives the one it holds whole
    assert plane_strip_plan((200, 600), CASE_SPANS, 32) == [(0, 3), (3, 5), (5, 6)]
    # a strip with no row left to give: (p1, p1)
    assert plane_strip_plan((64, 8), [(0, 48), (40, 12), (48, 16)], 16) == [(0, 3), (3, 3), (3, 4)]


def test_plane_strip_plan_refusals():
    from toad_amd.tissue import plane_strip_plan
    hw = (256, 1100)
    with pytest.raises(ValueError, match=r"plane row 6 \(slide rows 96 \.\. 112\) lies whole in no strip"):
        plane_strip_plan(hw, [(0, 104), (104, 152)], 16)              # abutting at a row that is no multiple of down
    assert plane_strip_plan(hw, [(0, 104), (104, 152)], 8) == [(0, 13), (13, 32)]         # ... and at one that is
    assert plane_strip_plan(hw, [(0, 104), (96, 160)], 16) == [(0, 6), (6, 16)]           # ... or overlapping by the rest of the box
    with pytest.raises(ValueError, match="lies whole in no strip"):
        plane_strip_plan(hw, [(0, 104), (100, 156)], 16)              # overlapping, by too little
    with pytest.raises(ValueError, match=r"a gap between strip 0, which ends at row 100, and strip 1, which starts at row 112"):
        plane_strip_plan(hw, [(0, 100), (112, 144)], 16)
    with pytest.raises(ValueError, match="is empty or not sorted after the strips before it"):
        plane_strip_plan(hw, [(0, 112), (64, 144), (64, 192)], 16)
    with pytest.raises(ValueError, match="is empty or not sorted"):
        plane_strip_plan(hw, [(0, 112), (64, 0), (64, 192)], 16)
    for spans in ([], [(16, 240)], [(0, 112), (64, 144)], [(0, 112), (64, 200)]):
        with pytest.raises(ValueError, match=r"the strips must cover rows 0 \.\. Hs = 256"):
            plane_strip_plan(hw, spans, 16)
    for bad in (0, 3, 64, "4", None):
        with pytest.raises(ValueError, match="down must be one of"):
            plane_strip_plan(hw, WALK_SPANS, bad)


# ---- the assembly, in numpy ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("down", DOWNS)
def test_planes_stacked_by_the_plan_are_the_plane_of_the_slide(down):
    from toad_amd.tissue import plane_strip_plan
    s = ref.slide(200, 600, 1)
    for vmin in (0, 40):
        want = ref.saturation_plane(s, down, vmin)
        for spans in (CASE_SPANS, [(0, 200)], [(0, 64), (64, 64), (128, 72)]):
            plan = plane_strip_plan((200, 600), spans, down)
            parts = []
            for (y, n), (p0, p1) in zip(spans, plan):
                strip = s[y:y + n]                                   # what the decoder hands over
                sub = strip[p0 * down - y:p1 * down - y]             # the rows that hold the boxes of plane rows p0 .. p1
                got = ref.saturation_plane(sub, down, vmin)
                assert got.shape == (p1 - p0, 600 // down)
                parts.append(got)
            assert np.array_equal(np.concatenate(parts, axis=0), want), (down, vmin, spans)


# ---- refusals of the ops and eval calls that need no device ---------------------------------------------------------------------------------------------------
def test_regions_saturation_refusals_cpu(monkeypatch):
    from toad_amd import _lib as L, ops

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(40, 64, 3, dtype=torch.uint8)
    for bad in (cpu, "regions", 7, None, iter([cpu])):
        with pytest.raises(ValueError, match="regions must be a sequence"):
            ops.regions_saturation(bad, 4)
    for outs in ([], [cpu[..., 0], cpu[..., 0]], cpu[..., 0], 3):
        with pytest.raises(ValueError, match="outs must be None or a sequence of 1 planes"):
            ops.regions_saturation([cpu], 4, outs=outs)
    assert ops.regions_saturation([], 4) == () and ops.regions_saturation((), 32, 5, outs=[]) == ()
    for bad in (0, 3, 64, "4", None):
        with pytest.raises(ValueError, match="regions_saturation: down must be one of"):
            ops.regions_saturation([cpu], bad)
    with pytest.raises(ValueError, match=r"val_min must be an int in \[0, 255\]"):
        ops.regions_saturation([cpu], 4, 256)
    with pytest.raises(RuntimeError, match=r"window 0: region must be a CUDA"):
        ops.regions_saturation([cpu], 4)
    # what comes after the device test, on stand-ins that claim to be on the device: region_saturation's checks, with the window named
    meta = torch.zeros(40, 128, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    reg = meta[:, :64]
    with pytest.raises(TypeError, match=r"window 1: region must be torch.uint8"):
        ops.regions_saturation([reg, reg.float()], 4)
    with pytest.raises(ValueError, match=r"window 2: expected a uint8 \[Hr,Wr,3\] region .*stride\(1\) == 3"):
        ops.regions_saturation([reg, reg, meta[:, ::2]], 4)
    plane = torch.zeros(10, 40, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match=r"window 0: outs\[0\] must be a uint8 \[10,16\] tensor"):
        ops.regions_saturation([reg, reg], 4, outs=[plane[:, :17], plane[:, :16]])
    with pytest.raises(ValueError, match=r"window 0: expected a uint8 \[Hp,Wp\] plane with stride\(1\) == 1"):
        ops.regions_saturation([reg], 4, outs=[plane[:, ::2][:, :16]])
    # windows without a plane row or column: returned empty, and still nothing is reached
    got = ops.regions_saturation([reg[:3], reg[:, :2]], 4)
    assert [tuple(g.shape) for g in got] == [(0, 16), (10, 0)] and all(g.dtype == torch.uint8 for g in got)


def test_slide_calls_refuse_before_a_device_is_touched(monkeypatch):
    from toad_amd import _lib as L
    from toad_amd.eval import slide_attention_heatmap
    from toad_amd.tissue import segment_tissue_strips, segmented_slide_origins, slide_saturation

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    hs, ws = 256, 1100
    slide = torch.zeros(hs, ws, 3, dtype=torch.uint8, device="meta")
    strips = [(slide[y:y + n], y) for y, n in WALK_SPANS]
    kw = dict(tile=(64, 256), stride=(64, 256))
    o = np.array([[0, 0]], dtype=np.int64)
    plane = torch.zeros(16, 68, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="segment selects the tiles, origins gives them"):
        slide_attention_heatmap(None, None, strips, (hs, ws), origins=o, segment=dict(down=16), **kw)
    with pytest.raises(ValueError, match="tissue_mask=True needs a segment dict"):
        slide_attention_heatmap(None, None, strips, (hs, ws), tissue_mask=True, **kw)
    with pytest.raises(ValueError, match="tissue_mask=True needs a segment dict"):
        slide_attention_heatmap(None, None, strips, (hs, ws), tissue_mask=True, origins=o, mask=(plane, 8, 16), **kw)
    with pytest.raises(ValueError, match="pass that or mask, not both"):
        slide_attention_heatmap(None, None, strips, (hs, ws), tissue_mask=True, segment=dict(down=16), mask=(plane, 8, 16), **kw)
    # the down rule, in region_tissue_attention_heatmap's words
    with pytest.raises(ValueError, match=r"tissue_mask=True: the segment down = 8 must be a multiple of the canvas down = 16 \(a canvas box must lie in one mask pixel\)"):
        slide_attention_heatmap(None, None, strips, (hs, ws), tissue_mask=True, segment=dict(down=8), down=16, **kw)
    with pytest.raises(ValueError, match=r"tissue_mask=True: the segment down = 4 must be a multiple of the largest canvas down = 16"):
        slide_attention_heatmap(None, None, strips, (hs, ws), tissue_mask=True, segment=dict(down=4), down=(1, 4, 16), **kw)
    # the segment dict, with the region call's text
    with pytest.raises(ValueError, match=r"segment must be None or a dict.*\['tile'\]"):
        slide_attention_heatmap(None, None, strips, (hs, ws), segment=dict(down=4, tile=64), **kw)
    with pytest.raises(ValueError, match="segment must be None or a dict"):
        slide_attention_heatmap(None, None, strips, (hs, ws), segment="otsu", **kw)
    with pytest.raises(ValueError, match="down must be one of"):
        slide_attention_heatmap(None, None, strips, (hs, ws), segment=dict(down=5), **kw)
    # what plane_strip_plan and the segmented lattice rule refuse
    meet = [(slide[:104], 0), (slide[104:], 104)]                    # abutting at 104: fine for tile rows 0 .. 64 and 128 .. 192, not for plane rows of 16
    with pytest.raises(ValueError, match="plane row 6 .* lies whole in no strip"):
        slide_attention_heatmap(None, None, meet, (hs, ws), tile=(64, 256), stride=(128, 256), segment=dict(down=16), tissue_mask=True, down=1)
    with pytest.raises(ValueError, match=r"tile height = 64 is not a multiple of 4 \* down = 128 \(down = 32\)"):
        slide_attention_heatmap(None, None, strips, (hs, ws), segment=dict(down=32), **kw)
    for call in (lambda s: slide_saturation(s, (hs, ws), 16), lambda s: segment_tissue_strips(s, (hs, ws)), lambda s: segmented_slide_origins(s, (hs, ws), 64)):
        with pytest.raises(ValueError, match="lies whole in no strip"):
            call(meet)
        with pytest.raises(ValueError, match=r"strip 1 must be a full-width uint8 \[H_k,1100,3\] region"):
            call([strips[0], (slide[64:208, :1000], 64), strips[2]])
        with pytest.raises(ValueError, match="a gap between strip 0"):
            call([strips[0], strips[2]])
    with pytest.raises(ValueError, match="down must be one of"):
        slide_saturation(strips, (hs, ws), 3)
    with pytest.raises(ValueError, match="median must be one of"):
        segment_tissue_strips(strips, (hs, ws), median=4)
    with pytest.raises(ValueError, match="min_fraction"):
        segmented_slide_origins(strips, (hs, ws), 64, min_fraction=2)
    # an empty lattice: an empty result, nothing launched
    o2, t = segmented_slide_origins(strips, (hs, ws), (512, 64), down=16, sat_thresh=40, return_threshold=True)
    assert o2.shape == (0, 2) and o2.dtype == np.int64 and t == 40
