"""CPU: closing and the component / hole area filters of the segmented tissue selection (toad_plane_close_u8, toad_plane_components_u8,
toad_plane_area_select_u8: an additive extension of ABI 15; the close / min_area / min_hole keywords of toad_amd/tissue.py). The entry points exist in the
header, the library and the ctypes table and refuse what the host can see before any device access; and the numpy reference the GPU tests compare against
(tests/tissue_morph_ref.py) is itself tested here, on the inputs of those tests: every condition the GPU tests rely on - each stage changes the mask, some
components go and some stay, some holes are filled and some are not - is a fact about the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tissue_morph_ref as ref
from tests import tissue_seg_ref as seg

MORPH_SYMBOLS = ("toad_plane_close_u8", "toad_plane_components_u8", "toad_plane_area_select_u8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 200), (200, 1), (63, 65), (129, 131), (130, 257))          # the shapes of the GPU tests


def flood_components(sel, conn):
    """The components once more: a flood fill with an explicit stack, seeds taken in row-major order, so a component's seed is its smallest index."""
    sel = np.asarray(sel).astype(bool)
    hp, wp = sel.shape
    labels = np.full((hp, wp), -1, dtype=np.int64)
    area = np.zeros(hp * wp, dtype=np.int64)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for y0 in range(hp):
        for x0 in range(wp):
            if not sel[y0, x0] or labels[y0, x0] >= 0:
                continue
            seed = y0 * wp + x0
            labels[y0, x0] = seed
            stack, n, edge = [(y0, x0)], 0, False
            while stack:
                y, x = stack.pop()
                n += 1
                edge |= y == 0 or x == 0 or y == hp - 1 or x == wp - 1
                for dy, dx in steps:
                    v, u = y + dy, x + dx
                    if 0 <= v < hp and 0 <= u < wp and sel[v, u] and labels[v, u] < 0:
                        labels[v, u] = seed
                        stack.append((v, u))
            area[seed] = n + (ref.BORDER if edge else 0)
    return labels, area


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------------------
def test_morph_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L, build
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in MORPH_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert "tissue_morph.hip" in build.SOURCES
    # the header states the definition and what it is not
    assert "lo = c / 2, hi = c - 1 - c / 2" in header and "not claimed bit-equal to OpenCV" in header
    assert "max_n_holes, polygon areas and several regions per call are not done" in header
    assert "contour and hole area filters" not in header


def test_morph_entries_report_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    base = 1 << 21
    one = ctypes.c_void_p(base)                               # non-null fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p(base + 1)                           # planes at odd addresses are fine; int32 arrays there are refused
    two = ctypes.c_void_p(base + 2)
    far = ctypes.c_void_p(base + (1 << 20))
    far4 = ctypes.c_void_p(base + (1 << 22))

    def close(s=odd, sp=33, hp=20, wp=31, t=8, c=4, d=far, dp=31):
        return lib.toad_plane_close_u8(s, sp, hp, wp, t, c, d, dp, None)

    def comp(p=odd, pitch=33, hp=20, wp=31, t=8, bg=0, lab=far, ar=far4):
        return lib.toad_plane_components_u8(p, pitch, hp, wp, t, bg, lab, ar, None)

    def select(lab=one, ar=far4, hp=20, wp=31, mode=0, limit=5, d=odd, dp=31):
        return lib.toad_plane_area_select_u8(lab, ar, hp, wp, mode, limit, d, dp, None)

    a, b, c = MORPH_SYMBOLS
    cases = [
        (a, lambda: close(s=None), -1, "null pointer"), (a, lambda: close(d=None), -1, "null pointer"),
        (a, lambda: close(t=-1), -1, "thresh"), (a, lambda: close(t=256), -1, "thresh"),
        (a, lambda: close(c=-1), -2, "c = -1"), (a, lambda: close(c=9), -2, "c = 9"),
        (a, lambda: close(hp=0), -2, "bad shape"), (a, lambda: close(wp=-3), -2, "bad shape"),
        (a, lambda: close(sp=30), -2, "pitch"), (a, lambda: close(dp=30), -2, "pitch"),
        (a, lambda: close(d=odd), -1, "overlap"),                                          # in place
        (a, lambda: close(d=ctypes.c_void_p(base + 1 + 19 * 33 + 30)), -1, "overlap"),     # dst starts on the last byte of src
        (a, lambda: close(s=ctypes.c_void_p(base + (1 << 20) + 19 * 31 + 30)), -1, "overlap"),
        (b, lambda: comp(p=None), -1, "null pointer"), (b, lambda: comp(lab=None), -1, "null pointer"), (b, lambda: comp(ar=None), -1, "null pointer"),
        (b, lambda: comp(t=-1), -1, "thresh"), (b, lambda: comp(t=256), -1, "thresh"),
        (b, lambda: comp(bg=2), -1, "background"), (b, lambda: comp(bg=-1), -1, "background"),
        (b, lambda: comp(hp=0), -2, "bad shape"), (b, lambda: comp(wp=0), -2, "bad shape"),
        (b, lambda: comp(pitch=30), -2, "pitch"),
        (b, lambda: comp(hp=1 << 15, wp=1 << 15, pitch=1 << 15), -2, "2^30"), (b, lambda: comp(hp=1, wp=1 << 30, pitch=1 << 30), -2, "2^30"),
        (b, lambda: comp(lab=odd), -4, "4-byte aligned"), (b, lambda: comp(ar=two), -4, "4-byte aligned"),
        (c, lambda: select(lab=None), -1, "null pointer"), (c, lambda: select(ar=None), -1, "null pointer"), (c, lambda: select(d=None), -1, "null pointer"),
        (c, lambda: select(mode=2), -1, "mode"), (c, lambda: select(mode=-1), -1, "mode"),
        (c, lambda: select(limit=-1), -1, "limit"),
        (c, lambda: select(hp=0), -2, "bad shape"), (c, lambda: select(wp=0), -2, "bad shape"),
        (c, lambda: select(dp=30), -2, "pitch"),
        (c, lambda: select(hp=1 << 15, wp=1 << 15, dp=1 << 15), -2, "2^30"),
        (c, lambda: select(lab=odd), -4, "4-byte aligned"), (c, lambda: select(ar=two), -4, "4-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)


# ---- Python validation -------------------------------------------------------------------------------------------------------------------------------------
def test_morph_refusals_cpu(monkeypatch):
    """Each refusal comes with the sibling wrappers' exception and before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops, tissue
    from toad_amd.eval import _SEGMENT_KEYS, region_tissue_attention_heatmap, region_tissue_attention_scores
    from toad_amd.tissue import segment_tissue, segmented_tissue_origins

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    assert ops.SEG_CLOSES == tuple(range(9)) and _SEGMENT_KEYS[-3:] == ("close", "min_area", "min_hole")
    cpu = torch.zeros(30, 40, dtype=torch.uint8)
    for call in (lambda: ops.plane_close(cpu, 4, 8), lambda: ops.plane_components(cpu, 8, 0),
                 lambda: ops.plane_area_select(torch.zeros(30, 40, dtype=torch.int32), torch.zeros(1200, dtype=torch.int32), 0, 5),
                 lambda: segmented_tissue_origins(torch.zeros(300, 520, 3, dtype=torch.uint8), 64, down=1, close=4),
                 lambda: segment_tissue(torch.zeros(300, 520, 3, dtype=torch.uint8), min_hole=5)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    pl = torch.zeros(30, 80, dtype=torch.uint8, device="meta")[:, :40]
    reg = torch.zeros(300, 1040, 3, dtype=torch.uint8, device="meta")[:, :520]
    lab, ar = torch.zeros(30, 40, dtype=torch.int32, device="meta"), torch.zeros(1200, dtype=torch.int32, device="meta")
    for bad in (-1, 9, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="close must be one of"):
            ops.plane_close(pl, bad, 8)
        with pytest.raises(ValueError, match="close must be one of"):
            segmented_tissue_origins(reg, 64, down=1, close=bad)
        with pytest.raises(ValueError, match="close must be one of"):
            segment_tissue(reg, close=bad)
    for bad in (-1, 2.0, "5", None, True):
        with pytest.raises(ValueError, match="min_area must be a non-negative int"):
            segmented_tissue_origins(reg, 64, down=1, min_area=bad)
        with pytest.raises(ValueError, match="min_hole must be a non-negative int"):
            segment_tissue(reg, min_hole=bad)
        with pytest.raises(ValueError, match="limit must be a non-negative int"):
            ops.plane_area_select(lab, ar, 0, bad)
    for bad in (-1, 256, 8.0, None, True):
        with pytest.raises(ValueError, match=r"thresh must be an int in \[0, 255\]"):
            ops.plane_close(pl, 4, bad)
        with pytest.raises(ValueError, match=r"thresh must be an int in \[0, 255\]"):
            ops.plane_components(pl, bad, 0)
    for bad in (2, -1, None, True, 1.0):
        with pytest.raises(ValueError, match="background must be 0 or 1"):
            ops.plane_components(pl, 8, bad)
        with pytest.raises(ValueError, match="mode must be 0"):
            ops.plane_area_select(lab, ar, bad, 5)
    with pytest.raises(TypeError, match="uint8"):
        ops.plane_close(pl.float(), 4, 8)
    with pytest.raises(ValueError, match=r"\[Hp,Wp\]"):
        ops.plane_components(reg, 8, 0)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        ops.plane_close(reg[:, :, 0], 4, 8)
    with pytest.raises(TypeError, match="int32"):
        ops.plane_area_select(lab.long(), ar, 0, 5)
    with pytest.raises(ValueError, match=r"area int32 \[Hp \* Wp\]"):
        ops.plane_area_select(lab, ar[:-1], 0, 5)
    for fn in (region_tissue_attention_scores, region_tissue_attention_heatmap):
        with pytest.raises(ValueError, match="close must be one of"):
            fn(None, None, reg, tile=64, segment=dict(down=1, close=11))
        with pytest.raises(ValueError, match="min_hole must be a non-negative int"):
            fn(None, None, reg, tile=64, segment=dict(down=1, min_hole=-2))
    # empty planes and lattices: empty results, nothing launched, whatever the three keywords say
    small = torch.zeros(40, 50, 3, dtype=torch.uint8, device="meta")
    o, t = segmented_tissue_origins(small, 64, down=1, close=4, min_area=50, min_hole=50, return_threshold=True)
    assert o.shape == (0, 2) and t == 8
    empty = torch.zeros(0, 5, dtype=torch.uint8, device="meta")
    assert tuple(ops.plane_close(empty, 4, 8).shape) == (0, 5)
    labels, area = ops.plane_components(empty, 8, 1)
    assert tuple(labels.shape) == (0, 5) and labels.dtype == torch.int32 and tuple(area.shape) == (0,)
    assert tuple(ops.plane_area_select(labels, area, 1, 3).shape) == (0, 5)
    # with the three keywords at their defaults - or at their other inactive values - the new wrappers are never reached
    for name in ("plane_close", "plane_components", "plane_area_select"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("a new wrapper was reached")))
    reached = []

    def stop(*a, **k):
        reached.append(a[1:])
        raise KeyError("as far as today's path")
    monkeypatch.setattr(ops, "region_saturation", stop)
    for kw in (dict(), dict(close=0, min_area=0, min_hole=0), dict(close=1, min_area=1)):
        with pytest.raises(KeyError):
            segmented_tissue_origins(reg, 64, down=1, **kw)
        with pytest.raises(KeyError):
            segment_tissue(reg, **kw)
    assert len(reached) == 6
    assert tissue._morph_args(0, 0, 0) is False and tissue._morph_args(1, 1, 0) is False
    assert tissue._morph_args(2, 0, 0) and tissue._morph_args(0, 2, 0) and tissue._morph_args(0, 0, 1)


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(9))
def test_reference_closing_against_a_plain_loop(c):
    rng = np.random.default_rng(c)
    lo, hi = c // 2, c - 1 - c // 2
    for m0 in (rng.random((9, 11)) < 0.3, rng.random((12, 7)) < 0.6, rng.random((2, 3)) < 0.5, np.ones((1, 1), dtype=bool), ref.serpentine(10, 9)):
        hp, wp = m0.shape
        if c <= 1:
            assert np.array_equal(ref.closing(m0, c), m0)
            continue
        d = np.zeros_like(m0)
        for y in range(hp):
            for x in range(wp):
                d[y, x] = any(m0[v, u] for v in range(max(y - lo, 0), min(y + hi, hp - 1) + 1) for u in range(max(x - lo, 0), min(x + hi, wp - 1) + 1))
        want = np.zeros_like(m0)
        for y in range(hp):
            for x in range(wp):
                want[y, x] = all(d[v, u] for v in range(max(y - lo, 0), min(y + hi, hp - 1) + 1) for u in range(max(x - lo, 0), min(x + hi, wp - 1) + 1))
        got = ref.closing(m0, c)
        assert np.array_equal(got, want), m0.shape
        if c % 2:
            assert not (m0 & ~got).any()                               # an odd window is symmetric: closing is extensive, nothing set is cleared
    # by hand. c = 3 closes gaps of one and two pixels. c = 2 (lo = 1, hi = 0): D[x] = M0[x-1] | M0[x], M1[x] = D[x-1] & D[x] - both halves look the same way,
    # so the gap of one closes and everything moves one pixel to the right (the last pixel leaves its place): the shift of an even c
    row = np.array([[1, 0, 1, 0, 0, 1]], dtype=bool)
    assert ref.closing(row, 3).astype(int).tolist() == [[1, 1, 1, 1, 1, 1]]
    assert ref.closing(row, 2).astype(int).tolist() == [[1, 1, 1, 1, 0, 0]]
    lone = np.zeros((21, 21), dtype=bool)
    lone[10, 10] = True
    for k in range(9):
        moved = np.zeros_like(lone)
        moved[10 + (k > 0 and k % 2 == 0), 10 + (k > 0 and k % 2 == 0)] = True
        assert np.array_equal(ref.closing(lone, k), moved), k
    # the window is clipped to the plane: on a plane smaller than the window one set pixel fills everything
    assert ref.closing(lone[8:13, 8:13], 8).all()


@pytest.mark.parametrize("hp,wp", SHAPES)
def test_reference_components_against_a_flood_fill(hp, wp):
    for name, m in ref.patterns(hp, wp).items():
        for sel, conn in ((m, 8), (~m, 4)):
            labels, area = ref.components(sel, conn)
            fl, fa = flood_components(sel, conn)
            assert np.array_equal(labels, fl) and np.array_equal(area, fa), (name, conn)
            assert (labels[sel] >= 0).all() and (labels[~sel] == -1).all() and int((area & ref.COUNT).sum()) == int(sel.sum())
            plane = np.where(m, 200, 3)
            pl, pa = ref.plane_components(plane, 8, 0 if conn == 8 else 1)
            assert np.array_equal(pl, labels) and np.array_equal(pa, area)


def test_reference_components_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, m in ref.patterns(63, 65).items():
        for sel, conn in ((m, 8), (~m, 4)):
            lab, n = ndimage.label(sel, structure=np.ones((3, 3)) if conn == 8 else None)
            idx = np.arange(sel.size).reshape(sel.shape)
            first = ndimage.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
            want = np.where(lab > 0, np.concatenate([[-1], first])[lab], -1)
            assert np.array_equal(ref.components(sel, conn)[0], want), (name, conn)


def test_reference_components_by_hand():
    two = np.array([[1, 0], [0, 1]], dtype=bool)                       # two pixels touching diagonally
    l8, a8 = ref.components(two, 8)
    l4, a4 = ref.components(two, 4)
    assert l8.tolist() == [[0, -1], [-1, 0]] and a8.tolist() == [2 + ref.BORDER, 0, 0, 0]
    assert l4.tolist() == [[0, -1], [-1, 3]] and a4.tolist() == [1 + ref.BORDER, 0, 0, 1 + ref.BORDER]
    # a background pocket linked to the border ring only diagonally is a hole: the background is 4-connected
    m = np.ones((5, 5), dtype=bool)
    m[0, 0] = m[1, 1] = False
    labels, area = ref.components(~m, 4)
    assert labels[0, 0] == 0 and labels[1, 1] == 6 and area[0] == 1 + ref.BORDER and area[6] == 1
    assert ref.fill_holes(m, 2)[1, 1] and not ref.fill_holes(m, 2)[0, 0] and not ref.fill_holes(m, 1)[1, 1]
    # ... while the tissue is 8-connected: the same two pixels as tissue are one component of two
    assert ref.components(~m, 8)[1].tolist()[0] == 2 + ref.BORDER
    # the selections' edges: kept iff count >= limit, filled iff count < limit
    blob = np.zeros((7, 9), dtype=bool)
    blob[1:3, 1:4] = True                                              # 6 pixels
    blob[5, 6:8] = True                                                # 2 pixels
    assert ref.drop_small(blob, 2).sum() == 8 and ref.drop_small(blob, 3).sum() == 6 and ref.drop_small(blob, 6).sum() == 6
    assert ref.drop_small(blob, 7).sum() == 0 and ref.drop_small(blob, 0).sum() == 8 and ref.drop_small(blob, 1).sum() == 8
    ring = np.zeros((7, 9), dtype=bool)
    ring[1:6, 1:7] = True
    ring[2:4, 2:5] = False                                             # a hole of 6
    assert ref.fill_holes(ring, 6).sum() == ring.sum() and ref.fill_holes(ring, 7).sum() == ring.sum() + 6 and ref.fill_holes(ring, 0).sum() == ring.sum()
    assert ref.fill_holes(ring, 1 << 29).sum() == ring.sum() + 6       # the background outside touches the border: never filled
    # an island removed in 6b merges into the hole around it before 6c counts the hole
    isl = ring.copy()
    isl[3, 3] = True                                                   # hole of 5 around an island of 1
    both = ref.fill_holes(ref.drop_small(isl, 2), 7)
    assert both.sum() == ring.sum() + 6 and ref.fill_holes(isl, 6).sum() == isl.sum() + 5 and ref.fill_holes(isl, 5).sum() == isl.sum()


def test_patterns_are_what_the_gpu_tests_take_them_for():
    hp, wp = 130, 257
    p = ref.patterns(hp, wp)
    inner, outer = ref.component_sizes(p["checkerboard"], 8)
    assert inner == [] and outer == [(hp * wp + 1) // 2]               # one 8-component
    inner, outer = ref.component_sizes(~p["checkerboard"], 4)
    assert set(inner + outer) == {1} and len(inner + outer) == hp * wp // 2      # the complement: all singletons
    for name in ("spiral_in", "spiral_out"):
        inner, outer = ref.component_sizes(p[name], 8)
        assert inner == [] and len(outer) == 1 and outer[0] > hp * wp // 3, name            # one long chain
        labels, _ = ref.components(p[name], 8)
        n8 = sum(np.roll(np.roll(np.pad(p[name], 1), dy, 0), dx, 1)[1:-1, 1:-1] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
        assert (n8[p[name]] <= 2).mean() > 0.9, name                   # ... of pixels with two neighbours (more only next to a corner)
        binner, bouter = ref.component_sizes(~p[name], 4)
        assert len(binner + bouter) <= 3 and max(binner + bouter) > hp * wp // 3, name       # and its complement another
    assert ref.components(p["spiral_in"], 8)[0].max() == 0 and p["spiral_out"][-1, -1] and np.array_equal(p["spiral_out"][::-1, ::-1], p["spiral_in"])
    inner, outer = ref.component_sizes(p["serpentine"], 4)
    assert inner == [] and len(outer) == 1
    inner, outer = ref.component_sizes(p["rings"], 8)
    assert len(outer) == 1 and len(inner) == 32                        # rings at distance 0, 2 .. 64 from the border: nested, the outermost on the border
    binner, bouter = ref.component_sizes(~p["rings"], 4)
    assert bouter == [] and len(binner) == 32                          # every background ring (distance 1, 3 .. 63) is a hole
    for name in ("corners", "corners_anti"):
        n = ((hp - 1) // 16) * ((wp - 1) // 16)
        inner, outer = ref.component_sizes(p[name], 8)
        assert inner + outer == [2] * n and p[name].sum() == 2 * n, name
        assert sum(ref.component_sizes(p[name], 4), []) == [1] * (2 * n), name
    assert p["corners"][15, 63] and p["corners"][16, 64] and p["corners_anti"][15, 64] and p["corners_anti"][16, 63] and p["corners"][63, 63]
    big = ref.component_sizes(p["random0.593"], 4)                     # near the site-percolation threshold: large, winding components
    assert max(big[0] + big[1]) > 2000


# ---- the end-to-end cases ------------------------------------------------------------------------------------------------------------------------------------
def test_holey_slide_has_the_features():
    """At down = 1, median = 3, t = 8: the figures of the reference on holey_slide(300, 520, 1), pinned."""
    key = ref.E2E_KEY
    plane, t = ref.segmented(None, 1, 3, 8, key=key)
    m0 = plane > t
    inner, outer = ref.component_sizes(m0, 8)
    assert inner == [109, 349, 1506, 6457, 9502] and outer == [1486, 24620]          # speck, island, speck, blob, rectangle; margin, ellipse with the band
    holes, open_bg = ref.component_sizes(~m0, 4)
    assert holes == [90, 114, 115, 1230, 3700] and open_bg == [1, 40471, 66250]
    assert int((ref.closing(m0, 4) != m0).sum()) == 2416
    # small hole, what the median left of the crack (two slits), medium hole, large hole around its island; closing heals the slits
    assert ref.component_sizes(~ref.closing(m0, 4), 4)[0] == [90, 1227, 3700]
    assert np.array_equal(seg.saturation_plane(ref.holey_slide(*key), 1)[:20], seg.saturation_plane(seg.slide(*key), 1)[:20])     # slide's own top rows


def test_every_stage_acts_on_every_end_to_end_case():
    key = ref.E2E_KEY
    tile, stride, origin = ref.E2E_LATTICE
    ran = 0
    for down, median in ref.E2E_DM:
        assert seg.lattice_allowed(ref.E2E_LATTICE, down)
        for sat in ref.E2E_SAT:
            _, c0, t0 = ref.selection(None, tile, stride, origin, 0.25, down, median, sat, key=key)
            for close, min_area, min_hole in ref.e2e_configs(down):
                m0, m1, m2, m3, t = ref.stages(None, down, median, sat, 0, close, min_area, min_hole, key=key)
                assert t == t0 and (close > 1) == bool((m1 != m0).any()) and (min_area > 1) == bool((m2 != m1).any())
                assert (min_hole > 0) == bool((m3 != m2).any()), (down, sat, close, min_area, min_hole)
                if min_area:
                    _, area = ref.components(m1, 8)
                    counts = area[area > 0] & ref.COUNT
                    assert (counts < min_area).any() and (counts >= min_area).any()        # some components go, some stay
                    assert not (m2 & ~m1).any()
                if min_hole:
                    _, area = ref.components(~m2, 4)
                    a = area[area > 0]
                    holes = a[a < ref.BORDER]
                    assert (holes < min_hole).any() and (holes >= min_hole).any() and (a >= ref.BORDER).any()      # filled, kept, and open background
                    assert not (m2 & ~m3).any()
                origins, c, _ = ref.selection(None, tile, stride, origin, 0.25, down, median, sat, 0, close, min_area, min_hole, key=key)
                assert (c != c0).any() and 0 < len(origins) < c.size
                ran += 1
    assert ran == 24
