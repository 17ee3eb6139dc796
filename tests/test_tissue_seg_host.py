"""CPU: segmented tissue selection (toad_region_saturation_u8, toad_plane_median_u8, toad_plane_cells_u8: an additive extension of ABI 15;
toad_amd/tissue.py otsu_threshold, segment_tissue, segmented_tissue_origins). The entry points exist in the header, the library and the ctypes table and
refuse what the host can see before any device access; Otsu's threshold is host code; and the numpy reference the GPU tests compare against
(tests/tissue_seg_ref.py) is itself tested here, on the inputs of those tests: every "mixed outcome" condition the GPU tests rely on is a fact about the
reference alone."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import tissue_ref as ref0
from tests import tissue_seg_ref as ref

SEG_SYMBOLS = ("toad_region_saturation_u8", "toad_plane_median_u8", "toad_plane_cells_u8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E2E_DM, E2E_SAT, E2E_LATTICES, lattice_allowed = ref.E2E_DM, ref.E2E_SAT, ref.E2E_LATTICES, ref.lattice_allowed


def otsu_by_fractions(h):
    """Definition 5 once more, with fractions.Fraction doing the comparison."""
    h = [int(v) for v in h]
    n, mt = sum(h), sum(i * v for i, v in enumerate(h))
    best, best_v = 0, None
    w0 = m0 = 0
    for t in range(255):
        w0, m0 = w0 + h[t], m0 + t * h[t]
        if w0 > 0 and n - w0 > 0:
            v = Fraction((mt * w0 - m0 * n) ** 2, w0 * (n - w0))
            if best_v is None or v > best_v:
                best, best_v = t, v
    return best


def otsu_histograms():
    """200 random histograms of mixed character, and the special cases: (name, hist, expected threshold or None)."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(200):
        kind = i % 4
        if kind == 0:
            h = rng.integers(0, 1000, size=256)
        elif kind == 1:                                              # sparse: most bins empty
            h = rng.integers(0, 50, size=256) * (rng.random(256) < 0.05)
        elif kind == 2:                                              # two humps
            x = np.arange(256)
            a, b = rng.integers(0, 128), rng.integers(128, 256)
            h = (5000 * np.exp(-((x - a) / 9.0) ** 2) + 3000 * np.exp(-((x - b) / 14.0) ** 2)).astype(np.int64) + rng.integers(0, 3, size=256)
        else:                                                        # a few large bins
            h = np.zeros(256, dtype=np.int64)
            h[rng.integers(0, 256, size=rng.integers(1, 6))] = rng.integers(1, 1 << 25, size=1)
        out.append((f"random{i}", [int(v) for v in h], None))
    one = [0] * 256
    one[77] = 12345
    spikes = [0] * 256
    spikes[10] = spikes[200] = 500
    big = [int(v) for v in (1 << 25) - np.random.default_rng(6).integers(0, 1000, size=256)]
    out += [("one bin", one, 0), ("empty", [0] * 256, 0), ("two equal spikes", spikes, 10), ("near 2^25 per bin", big, None)]
    return out


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------------------
def test_seg_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in SEG_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    # the header states the definition and what it is not
    assert "S = (255 * (mx - mn) + (mx >> 1)) / mx" in header and "NOT claimed to be bit-equal to OpenCV" in header
    assert "(MT * W0 - M0 * N)^2 / (W0 * W1)" in header and "replicate border" in header


def test_seg_entries_report_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    base = 1 << 21
    one = ctypes.c_void_p(base)                               # non-null fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p(base + 1)                           # regions and planes at odd addresses are fine; int32 arrays there are refused
    two = ctypes.c_void_p(base + 2)
    far = ctypes.c_void_p(base + (1 << 20))

    def sat(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, down=2, vmin=0, p=far, pp=15):
        return lib.toad_region_saturation_u8(r, pitch, hr, wr, down, vmin, p, pp, None)

    def med(s=odd, sp=33, hp=20, wp=31, k=3, d=far, dp=31, h=one):
        return lib.toad_plane_median_u8(s, sp, hp, wp, k, d, dp, h, None)

    def cells(p=odd, pitch=33, hp=20, wp=31, cell=16, t=8, c=one):
        return lib.toad_plane_cells_u8(p, pitch, hp, wp, cell, t, c, None)

    a, b, c = SEG_SYMBOLS
    cases = [
        (a, lambda: sat(r=None), -1, "null pointer"), (a, lambda: sat(p=None), -1, "null pointer"),
        (a, lambda: sat(vmin=-1), -1, "val_min"), (a, lambda: sat(vmin=256), -1, "val_min"),
        (a, lambda: sat(down=3), -2, "down = 3"), (a, lambda: sat(down=0), -2, "down"), (a, lambda: sat(down=64), -2, "down"),
        (a, lambda: sat(hr=0), -2, "bad shape"), (a, lambda: sat(wr=-1), -2, "bad shape"),
        (a, lambda: sat(pitch=3 * 31 - 1), -2, "pitch"), (a, lambda: sat(pitch=0), -2, "pitch"),
        (a, lambda: sat(pp=14), -2, "plane_pitch"), (a, lambda: sat(down=1, pp=30), -2, "plane_pitch"),
        (a, lambda: sat(wr=715827883, pitch=1 << 32, pp=1 << 30), -2, "2^31"),
        (b, lambda: med(s=None), -1, "null pointer"), (b, lambda: med(d=None), -1, "null pointer"),
        (b, lambda: med(k=4), -2, "k = 4"), (b, lambda: med(k=0), -2, "k = 0"), (b, lambda: med(k=9), -2, "k = 9"), (b, lambda: med(k=-3), -2, "k"),
        (b, lambda: med(hp=0), -2, "bad shape"), (b, lambda: med(wp=0), -2, "bad shape"),
        (b, lambda: med(sp=30), -2, "pitch"), (b, lambda: med(dp=30), -2, "pitch"),
        (b, lambda: med(d=odd), -1, "overlap"),                                        # in place
        (b, lambda: med(d=ctypes.c_void_p(base + 1 + 19 * 33 + 30)), -1, "overlap"),   # dst starts on the last byte of src
        (b, lambda: med(s=ctypes.c_void_p(base + (1 << 20) + 19 * 31 + 30)), -1, "overlap"),   # src starts on the last byte of dst
        (b, lambda: med(h=odd), -4, "4-byte aligned"), (b, lambda: med(h=two), -4, "4-byte aligned"),
        (c, lambda: cells(p=None), -1, "null pointer"), (c, lambda: cells(c=None), -1, "null pointer"),
        (c, lambda: cells(t=-1), -1, "thresh"), (c, lambda: cells(t=256), -1, "thresh"),
        (c, lambda: cells(cell=12), -2, "cell"), (c, lambda: cells(cell=2), -2, "cell"), (c, lambda: cells(cell=128), -2, "cell"),
        (c, lambda: cells(hp=0), -2, "bad shape"), (c, lambda: cells(wp=0), -2, "bad shape"),
        (c, lambda: cells(pitch=30), -2, "pitch"),
        (c, lambda: cells(c=odd), -4, "4-byte aligned"), (c, lambda: cells(c=two), -4, "4-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)
    # the first address after src is a legal dst: only the later alignment check stops this call
    assert med(d=ctypes.c_void_p(base + 1 + 19 * 33 + 31), h=odd) == -4
    # an empty plane is no error and launches nothing (a 3-row region at down = 4, a 1-column region at down = 2)
    assert sat(hr=3, down=4, pp=7) == 0 and sat(wr=1, pitch=3, down=2, pp=0) == 0


# ---- Otsu ------------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_otsu_against_fractions_and_the_special_cases():
    for name, h, want in otsu_histograms():
        got = ref.otsu(h)
        assert got == otsu_by_fractions(h), name
        if want is not None:
            assert got == want, name


def test_otsu_threshold_equals_the_reference():
    from toad_amd.tissue import otsu_threshold
    for name, h, want in otsu_histograms():
        assert otsu_threshold(h) == ref.otsu(h), name
    _, h, _ = otsu_histograms()[2]
    assert otsu_threshold(np.array(h, dtype=np.int32)) == otsu_threshold(torch.tensor(h, dtype=torch.int32)) == otsu_threshold(tuple(h)) == ref.otsu(h)
    assert isinstance(otsu_threshold(h), int)
    with pytest.raises(ValueError, match="256"):
        otsu_threshold([1] * 255)
    with pytest.raises(ValueError, match="negative"):
        otsu_threshold([1] * 255 + [-1])


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_saturation_by_hand_and_on_every_pair():
    px = np.array([[[0, 0, 0], [1, 0, 0], [128, 128, 128], [255, 247, 255], [200, 100, 150], [3, 2, 3], [255, 254, 255]]], dtype=np.uint8)
    # (255, 247, 255): (2040 + 127) // 255 = 8; (200, 100, 150): (25500 + 100) // 200 = 128; (3, 2, 3): (255 + 1) // 3 = 85; (255, 254, 255): 382 // 255 = 1
    assert ref.saturation_plane(px, 1).tolist() == [[0, 255, 0, 8, 128, 85, 1]]
    assert ref.saturation_plane(px, 1, 4).tolist() == [[0, 0, 0, 8, 128, 0, 1]]
    img, mx, mn = ref.probe_blocks()
    s = ref.saturation_plane(img, 1)
    probe = s.reshape(384, 4, 257, 4).max(axis=(1, 3))             # everything but the probe is grey: S = 0
    want = np.array([[round(Fraction(255 * int(a - b), int(a)) + Fraction(1, 10 ** 9)) if a else 0 for a, b in zip(ra, rb)] for ra, rb in zip(mx[::16], mn[::16])])
    assert np.array_equal(probe[::16], want)                        # round half up, by fractions, on a sixteenth of the rows
    assert int(s.sum()) == int(probe.sum()) and probe.max() == 255
    # a box filter by hand: the 2 x 2 mean of (10, 20, 30), (11, 21, 31), (12, 22, 33), (13, 23, 33) is (12, 22, 32): (46 + 2) // 4, (86 + 2) // 4, (127 + 2) // 4
    box = np.array([[[10, 20, 30], [11, 21, 31], [9, 9, 9]], [[12, 22, 33], [13, 23, 33], [9, 9, 9]], [[7, 7, 7]] * 3], dtype=np.uint8)
    assert ref.saturation_plane(box, 2).tolist() == [[(255 * 20 + 16) // 32]]
    assert ref.saturation_plane(box, 4).shape == (0, 0) and ref.saturation_plane(box[:, :1], 2).shape == (1, 0)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_reference_median_against_a_plain_loop(k):
    rng = np.random.default_rng(k)
    for plane in (rng.integers(0, 256, size=(9, 11)), rng.integers(0, 4, size=(9, 11)), rng.integers(0, 256, size=(2, 3)), rng.integers(0, 256, size=(1, 1))):
        hp, wp = plane.shape
        want = np.zeros_like(plane)
        for y in range(hp):
            for x in range(wp):
                win = sorted(int(plane[min(max(y + dy, 0), hp - 1), min(max(x + dx, 0), wp - 1)]) for dy in range(-(k // 2), k // 2 + 1)
                             for dx in range(-(k // 2), k // 2 + 1))
                want[y, x] = win[(k * k) // 2]
        assert np.array_equal(ref.median_plane(plane, k), want)
    assert np.array_equal(ref.median_plane(plane, 1), plane)
    assert np.array_equal(ref.histogram(np.array([[0, 255, 3], [3, 3, 0]]))[[0, 3, 255]], [2, 3, 1]) and ref.histogram(np.zeros((0, 4))).sum() == 0


@pytest.mark.parametrize("key,down,want", [((300, 520, 1), 1, 61), ((300, 520, 1), 4, 59), ((300, 520, 1), 16, 56),
                                           ((1024, 2048, 2), 1, 60), ((1024, 2048, 2), 4, 59), ((1024, 2048, 2), 16, 57)])
def test_pinned_otsu_thresholds_of_the_slides(key, down, want):
    """Values computed with a throwaway numpy prototype of the definitions when the feature was specified. Otsu's threshold separates the pink tissue from
    the rest, pale blob included: its tissue share is below the share at sat_thresh = 8, which keeps the blob."""
    from toad_amd.tissue import otsu_threshold
    s = ref.slide(*key)
    for k in (1, 3, 7):
        plane, t = ref.segmented(s, down, k, "otsu", key=key)
        assert t == want == otsu_threshold(ref.histogram(plane)), (k, t)
        assert 0 < (plane > t).mean() < (plane > 8).mean() < 1, k
    if (key, down) == ((300, 520, 1), 1):
        plane, t = ref.segmented(s, 1, 7, "otsu", key=key)
        assert round(float((plane > t).mean()), 4) == 0.2616 and round(float((plane > 8).mean()), 4) == 0.3031


def test_dust_is_tissue_per_pixel_and_gone_after_the_median():
    d = ref.dusty_glass(64, 64, 1)
    assert int(ref0.tissue_mask(d, 8, 0).sum()) == 64                # the 8 x 8 red pixels, and nothing else
    sat = ref.saturation_plane(d, 1)
    assert int((sat > 8).sum()) == 64 and sat.max() == 255
    assert ref.median_plane(sat, 3).max() <= 2
    big = ref.dusty_glass(256, 256, 1)                               # the GPU test's input: every 64 x 64 tile holds 64 red pixels = 1 / 64 of its area
    every, total, _ = ref.selection(big, (64, 64), (64, 64), (0, 0), 1 / 64, 1, 1, 8)
    none, _, _ = ref.selection(big, (64, 64), (64, 64), (0, 0), 1 / 64, 1, 3, 8)
    assert total == 16 and len(every) == 16 and len(none) == 0
    assert len(ref0.selection(big, (64, 64), (64, 64), (0, 0), 1 / 64, 8, 0)[0]) == 16


def test_reference_selection_is_mixed_on_the_end_to_end_cases():
    key = (300, 520, 1)
    s = ref.slide(*key)
    ran = mixed = 0
    for down, median in E2E_DM:
        for lat in E2E_LATTICES:
            if not lattice_allowed(lat, down):
                continue
            tile, stride, origin = lat
            for sat in E2E_SAT:
                every, total, t = ref.selection(s, tile, stride, origin, 0, down, median, sat, key=key)
                assert len(every) == total > 0 and every[0].tolist() == list(origin)
                assert t == (ref.segmented(s, down, median, "otsu", key=key)[1] if sat == "otsu" else sat)
                some, _, _ = ref.selection(s, tile, stride, origin, 0.25, down, median, sat, key=key)
                full, _, _ = ref.selection(s, tile, stride, origin, 1, down, median, sat, key=key)
                assert len(full) <= len(some) <= total
                ran += 1
                mixed += 0 < len(some) < total
                # the tile sums equal the sums of the 4 x 4 cells of the plane: the route the device takes
                plane, _ = ref.segmented(s, down, median, sat, key=key)
                c4 = ref.plane_cell_counts(plane, 4, t)
                tc = ref.tile_counts(plane, t, tile, stride, origin, down, (300, 520))
                ys, xs, ph, pw = origin[1] // down // 4, origin[0] // down // 4, tile[0] // down // 4, tile[1] // down // 4
                assert tc[0, 0] == c4[ys:ys + ph, xs:xs + pw].sum()
    assert ran == 24 and mixed == ran                                # the rule admits both lattices at every down here; every case keeps some but not all tiles
    key = (1024, 2048, 2)
    some, total, _ = ref.selection(ref.slide(*key), (256, 256), (256, 256), (0, 0), 0.25, 16, 7, 8, key=key)
    assert total == 32 and 0 < len(some) < total
    key = (48, 1100, 1)                                              # the pipeline case: 3 x 4 tiles of 16 x 256
    some, total, t = ref.selection(ref.slide(*key), (16, 256), (16, 256), (0, 0), 0.25, 4, 3, "otsu", key=key)
    assert total == 12 and 0 < len(some) < total and t > 8
    assert len(ref.selection(ref.slide(*key), (16, 256), (16, 256), (0, 0), 0.25, 4, 3, 255, key=key)[0]) == 0


# ---- Python validation -------------------------------------------------------------------------------------------------------------------------------------
def test_segmented_refusals_cpu(monkeypatch):
    """Each refusal comes with the region wrappers' exception and before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.eval import region_tissue_attention_heatmap, region_tissue_attention_scores
    from toad_amd.tissue import segment_tissue, segmented_tissue_origins

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    region = torch.zeros(300, 520, 3, dtype=torch.uint8)
    calls = (lambda r: segmented_tissue_origins(r, 64, down=1), lambda r: segment_tissue(r), lambda r: ops.region_saturation(r, 4))
    for call in calls:
        with pytest.raises(RuntimeError, match="CUDA"):
            call(region)                                               # on the CPU
    for call in (lambda p: ops.plane_median(p, 3), lambda p: ops.plane_cells(p, 16, 8)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call(region[..., 0])
    # what comes after the device test, on a stand-in that claims to be on the device
    meta = torch.zeros(300, 1040, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for call in calls:
        with pytest.raises(TypeError, match="uint8"):
            call(meta.float())
        with pytest.raises(ValueError, match=r"stride\(1\) == 3"):
            call(meta[:, ::2])
    reg = meta[:, :520]
    pl = torch.zeros(30, 80, dtype=torch.uint8, device="meta")[:, :40]
    for bad in (0, 3, 64, "4", None):
        with pytest.raises(ValueError, match="down must be one of"):
            segmented_tissue_origins(reg, 256, down=bad)
        with pytest.raises(ValueError, match="down must be one of"):
            ops.region_saturation(reg, bad)
    for bad in (0, 2, 4, 9, -3, "7"):
        with pytest.raises(ValueError, match="median must be one of"):
            segmented_tissue_origins(reg, 64, down=1, median=bad)
        with pytest.raises(ValueError, match="k must be one of"):
            ops.plane_median(pl, bad)
    for bad in (-1, 256, 8.0, "Otsu", None, True):
        with pytest.raises(ValueError, match=r"sat_thresh must be 'otsu' or an int in \[0, 255\]"):
            segmented_tissue_origins(reg, 64, down=1, sat_thresh=bad)
        with pytest.raises(ValueError, match="sat_thresh"):
            segment_tissue(reg, sat_thresh=bad)
    for bad in (-1, 256, 1.0):
        with pytest.raises(ValueError, match=r"val_min must be an int in \[0, 255\]"):
            segmented_tissue_origins(reg, 64, down=1, val_min=bad)
    for bad in (-0.01, 1.01, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="min_fraction"):
            segmented_tissue_origins(reg, 64, down=1, min_fraction=bad)
    # the lattice: every number a multiple of 4 * down, and the message names the value and down
    with pytest.raises(ValueError, match=r"tile height = 64 is not a multiple of 4 \* down = 128 \(down = 32\)"):
        segmented_tissue_origins(reg, 64, down=32)
    with pytest.raises(ValueError, match=r"stride x = 32 .*4 \* down = 64 \(down = 16\)"):
        segmented_tissue_origins(reg, 64, (64, 32), down=16)
    with pytest.raises(ValueError, match=r"origin y = 8 .*down = 4"):
        segmented_tissue_origins(reg, 64, 32, origin=(16, 8), down=4)
    with pytest.raises(ValueError, match=r"tile width = 30 .*down = 1\)"):
        segmented_tissue_origins(reg, (64, 30), down=1)
    with pytest.raises(ValueError, match="cell must be one of"):
        ops.plane_cells(pl, 12, 8)
    with pytest.raises(ValueError, match=r"thresh must be an int in \[0, 255\]"):
        ops.plane_cells(pl, 16, 256)
    with pytest.raises(ValueError, match=r"\[Hp,Wp\]"):
        ops.plane_median(meta, 3)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        ops.plane_median(meta[:, :, 0], 3)                             # stride(1) == 3
    # the eval hooks: an unknown key, or no dict at all
    for fn in (region_tissue_attention_scores, region_tissue_attention_heatmap):
        with pytest.raises(ValueError, match=r"segment must be None or a dict.*\['tile'\]"):
            fn(None, None, reg, tile=64, segment=dict(down=4, tile=64))
        with pytest.raises(ValueError, match="segment must be None or a dict"):
            fn(None, None, reg, tile=64, segment="otsu")
        with pytest.raises(ValueError, match="down must be one of"):
            fn(None, None, reg, tile=64, segment=dict(down=5))
    # an empty lattice or an empty plane: empty results, and still nothing is launched
    small = torch.zeros(40, 50, 3, dtype=torch.uint8, device="meta")
    o = segmented_tissue_origins(small, 64, down=16)
    assert isinstance(o, np.ndarray) and o.shape == (0, 2) and o.dtype == np.int64
    o, c, t = segmented_tissue_origins(small, 64, down=1, sat_thresh="otsu", return_counts=True, return_threshold=True)
    assert o.shape == (0, 2) and c.shape == (0,) and t == 0
    o, t = segmented_tissue_origins(small, 64, down=1, sat_thresh=40, return_threshold=True)
    assert o.shape == (0, 2) and t == 40
    assert tuple(ops.region_saturation(small[:20], 32).shape) == (0, 1)
    assert tuple(ops.plane_median(torch.zeros(0, 5, dtype=torch.uint8, device="meta"), 7).shape) == (0, 5)
