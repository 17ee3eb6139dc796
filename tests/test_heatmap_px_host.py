"""CPU: the per-pixel heat-map blend (toad_region_heat_blend_px_u8: an additive extension of ABI 15; ops.region_heat_blend_px and the smooth / mask /
thresh / binarize keywords of toad_amd/heatmap.py and eval.region_tissue_attention_heatmap). The entry point exists in the header, the library and the
ctypes table and refuses what the host can see before any device access; the score selection is host-testable torch code; and the numpy reference the GPU
tests compare against (tests/heat_px_ref.py) is itself tested here, by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import heat_px_ref as ref
from tests import heat_ref

NAME = "toad_region_heat_blend_px_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_px_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\b" + NAME + r"\s*\(", header), f"{NAME} is not declared in include/toad_hip.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 21
    # the header states the definition
    for text in ("p = 2 * down * ox + down - cell", "g0 = floor(p / (2 * cell))", "f = p - 2 * cell * g0", "(sum wy * wx * v + 2 * cell * cell) >> (2 * log2(cell) + 2)",
                 "mask[my][mx] > mask_thresh", "(alpha * lut[idx_px][c] + (256 - alpha) * m + 128) >> 8"):
        assert text in header, text


def test_px_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # the region, the mask and the canvas may lie at an odd address; int32 cells may not
    two = ctypes.c_void_p((1 << 21) + 2)

    def px(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, c=one, gy=2, gx=2, cell=16, lut=odd, alpha=102, down=2, smooth=1, mask=odd, mpitch=8, hm=5, wm=7, md=4,
           mt=8, out=odd, opitch=3 * 15 + 2):
        return lib.toad_region_heat_blend_px_u8(r, pitch, hr, wr, c, gy, gx, cell, lut, alpha, down, smooth, mask, mpitch, hm, wm, md, mt, out, opitch, None)

    cases = [
        (lambda: px(r=None), -1, "null pointer"), (lambda: px(c=None), -1, "null pointer"), (lambda: px(lut=None), -1, "null pointer"),
        (lambda: px(out=None), -1, "null pointer"),
        (lambda: px(cell=12), -2, "cell"), (lambda: px(cell=2), -2, "cell"), (lambda: px(hr=0), -2, "bad shape"), (lambda: px(wr=-1), -2, "bad shape"),
        (lambda: px(alpha=-1), -2, "alpha"), (lambda: px(alpha=257), -2, "alpha"),
        (lambda: px(down=0), -2, "down"), (lambda: px(down=3), -2, "down"), (lambda: px(down=8), -2, "down"),
        (lambda: px(smooth=2), -1, "smooth"), (lambda: px(smooth=-1), -1, "smooth"),
        (lambda: px(pitch=3 * 31 - 1), -2, "pitch"), (lambda: px(pitch=-94), -2, "pitch"),
        (lambda: px(md=0), -2, "mask_down"), (lambda: px(md=3), -2, "mask_down"), (lambda: px(md=64), -2, "mask_down"), (lambda: px(md=-4), -2, "mask_down"),
        (lambda: px(md=1, hm=20, wm=31, mpitch=31), -2, "multiple of down"),                       # down = 2
        (lambda: px(down=4, md=2, hm=10, wm=15, mpitch=15, opitch=21), -2, "multiple of down"),
        (lambda: px(hm=4), -2, "Hm x Wm"), (lambda: px(hm=6), -2, "Hm x Wm"), (lambda: px(wm=8), -2, "Hm x Wm"), (lambda: px(wm=6), -2, "Hm x Wm"),
        (lambda: px(md=8), -2, "Hm x Wm"),                                                          # 20 // 8 x 31 // 8 = 2 x 3
        (lambda: px(mpitch=6), -2, "mask_pitch"), (lambda: px(mpitch=0), -2, "mask_pitch"), (lambda: px(mpitch=-8), -2, "mask_pitch"),
        (lambda: px(mt=-1), -1, "mask_thresh"), (lambda: px(mt=256), -1, "mask_thresh"),
        (lambda: px(opitch=3 * 15 - 1), -2, "out_pitch"), (lambda: px(down=1, md=4, opitch=3 * 31 - 1), -2, "out_pitch"),
        (lambda: px(wr=715827883, pitch=1 << 32, opitch=1 << 32, gx=44739243, mask=None), -2, "2^31"),
        (lambda: px(hr=1 << 30, wr=16385, pitch=1 << 20, gy=1 << 26, gx=1025, opitch=1 << 20, mask=None), -2, "workgroups"),
        (lambda: px(gy=1), -2, "Gy x Gx"), (lambda: px(gx=3), -2, "Gy x Gx"), (lambda: px(cell=8), -2, "Gy x Gx"),
        (lambda: px(c=odd), -4, "4-byte aligned"), (lambda: px(c=two), -4, "4-byte aligned"),
    ]
    for call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # what is taken: only the later alignment check stops these calls
    for ok in (dict(smooth=0), dict(smooth=1), dict(mt=0), dict(mt=255), dict(mpitch=7), dict(md=2, hm=10, wm=15, mpitch=15),
               dict(md=32, hm=0, wm=0, mpitch=0), dict(down=1, md=1, hm=20, wm=31, mpitch=31, opitch=93), dict(down=4, md=4, opitch=21),
               dict(down=4, md=16, hm=1, wm=1, mpitch=1, opitch=21), dict(alpha=0), dict(alpha=256)):
        assert px(c=odd, **ok) == -4, ok
    # mask == NULL means no mask: its other arguments are not looked at
    assert px(c=odd, mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999) == -4
    # an empty canvas: everything is checked, nothing is launched, 0 is returned (no device is present here, so a launch would fail)
    assert px(hr=1, wr=1, pitch=3, gy=1, gx=1, down=4, opitch=0, md=4, hm=0, wm=0, mpitch=0) == 0 and px(hr=3, wr=31, gy=1, down=4, hm=0) == 0
    assert px(hr=1, wr=1, pitch=3, gy=1, gx=1, down=4, opitch=0, mask=None) == 0
    assert px(hr=1, wr=1, pitch=3, gy=1, gx=1, down=4, opitch=0, mask=None, c=odd) == -4


def test_select_scores_on_the_host():
    from toad_amd.heatmap import quantise_scores, select_scores
    s = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, float("nan"), 0.4999, 2.0, -1.0])
    q = quantise_scores(s)
    assert select_scores(s, q) is q                                                                 # neither keyword: untouched
    got = select_scores(s, q, thresh=0.5)
    assert got.dtype == torch.int32 and got.tolist() == [-1, -1, 32768, 49151, 65535, -1, -1, 65535, -1]      # score >= thresh stays; NaN stays absent
    assert select_scores(s, q, binarize=True).tolist() == [65535] * 5 + [-1] + [65535] * 3
    assert select_scores(s, q, thresh=0.5, binarize=True).tolist() == [-1, -1, 65535, 65535, 65535, -1, -1, 65535, -1]
    assert select_scores(s, q, thresh=-5.0).tolist() == q.tolist() and select_scores(s, q, thresh=3).tolist() == [-1] * 9
    r = torch.rand(2048, generator=torch.Generator().manual_seed(8))
    r[::97] = float("nan")
    for kw in (dict(thresh=0.3), dict(binarize=True), dict(thresh=0.9, binarize=True)):
        assert select_scores(r, quantise_scores(r), **kw).tolist() == ref.select(r.numpy(), heat_ref.quantise(r.numpy()), **kw).tolist()


def test_px_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.eval import region_tissue_attention_heatmap
    from toad_amd.heatmap import attention_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_blend_px(cpu, torch.zeros(4, 4, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, 1, smooth=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        attention_canvas(cpu, np.zeros((0, 2), dtype=np.int64), torch.zeros(0), 16, smooth=True)
    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells, lut = torch.zeros(4, 4, dtype=torch.int32, device="meta"), torch.zeros(256, 3, dtype=torch.uint8, device="meta")
    m16 = torch.zeros(16, 16, dtype=torch.uint8, device="meta")
    for k, text in ((dict(cell=12), "cell"), (dict(down=3), "down"), (dict(alpha=257), "alpha"), (dict(cells=cells[:3]), r"\[Gy,Gx\]"), (dict(lut=lut[:255]), "lut"),
                    (dict(out=torch.zeros(32, 64, 3, dtype=torch.uint8, device="meta")), "out must be"),
                    (dict(smooth=2), "smooth"), (dict(smooth="yes"), "smooth"), (dict(smooth=None), "smooth"),
                    (dict(mask_down=4), "without a mask"),
                    (dict(mask=m16), "mask_down"), (dict(mask=m16, mask_down=3), "mask_down"), (dict(mask=m16, mask_down=64), "mask_down"),
                    (dict(mask=torch.zeros(64, 64, dtype=torch.uint8, device="meta"), mask_down=1, down=2), "multiple of down"),
                    (dict(mask=m16, mask_down=2, down=4), "multiple of down"),
                    (dict(mask=m16, mask_down=8), r"\[8,8\] mask"), (dict(mask=m16[:15], mask_down=4), r"\[16,16\] mask"),
                    (dict(mask=m16, mask_down=4, mask_thresh=256), "mask_thresh"), (dict(mask=m16, mask_down=4, mask_thresh=-1), "mask_thresh"),
                    (dict(mask=m16, mask_down=4, mask_thresh=0.5), "mask_thresh"),
                    (dict(mask=torch.zeros(16, 32, dtype=torch.uint8, device="meta")[:, ::2], mask_down=4), "stride"),
                    (dict(mask=torch.zeros(16, 16, 1, dtype=torch.uint8, device="meta"), mask_down=4), r"\[Hp,Wp\]")):
        args = dict(region=meta, cells=cells, cell=16, lut=lut, alpha=102, down=1)
        args.update(k)
        with pytest.raises(ValueError, match=text):
            ops.region_heat_blend_px(**args)
    with pytest.raises(TypeError, match="uint8"):
        ops.region_heat_blend_px(meta, cells, 16, lut, 102, 1, mask=m16.float(), mask_down=4)
    none = (np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"), 16)
    for k, text in ((dict(smooth=1), "bools"), (dict(binarize="no"), "bools"), (dict(thresh="0.5"), "thresh"), (dict(thresh=True), "thresh"),
                    (dict(thresh=float("nan")), "thresh"), (dict(mask=m16), "triple"), (dict(mask=(m16, 8)), "triple")):
        with pytest.raises(ValueError, match=text):
            attention_canvas(meta, *none, **k)
    with pytest.raises(ValueError, match="mask_down"):
        attention_canvas(meta, *none, mask=(m16, 8, 3))
    with pytest.raises(ValueError, match="multiple of down"):
        attention_canvas(meta, *none, down=4, mask=(torch.zeros(32, 32, dtype=torch.uint8, device="meta"), 8, 2))
    # the pipeline call: a tissue mask needs a segment dict whose down the canvas down divides - refused before the selection runs
    with pytest.raises(ValueError, match="segment dict"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True)
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True, segment=dict(down=2), down=4)
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True, segment=dict(down=1, median=3), down=2)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------------------
def test_reference_tent_by_hand():
    """cell 4, a 2 x 2 table with one cell absent: [[10, 50], [-1, 200]] on an 8 x 8 region."""
    t = np.array([[10, 50], [-1, 200]])
    # the axis: p = 2 ox + 1 - 4 = -3, -1, 1, 3, 5, 7, 9, 11 -> g0 = -1, -1, 0, 0, 0, 0, 1, 1 and f = 5, 7, 1, 3, 5, 7, 1, 3
    assert ref.tent_axis(8, 1, 4) == [(-1, 3, 5), (-1, 1, 7), (0, 7, 1), (0, 5, 3), (0, 3, 5), (0, 1, 7), (1, 7, 1), (1, 5, 3)]
    assert ref.tent_axis(4, 2, 4) == [(-1, 2, 6), (0, 6, 2), (0, 2, 6), (1, 6, 2)] and ref.tent_axis(2, 4, 4) == [(0, 8, 0), (1, 8, 0)]
    assert ref.tent_axis(3, 1, 64)[0] == (-1, 63, 65) and ref.tent_axis(64, 2, 64)[15:17] == [(-1, 2, 126), (0, 126, 2)]
    i1 = ref.index_px(t, 4, 1, 8, 8, True)
    # (ox 3, oy 1): rows -1 (outside -> own 10) and 0 with weights 1 and 7, columns 0 and 1 with 5 and 3: 1 (50 + 30) + 7 (50 + 150) = 1480 -> (1480 + 32) >> 6
    assert i1[1, 3] == 23
    # (3, 3): rows 0 and 1 with 5 and 3; cell (1, 0) is absent -> own 10: 5 (50 + 150) + 3 (50 + 600) = 2950 -> 46
    assert i1[3, 3] == 46
    # (4, 4), own 200: rows and columns 0 and 1 with 3 and 5; (1, 0) absent -> 200: 3 (30 + 250) + 5 (600 + 1000) = 8840 -> 138
    assert i1[4, 4] == 138
    # the corner: only own around it. (4, 0), own 50: row -1 is outside -> 50 on both sides, row 0 holds 10 and 50: 3 (150 + 250) + 5 (30 + 250) = 2600 -> 41
    assert i1[0, 7] == 50 and i1[0, 4] == 41
    assert (i1[4:, :4] == -1).all() and (i1[:4] >= 0).all() and (i1[4:, 4:] >= 0).all()               # the absent cell stays absent, its edge sharp
    assert (i1[:4, :4] >= 10).all() and (i1[:4, :4] <= 50).all() and i1[0, 0] == 10                  # between the neighbours' values
    i2 = ref.index_px(t, 4, 2, 4, 4, True)
    assert i2[0, 1] == (2 * (60 + 20) + 6 * (60 + 100) + 32) >> 6 == 18                               # down 2: columns 0, 1 with 6, 2; rows -1, 0 with 2, 6
    i4 = ref.index_px(t, 4, 4, 2, 2, True)
    assert i4.tolist() == [[10, 50], [-1, 200]]                                                       # a canvas pixel is a whole cell: nothing to interpolate
    flat = ref.index_px(t, 4, 1, 8, 8, False)
    assert np.array_equal(flat, np.repeat(np.repeat(t, 4, axis=0), 4, axis=1)) and (i1 != flat).any()
    assert ref.index_px(np.array([[300, 256], [255, 999]]), 4, 1, 8, 8, True).tolist() == [[255] * 8] * 8      # above 255 reads as 255


def test_reference_reproduces_a_constant_field_and_equals_the_flat_reference():
    rng = np.random.default_rng(4)
    region = rng.integers(0, 256, size=(37, 70, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    for cell in (4, 8, 16, 32, 64):
        gy, gx = -(-37 // cell), -(-70 // cell)
        for down in (1, 2, 4):
            for value in (0, 1, 127, 255):
                const = np.full((gy, gx), value)
                assert (ref.index_px(const, cell, down, 37 // down, 70 // down, True) == value).all(), (cell, down, value)
            holes = np.full((gy, gx), 99)
            holes[rng.random((gy, gx)) < 0.4] = -1                   # absent cells count as own: still constant where there is a value
            got = ref.index_px(holes, cell, down, 37 // down, 70 // down, True)
            assert set(np.unique(got).tolist()) <= {-1, 99}
            idx = rng.integers(-1, 256, size=(gy, gx))
            assert np.array_equal(ref.canvas(region, idx, cell, lut, 102, down), heat_ref.canvas(region, idx, cell, lut, 102, down))      # smooth = 0, no mask
            assert np.array_equal(ref.canvas(region, holes, cell, lut, 102, down, smooth=True), heat_ref.canvas(region, holes, cell, lut, 102, down))


def test_reference_mask_by_hand():
    region = np.full((9, 10, 3), 40, dtype=np.uint8)
    lut = np.full((256, 3), 200, dtype=np.uint8)
    idx = np.full((3, 3), 7)
    mask = np.array([[0, 255, 9, 8, 0], [255, 0, 0, 0, 255], [0, 0, 255, 0, 0], [9, 9, 9, 9, 9]], dtype=np.uint8)       # 9 // 2 x 10 // 2
    on, off = (102 * 200 + 154 * 40 + 128) >> 8, 40
    out = ref.canvas(region, idx, 4, lut, 102, 1, mask=mask, mask_down=2, mask_thresh=8)
    want = np.repeat(np.repeat(mask > 8, 2, axis=0), 2, axis=1)
    want = np.concatenate([want, np.zeros((1, 10), dtype=bool)])      # row 8 lies in the partial boxes the plane dropped: not tissue
    assert out.shape == (9, 10, 3) and np.array_equal(out[..., 0] == on, want) and set(np.unique(out).tolist()) == {on, off} == {104, 40}
    assert np.array_equal(ref.tissue_px(mask, 2, 8, 2, 4, 5), mask > 8) and ref.tissue_px(mask, 2, 8, 2, 4, 5).sum() == 10
    assert ref.tissue_px(mask, 2, 254, 1, 9, 10).sum() == 4 * 4 and ref.tissue_px(None, None, 0, 1, 9, 10).all()
    assert not ref.tissue_px(np.zeros((0, 1), dtype=np.uint8), 16, 0, 1, 9, 16).any()                 # a plane without rows: nothing is tissue
    full = ref.canvas(region, idx, 4, lut, 102, 1, mask=np.full((9, 10), 255, dtype=np.uint8), mask_down=1)
    assert np.array_equal(full, heat_ref.canvas(region, idx, 4, lut, 102, 1))
    absent = idx.copy()
    absent[0, 0] = -1                                                # no value and tissue: still the region
    out = ref.canvas(region, absent, 4, lut, 102, 1, mask=np.full((4, 5), 255, dtype=np.uint8), mask_down=2)
    assert (out[:4, :4] == 40).all() and (out[:8, 4:] == on).all() and (out[8] == 40).all()


def test_reference_tables_are_what_the_gpu_tests_need():
    for k in (0, 1, 2, 4):
        (hr, wr), _, _, _, cell = heat_ref.LATTICES[k]
        assert cell == {0: 32, 1: 4, 2: 8, 4: 16}[k]
        gy, gx = -(-hr // cell), -(-wr // cell)
        t = ref.tables(gy, gx, k)
        assert t["ramp"].min() == 0 and t["ramp"].max() == 255 and (t["ramp"] >= 0).all()
        assert (t["hole"] == -1).sum() == 1 and t["hole"][gy // 2, gx // 2] == -1 and 0 < gy // 2 < gy - 1 and 0 < gx // 2 < gx - 1      # interior
        assert (t["checker"][0, 1::2] == -1).all() and (t["checker"][0, ::2] >= 0).all() and (t["checker"][1, ::2] == -1).all()
        assert (t["border"][0] == -1).all() and (t["border"][:, -1] == -1).all() and (t["border"][1:-1, 1:-1] >= 0).all()
        if k not in (1, 4):
            continue
        for name, tab in t.items():                                  # smoothing changes covered pixels unless a canvas pixel is a whole cell
            for down in (2, 4):
                flat = ref.index_px(tab, cell, down, hr // down, wr // down, False)
                tent = ref.index_px(tab, cell, down, hr // down, wr // down, True)
                assert np.array_equal(flat < 0, tent < 0)
                assert (flat != tent).any() == (cell != down), (k, name, down)
