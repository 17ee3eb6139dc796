"""CPU: the overview heat-map canvas (toad_region_heat_thumb_u8: an additive extension of ABI 15; ops.region_heat_thumb and down = 8, 16, 32 of
toad_amd/heatmap.py and eval.region_tissue_attention_heatmap). The entry point exists in the header, the library and the ctypes table and refuses what the
host can see before any device access; and the numpy reference the GPU tests compare against (tests/heat_px_ref.py, unchanged: it states the definition
for any down) is checked at the new down values against a per-pixel loop written out here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import heat_px_ref as ref

NAME = "toad_region_heat_thumb_u8"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thumb_symbol_is_declared_exported_and_bound():
    from toad_amd import _lib as L, ops
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)      # additive: still 15
    assert re.search(r"\b" + NAME + r"\s*\(", header), f"{NAME} is not declared in include/toad_hip.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 21
    assert L.SIGNATURES[NAME] == L.SIGNATURES["toad_region_heat_blend_px_u8"]                        # the same 21 arguments in the same order
    assert ops.HEAT_THUMB_DOWNS == (8, 16, 32) and ops.HEAT_DOWNS == (1, 2, 4)
    # the header states the definition next to the px block
    block = header[header.index("toad_region_heat_blend_px_u8("):header.index(NAME + "(")]
    for text in ("down in {8, 16, 32}", "m = (sum of the down x down box + down * down / 2) / (down * down)", "own = cells[(down * oy) / cell][(down * ox) / cell]",
                 "down <= cell", "p = 2 * down * ox + down - cell", "g0 = floor(p / (2 * cell))", "f = p - 2 * cell * g0",
                 "(sum wy * wx * v + 2 * cell * cell) >> (2 * log2(cell) + 2)", "mask[my][mx] > mask_thresh", "multiple of down",
                 "(alpha * lut[idx_px][c] + (256 - alpha) * m + 128) >> 8"):
        assert text in block, text


def test_thumb_entry_reports_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # the region, the mask and the canvas may lie at an odd address; int32 cells may not
    two = ctypes.c_void_p((1 << 21) + 2)

    # a 40 x 61 region in 16-pixel cells (3 x 4), canvas down 8 (5 x 7), a 16-box mask plane (2 x 3)
    def th(r=odd, pitch=3 * 61 + 1, hr=40, wr=61, c=one, gy=3, gx=4, cell=16, lut=odd, alpha=102, down=8, smooth=1, mask=odd, mpitch=4, hm=2, wm=3, md=16,
           mt=8, out=odd, opitch=3 * 7 + 2):
        return lib.toad_region_heat_thumb_u8(r, pitch, hr, wr, c, gy, gx, cell, lut, alpha, down, smooth, mask, mpitch, hm, wm, md, mt, out, opitch, None)

    cases = [
        (lambda: th(r=None), -1, "null pointer"), (lambda: th(c=None), -1, "null pointer"), (lambda: th(lut=None), -1, "null pointer"),
        (lambda: th(out=None), -1, "null pointer"),
        (lambda: th(cell=12), -2, "cell"), (lambda: th(cell=2), -2, "cell"), (lambda: th(hr=0), -2, "bad shape"), (lambda: th(wr=-1), -2, "bad shape"),
        (lambda: th(alpha=-1), -2, "alpha"), (lambda: th(alpha=257), -2, "alpha"),
        (lambda: th(down=0), -2, "down"), (lambda: th(down=1), -2, "down"), (lambda: th(down=2), -2, "down"), (lambda: th(down=3), -2, "down"),
        (lambda: th(down=4), -2, "down"), (lambda: th(down=64), -2, "down"), (lambda: th(down=64, cell=64), -2, "not one of 8, 16, 32"),
        (lambda: th(down=16, cell=8), -2, "cell"), (lambda: th(down=16, cell=8), -2, "down = 16"), (lambda: th(down=16, cell=8), -2, "cell = 8"),
        (lambda: th(cell=4), -2, "cell = 4"), (lambda: th(down=32), -2, "cell = 16"),
        (lambda: th(down=16, cell=8, alpha=300), -2, "alpha"),                                      # the first failing check wins: alpha, down, then down <= cell,
        (lambda: th(down=3, cell=4), -2, "not one of"), (lambda: th(down=16, cell=8, smooth=2), -2, "cell"),      # then smooth
        (lambda: th(smooth=2), -1, "smooth"), (lambda: th(smooth=-1), -1, "smooth"),
        (lambda: th(pitch=3 * 61 - 1), -2, "pitch"), (lambda: th(pitch=-184), -2, "pitch"),
        (lambda: th(md=0), -2, "mask_down"), (lambda: th(md=3), -2, "mask_down"), (lambda: th(md=64), -2, "mask_down"), (lambda: th(md=-8), -2, "mask_down"),
        (lambda: th(down=16, md=8, hm=5, wm=7, mpitch=7, opitch=9), -2, "multiple of down"),
        (lambda: th(md=4, hm=10, wm=15, mpitch=15), -2, "multiple of down"), (lambda: th(md=1, hm=40, wm=61, mpitch=61), -2, "multiple of down"),
        (lambda: th(cell=32, gy=2, gx=2, down=32, md=16, opitch=3), -2, "multiple of down"),
        (lambda: th(hm=1), -2, "Hm x Wm"), (lambda: th(hm=3), -2, "Hm x Wm"), (lambda: th(wm=4), -2, "Hm x Wm"), (lambda: th(wm=2), -2, "Hm x Wm"),
        (lambda: th(md=8), -2, "Hm x Wm"),                                                          # 40 // 8 x 61 // 8 = 5 x 7
        (lambda: th(mpitch=2), -2, "mask_pitch"), (lambda: th(mpitch=0), -2, "mask_pitch"), (lambda: th(mpitch=-4), -2, "mask_pitch"),
        (lambda: th(mt=-1), -1, "mask_thresh"), (lambda: th(mt=256), -1, "mask_thresh"),
        (lambda: th(opitch=3 * 7 - 1), -2, "out_pitch"), (lambda: th(down=16, opitch=3 * 3 - 1), -2, "out_pitch"),      # 3 (Wr / down)
        (lambda: th(wr=715827883, pitch=1 << 32, opitch=1 << 32, gx=44739243, mask=None), -2, "2^31"),
        (lambda: th(hr=1 << 30, wr=16385, pitch=1 << 20, gy=1 << 26, gx=1025, opitch=1 << 20, mask=None), -2, "workgroups"),
        (lambda: th(hr=1 << 29, wr=16385, pitch=1 << 20, gy=1 << 25, gx=1025, opitch=1 << 20, mask=None), -2, "workgroups"),      # 64 chunks x 2^25 strips of 16 rows
        (lambda: th(gy=2), -2, "Gy x Gx"), (lambda: th(gx=5), -2, "Gy x Gx"), (lambda: th(cell=8), -2, "Gy x Gx"),
        (lambda: th(c=odd), -4, "4-byte aligned"), (lambda: th(c=two), -4, "4-byte aligned"),
    ]
    for call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(NAME + ":"), (text, got, msg)
    # what is taken: only the later alignment check stops these calls
    for ok in (dict(smooth=0), dict(smooth=1), dict(mt=0), dict(mt=255), dict(mpitch=3), dict(md=8, hm=5, wm=7, mpitch=7), dict(md=32, hm=1, wm=1, mpitch=1),
               dict(down=16, opitch=9), dict(down=16, md=32, hm=1, wm=1, mpitch=1, opitch=9), dict(cell=8, gy=5, gx=8, md=8, hm=5, wm=7, mpitch=7),
               dict(cell=32, gy=2, gx=2, down=32, md=32, hm=1, wm=1, mpitch=1, opitch=3), dict(cell=64, gy=1, gx=1), dict(alpha=0), dict(alpha=256),
               dict(hr=1 << 29, wr=16385, pitch=1 << 20, gy=1 << 24, gx=513, cell=32, down=32, opitch=1 << 20, mask=None)):      # 32-row strips: half as many
        assert th(c=odd, **ok) == -4, ok
    # mask == NULL means no mask: its other arguments are not looked at
    assert th(c=odd, mask=None, mpitch=-1, hm=-1, wm=-1, md=3, mt=999) == -4
    # an empty canvas (Hr < down or Wr < down): everything is checked, nothing is launched, 0 is returned (no device is present here, so a launch would fail)
    assert th(hr=7, gy=1, hm=0) == 0 and th(hr=7, gy=1, mask=None) == 0 and th(hr=7, gy=1, hm=0, opitch=20) == -2      # out_pitch is still checked
    assert th(wr=7, pitch=21, gx=1, wm=0, mpitch=0, opitch=0) == 0
    assert th(hr=15, wr=61, gy=1, cell=16, down=16, md=16, hm=0, wm=3, opitch=9) == 0
    assert th(hr=7, gy=1, mask=None, c=odd) == -4 and th(hr=7, gy=1, mask=None, down=4) == -2
    # the two older entries still refuse every overview down
    for down in (8, 16, 32):
        assert lib.toad_region_heat_blend_px_u8(odd, 184, 40, 61, one, 1, 1, 64, odd, 102, down, 0, None, 0, 0, 0, 0, 0, odd, 23, None) == -2 and "down" in err()
        assert lib.toad_region_heat_blend_u8(odd, 184, 40, 61, one, 1, 1, 64, odd, 102, down, odd, 23, None) == -2 and "down" in err()


# ---- the reference at the new down values ---------------------------------------------------------------------------------------------------------------
def by_hand(region, cells, cell, lut, alpha, down, smooth, mask, mask_down, mask_thresh):
    """The definition of include/toad_hip.h, one canvas pixel at a time, in Python integers."""
    hr, wr, _ = region.shape
    ho, wo = hr // down, wr // down
    gy_n, gx_n = cells.shape
    val = lambda gy, gx, own: min(int(cells[gy, gx]), 255) if 0 <= gy < gy_n and 0 <= gx < gx_n and cells[gy, gx] >= 0 else own      # noqa: E731
    out = np.zeros((ho, wo, 3), dtype=np.uint8)
    for oy in range(ho):
        for ox in range(wo):
            m = [(int(region[down * oy:down * oy + down, down * ox:down * ox + down, c].astype(np.int64).sum()) + down * down // 2) // (down * down) for c in range(3)]
            own = min(int(cells[down * oy // cell, down * ox // cell]), 255)
            idx = own
            if smooth and own >= 0:
                px, py = 2 * down * ox + down - cell, 2 * down * oy + down - cell
                gx0, gy0 = px // (2 * cell), py // (2 * cell)
                fx, fy = px - 2 * cell * gx0, py - 2 * cell * gy0
                s = sum(wy * wx * val(gy0 + r, gx0 + c, own) for r, wy in ((0, 2 * cell - fy), (1, fy)) for c, wx in ((0, 2 * cell - fx), (1, fx)))
                idx = (s + 2 * cell * cell) >> (2 * (cell.bit_length() - 1) + 2)
            my, mx = down * oy // mask_down, down * ox // mask_down
            tissue = my < mask.shape[0] and mx < mask.shape[1] and mask[my, mx] > mask_thresh
            out[oy, ox] = [(alpha * int(lut[idx, c]) + (256 - alpha) * m[c] + 128) >> 8 for c in range(3)] if own >= 0 and tissue else m
    return out


def test_reference_at_overview_scale_by_hand():
    """A 17 x 26 region in 8-pixel cells at down = 8: a 2 x 3 canvas over a 3 x 4 table with an absent cell and a value above 255, the row and the columns
    past 16 x 24 dropped, under an 8-box mask with one pixel at the threshold."""
    rng = np.random.default_rng(26)
    region = rng.integers(0, 256, size=(17, 26, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    cells = np.array([[10, 250, -1, 7], [300, 0, 90, 7], [5, 5, 5, 5]])
    mask = np.array([[255, 9, 8], [0, 255, 255]], dtype=np.uint8)
    outs = {}
    for smooth in (False, True):
        want = by_hand(region, cells, 8, lut, 102, 8, smooth, mask, 8, 8)
        got = ref.canvas(region, cells, 8, lut, 102, 8, smooth=smooth, mask=mask, mask_down=8, mask_thresh=8)
        assert got.shape == (2, 3, 3) and np.array_equal(got, want), smooth
        outs[smooth] = got
    assert np.array_equal(outs[True], outs[False])                   # cell == down: a canvas pixel is a whole cell, the tent is the own value
    plain = ref.canvas(region, cells, 8, lut, 0, 8)
    blended = (outs[False] != plain).any(axis=2)
    assert blended.tolist() == [[True, True, False], [False, True, True]]      # (0, 2): absent and at the threshold; (1, 0): mask 0
    assert np.array_equal(outs[False][1, 0], plain[1, 0])
    # a coarser table over the same region: cell 16 at down = 8 has a real tent, and the 16-box mask plane is 1 x 1
    cells16 = np.array([[40, 200], [-1, 90]])
    m16 = np.array([[200]], dtype=np.uint8)
    for smooth in (False, True):
        want = by_hand(region, cells16, 16, lut, 128, 8, smooth, m16, 16, 199)
        outs[smooth] = ref.canvas(region, cells16, 16, lut, 128, 8, smooth=smooth, mask=m16, mask_down=16, mask_thresh=199)
        assert np.array_equal(outs[smooth], want), smooth
    assert not np.array_equal(outs[True], outs[False])
    assert np.array_equal(outs[True][:, 2], ref.canvas(region, cells16, 16, lut, 0, 8)[:, 2])      # column 2 lies past the plane: not tissue
    # the index alone, by hand: (ox 1, oy 0) at cell 16, down 8: p = 16 + 8 - 16 = 8 along x -> g0 = 0, f = 8 (weights 24, 8); along y p = -8 -> g0 = -1,
    # f = 24 (8 for the row outside -> own 40 in both columns, 24 for row 0): 8 (24 * 40 + 8 * 40) + 24 (24 * 40 + 8 * 200) = 71680 -> (71680 + 512) >> 10 = 70
    assert ref.index_px(cells16, 16, 8, 2, 3, True)[0, 1] == 70


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------------------
def test_thumb_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.eval import region_tissue_attention_heatmap
    from toad_amd.heatmap import attention_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_thumb(cpu, torch.zeros(4, 4, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, 8, smooth=True)
    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells, lut = torch.zeros(4, 4, dtype=torch.int32, device="meta"), torch.zeros(256, 3, dtype=torch.uint8, device="meta")
    m4 = torch.zeros(4, 4, dtype=torch.uint8, device="meta")
    for k, text in ((dict(cell=12), "cell"), (dict(down=4), "down must be one of"), (dict(down=1), "down must be one of"), (dict(down=64), "down must be one of"),
                    (dict(down=3), "down"), (dict(down=32), "exceeds cell = 16"),
                    (dict(cell=8, cells=torch.zeros(8, 8, dtype=torch.int32, device="meta"), down=16), "exceeds cell = 8"),
                    (dict(alpha=257), "alpha"), (dict(cells=cells[:3]), r"\[Gy,Gx\]"), (dict(lut=lut[:255]), "lut"),
                    (dict(out=torch.zeros(16, 16, 3, dtype=torch.uint8, device="meta")), "out must be"),
                    (dict(smooth=2), "smooth"), (dict(smooth=None), "smooth"),
                    (dict(mask_down=16), "without a mask"),
                    (dict(mask=m4), "mask_down"), (dict(mask=m4, mask_down=3), "mask_down"), (dict(mask=m4, mask_down=64), "mask_down"),
                    (dict(mask=torch.zeros(16, 16, dtype=torch.uint8, device="meta"), mask_down=4), "multiple of down"),
                    (dict(mask=m4, mask_down=8, down=16), "multiple of down"),
                    (dict(mask=m4, mask_down=8), r"\[8,8\] mask"), (dict(mask=m4[:3], mask_down=16), r"\[4,4\] mask"),
                    (dict(mask=m4, mask_down=16, mask_thresh=256), "mask_thresh"), (dict(mask=m4, mask_down=16, mask_thresh=-1), "mask_thresh"),
                    (dict(mask=torch.zeros(4, 8, dtype=torch.uint8, device="meta")[:, ::2], mask_down=16), "stride")):
        args = dict(region=meta, cells=cells, cell=16, lut=lut, alpha=102, down=8)
        args.update(k)
        with pytest.raises(ValueError, match=text):
            ops.region_heat_thumb(**args)
    with pytest.raises(TypeError, match="uint8"):
        ops.region_heat_thumb(meta, cells, 16, lut, 102, 8, mask=m4.float(), mask_down=16)
    # the older calls keep their down list
    for fn in (ops.region_heat_blend, ops.region_heat_blend_px):
        with pytest.raises(ValueError, match=r"one of \(1, 2, 4\)"):
            fn(meta, cells, 16, lut, 102, 8)
    # attention_canvas: the lattice's cell must be at least down, and the message names it
    none = (np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"))
    with pytest.raises(ValueError, match="cell = 4"):
        attention_canvas(meta, *none, tile=16, stride=4, down=8)
    with pytest.raises(ValueError, match="cell = 16"):
        attention_canvas(meta, *none, tile=16, down=32)
    with pytest.raises(ValueError, match="multiple of down"):
        attention_canvas(meta, *none, tile=16, down=16, mask=(torch.zeros(8, 8, dtype=torch.uint8, device="meta"), 8, 8))
    with pytest.raises(ValueError, match="bools"):
        attention_canvas(meta, *none, tile=16, down=8, smooth=1)
    # the pipeline call: the canvas down may now be any of 1 .. 32, the segment down still a multiple of it - refused before the selection runs
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True, segment=dict(median=3), down=32)      # the default segment down is 16
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True, segment=dict(down=8), down=16)
    with pytest.raises(ValueError, match="multiple of the canvas down"):
        region_tissue_attention_heatmap(None, None, meta, tile=16, tissue_mask=True, segment=dict(down=32), down=64)
