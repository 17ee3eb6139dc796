"""CPU: attention heat maps (toad_heat_cells, toad_region_heat_blend_u8: an additive extension of ABI 15; toad_amd/heatmap.py). The entry points exist in
the header, the library and the ctypes table and refuse what the host can see before any device access; the table and colour arithmetic is host code;
and the numpy reference the GPU tests compare against (tests/heat_ref.py) is itself tested here, by hand and on the inputs of those tests: every "mixed
outcome" condition the GPU tests rely on is a fact about the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import heat_ref as ref

HEAT_SYMBOLS = ("toad_heat_cells", "toad_region_heat_blend_u8")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heat_symbols_are_declared_exported_and_bound():
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in HEAT_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    assert "(2 * S + 257 * n) / (514 * n)" in header and "(alpha * lut[idx][c] + (256 - alpha) * m + 128) >> 8" in header      # the header states the definition


def test_heat_entries_report_argument_errors_without_a_gpu():
    from toad_amd import _lib as L
    lib = L.load()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 1)                      # a region or a canvas at an odd address is fine; int32 arrays there are refused
    two = ctypes.c_void_p((1 << 21) + 2)

    def cells(q=one, nx=4, ny=3, cell=16, x0=16, y0=0, h=32, w=64, sx=16, sy=16, gy=5, gx=9, c=one):
        return lib.toad_heat_cells(q, nx, ny, cell, x0, y0, h, w, sx, sy, gy, gx, c, None)      # ends at x = 16 + 48 + 64 = 128 <= 144, y = 64 <= 80

    def blend(r=odd, pitch=3 * 31 + 1, hr=20, wr=31, c=one, gy=2, gx=2, cell=16, lut=odd, alpha=102, down=2, out=odd, opitch=3 * 15 + 2):
        return lib.toad_region_heat_blend_u8(r, pitch, hr, wr, c, gy, gx, cell, lut, alpha, down, out, opitch, None)

    a, b = "toad_heat_cells", "toad_region_heat_blend_u8"
    cases = [
        (a, lambda: cells(q=None), -1, "null pointer"), (a, lambda: cells(c=None), -1, "null pointer"),
        (a, lambda: cells(cell=24), -2, "cell"), (a, lambda: cells(cell=1), -2, "cell"), (a, lambda: cells(cell=128), -2, "cell"),
        (a, lambda: cells(nx=0), -2, "bad shape"), (a, lambda: cells(ny=0), -2, "bad shape"), (a, lambda: cells(h=0), -2, "bad shape"),
        (a, lambda: cells(w=0), -2, "bad shape"), (a, lambda: cells(sx=0), -2, "bad shape"), (a, lambda: cells(sy=-16), -2, "bad shape"),
        (a, lambda: cells(gy=0), -2, "bad shape"), (a, lambda: cells(gx=-1), -2, "bad shape"),
        (a, lambda: cells(x0=-16), -2, "x0"), (a, lambda: cells(y0=-16), -2, "y0"), (a, lambda: cells(x0=8), -2, "x0"), (a, lambda: cells(y0=4), -2, "y0"),
        (a, lambda: cells(h=40), -2, "H = 40"), (a, lambda: cells(w=72), -2, "W = 72"), (a, lambda: cells(sx=24), -2, "sx"), (a, lambda: cells(sy=8), -2, "sy"),
        (a, lambda: cells(nx=6), -2, "last tile"),                                     # ends at x = 16 + 80 + 64 = 160 > 144
        (a, lambda: cells(ny=5), -2, "last tile"),                                     # ends at y = 64 + 32 = 96 > 80
        # coverage 65 * 64 = 4160 > 4096: 260 / 4 rows of tiles by 256 / 4 columns cover a cell
        (a, lambda: cells(cell=4, x0=0, h=260, w=256, sx=4, sy=4, nx=1, ny=1, gy=65, gx=64), -2, "4096"),
        (a, lambda: cells(q=two), -4, "4-byte aligned"), (a, lambda: cells(c=odd), -4, "4-byte aligned"),
        (b, lambda: blend(r=None), -1, "null pointer"), (b, lambda: blend(c=None), -1, "null pointer"), (b, lambda: blend(lut=None), -1, "null pointer"),
        (b, lambda: blend(out=None), -1, "null pointer"),
        (b, lambda: blend(cell=12), -2, "cell"), (b, lambda: blend(cell=0), -2, "cell"), (b, lambda: blend(cell=2), -2, "cell"),
        (b, lambda: blend(hr=0), -2, "bad shape"), (b, lambda: blend(wr=-1), -2, "bad shape"),
        (b, lambda: blend(alpha=-1), -2, "alpha"), (b, lambda: blend(alpha=257), -2, "alpha"),
        (b, lambda: blend(down=0), -2, "down"), (b, lambda: blend(down=3), -2, "down"), (b, lambda: blend(down=8), -2, "down"),
        (b, lambda: blend(pitch=3 * 31 - 1), -2, "pitch"), (b, lambda: blend(pitch=0), -2, "pitch"), (b, lambda: blend(pitch=-94), -2, "pitch"),
        (b, lambda: blend(opitch=3 * 15 - 1), -2, "out_pitch"), (b, lambda: blend(opitch=-45), -2, "out_pitch"),
        (b, lambda: blend(down=1, opitch=3 * 31 - 1), -2, "out_pitch"),                 # Wo = 31 at down = 1
        (b, lambda: blend(wr=715827883, pitch=1 << 32, opitch=1 << 32, gx=44739243), -2, "2^31"),      # 3 Wr = 2^31 + 1
        (b, lambda: blend(hr=1 << 30, wr=16385, pitch=1 << 20, gy=1 << 26, gx=1025, opitch=1 << 20), -2, "workgroups"),      # down = 2: 64 chunks x 2^26 row blocks
        (b, lambda: blend(gy=1), -2, "Gy x Gx"), (b, lambda: blend(gx=3), -2, "Gy x Gx"), (b, lambda: blend(cell=8), -2, "Gy x Gx"),
        (b, lambda: blend(c=odd), -4, "4-byte aligned"), (b, lambda: blend(c=two), -4, "4-byte aligned"),
    ]
    for name, call, rc, text in cases:
        got = call()
        msg = err()
        assert got == rc and text in msg and msg.startswith(name + ":"), (name, text, got, msg)
    # the largest that is taken: only the later alignment check stops these calls
    assert cells(nx=5, ny=4, c=odd) == -4 and cells(x0=0, nx=6, ny=4, c=odd) == -4
    assert cells(cell=4, x0=0, h=256, w=256, sx=4, sy=4, nx=1, ny=1, gy=64, gx=64, c=odd) == -4       # coverage 64 * 64 = 4096 is taken
    assert blend(alpha=0, c=odd) == -4 and blend(alpha=256, c=odd) == -4
    assert blend(wr=715827882, pitch=1 << 32, opitch=1 << 32, gx=44739243, c=odd) == -4                # 3 Wr = 2^31 - 2 is taken
    # an empty canvas: everything is checked, nothing is launched, 0 is returned (no device is present here, so a launch would fail)
    assert blend(hr=1, wr=1, pitch=3, gy=1, gx=1, down=4, opitch=0) == 0 and blend(hr=3, wr=31, gy=1, down=4) == 0
    assert blend(hr=1, wr=1, pitch=3, gy=1, gx=1, down=4, opitch=0, c=odd) == -4


def test_tile_table_refuses_what_is_not_on_the_lattice():
    from toad_amd.heatmap import tile_table
    q = lambda n: torch.arange(n, dtype=torch.int32)          # noqa: E731
    lat = dict(tile=(32, 64), stride=(8, 16), origin=(8, 4), n=(5, 3))
    t = tile_table(np.array([[8, 4], [72, 20], [24, 12]]), torch.tensor([7, 65535, -1], dtype=torch.int32), **lat)
    assert t.dtype == torch.int32 and t.tolist() == [[7, -1, -1, -1, -1], [-1, -1, -1, -1, -1], [-1, -1, -1, -1, 65535]]
    assert t[1, 1] == -1 and t[2, 4] == 65535 and t[0, 0] == 7          # (24, 12) -> (j, i) = (1, 1) holds its -1: a NaN score is an absent tile
    assert tile_table(np.zeros((0, 2), dtype=np.int64), q(0), **lat).tolist() == [[-1] * 5] * 3
    for bad, text in (([[9, 4]], "off the lattice"), ([[8, 8]], "off the lattice"), ([[8, 4], [24, 6]], r"origins\[1\].*off the lattice"),
                      ([[-8, 4]], "outside the lattice"), ([[8, -4]], "outside the lattice"), ([[88, 4]], "outside the lattice"),
                      ([[8, 28]], "outside the lattice"), ([[8, 4], [24, 4], [8, 4]], r"origins\[2\].*twice")):
        with pytest.raises(ValueError, match=text):
            tile_table(np.array(bad), q(len(bad)), **lat)
    with pytest.raises(ValueError, match="integers"):
        tile_table(np.array([[8.0, 4.0]]), q(1), **lat)
    with pytest.raises(ValueError, match="one per origin"):
        tile_table(np.array([[8, 4]]), q(2), **lat)
    with pytest.raises(ValueError, match="one per origin"):
        tile_table(np.array([[8, 4]]), torch.zeros(1), **lat)


def test_quantise_scores_and_alpha_on_the_host():
    from toad_amd.heatmap import _alpha_arg, quantise_scores
    s = torch.tensor([0.0, 1.0, -0.5, 2.0, float("nan"), 0.25, 1e-9, float("inf"), float("-inf")])
    assert quantise_scores(s).tolist() == [0, 65535, 0, 65535, -1, 16384, 0, 65535, 0] and quantise_scores(s).dtype == torch.int32
    assert quantise_scores(s).tolist() == ref.quantise(s.numpy()).tolist()
    r = torch.rand(4096, generator=torch.Generator().manual_seed(5))
    assert torch.equal(quantise_scores(r), torch.round(r.clamp(0, 1) * 65535).to(torch.int32)) and quantise_scores(r).tolist() == ref.quantise(r.numpy()).tolist()
    assert quantise_scores(torch.tensor([-3.0, -1.0, 1.0, float("nan")]), (-3, 1)).tolist() == [0, 32768, 65535, -1]
    with pytest.raises(ValueError, match="score_range"):
        quantise_scores(s, (1, 1))
    assert [_alpha_arg(a) for a in (0, 102, 256, 0.0, 0.4, 0.5, 1.0)] == [0, 102, 256, 0, 102, 128, 256]
    for bad in (-1, 257, 1.5, -0.1, True, "0.4", None):
        with pytest.raises(ValueError, match="alpha"):
            _alpha_arg(bad)


def test_jet_lut():
    from toad_amd.heatmap import jet_lut
    lut = jet_lut("cpu")
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and np.array_equal(lut.numpy(), ref.jet())
    assert lut[0].tolist() == [0, 0, 127] and lut[255].tolist() == [127, 0, 0]
    assert jet_lut("cpu") is lut and jet_lut(torch.device("cpu")) is lut          # built once per device
    # by hand at i = 127: r 765 - |1016 - 1530| = 251 -> 125, g 765 - |1016 - 1020| = 761 -> 510 -> 255, b 765 - |1016 - 510| = 259 -> 129
    assert lut[127].tolist() == [125, 255, 129] and lut[128].tolist() == [129, 255, 125]
    distinct = (lut[1:] != lut[:-1]).any(dim=1)
    assert int(distinct.sum()) > 127                                   # consecutive entries differ at more than half of the 255 steps
    assert int(lut[:64, 2].max()) == 255 and int(lut[:64, 0].max()) == 0 and int(lut[192:, 0].max()) == 255 and int(lut[192:, 2].max()) == 0      # blue first, red last


def test_heat_wrappers_refuse_on_the_host(monkeypatch):
    """Each refusal comes before anything is launched: the library is not even loaded."""
    from toad_amd import _lib as L, ops
    from toad_amd.heatmap import attention_canvas

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    cpu = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        attention_canvas(cpu, np.zeros((0, 2), dtype=np.int64), torch.zeros(0), 16)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.region_heat_blend(cpu, torch.zeros(4, 4, dtype=torch.int32), 16, torch.zeros(256, 3, dtype=torch.uint8), 102, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.heat_cells(torch.zeros(4, 4, dtype=torch.int32), 16, (0, 0), (16, 16), (16, 16), (4, 4), (64, 64))
    meta = torch.zeros(64, 64, 3, dtype=torch.uint8, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cells, lut = torch.zeros(4, 4, dtype=torch.int32, device="meta"), torch.zeros(256, 3, dtype=torch.uint8, device="meta")
    for k, text in ((dict(cell=12), "cell"), (dict(down=3), "down"), (dict(alpha=257), "alpha"), (dict(alpha=0.4), "alpha"),
                    (dict(cells=cells[:3]), r"\[Gy,Gx\]"), (dict(lut=lut[:255]), "lut"), (dict(out=torch.zeros(64, 64, 3, device="meta")), "out must be"),
                    (dict(out=torch.zeros(32, 64, 3, dtype=torch.uint8, device="meta")), "out must be"),
                    (dict(out=torch.zeros(64, 128, 3, dtype=torch.uint8, device="meta")[:, ::2]), "strides")):
        args = dict(region=meta, cells=cells, cell=16, lut=lut, alpha=102, down=1)
        args.update(k)
        with pytest.raises(ValueError, match=text):
            ops.region_heat_blend(**args)
    with pytest.raises(TypeError, match="uint8"):
        ops.region_heat_blend(meta.float(), cells, 16, lut, 102, 1)
    with pytest.raises(ValueError, match="multiple of 4"):
        attention_canvas(meta, np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"), 16, 6)
    with pytest.raises(ValueError, match="alpha"):
        attention_canvas(meta, np.zeros((0, 2), dtype=np.int64), torch.zeros(0, device="meta"), 16, alpha=1.5)
    with pytest.raises(ValueError, match="region's device"):
        attention_canvas(meta, np.zeros((0, 2), dtype=np.int64), torch.zeros(0), 16)       # scores on another device than the region


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------------------
def test_reference_cell_value_by_hand():
    lat = dict(cell=4, tile=(8, 8), stride=(4, 4), origin=(0, 0), region_hw=(12, 12))
    for k in (0, 1, 100, 127):                                         # n = 2 and S = 257 (2 k + 1): 255 S / (65535 n) = k + 1/2, a tie, rounds up
        for q0 in (0, 257 * k, 257 * (2 * k + 1)):
            t = np.array([[q0, 257 * (2 * k + 1) - q0], [-1, -1]])
            c = ref.cells(t, **lat)
            assert c[0, 1] == k + 1, (k, q0)                           # cell (0, 1) is covered by both tiles of the first row
            assert c[0, 0] == (2 * q0 + 257) // 514 and c[2, 0] == -1 and c[1, 1] == k + 1
    n, s = ref.coverage(np.array([[5, 7], [-1, 11]]), **lat)
    assert n.tolist() == [[1, 2, 1], [1, 3, 2], [0, 1, 1]] and s.tolist() == [[5, 12, 7], [5, 23, 18], [0, 11, 11]]
    assert (ref.cells(np.zeros((2, 2), dtype=np.int64), **lat) == 0).all()
    for nn in (1, 2, 3, 4):                                            # q = 65535 with any n gives 255
        t = np.full((2, 2), -1)
        t.reshape(-1)[:nn] = 65535
        c = ref.cells(t, **lat)
        assert set(c[c >= 0].tolist()) == {255}
    assert ref.cells(np.array([[128, -1], [-1, -1]]), **lat)[0, 0] == 0 and ref.cells(np.array([[129, -1], [-1, -1]]), **lat)[0, 0] == 1      # 128.5 is the first tie
    assert (ref.cells(np.full((2, 2), -1), **lat) == -1).all()


def test_reference_blend_by_hand():
    rng = np.random.default_rng(3)
    region = rng.integers(0, 256, size=(9, 14, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    idx = np.array([[5, -1, 200, 0], [-1, 255, 7, -1], [1, 2, -1, 3]])
    for down in (1, 2, 4):
        m = ref.box(region, down)
        assert m.shape == (9 // down, 14 // down, 3)
        assert np.array_equal(ref.canvas(region, idx, 4, lut, 0, down), m.astype(np.uint8))                   # alpha = 0: the box-filtered region
        flat = ref.canvas(region, idx, 4, lut, 256, down)
        per = np.repeat(np.repeat(idx, 4 // down, axis=0), 4 // down, axis=1)[:m.shape[0], :m.shape[1]]
        assert np.array_equal(flat[per >= 0], lut[per[per >= 0]]) and np.array_equal(flat[per < 0], m[per < 0].astype(np.uint8))
    assert np.array_equal(ref.box(region, 1), region.astype(np.int64))
    px = region[0:2, 4:6, 1].astype(int)
    assert ref.box(region, 2)[0, 2, 1] == (px.sum() + 2) // 4
    assert ref.box(np.array([[[1, 2, 3], [2, 2, 4]], [[1, 3, 3], [2, 3, 4]]], dtype=np.uint8), 2).tolist() == [[[2, 3, 4]]]      # 6/4 -> 2 (tie up), 10/4 -> 3, 14/4 -> 4
    one = ref.canvas(np.full((4, 4, 3), 10, dtype=np.uint8), np.array([[9]]), 4, np.full((256, 3), 200, dtype=np.uint8), 102, 1)
    assert set(one.reshape(-1).tolist()) == {(102 * 200 + 154 * 10 + 128) >> 8} == {86}
    assert ref.canvas(np.zeros((1, 1, 3), dtype=np.uint8), np.array([[3]]), 4, lut, 102, 4).shape == (0, 0, 3)


@pytest.mark.parametrize("k", range(len(ref.LATTICES)))
def test_reference_cases_are_mixed(k):
    """The facts the GPU tests rely on: covered and uncovered cells, overlap up to n, several colours, a canvas that differs from the region."""
    from toad_amd.tissue import lattice, lattice_cell
    (hr, wr), tile, stride, origin, cell = ref.LATTICES[k]
    assert lattice_cell(tile, stride, origin) == cell
    s, origins, q, t, (nx, ny) = ref.case(k)
    assert (nx, ny) == lattice(hr, wr, tile, stride, origin) and t.shape == (ny, nx)
    assert 0 < len(origins) < t.size and (t >= 0).sum() == len(origins) and q.min() == 0 and q.max() == 65535
    n, _ = ref.coverage(t, cell, tile, stride, origin, (hr, wr))
    c = ref.cells(t, cell, tile, stride, origin, (hr, wr))
    assert n.shape == (-(-hr // cell), -(-wr // cell)) and n.max() == (4, 1, 16, 4, 1, 16)[k]
    assert (n == 0).any() and (n > 0).any() and np.array_equal(c == -1, n == 0) and c.min() == -1 and c.max() <= 255 and len(np.unique(c)) >= 8
    if k == 0:
        assert ((n == 0).sum(), n.size) == (77, 170)
    if k == 2:
        assert ((n == 0).sum(), n.size) == (328, 1092)
    if k == 3:
        assert t.size == 5 and len(origins) == 4
    for fine in (f for f in (4, 8, 16, 32, 64) if f < cell):            # a finer cell size repeats the coarse cells
        r = cell // fine
        cf = ref.cells(t, fine, tile, stride, origin, (hr, wr))
        assert np.array_equal(cf, np.repeat(np.repeat(c, r, axis=0), r, axis=1)[:cf.shape[0], :cf.shape[1]])
    for down in (1, 2, 4):
        out = ref.canvas(s, c, cell, ref.jet(), 102, down)
        plain = ref.box(s, down).astype(np.uint8)
        changed = (out != plain).any(axis=2)
        assert out.shape == (hr // down, wr // down, 3) and changed.any() and not changed.all()
