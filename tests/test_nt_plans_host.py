"""CPU: the restated NT plan of tests/nt_ref.py against the library's own (toad_nt_plan, toad_relu_bits_plan), the regime table behind
tests/test_gpu_nt_plans.py, the operand families' preconditions on the very operands the GPU file runs, and the numpy emulation of the two-piece
arithmetic: bitwise on the integer families in every mode under every listed plan of at most 2,561 rows, inside the derived bound on the real ones."""
import ctypes

import numpy as np
import pytest

from tests import nt_ref as R

READER, ADDEND, POOL, SELF = 1, 2, 4, 64                 # include/toad_hip.h TOAD_BITS_*
FLAGS = {"plain": 0, "addend": ADDEND, "mask": READER, "addend_mask": READER | ADDEND, "bits": READER, "pool_mask": READER | POOL,
         "pool_bits": READER | POOL, "pool": POOL}


def _lib():
    from toad_amd import _lib
    return _lib.load()


def _library_plan(lib, m, n, k, flags):
    out = (ctypes.c_int * 34)()
    assert lib.toad_nt_plan(m, n, k, flags, ctypes.addressof(out)) == 0, (m, n, k, flags, lib.toad_last_error())
    return list(out)


def _restated_plan(m, n, k, epilogue):
    lp = R.launch_plan(m, n, k, R.nt_route(m, n, k, epilogue)[0])
    return [int(lp.half), lp.fixup] + [v for p in lp.xcd for v in (p.rounds, p.rem, p.g, p.tiles)]


def test_plan_query_validates_its_arguments():
    lib = _lib()
    out = (ctypes.c_int * 34)()
    assert lib.toad_nt_plan(300, 512, 512, 0, None) == -1
    assert lib.toad_nt_plan(300, 512, 512, 1 << 12, ctypes.addressof(out)) == -1                 # unknown flag
    assert lib.toad_nt_plan(300, 512, 500, 0, ctypes.addressof(out)) == -2                       # not a shape of the two-piece kernel
    assert lib.toad_nt_plan(2_000_000, 512, 1024, 128, ctypes.addressof(out)) == -2 and b"row chunks" in lib.toad_last_error()
    assert lib.toad_nt_plan(300, 512, 512, SELF | ADDEND, ctypes.addressof(out)) == -1           # the launcher refuses the combination


@pytest.mark.parametrize("n", [4, 256, 260, 512, 768, 1024])
def test_restated_plan_equals_the_library_plan(n):
    """Every row-tile count 1 .. 600, at the first and last row of the last tile and at rows 128 / 129 of it (the half-height tile count changes
    there), six reduction depths, on both tile-height routes: the plain one (half-height tiles inside their range) and the addend one (never)."""
    lib = _lib()
    halves = 0
    for t in range(1, 601):
        for r in (1, 128, 129, 256):
            m = (t - 1) * 256 + r
            for nk in (1, 2, 3, 16, 24, 32):
                for epilogue in ("plain", "addend"):
                    got = _library_plan(lib, m, n, 32 * nk, FLAGS[epilogue])
                    assert got == _restated_plan(m, n, 32 * nk, epilogue), (m, n, nk, epilogue)
                    halves += got[0]
                    assert epilogue == "plain" or got[0] == 0
    assert halves > 0                                            # (every width has a half-height range; nt_ref.HALF_RANGE lists four)
    for first, last in [R.HALF_RANGE[n]] if n in R.HALF_RANGE else []:
        assert [R.nt_half_tiles(m, n) for m in (first - 1, first, last, last + 1)] == [False, True, True, False]


def _restated_map(m, n, k, epilogue):
    half, read_bits = R.nt_route(m, n, k, epilogue)
    lp = R.launch_plan(m, n, k, half)
    tiles_m, tiles_n = R._cdiv(m, R.PB), lp.tiles_n
    out = np.zeros((tiles_m, tiles_n), dtype=np.uint8)
    if epilogue.endswith("bits") and not read_bits:
        return out
    if half:
        out[:] = 2
        return out
    for (tm, tn), sl in R.tile_slices(lp).items():
        if len(sl) == 1:
            out[tm, tn] = 1
    return out


def test_restated_whole_tile_map_equals_the_bit_image_plan():
    lib = _lib()
    shapes = [(c.M, c.N, c.K) for c in R.CASES + [R.ADDEND_CASE]] + [(m, 512, 32 * nk) for m in (300, 2049, 4100, 16385, 20000, 40000) for nk in (1, 2, 24)]
    for m, n, k in shapes:
        for epilogue in ("plain", "addend", "bits"):
            buf = np.full(R._cdiv(m, 256) * R._cdiv(n, 256), 255, dtype=np.uint8)
            assert lib.toad_relu_bits_plan(m, n, k, FLAGS[epilogue], buf.ctypes.data) == 0
            assert np.array_equal(buf.reshape(-1, R._cdiv(n, 256)), _restated_map(m, n, k, epilogue)), (m, n, k, epilogue)


def test_every_case_reaches_the_regime_it_is_listed_under():
    for c in R.CASES:
        got = R.regimes(c.M, c.N, c.K)
        assert c.want <= got, (c, sorted(got))
        f = R.plan_facts(c.M, c.N, c.K)
        for key, v in c.facts.items():
            assert (f["plans"][0].tiles if key == "xcd0_tiles" else f[key]) == v, (c, key)
    c = R.ADDEND_CASE
    assert c.want <= R.regimes(c.M, c.N, c.K, "addend_mask") and "half" in R.regimes(c.M, c.N, c.K, "mask")
    # the plans of single rows, XCD by XCD
    p = R.plan_facts(32769, 512, 768)["plans"]
    assert (p[0].rounds, p[0].rem, p[0].g) == (1, 2, 16) and all((q.rounds, q.rem, q.g) == (1, 0, 0) for q in p[1:])
    p = R.plan_facts(20481, 768, 64)["plans"]
    assert (p[0].rounds, p[0].rem, p[0].g) == (1, 1, 2) and all((q.rounds, q.rem, q.g) == (0, 30, 1) for q in p[1:])
    p = R.plan_facts(16385, 512, 64)["plans"]
    assert [(q.tiles, q.g) for q in p] == [(18, 1)] + [(16, 1)] * 7 and R.plan_facts(16385, 512, 64)["natural"] == [1] + [2] * 7
    p = R.plan_facts(65281, 512, 64)["plans"]
    assert all((q.rounds, q.rem) == (2, 0) for q in p)
    assert "stagger" not in R.regimes(65280 - 256, 512, 64)                                     # 510 tiles: below the threshold
    assert "bits_not_read" in R.regimes(1, 512, 32, "bits") and "bits_not_read" not in R.regimes(1, 512, 64, "bits")
    assert R.plan_facts(10000, 512, 768, "addend_mask")["gs"] == [2]
    for m, n, k in R.REAL_CASES:
        assert (m, n, k) in {(c.M, c.N, c.K) for c in R.CASES}


def test_slices_tile_the_reduction_exactly_once():
    for nk in range(1, 33):
        for g in range(1, min(nk, R.PB_GMAX) + 1):
            cuts = [((p * nk) // g, ((p + 1) * nk) // g) for p in range(g)]
            assert cuts[0][0] == 0 and cuts[-1][1] == nk and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and all(b > a for a, b in cuts)
    for c in R.CASES + [R.ADDEND_CASE]:
        for epilogue in ("plain", "addend"):
            lp = R.launch_plan(c.M, c.N, c.K, R.nt_route(c.M, c.N, c.K, epilogue)[0])
            sl = R.tile_slices(lp)
            assert set(sl) == {(tm, tn) for tm in range(lp.tiles_m) for tn in range(lp.tiles_n)}, c
            for cuts in sl.values():
                assert cuts[0][0] == 0 and cuts[-1][1] == lp.nk and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), c
            assert len(R.walk(lp)) == sum(len(v) for v in sl.values())
            per_wg = {}
            for it in R.walk(lp):
                per_wg.setdefault(it.wg, []).append(it)
            assert all(sum(1 for it in v if it.part is not None) <= 1 for v in per_wg.values())       # one slab per workgroup


@pytest.mark.parametrize("case", R.CASES + [R.ADDEND_CASE], ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_family_preconditions_hold_on_the_operands_the_gpu_runs(case):
    for family in R.case_families(case):
        seed = R.CASE_SEED + case.M
        a, w = R.int_operands(family, case.M, case.N, case.K, seed)
        assert a.shape == (case.M, case.K) and w.shape == (case.N, case.K) and a.dtype == np.float32
        assert R.int_ok(family, a, w, case.M, case.N, seed), (case, family)
        bias, addend = R.int_sides(case.M, case.N, seed)
        assert np.abs(bias).max() <= R.INT_SIDE_MAX and np.abs(addend).max() <= R.INT_SIDE_MAX and np.array_equal(bias, np.rint(bias))


EMU_CASES = [c for c in R.CASES if c.M <= R.EMU_MAX_ROWS]


@pytest.mark.parametrize("case", EMU_CASES, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_emulation_equals_the_exact_reference_on_the_integer_families(case):
    """Settles the exactness argument of nt_ref's docstring before any GPU run: in every mode of the GPU file the emulated arithmetic - with the
    launch's own tile height and K-slices - reproduces the int64 reference and the exact block maxima, and every split was exact."""
    m, n, k = case.M, case.N, case.K
    seed = R.CASE_SEED + m
    poisoned = 0
    for family in R.INT_FAMILIES:
        a, w = R.int_operands(family, m, n, k, seed)
        bias, addend = R.mode_sides(family, m, n, seed)
        src = None
        for mode in R.MODES:
            epi = R.mode_epilogue(mode, bias, addend, src)
            lp = R.launch_plan(m, n, k, R.nt_route(m, n, k, R.MODE_ROUTE[mode])[0])
            y, y_amax, info = R.emulate_nt(a, w, lp, R.MODE_OPERAND[mode], **epi)
            ref = R.ref_exact(family, a, w, **epi)
            assert info["exact_split"], (case, family, mode)
            assert np.array_equal(y, ref), (case, family, mode, int((y != ref).sum()))
            assert np.array_equal(y_amax, R.exact_amax(ref)), (case, family, mode)
            if mode == "fwd_bias_relu":
                src = ref
            if family == "late_outlier_int" and mode == "fwd_self":
                poisoned += info["poisoned"]
    if R.deep_last_slice(R.launch_plan(m, n, k, R.nt_route(m, n, k)[0])):
        assert poisoned > 0, "late_outlier_int must reach the poisoned second pass"


@pytest.mark.parametrize("family", R.REAL_FAMILIES)
def test_emulation_stays_inside_the_bound_on_the_real_families(family):
    for m, n, k in R.REAL_CASES[:2] + [(513, 512, 768)]:
        a, w = R.real_family(family, m, n, k, R.REAL_SEED + m)
        bias, addend = R.real_sides(m, n, R.REAL_SEED + m)
        for mode in ("fwd_given", "fwd_self", "fwd_bias_relu", "dgrad_plain", "dgrad_addend_mask", "dgrad_bits"):
            src = R.ref_f64(a, w, bias=bias, relu=True)
            epi = R.mode_epilogue(mode, bias, addend, src)
            lp = R.launch_plan(m, n, k, R.nt_route(m, n, k, R.MODE_ROUTE[mode])[0])
            y, _, info = R.emulate_nt(a, w, lp, R.MODE_OPERAND[mode], **epi)
            bound = R.nt_bound(a, w, R.max_g(lp), R.MODE_OPERAND[mode], epi.get("bias"), epi.get("addend")) * epi.get("mask_scale", 1.0)
            ratio = float((np.abs(y.astype(np.float64) - R.ref_f64(a, w, **epi)) / bound).max())
            print(f"nt bound (emulation) {family} {m}x{n}x{k} {mode}: err/bound {ratio:.3e}")
            assert np.isfinite(y).all() and ratio <= 1.0, (family, m, mode, ratio)
            assert family != "late_giant" or mode != "fwd_self" or info["poisoned"] > 0 or not R.deep_last_slice(lp)
