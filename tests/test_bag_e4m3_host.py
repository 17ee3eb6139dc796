"""CPU: the e4m3 bag format (toad_amd/ingest.py, DESIGN.md "e4m3 bags") - the code table, the exactness of the decode in fp16, the quantiser of the
product's CPU path against the numpy twin (tests/e4m3_ref.py), the derived error bound, the exponent rule, the file form, the loader's refusals, the
prefetcher on device="cpu" and the argument checks of the two C entry points. Every comparison is == on bits unless it says otherwise."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import e4m3_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPS = (-7, 0, 5, 15)


def _codes_of(x: torch.Tensor, exp: int) -> np.ndarray:
    """The product's CPU quantiser on a flat tensor."""
    from toad_amd import ops
    codes, e = ops.bag_quantise_e4m3(x.reshape(1, -1).contiguous(), exp)
    assert e == exp and codes.dtype == torch.uint8
    return codes.reshape(-1).numpy()


def _assert_codes(got: np.ndarray, x64: np.ndarray, exp: int, what: str):
    ref = R.quantise(x64, exp)
    nan = np.isnan(x64)
    bad = np.nonzero((got != ref) & ~nan)[0]
    assert bad.size == 0, f"{what}, exp {exp}: {bad.size} codes differ, first x = {x64[bad[0]]!r}: {got[bad[0]]:#x} != {ref[bad[0]]:#x}"
    assert ((got[nan] & 0x7F) == 0x7F).all() and ((ref[nan] & 0x7F) == 0x7F).all(), f"{what}: a NaN did not become a NaN code"


def boundary_values(exp: int) -> np.ndarray:
    """fp32: the neighbours (-1, 0, +1 ulp) of every midpoint between adjacent codes, divided by 2^exp, both signs."""
    m = (R.MIDS * 2.0 ** -exp).astype(np.float32)
    assert np.array_equal(m.astype(np.float64), R.MIDS * 2.0 ** -exp)                     # the midpoints themselves are fp32 numbers
    v = np.concatenate([(m.view(np.int32) + d).view(np.float32) for d in (-1, 0, 1)])
    return np.concatenate([v, -v])


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)


def above_max(exp: int) -> np.ndarray:
    top = np.float32(448.0 * 2.0 ** -exp)
    v = np.array([top, np.nextafter(top, np.float32(np.inf)), top * np.float32(1.01), top * np.float32(1.0357), top * np.float32(1.0715), top * np.float32(2),
                  top * np.float32(100)], dtype=np.float32)
    return np.concatenate([v, -v])


def test_the_table_is_torchs_and_exact_in_fp16_inside_the_exponent_range():
    codes = torch.arange(256, dtype=torch.uint8)
    tv = codes.view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    assert np.array_equal(np.isnan(tv), np.isnan(R.TABLE)) and np.isnan(R.TABLE).sum() == 2 and np.isnan(R.TABLE[[0x7F, 0xFF]]).all()
    fin = ~np.isnan(tv)
    assert np.array_equal(tv[fin], R.TABLE[fin]) and np.array_equal(np.signbit(tv[fin]), np.signbit(R.TABLE[fin]))
    assert R.TABLE[0x7E] == 448.0 and R.TABLE[1] == 2.0 ** -9 and not np.isinf(R.TABLE).any()
    for exp in range(R.EXP_MIN, R.EXP_MAX + 1):
        v = R.TABLE[fin] * 2.0 ** -exp
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v), exp
    assert R.TABLE[1] * 2.0 ** -15 == 2.0 ** -24
    for exp in (R.EXP_MIN - 1, R.EXP_MAX + 1):                                            # 448 * 2^8 overflows fp16; 2^-9 * 2^-16 is below its least subnormal
        with np.errstate(over="ignore"):
            v = R.TABLE[fin] * 2.0 ** -exp
            assert not np.array_equal(v.astype(np.float16).astype(np.float64), v), exp


def test_cpu_decode_equals_the_twin_for_every_code_and_exponent():
    from toad_amd import ops
    codes = torch.arange(256, dtype=torch.uint8).reshape(16, 16)
    for exp in range(R.EXP_MIN, R.EXP_MAX + 1):
        for dt, nd, bits in ((torch.float16, np.float16, np.uint16), (torch.float32, np.float32, np.uint32)):
            got = ops.bag_dequantise_e4m3(codes, exp, out_dtype=dt).numpy().reshape(-1)
            got8 = ops.bag_dequantise_e4m3(codes.view(torch.float8_e4m3fn), exp, out_dtype=dt).numpy().reshape(-1)
            ref = R.decode_bits(np.arange(256), exp, nd)
            fin = ~np.isnan(ref)
            assert np.array_equal(got.view(bits)[fin], ref.view(bits)[fin]) and np.isnan(got[~fin]).all(), (exp, dt)
            assert np.array_equal(got8.view(bits)[fin], got.view(bits)[fin]) and np.isnan(got8[~fin]).all()
    for bad in (dict(codes=codes.float(), exp=0), dict(codes=codes, exp=16), dict(codes=codes, exp=-8), dict(codes=codes[0], exp=0),
                dict(codes=codes.t(), exp=0), dict(codes=codes, exp=0, out=torch.empty(16, 16, dtype=torch.bfloat16)),
                dict(codes=codes, exp=0, out=torch.empty(16, 15, dtype=torch.float16)), dict(codes=codes, exp=0, out_dtype=torch.bfloat16),
                dict(codes=codes, exp=1.0)):
        with pytest.raises(ValueError):
            ops.bag_dequantise_e4m3(**bad)


def test_cpu_quantiser_equals_the_twin_on_every_fp16_pattern():
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x64 = h.numpy().astype(np.float64)
    for exp in EXPS:
        _assert_codes(_codes_of(h, exp), x64, exp, "fp16 input")
        _assert_codes(_codes_of(h.float(), exp), x64, exp, "fp16 values as fp32")


def test_cpu_quantiser_equals_the_twin_at_the_code_boundaries_and_specials():
    for exp in EXPS:
        for what, v in (("midpoint neighbours", boundary_values(exp)), ("specials", SPECIALS), ("just above 448", above_max(exp))):
            _assert_codes(_codes_of(torch.from_numpy(v.copy()), exp), v.astype(np.float64), exp, what)
        top = above_max(exp)
        assert (R.quantise(top, exp) & 0x7F == 0x7E).all()                                # everything from 448 up saturates, nothing becomes NaN
    got = _codes_of(torch.from_numpy(SPECIALS.copy()), 0)
    assert list(got[:4]) == [0x00, 0x80, 0x7E, 0xFE] and (got[4:] & 0x7F == 0x7F).all()


def test_fp32_is_rounded_once():
    """1 + 2^-4 + 2^-12 lies above the midpoint of the codes 1.0 and 1.125, its fp16 rounding 1 + 2^-4 on it: a tie that goes to the even code."""
    x = np.array([1 + 2.0 ** -4 + 2.0 ** -12], dtype=np.float32)
    assert x.astype(np.float16)[0] == 1 + 2.0 ** -4
    assert _codes_of(torch.from_numpy(x), 0)[0] == 0x39 == R.quantise(x, 0)[0]
    assert _codes_of(torch.from_numpy(x).half(), 0)[0] == 0x38 == R.quantise(x.astype(np.float16), 0)[0]


def test_the_derived_error_bound_holds():
    rng = np.random.default_rng(5)
    x = (np.exp(rng.uniform(math.log(1e-6), math.log(400.0), 100000)) * rng.choice([-1.0, 1.0], 100000)).astype(np.float32)
    for exp in (0, -3):                                                                   # 400 * 2^0 and 400 * 2^-3 stay inside 448
        codes = _codes_of(torch.from_numpy(x), exp)
        err = np.abs(R.decode(codes, exp) - x.astype(np.float64))
        assert (err <= R.error_bound(x, exp)).all(), (exp, float((err / R.error_bound(x, exp)).max()))
        assert np.array_equal(codes, R.quantise(x, exp))
    small = x[np.abs(x) <= 0.01]
    codes = _codes_of(torch.from_numpy(small), 15)                                        # 0.01 * 2^15 = 328
    assert (np.abs(R.decode(codes, 15) - small.astype(np.float64)) <= R.error_bound(small, 15)).all()


def test_e4m3_exponent():
    from toad_amd import ops
    want = {0: 0, 1e-30: 15, 0.0136: 15, 0.0137: 14, 447.9: 0, 448: 0, 448.1: -1, 57344: -7, 57345: -7, 65504: -7}
    for amax, e in want.items():
        assert ops.e4m3_exponent(amax) == e == R.e4m3_exponent(amax), amax
        assert ops.e4m3_exponent(-amax) == e
    for amax in np.exp(np.random.default_rng(1).uniform(math.log(1e-9), math.log(6e4), 2000)):
        e = ops.e4m3_exponent(float(amax))
        assert e == R.e4m3_exponent(float(amax)) and (amax * 2.0 ** e <= 448 or e == -7) and (e == 15 or amax * 2.0 ** (e + 1) > 448)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            ops.e4m3_exponent(bad)
    x = torch.tensor([[1.0, -3.5, 0.25]])
    assert ops.bag_quantise_e4m3(x)[1] == ops.e4m3_exponent(3.5) == 7
    with pytest.raises(ValueError):
        ops.bag_quantise_e4m3(torch.tensor([[1.0, math.nan]]))
    assert ops.bag_quantise_e4m3(torch.tensor([[1.0, math.nan]]), 0)[0].tolist() == [[0x38, 0x7F]]
    for bad in (x.double(), x[0], torch.zeros(3, 2).t(), x.to(torch.bfloat16)):
        with pytest.raises(ValueError):
            ops.bag_quantise_e4m3(bad, 0)
    with pytest.raises(ValueError):
        ops.bag_quantise_e4m3(x, 16)


def _bag(n, k, seed, scale=0.7):
    return (torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * scale).abs()


def test_file_round_trip_with_weights_only(tmp_path):
    from toad_amd import ingest, ops
    x = _bag(37, 1024, 3)
    bag = ingest.save_bag_e4m3(str(tmp_path / "a.pt"), x)
    assert isinstance(bag, ingest.E4M3Bag) and bag.exp == ops.e4m3_exponent(x.abs().max().item()) and bag.codes.dtype == torch.uint8
    d = torch.load(str(tmp_path / "a.pt"), map_location="cpu", weights_only=True)
    assert sorted(d) == ["e4m3", "exp"] and d["e4m3"].dtype == torch.float8_e4m3fn and type(d["exp"]) is int and d["exp"] == bag.exp
    assert torch.equal(d["e4m3"].view(torch.uint8), bag.codes)
    assert np.array_equal(bag.codes.numpy(), R.quantise(x.numpy(), bag.exp))
    back = ingest._load(str(tmp_path / "a.pt"))
    assert isinstance(back, ingest.E4M3Bag) and back.exp == bag.exp and torch.equal(back.codes, bag.codes)
    ingest.save_bag_e4m3(str(tmp_path / "b.pt"), x, exp=3)
    assert ingest._load(str(tmp_path / "b.pt")).exp == 3
    q = ingest.quantise_bag(x.half())
    assert q.exp == bag.exp and np.array_equal(q.codes.numpy(), R.quantise(x.half().numpy(), q.exp))


def test_load_refuses_malformed_e4m3_bags():
    from toad_amd import ingest
    codes = torch.zeros(4, 8, dtype=torch.uint8)
    ok = ingest._load({"e4m3": codes.view(torch.float8_e4m3fn), "exp": 2})
    assert isinstance(ok, ingest.E4M3Bag) and ok.exp == 2 and ok.codes.dtype == torch.uint8
    assert isinstance(ingest._load(lambda: {"e4m3": codes, "exp": -7}), ingest.E4M3Bag)
    assert ingest._load(ingest.E4M3Bag(codes, 15)).exp == 15
    for bad in ({"e4m3": codes[0], "exp": 0}, {"e4m3": codes, "exp": 16}, {"e4m3": codes, "exp": -8}, {"e4m3": codes}, {"exp": 0},
                {"e4m3": codes.float(), "exp": 0}, {"e4m3": codes, "exp": 1.5}):
        with pytest.raises(ValueError):
            ingest._load(bad)
        with pytest.raises(ValueError):
            ingest._load(lambda bad=bad: bad)
    with pytest.raises(ValueError):
        ingest.E4M3Bag(codes[0], 0)


@pytest.mark.parametrize("arena_rows,dtype,arena_dtype", [(0, torch.float32, torch.float32), (0, torch.float16, torch.float32), (0, None, torch.float32),
                                                          (512, torch.float16, torch.float16), (512, torch.float32, torch.float32)],
                         ids=["no_arena_fp32", "no_arena_fp16", "no_arena_own_dtype", "arena_fp16", "arena_fp32"])
def test_prefetcher_on_cpu_takes_mixed_records(tmp_path, arena_rows, dtype, arena_dtype):
    from toad_amd import ingest, ops
    lens = [40, 100, 7, 200, 150, 64, 300]
    kinds = ["f32", "e4m3", "f16", "e4m3_file", "e4m3_dict", "e4m3", "e4m3_call"]
    recs, want = [], []
    for i, (n, kind) in enumerate(zip(lens, kinds)):
        x = _bag(n, 96, 10 + i, scale=0.7 if i % 2 else 40.0) * (1 if i % 3 else -1)
        if kind == "f32":
            src, ref = x, x.numpy().astype(np.float64)
        elif kind == "f16":
            src, ref = x.half(), x.half().numpy().astype(np.float64)
        else:
            exp = R.e4m3_exponent(float(np.abs(x.numpy()).max()))
            codes = R.quantise(x.numpy(), exp)
            ref = R.decode(codes, exp)
            bag = ingest.E4M3Bag(torch.from_numpy(codes), exp)
            if kind == "e4m3_file":
                src = str(tmp_path / f"{i}.pt")
                ingest.save_bag_e4m3(src, bag)
            elif kind == "e4m3_dict":
                src = {"e4m3": bag.codes.view(torch.float8_e4m3fn), "exp": exp}
            elif kind == "e4m3_call":
                src = lambda bag=bag: bag
            else:
                src = bag
        recs.append((src, i % 5, i % 2, float(i % 2)))
        want.append(ref)
    out = list(ingest.BagPrefetcher(recs, "cpu", depth=3, dtype=dtype, arena_rows=arena_rows, arena_dtype=arena_dtype))
    assert len(out) == len(recs)
    for i, ((bag, label, site, sex), ref, kind) in enumerate(zip(out, want, kinds)):
        assert int(label) == i % 5 and int(site) == i % 2 and float(sex) == float(i % 2)
        own = {"f32": torch.float32, "f16": torch.float16}.get(kind, torch.float16)
        assert bag.dtype == (own if dtype is None else dtype) and bag.shape == (lens[i], 96)
        if kind.startswith("e4m3") or bag.dtype == torch.float32 or kind == "f16":
            assert np.array_equal(bag.numpy().astype(np.float64), ref), (i, kind)        # exact: an e4m3 bag IS an fp16 bag
            assert np.array_equal(np.signbit(bag.numpy()), np.signbit(ref))
        else:
            assert torch.equal(bag, torch.from_numpy(ref).to(bag.dtype))                 # an fp32 record asked for as fp16: the caller's down-cast
    if arena_rows:
        # 40 + 100 + 7 + 200 + 150 = 497 rows share the first buffer, 64 + 300 the second
        bags = [o[0] for o in out]
        for group in (bags[:5], bags[5:]):
            view = ops._adjacent_rows(group)
            assert view is not None and view.data_ptr() == group[0].data_ptr() and view.shape[0] == sum(b.shape[0] for b in group)
            for a, b in zip(group, group[1:]):
                assert b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()
        assert ops._adjacent_rows(bags[4:6]) is None


def test_c_entry_points_check_their_arguments_without_a_gpu():
    from toad_amd import _lib, build
    lib = _lib.load()
    assert "bag_e4m3.hip" in build.SOURCES
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    one = ctypes.c_void_p(1 << 21)
    err = lambda: lib.toad_last_error().decode()
    for name in ("toad_bag_dequant_e4m3", "toad_bag_quant_e4m3"):
        assert name in _lib.SIGNATURES and name + "(" in header
        assert "datasets/dataset_mtl_concat.py:369-373" in header and "utils/core_utils_mtl_concat.py:201-204" in header
    dq, qz = lib.toad_bag_dequant_e4m3, lib.toad_bag_quant_e4m3
    assert dq(None, one, 0, 16, 0, None) == -1 and "null pointer" in err()
    assert dq(one, None, 1, 16, 0, None) == -1 and "null pointer" in err()
    assert dq(one, one, 0, -1, 0, None) == -1 and "n = -1" in err()
    assert dq(one, one, 0, 16, 16, None) == -1 and "exp = 16" in err()
    assert dq(one, one, 1, 16, -8, None) == -1 and "exp = -8" in err()
    assert dq(one, one, 0, 0, 0, None) == 0 and dq(one, one, 1, 0, 15, None) == 0
    assert qz(None, 0, one, 16, 0, None) == -1 and "null pointer" in err()
    assert qz(one, 1, None, 16, 0, None) == -1 and "null pointer" in err()
    assert qz(one, 0, one, -1, 0, None) == -1 and "n = -1" in err()
    assert qz(one, 0, one, 16, 16, None) == -1 and "exp = 16" in err()
    assert qz(one, 1, one, 0, -7, None) == 0 and qz(one, 0, one, 0, 0, None) == 0
    assert lib.toad_abi_version() == 15
