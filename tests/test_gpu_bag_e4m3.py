"""GPU: e4m3 bags (csrc/bag_e4m3.hip) - the decode and the quantiser against the numpy twin (tests/e4m3_ref.py) bit for bit, on every code and
exponent, on every fp16 pattern and code boundary, at every alignment of either array inside guard-filled buffers, past 2^31 output bytes, and through
BagPrefetcher into the x16 multi-slide step. The reference loads a bag and copies it to the device (datasets/dataset_mtl_concat.py:369-373,
utils/core_utils_mtl_concat.py:201-204); here the codes cross the link and the decode runs behind the copy."""
import numpy as np
import pytest
import torch

from tests import e4m3_ref as R
from tests.test_bag_e4m3_host import EXPS, SPECIALS, above_max, boundary_values

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 7), (5, 1000), (64, 1024), (1031, 1024)]
ROW_OFFSETS = (0, 1, 3)
BYTE_OFFSETS = (0, 1, 2, 3, 5, 16)
GUARD = 0xA5
NP = {torch.float16: (np.float16, torch.int16), torch.float32: (np.float32, torch.int32)}


def _table(exp, dt, cuda):
    """The twin's 256 decoded values as a device tensor of dt (NaN at 0x7F and 0xFF)."""
    return torch.from_numpy(R.decode_bits(np.arange(256), exp, NP[dt][0])).to(cuda)


def _assert_bits(got, ref, what):
    """Equal bit patterns where the reference is a number, NaN where it is NaN."""
    ib = NP[got.dtype][1]
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    bad = (got.view(ib) != ref.view(ib)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ in bits"


def test_decode_of_every_code_at_every_exponent(cuda):
    from toad_amd import ops
    codes = torch.arange(256, dtype=torch.uint8).reshape(16, 16).to(cuda)
    for exp in range(R.EXP_MIN, R.EXP_MAX + 1):
        for dt in (torch.float16, torch.float32):
            got = ops.bag_dequantise_e4m3(codes, exp, out_dtype=dt)
            assert got.dtype == dt and got.shape == (16, 16)
            _assert_bits(got.reshape(-1), _table(exp, dt, cuda), f"exp {exp} {dt}")
            got8 = ops.bag_dequantise_e4m3(codes.view(torch.float8_e4m3fn), exp, out_dtype=dt)
            _assert_bits(got8.reshape(-1), _table(exp, dt, cuda), f"float8 view, exp {exp} {dt}")
    # every code in every lane position of the 16-code body, and in the element path (an odd byte offset)
    flat = torch.arange(256, dtype=torch.uint8).repeat(17)[: 16 * 271 + 1].to(cuda)
    # ... and behind a head of 15 or 11 elements (codes and output reach 16-byte alignment at the same element: offsets (1, 1) and (5, 5))
    for off, oo in ((0, 0), (1, 0), (1, 1), (5, 5)):
        c = flat[off:off + 16 * 270].view(270, 16)
        obuf = torch.full((oo + 16 * 270 + 8,), 9.0, dtype=torch.float16, device=cuda)
        o = obuf[oo:oo + 16 * 270].view(270, 16)
        ops.bag_dequantise_e4m3(c, 15, out=o)
        _assert_bits(o.reshape(-1), _table(15, torch.float16, cuda)[c.reshape(-1).long()], f"lanes, offsets {off}, {oo}")
        assert (obuf[:oo] == 9.0).all() and (obuf[oo + 16 * 270:] == 9.0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_decode_at_every_alignment_touches_nothing_else(cuda, shape):
    from toad_amd import ops
    n, k = shape
    g = torch.Generator(device=cuda).manual_seed(n * 1031 + k)
    src = torch.randint(0, 256, (n * k,), generator=g, device=cuda, dtype=torch.uint8)
    case = 0
    for dt in (torch.float16, torch.float32):
        gbits = torch.tensor([0x5A5A if dt == torch.float16 else 0x5A5A5A5A], dtype=NP[dt][1], device=cuda)
        for row in ROW_OFFSETS:
            for off in BYTE_OFFSETS:
                exp = (-7, 3, 15, 0)[case % 4]
                case += 1
                flat = torch.full((off + n * k + 32,), GUARD, dtype=torch.uint8, device=cuda)
                flat[off:off + n * k] = src
                codes = flat[off:off + n * k].view(n, k)
                buf = torch.empty((row + n + 2, k), dtype=dt, device=cuda)
                buf.view(NP[dt][1]).fill_(gbits.item())
                out = buf[row:row + n]
                assert codes.data_ptr() == flat.data_ptr() + off and out.data_ptr() == buf.data_ptr() + row * k * buf.element_size()
                ret = ops.bag_dequantise_e4m3(codes, exp, out=out)
                assert ret is out
                what = f"{shape} {dt} row {row} byte offset {off} exp {exp}"
                _assert_bits(out.reshape(-1), _table(exp, dt, cuda)[src.long()], what)
                ib = buf.view(NP[dt][1])
                assert (ib[:row] == gbits).all() and (ib[row + n:] == gbits).all(), f"{what}: the output guard changed"
                assert (flat[:off] == GUARD).all() and (flat[off + n * k:] == GUARD).all() and torch.equal(flat[off:off + n * k], src), f"{what}: codes changed"


def test_empty_bags_launch_nothing(cuda):
    from toad_amd import ops
    ops.enable_timing(False)
    out = torch.full((2, 1024), 7.0, dtype=torch.float16, device=cuda)
    got = ops.bag_dequantise_e4m3(torch.empty((0, 1024), dtype=torch.uint8, device=cuda), 0, out=out[:0])
    assert got.shape == (0, 1024) and (out == 7.0).all()
    assert ops.bag_dequantise_e4m3(torch.empty((0, 1024), dtype=torch.uint8, device=cuda), 0, out_dtype=torch.float32).shape == (0, 1024)
    codes, exp = ops.bag_quantise_e4m3(torch.empty((0, 1024), device=cuda))
    assert codes.shape == (0, 1024) and codes.dtype == torch.uint8 and exp == 0


def _quant_dev(x: torch.Tensor, exp: int, cuda) -> np.ndarray:
    from toad_amd import ops
    codes, e = ops.bag_quantise_e4m3(x.reshape(1, -1).contiguous().to(cuda), exp)
    assert e == exp and codes.dtype == torch.uint8 and codes.is_cuda
    return codes.reshape(-1).cpu().numpy()


def _assert_codes(got, x64, exp, what):
    ref = R.quantise(x64, exp)
    nan = np.isnan(x64)
    bad = np.nonzero((got != ref) & ~nan)[0]
    assert bad.size == 0, f"{what}, exp {exp}: {bad.size} codes differ, first x = {x64[bad[0]]!r}: {got[bad[0]]:#x} != {ref[bad[0]]:#x}"
    assert ((got[nan] & 0x7F) == 0x7F).all(), f"{what}: a NaN did not become a NaN code"


def test_quantiser_on_every_fp16_pattern_and_code_boundary(cuda):
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x64 = h.numpy().astype(np.float64)
    for exp in EXPS:
        _assert_codes(_quant_dev(h, exp, cuda), x64, exp, "fp16 input")
        _assert_codes(_quant_dev(h.float(), exp, cuda), x64, exp, "fp16 values as fp32")
        _assert_codes(_quant_dev(h[1:], exp, cuda), x64[1:], exp, "fp16 input, shifted by one lane")
        for what, v in (("midpoint neighbours", boundary_values(exp)), ("specials", SPECIALS), ("just above 448", above_max(exp))):
            _assert_codes(_quant_dev(torch.from_numpy(v.copy()), exp, cuda), v.astype(np.float64), exp, what)
    got = _quant_dev(torch.from_numpy(SPECIALS.copy()), 0, cuda)
    assert list(got[:4]) == [0x00, 0x80, 0x7E, 0xFE] and (got[4:] & 0x7F == 0x7F).all()
    x = np.array([1 + 2.0 ** -4 + 2.0 ** -12], dtype=np.float32)                         # fp32 is rounded once (tests/test_bag_e4m3_host.py)
    assert _quant_dev(torch.from_numpy(x), 0, cuda)[0] == 0x39 and _quant_dev(torch.from_numpy(x).half(), 0, cuda)[0] == 0x38


_QUANT_REF = {}


def _quant_case(shape, dt, exp):
    """(x on the host, the twin's codes): computed once per shape and dtype."""
    key = (shape, dt, exp)
    if key not in _QUANT_REF:
        n, k = shape
        g = torch.Generator().manual_seed(n * 7 + k)
        x = (torch.randn(n * k, generator=g) * torch.exp(torch.randn(n * k, generator=g) * 3)).to(dt)
        _QUANT_REF[key] = (x, torch.from_numpy(R.quantise(x.numpy(), exp)))
    return _QUANT_REF[key]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_quantiser_at_every_alignment_touches_nothing_else(cuda, shape):
    from toad_amd import _lib
    lib = _lib.load()
    n, k = shape
    for dt in (torch.float32, torch.float16):
        exp = 2 if dt == torch.float32 else 7
        x, ref = _quant_case(shape, dt, exp)
        xd, ref = x.to(cuda), ref.to(cuda)
        gval = torch.tensor([12345.0], dtype=dt, device=cuda)
        for xo in ROW_OFFSETS:                                                            # x starts xo ELEMENTS into its buffer
            for off in BYTE_OFFSETS:
                xbuf = torch.full((xo + n * k + 8,), gval.item(), dtype=dt, device=cuda)
                xbuf[xo:xo + n * k] = xd
                flat = torch.full((off + n * k + 32,), GUARD, dtype=torch.uint8, device=cuda)
                xv, cv = xbuf[xo:xo + n * k], flat[off:off + n * k]
                _lib.check(lib.toad_bag_quant_e4m3(xv.data_ptr(), int(dt == torch.float16), cv.data_ptr(), n * k, exp,
                                                   torch.cuda.current_stream().cuda_stream), "toad_bag_quant_e4m3")
                what = f"{shape} {dt} x element offset {xo} code byte offset {off}"
                assert torch.equal(cv, ref), f"{what}: {int((cv != ref).sum())} codes differ"
                assert (flat[:off] == GUARD).all() and (flat[off + n * k:] == GUARD).all(), f"{what}: the code guard changed"
                assert (xbuf[:xo] == gval).all() and (xbuf[xo + n * k:] == gval).all() and torch.equal(xv.view(NP[dt][1]), xd.view(NP[dt][1])), f"{what}: x changed"


@pytest.mark.parametrize("scale", [0.7, 40.0])
def test_round_trip_picks_the_exponent_and_equals_the_twin(cuda, scale):
    from toad_amd import ops
    x = torch.randn(257, 1024, generator=torch.Generator().manual_seed(11)).abs() * scale
    for xd in (x.to(cuda), x.half().to(cuda)):
        host = xd.cpu().numpy()
        codes, exp = ops.bag_quantise_e4m3(xd)
        assert exp == R.e4m3_exponent(float(host.max())) == ops.e4m3_exponent(float(host.max()))
        ref_codes = R.quantise(host, exp)
        assert np.array_equal(codes.cpu().numpy(), ref_codes)
        for dt in (torch.float16, torch.float32):
            back = ops.bag_dequantise_e4m3(codes, exp, out_dtype=dt)
            assert np.array_equal(back.cpu().numpy().view(NP[dt][0]).astype(np.float64), R.decode(ref_codes, exp))
        err = np.abs(R.decode(ref_codes, exp) - host.astype(np.float64))
        assert (err <= R.error_bound(host, exp)).all()
        # the CPU path of the same two calls gives the same bits
        ccodes, cexp = ops.bag_quantise_e4m3(xd.cpu())
        assert cexp == exp and torch.equal(ccodes, codes.cpu())


def test_offsets_past_two_to_the_31_output_bytes(cuda):
    """One bag of 1,048,704 x 1024 codes: its fp16 output ends 262,144 bytes past 2^31. Three 4,096-row chunks against the twin's table applied on the
    device - the first, the one straddling output byte 2^31 (row 1,048,576), the last - and the guard rows on either side."""
    from toad_amd import ops
    n, k, exp = 1048704, 1024, 4
    g = torch.Generator(device=cuda).manual_seed(3)
    tile = torch.randint(0, 256, (4099, k), generator=g, device=cuda, dtype=torch.uint8)   # 4,099 rows, a prime: no period the indexing could share
    codes = tile.repeat(n // 4099 + 1, 1)[:n]
    del tile
    assert codes.is_contiguous() and codes.shape == (n, k)
    buf = torch.empty((n + 2, k), dtype=torch.float16, device=cuda)
    buf.view(torch.int16).fill_(0x5A5A)
    out = buf[1:n + 1]
    assert out.numel() * 2 > 2 ** 31
    ops.bag_dequantise_e4m3(codes, exp, out=out)
    table = _table(exp, torch.float16, cuda)
    for lo in (0, (2 ** 30) // k - 2048, n - 4096):
        _assert_bits(out[lo:lo + 4096].reshape(-1), table[codes[lo:lo + 4096].reshape(-1).long()], f"rows {lo} .. {lo + 4096}")
    ib = buf.view(torch.int16)
    assert (ib[0] == 0x5A5A).all() and (ib[n + 1] == 0x5A5A).all()
    # the quantiser at the same size would need the fp32 bag (4.3 GB): its 64-bit offsets are the same expressions, exercised here on the fp16 output
    # quantised back in place of the codes' last chunk
    back, _ = ops.bag_quantise_e4m3(out[n - 4096:], exp)
    fin = (codes[n - 4096:] & 0x7F) != 0x7F
    zero = (codes[n - 4096:] & 0x7F) == 0
    assert torch.equal(back[fin & ~zero], codes[n - 4096:][fin & ~zero]) and ((back[~fin] & 0x7F) == 0x7F).all()


def _model(cuda, seed=0):
    from toad_amd import TOAD_fc_mtl_concat
    torch.manual_seed(seed)
    m = TOAD_fc_mtl_concat(n_classes=18, dropout=False)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    m.relocate()
    return m


def test_ingest_of_e4m3_records_feeds_the_x16_multi_slide_step(cuda):
    from toad_amd import ops
    from toad_amd.dp import SlideShardedDP
    from toad_amd.ingest import BagPrefetcher, E4M3Bag
    lens = [200, 3000, 777, 1500, 300, 2048, 257, 1000]                                   # 8,082 rows fill the first buffer of 8,192; the last bag opens a second
    g = torch.Generator().manual_seed(17)
    e4, f16, ref = [], [], []
    for i, n in enumerate(lens):
        x = (torch.randn(n, 1024, generator=g) * 0.7).numpy()
        exp = R.e4m3_exponent(float(np.abs(x).max()))
        codes = R.quantise(x, exp)
        dec = R.decode_bits(codes, exp, np.float16)
        meta = ((3 * i) % 18, i % 2, float(i % 2))
        e4.append((E4M3Bag(torch.from_numpy(codes), exp),) + meta)
        f16.append((torch.from_numpy(dec),) + meta)
        ref.append(dec)
    feeds = {}
    for name, recs in (("e4m3", e4), ("fp16", f16)):
        landed = [(b, sx, lb, st) for (b, lb, st, sx) in BagPrefetcher(recs, cuda, depth=3, dtype=torch.float16, arena_rows=8192, arena_dtype=torch.float16)]
        torch.cuda.synchronize()
        bags = [s[0] for s in landed]
        for b, r in zip(bags, ref):
            assert b.dtype == torch.float16 and np.array_equal(b.cpu().numpy().view(np.uint16), r.view(np.uint16)), name
        view = ops._adjacent_rows(bags[:7])
        assert view is not None and view.dtype == torch.float16 and view.data_ptr() == bags[0].data_ptr() and view.shape == (sum(lens[:7]), 1024)
        assert ops._adjacent_rows(bags) is None
        model = _model(cuda, seed=2)
        model.train()
        dp = SlideShardedDP(model, {"lr": 1e-3, "weight_decay": 1e-5})
        ops.enable_timing(True)
        losses = dp.step(landed, len(landed))
        names = ops.collect_timing()
        ops.enable_timing(False)
        assert "mil_multi_step_x16" in names and "mil_multi_step" not in names, sorted(names)
        feeds[name] = (torch.stack([l.reshape(-1) for l in losses]), dp.flat_grad.clone())
    for a, b, what in zip(feeds["e4m3"], feeds["fp16"], ("losses", "gradient")):
        assert a.shape == b.shape and torch.isfinite(b).all()
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item(), what                # the bound of tests/test_gpu_multi_x16.py between two feeds
    # fp32 landing buffers, and prepared bags: the exact fp32 values
    landed = [s[0] for s in BagPrefetcher(e4, cuda, depth=2, arena_rows=8192)]
    torch.cuda.synchronize()
    for b, r in zip(landed, ref):
        assert b.dtype == torch.float32 and np.array_equal(b.cpu().numpy().view(np.uint32), r.astype(np.float32).view(np.uint32))
    assert ops._adjacent_rows(landed[:7]) is not None
    prepared = [s[0] for s in BagPrefetcher(e4, cuda, depth=2, prepare=True)]
    torch.cuda.synchronize()
    for p, r in zip(prepared, ref):
        want = ops.prepare_bag(torch.from_numpy(r.astype(np.float32)).to(cuda))
        assert getattr(p, "is_prepared_bag", False) and p.shape == want.shape
        assert torch.equal(p.amax, want.amax) and torch.equal(p.planes, want.planes)
    # without a landing buffer, every file's own dtype: an e4m3 bag is fp16
    own = [s[0] for s in BagPrefetcher(e4[:2] + f16[:1], cuda, dtype=None)]
    torch.cuda.synchronize()
    assert [b.dtype for b in own] == [torch.float16] * 3 and np.array_equal(own[1].cpu().numpy().view(np.uint16), ref[1].view(np.uint16))
