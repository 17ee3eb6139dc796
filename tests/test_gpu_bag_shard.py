"""GPU: e4m3 shards (csrc/bag_e4m3.hip "a LIST of bags") - the list decode, quantiser and abs-max against the numpy twin (tests/e4m3_ref.py) and against
the per-bag calls, bit for bit: one bag per exponent with boundaries at any byte inside guard-filled buffers, every code in every lane position, lists of
exactly and one more than E4M3_LIST_MAX bags, a bag that starts at output byte 2^31, and a shard through ShardPrefetcher into step_batch against the same
bags through BagPrefetcher into step. The reference loads one bag and copies it to the device (datasets/dataset_mtl_concat.py:369-373,
utils/core_utils_mtl_concat.py:201-204); here a step's bags cross the link as one record and one launch decodes them."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import e4m3_ref as R
from tests.test_bag_e4m3_host import SPECIALS, above_max, boundary_values

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NP = {torch.float16: (np.float16, torch.int16), torch.float32: (np.float32, torch.int32)}
EXPS23 = list(range(R.EXP_MIN, R.EXP_MAX + 1))                          # 23 bags, one per exponent
ROWS23 = [(0, 1, 3, 17, 64, 5)[i % 6] for i in range(23)]


def _offsets(rows):
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + r)
    return offs


_TABLES = {}


def _tables(dt, cuda):
    """[23, 256]: the twin's decoded values of every code at every exponent (row e + 7), as a device tensor of dt. Computed once."""
    if dt not in _TABLES:
        _TABLES[dt] = torch.from_numpy(np.stack([R.decode_bits(np.arange(256), e, NP[dt][0]) for e in EXPS23])).to(cuda)
    return _TABLES[dt]


def _twin(codes, offs, exps, dt, cuda):
    """The twin's decode of a list: every row looks its codes up in the table of its bag's exponent."""
    rows = torch.tensor([b - a for a, b in zip(offs, offs[1:])], device=cuda)
    which = torch.repeat_interleave(torch.tensor([e - R.EXP_MIN for e in exps], device=cuda), rows)
    return _tables(dt, cuda)[which[:, None].expand(codes.shape), codes.long()]


def _assert_bits(got, ref, what):
    """Equal bit patterns where the reference is a number, NaN where it is NaN."""
    ib = NP[got.dtype][1]
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    bad = (got.view(ib) != ref.view(ib)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ in bits"


def _guarded(src, off, row, dt, cuda):
    """(flat code buffer, codes view at byte offset off, output buffer, out view at row offset `row`, the output guard word)."""
    n, k = src.shape
    flat = torch.full((off + n * k + 32,), GUARD, dtype=torch.uint8, device=cuda)
    flat[off:off + n * k] = src.reshape(-1)
    gbits = 0x5A5A if dt == torch.float16 else 0x5A5A5A5A
    buf = torch.empty((row + n + 2, k), dtype=dt, device=cuda)
    buf.view(NP[dt][1]).fill_(gbits)
    return flat, flat[off:off + n * k].view(n, k), buf, buf[row:row + n], gbits


@pytest.mark.parametrize("k", [1, 7, 16, 1000, 1024])
def test_decode_one_bag_per_exponent_at_every_alignment_touches_nothing_else(cuda, k):
    from toad_amd import ops
    offs, n = _offsets(ROWS23), sum(ROWS23)
    g = torch.Generator(device=cuda).manual_seed(1031 + k)
    src = torch.randint(0, 256, (n, k), generator=g, device=cuda, dtype=torch.uint8)
    for dt in (torch.float16, torch.float32):
        ref = _twin(src, offs, EXPS23, dt, cuda)
        for off in (0, 1, 5):
            for row in (0, 1):
                flat, codes, buf, out, gbits = _guarded(src, off, row, dt, cuda)
                assert codes.data_ptr() == flat.data_ptr() + off and out.data_ptr() == buf.data_ptr() + row * k * buf.element_size()
                assert ops.bags_dequantise_e4m3(codes, offs, EXPS23, out=out) is out
                what = f"K {k} {dt} code byte offset {off} output row {row}"
                _assert_bits(out, ref, what)
                ib = buf.view(NP[dt][1])
                assert (ib[:row] == gbits).all() and (ib[row + n:] == gbits).all(), f"{what}: the output guard changed"
                assert (flat[:off] == GUARD).all() and (flat[off + n * k:] == GUARD).all() and torch.equal(codes, src), f"{what}: codes changed"
                # ... and the per-bag call on every slice, into a second guarded buffer, writes the same bytes
                _, _, buf1, out1, _ = _guarded(src, off, row, dt, cuda)
                for b, e in enumerate(EXPS23):
                    ops.bag_dequantise_e4m3(codes[offs[b]:offs[b + 1]], e, out=out1[offs[b]:offs[b + 1]])
                assert torch.equal(buf.view(NP[dt][1]), buf1.view(NP[dt][1])), f"{what}: the list call and the per-bag calls differ"


def test_decode_of_every_code_in_every_lane_position(cuda):
    from toad_amd import ops
    i = torch.arange(3 * 4096 + 16)
    flat = ((i + i // 256) % 256).to(torch.uint8).to(cuda)                  # every block of 256 codes is shifted by one lane against the one before
    rows, exps = [256, 255, 257], [-7, 3, 15]
    offs = _offsets(rows)
    for off in (0, 3):                                                    # 3: no element at which both arrays are 16-byte aligned - the element path
        codes = flat[off:off + 3 * 4096].view(768, 16)
        for dt in (torch.float16, torch.float32):
            got = ops.bags_dequantise_e4m3(codes, offs, exps, out_dtype=dt)
            assert got.dtype == dt and got.shape == (768, 16)
            _assert_bits(got, _twin(codes, offs, exps, dt, cuda), f"lanes, offset {off}, {dt}")
            got8 = ops.bags_dequantise_e4m3(codes.clone().view(torch.float8_e4m3fn), offs, exps, out_dtype=dt)
            assert torch.equal(got8.view(NP[dt][1]), got.view(NP[dt][1]))
    lanes = (torch.arange(4096) % 16).to(cuda)                             # bag 0 at offset 0: its body starts at element 0
    pairs = torch.unique(flat[:4096].long() * 16 + lanes)
    assert pairs.numel() == 256 * 16


@pytest.mark.parametrize("nb", ["max", "max_plus_1", "one", "all_empty"])
def test_list_lengths(cuda, nb):
    from toad_amd import ops
    m = ops.E4M3_LIST_MAX
    assert m >= 64
    # empty bags do not count against a launch: m (or m + 1) NON-EMPTY bags with empty ones in between, first and last
    if nb == "all_empty":
        rows = [0] * 5
    elif nb == "one":
        rows = [37]
    else:
        rows = [0]
        for i in range(m + (nb == "max_plus_1")):
            rows += [1 + i % 3] + ([0] if i % 7 == 0 else [])
    k = 40
    offs, n = _offsets(rows), sum(rows)
    exps = [EXPS23[i % 23] for i in range(len(rows))]
    g = torch.Generator(device=cuda).manual_seed(len(rows))
    src = torch.randint(0, 256, (n, k), generator=g, device=cuda, dtype=torch.uint8)
    flat, codes, buf, out, gbits = _guarded(src, 1, 1, torch.float16, cuda)
    ops.bags_dequantise_e4m3(codes, offs, exps, out=out)
    ib = buf.view(torch.int16)
    assert (ib[:1] == gbits).all() and (ib[1 + n:] == gbits).all() and (flat[:1] == GUARD).all() and (flat[1 + n * k:] == GUARD).all()
    if n:
        _assert_bits(out, _twin(src, offs, exps, torch.float16, cuda), nb)
        x = out.float()                                                   # finite or NaN; quantising the decode back at the same exponents gives the codes
        back, e2 = ops.bags_quantise_e4m3(x, offs, exps)
        fin = (src & 0x7F) != 0x7F
        assert e2 == exps and torch.equal(back[fin], src[fin]) and ((back[~fin] & 0x7F) == 0x7F).all()
        bits = ops.bags_absmax(x.nan_to_num(0.0), offs)
        want = torch.stack([x.nan_to_num(0.0)[a:b].abs().amax() if b > a else x.new_zeros(()) for a, b in zip(offs, offs[1:])])
        assert torch.equal(bits.view(torch.int32), want.view(torch.int32))
    else:
        assert ops.bags_absmax(torch.empty(0, k, device=cuda), offs).view(torch.int32).tolist() == [0] * len(rows)
        assert ops.bags_quantise_e4m3(torch.empty(0, k, device=cuda), offs)[1] == [0] * len(rows)


def test_second_bag_starts_at_output_byte_two_to_the_31(cuda):
    from toad_amd import ops
    rows, k, exps = [1048576, 128], 1024, [4, -3]
    offs, n = _offsets(rows), sum(rows)
    g = torch.Generator(device=cuda).manual_seed(3)
    tile = torch.randint(0, 256, (4099, k), generator=g, device=cuda, dtype=torch.uint8)   # 4,099 rows, a prime: no period the indexing could share
    codes = tile.repeat(n // 4099 + 1, 1)[:n]
    del tile
    buf = torch.empty((n + 1, k), dtype=torch.float16, device=cuda)
    buf.view(torch.int16).fill_(0x5A5A)
    out = buf[:n]
    assert out.data_ptr() % 16 == 0 and offs[1] * k * 2 == 2 ** 31
    ops.bags_dequantise_e4m3(codes, offs, exps, out=out)
    for lo, hi, e in ((0, 4096, 4), (rows[0] // 2, rows[0] // 2 + 4096, 4), (rows[0] - 4096, rows[0], 4), (rows[0], n, -3)):
        _assert_bits(out[lo:hi], _twin(codes[lo:hi], [0, hi - lo], [e], torch.float16, cuda), f"rows {lo} .. {hi}")
    assert (buf.view(torch.int16)[n] == 0x5A5A).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("k", [7, 1000])
def test_absmax_is_the_unsigned_maximum_of_the_patterns(cuda, dt, k):
    from toad_amd import _lib
    lib = _lib.load()
    rows = [0, 1, 300, 0, 17, 64, 5, 2000, 0, 3, 2]                       # 2000 x 1000: more lanes than one round of the bag's workgroups
    offs, n = _offsets(rows), sum(rows)
    g = torch.Generator().manual_seed(k)
    x = torch.randn(n, k, generator=g) * torch.exp(torch.randn(n, 1, generator=g) * 2)
    x[offs[1]] = -0.0                                                      # bag 1: zeros of both signs only
    x[offs[1], 0] = 0.0
    x[offs[4]:offs[5]] = (torch.randint(1, 1000, (17, k), generator=g).float() * (2.0 ** -149 if dt == torch.float32 else 2.0 ** -24))   # bag 4: subnormals
    x[offs[5] + 9, k // 2] = -math.inf                                     # bag 5: an Inf
    x[offs[7] + 1234, k - 1] = math.nan                                    # bag 7: a NaN, and ...
    x[offs[7] + 77, 0] = math.inf                                          # ... an Inf beside it
    x[offs[9]:offs[10]] = -x[offs[9]:offs[10]].abs() - 1.0                 # bag 9: negative numbers only
    x = x.to(dt)
    assert (x[offs[4]:offs[5]] != 0).all()
    want = [int(np.float32(x[a:b].float().abs().amax().item()).view(np.uint32)) if b > a else 0 for a, b in zip(offs, offs[1:])]
    assert want[1] == 0 and 0 < want[4] < 0x38800000 and want[5] == 0x7F800000
    c_offs = (ctypes.c_int64 * len(offs))(*offs)
    stream = torch.cuda.current_stream().cuda_stream
    for xo in (0, 1):                                                      # x starts xo ELEMENTS into its buffer: another head in every bag
        xbuf = torch.zeros(xo + n * k + 8, dtype=dt, device=cuda)
        xbuf[xo:xo + n * k] = x.reshape(-1).to(cuda)
        xv = xbuf[xo:xo + n * k]
        runs = []
        for _ in range(2):
            amax = torch.full((len(rows) + 2,), -1, dtype=torch.int32, device=cuda)           # 0xFFFFFFFF everywhere: the call must not build on it
            _lib.check(lib.toad_bags_absmax_bits(xv.data_ptr(), int(dt == torch.float16), amax[1:].data_ptr(), k, c_offs, len(rows), stream),
                       "toad_bags_absmax_bits")
            assert amax[0] == -1 and amax[-1] == -1
            runs.append([b & 0xFFFFFFFF for b in amax[1:-1].tolist()])
        assert runs[0] == runs[1]
        got = runs[0]
        for b, (g_, w_) in enumerate(zip(got, want)):
            if b == 7:
                assert g_ > 0x7F800000, f"bag 7 holds a NaN: {g_:#x}"
            else:
                assert g_ == w_ and g_ <= 0x7F800000, f"bag {b}, element offset {xo}: {g_:#x} != {w_:#x}"


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_list_quantiser_equals_the_per_bag_call_and_the_twin_at_the_code_boundaries(cuda, dt):
    from toad_amd import ops
    exps = [-7, 0, 5, 15, 3]
    fams = [np.concatenate([boundary_values(e), SPECIALS, above_max(e)]) for e in exps[:4]] + [np.zeros(0, dtype=np.float32)]
    with np.errstate(over="ignore"):
        fams = [f.astype(NP[dt][0]) for f in fams]                        # (fp16: the neighbours collapse onto fp16 numbers, ties included)
    offs = _offsets([len(f) for f in fams])                               # K = 1: a bag boundary at any byte
    host = np.concatenate(fams).reshape(-1, 1)
    for xo in (0, 1):
        xbuf = torch.zeros(xo + host.size + 8, dtype=dt, device=cuda)
        xbuf[xo:xo + host.size] = torch.from_numpy(host.reshape(-1).copy()).to(cuda)
        x = xbuf[xo:xo + host.size].view(-1, 1)
        codes, e2 = ops.bags_quantise_e4m3(x, offs, exps)
        assert e2 == exps and codes.dtype == torch.uint8 and codes.shape == x.shape
        got = codes.cpu().numpy()
        for b, e in enumerate(exps):
            a, z = offs[b], offs[b + 1]
            xs = host[a:z].astype(np.float64)
            ref, nan = R.quantise(xs, e), np.isnan(xs)
            assert np.array_equal(got[a:z][~nan], ref[~nan]) and ((got[a:z][nan] & 0x7F) == 0x7F).all(), f"bag {b} exp {e} element offset {xo}"
            one, _ = ops.bag_quantise_e4m3(x[a:z].contiguous(), e)
            assert torch.equal(codes[a:z], one), f"bag {b}: the list call and the per-bag call differ"


def test_list_quantiser_picks_each_bags_exponent_with_one_read_back(cuda):
    from toad_amd import ops
    rows = [0, 3, 17, 0, 64, 5, 1, 257, 0]
    offs, k = _offsets(rows), 1000
    g = torch.Generator().manual_seed(23)
    x = torch.cat([torch.randn(r, k, generator=g) * (10.0 ** (i % 5 - 2)) for i, r in enumerate(rows)])
    for xd in (x.to(cuda), x.half().to(cuda)):
        host = xd.cpu().numpy()
        codes, exps = ops.bags_quantise_e4m3(xd, offs)
        want = [R.e4m3_exponent(float(np.abs(host[a:b]).max())) if b > a else 0 for a, b in zip(offs, offs[1:])]
        assert exps == want and len(set(want)) > 3
        ref = np.concatenate([R.quantise(host[a:b], e) for (a, b), e in zip(zip(offs, offs[1:]), want)])
        assert np.array_equal(codes.cpu().numpy(), ref)
        ccodes, cexps = ops.bags_quantise_e4m3(xd.cpu(), offs)             # the CPU path of the same call gives the same bits
        assert cexps == exps and torch.equal(ccodes, codes.cpu())
        assert torch.equal(ops.bags_absmax(xd, offs).view(torch.int32).cpu(), ops.bags_absmax(xd.cpu(), offs).view(torch.int32))
    for poison, bag in ((math.nan, 4), (math.inf, 7)):
        y = x.clone()
        y[offs[bag] + 1, 5] = poison
        with pytest.raises(ValueError, match=f"bag {bag}:"):
            ops.bags_quantise_e4m3(y.to(cuda), offs)


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


def test_a_shard_feeds_the_x16_multi_slide_step_like_its_records(cuda):
    from toad_amd import ops
    from toad_amd.dp import SlideShardedDP
    from toad_amd.ingest import BagPrefetcher, E4M3Shard, ShardPrefetcher
    lens = [200, 3000, 777, 1500, 300, 2048, 257, 1000]                   # the lengths of the per-record ingest test, as ONE shard
    offs = _offsets(lens)
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(sum(lens), 1024, generator=g) * 0.7).numpy()
    exps = [R.e4m3_exponent(float(np.abs(x[a:b]).max())) for a, b in zip(offs, offs[1:])]
    codes = np.concatenate([R.quantise(x[a:b], e) for (a, b), e in zip(zip(offs, offs[1:]), exps)])
    ref = np.concatenate([R.decode_bits(codes[a:b], e, np.float16) for (a, b), e in zip(zip(offs, offs[1:]), exps)])
    b = len(lens)
    shard = E4M3Shard(torch.from_numpy(codes), lens, exps, torch.tensor([(3 * i) % 18 for i in range(b)]), torch.arange(b) % 2, (torch.arange(b) % 2).float())
    second = E4M3Shard(torch.from_numpy(codes[:offs[3]].copy()), lens[:3], exps[:3], shard.label[:3], shard.site[:3], shard.sex[:3])
    batches = list(ShardPrefetcher([shard, second], cuda, depth=2))
    torch.cuda.synchronize()
    assert len(batches) == 2
    batch = batches[0]
    assert batch.bags.dtype == torch.float16 and batch.bags.is_cuda and batch.offsets == offs and len(batch) == b
    assert np.array_equal(batch.bags.cpu().numpy().view(np.uint16), ref.view(np.uint16))
    assert torch.equal(batch.label.cpu(), shard.label) and torch.equal(batch.site.cpu(), shard.site) and torch.equal(batch.sex.cpu(), shard.sex)
    # the second shard through the same prefetcher (double buffering): its own rows, and the first batch is still intact
    assert batches[1].offsets == offs[:4] and np.array_equal(batches[1].bags.cpu().numpy().view(np.uint16), ref[:offs[3]].view(np.uint16))
    assert torch.equal(batches[1].label.cpu(), shard.label[:3]) and batches[1].bags.data_ptr() != batch.bags.data_ptr()
    feeds = {}
    for name in ("shard", "records"):
        model = _model(cuda, seed=2)
        model.train()
        dp = SlideShardedDP(model, {"lr": 1e-3, "weight_decay": 1e-5})
        if name == "records":
            landed = [(bg, sx, lb, st) for (bg, lb, st, sx) in
                      BagPrefetcher(shard.records(), cuda, depth=3, dtype=torch.float16, arena_rows=8192, arena_dtype=torch.float16)]
            torch.cuda.synchronize()
            for (bg, _, _, _), (a, z) in zip(landed, zip(offs, offs[1:])):
                assert np.array_equal(bg.cpu().numpy().view(np.uint16), ref[a:z].view(np.uint16))
        ops.enable_timing(True)
        losses = dp.step_batch(batch, b) if name == "shard" else dp.step(landed, b)
        names = ops.collect_timing()
        ops.enable_timing(False)
        assert "mil_multi_step_x16" in names and "mil_multi_step" not in names, (name, sorted(names))
        assert len(losses) == b
        feeds[name] = (torch.stack([l.reshape(-1) for l in losses]), dp.flat_grad.clone())
    for a, r, what in zip(feeds["shard"], feeds["records"], ("losses", "gradient")):
        assert a.shape == r.shape and torch.isfinite(r).all()
        assert (a - r).abs().max().item() <= 1e-6 * r.abs().max().item(), what               # the bound of tests/test_gpu_multi_x16.py between two feeds
    # fp32 batches hold the same numbers
    b32 = list(ShardPrefetcher([second], cuda, dtype=torch.float32))[0]
    torch.cuda.synchronize()
    assert b32.bags.dtype == torch.float32 and np.array_equal(b32.bags.cpu().numpy().view(np.uint32), ref[:offs[3]].astype(np.float32).view(np.uint32))
