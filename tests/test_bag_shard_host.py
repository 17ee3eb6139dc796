"""CPU: e4m3 shards (toad_amd/ingest.py "e4m3 shards", csrc/bag_e4m3.hip "a LIST of bags") - the refusals of the three list entry points through fake
pointers, the refusals of the list ops, E4M3Shard's validation, the file form, the CPU path of the list ops against the per-bag ops and the numpy twin
(tests/e4m3_ref.py), ShardPrefetcher on device="cpu" against BagPrefetcher on the shard's records, and tools/bags_to_e4m3.py --shard. Every comparison
is == on bits."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import e4m3_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [0, 3, 17, 0, 0, 5, 64, 1, 0]                                  # empty bags first, in the middle (two in a row) and last
K = 24


def _offsets(rows):
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + r)
    return offs


def _data(rows=ROWS, k=K, seed=0):
    """x fp32 [R, k] with a different magnitude per bag, and its offsets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.randn(r, k, generator=g) * (10.0 ** (i % 5 - 2)) for i, r in enumerate(rows)])
    return x, _offsets(rows)


def test_c_entry_points_check_their_arguments_without_a_gpu():
    from toad_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "toad_hip.h")).read()
    for name in ("toad_bags_dequant_e4m3", "toad_bags_quant_e4m3", "toad_bags_absmax_bits"):
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(lib, name)
    assert "#define TOAD_E4M3_LIST_MAX 64" in header and ops.E4M3_LIST_MAX == 64 >= 64
    assert lib.toad_abi_version() == 15
    one, odd = ctypes.c_void_p(1 << 21), ctypes.c_void_p((1 << 21) + 1)
    err = lambda: lib.toad_last_error().decode()
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    i32 = lambda *v: (ctypes.c_int * len(v))(*v)
    no_offs, no_exps = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_int)()
    dq, qz, am = lib.toad_bags_dequant_e4m3, lib.toad_bags_quant_e4m3, lib.toad_bags_absmax_bits
    # each entry as f(a, b, k, offsets, exps, nb) with its two arrays first
    entries = {"toad_bags_dequant_e4m3": lambda a, b, k, o, e, nb: dq(a, b, 0, k, o, e, nb, None),
               "toad_bags_quant_e4m3": lambda a, b, k, o, e, nb: qz(a, 1, b, k, o, e, nb, None),
               "toad_bags_absmax_bits": lambda a, b, k, o, e, nb: am(a, 0, b, k, o, nb, None)}
    for name, f in entries.items():
        ok_o, ok_e = i64(0, 2, 2, 5), i32(0, -7, 15)
        assert f(None, one, 8, ok_o, ok_e, 3) == -1 and "null pointer" in err() and name in err()
        assert f(one, None, 8, ok_o, ok_e, 3) == -1 and "null pointer" in err()
        assert f(one, one, 8, no_offs, ok_e, 3) == -1 and "null pointer" in err()
        assert f(one, one, 8, ok_o, ok_e, -1) == -1 and "nb = -1" in err()
        assert f(one, one, 0, ok_o, ok_e, 3) == -1 and "k = 0" in err()
        assert f(one, one, -3, ok_o, ok_e, 3) == -1 and "k = -3" in err()
        assert f(one, one, 8, i64(1, 2, 2, 5), ok_e, 3) == -1 and "row_offsets[0] = 1" in err()
        assert f(one, one, 8, i64(0, 4, 3, 5), ok_e, 3) == -1 and err().startswith("bag 1:") and "decrease" in err()
        assert f(one, one, 8, i64(0, 4, 4, 3), ok_e, 3) == -1 and err().startswith("bag 2:")
        assert f(one, one, 1 << 40, i64(0, 1 << 40), i32(0), 1) == -2                  # more elements than byte offsets hold
        # nothing to launch: no bags, or empty bags only - the fake pointers are never touched
        assert f(one, one, 8, i64(0), ok_e, 0) == 0
        if name != "toad_bags_absmax_bits":                                            # (the abs-max call still has its three zeros to write)
            assert f(one, one, 8, i64(0, 0, 0, 0), ok_e, 3) == 0
    for f in (entries["toad_bags_dequant_e4m3"], entries["toad_bags_quant_e4m3"]):
        assert f(one, one, 8, i64(0, 2, 2, 5), no_exps, 3) == -1 and "null pointer" in err()
        assert f(one, one, 8, i64(0, 2, 2, 5), i32(0, 16, -8), 3) == -1 and err().startswith("bag 1:") and "exp = 16" in err()
        assert f(one, one, 8, i64(0, 2, 2, 5), i32(0, 0, -8), 3) == -1 and err().startswith("bag 2:") and "exp = -8" in err()
        assert f(one, one, 8, i64(0, 2, 1, 5), i32(99, 0, 0), 3) == -1 and err().startswith("bag 0:")   # the first failing bag wins
    # alignment, after everything else: out / x to their element, amax_bits to 4 bytes
    o, e = i64(0, 0), i32(0)
    assert dq(one, odd, 0, 8, o, e, 1, None) == -4 and "2-byte aligned" in err()
    assert dq(one, ctypes.c_void_p((1 << 21) + 2), 1, 8, o, e, 1, None) == -4 and "4-byte aligned" in err()
    assert dq(odd, one, 1, 8, o, e, 1, None) == 0                                       # codes may lie at any byte
    assert qz(odd, 1, one, 8, o, e, 1, None) == -4 and "2-byte aligned" in err()
    assert qz(ctypes.c_void_p((1 << 21) + 2), 0, one, 8, o, e, 1, None) == -4 and "4-byte aligned" in err()
    assert qz(one, 0, odd, 8, o, e, 1, None) == 0
    assert am(odd, 1, one, 8, o, 1, None) == -4 and "x must be 2-byte aligned" in err()
    assert am(one, 0, ctypes.c_void_p((1 << 21) + 2), 8, o, 1, None) == -4 and "amax_bits must be 4-byte aligned" in err()
    assert dq(one, odd, 0, 8, i64(0, 1), i32(77), 1, None) == -1 and "bag 0:" in err()  # the exponent is refused before the alignment


def test_ops_refuse_bad_arguments_and_name_the_bag():
    from toad_amd import ops
    x, offs = _data()
    codes, exps = ops.bags_quantise_e4m3(x, offs)
    good = dict(codes=codes, offsets=offs, exps=exps)
    for bad, word in ((dict(codes=codes.float()), "codes"), (dict(codes=codes[0]), "codes"), (dict(codes=codes.t()), "codes"),
                      (dict(offsets=[1] + offs[1:]), "start with 0"), (dict(offsets=offs[:-1] + [offs[-1] + 1]), "rows"),
                      (dict(offsets=offs[:2] + [offs[1] - 1] + offs[3:]), "bag 1:"), (dict(offsets=[]), "start with 0"), (dict(offsets=None), "integers"),
                      (dict(exps=exps[:-1]), "exponents"), (dict(exps=exps[:4] + [16] + exps[5:]), "bag 4:"), (dict(exps=exps[:2] + [1.0] + exps[3:]), "bag 2:"),
                      (dict(exps=[True] + exps[1:]), "bag 0:"), (dict(out=torch.empty(codes.shape, dtype=torch.bfloat16)), "out"),
                      (dict(out=torch.empty(codes.shape[0], K + 1, dtype=torch.float16)), "out"), (dict(out_dtype=torch.bfloat16), "out_dtype")):
        with pytest.raises(ValueError, match=word):
            ops.bags_dequantise_e4m3(**{**good, **bad})
    for bad in (x.double(), x[0], x.t(), x.to(torch.bfloat16)):
        with pytest.raises(ValueError, match="x must be"):
            ops.bags_quantise_e4m3(bad, offs, exps)
        with pytest.raises(ValueError, match="x must be"):
            ops.bags_absmax(bad, offs)
    with pytest.raises(ValueError, match="bag 1:"):
        ops.bags_absmax(x, offs[:2] + [offs[1] - 1] + offs[3:])
    with pytest.raises(ValueError, match="bag 5:"):
        ops.bags_quantise_e4m3(x, offs, exps[:5] + [-8] + exps[6:])
    for poison in (math.nan, math.inf, -math.inf):                                       # bag 2 is rows 3 .. 20
        y = x.clone()
        y[7, 3] = poison
        with pytest.raises(ValueError, match="bag 2:"):
            ops.bags_quantise_e4m3(y, offs)
    y = x.clone()
    y[7, 3] = math.nan
    assert (ops.bags_quantise_e4m3(y, offs, exps)[0][7, 3] & 0x7F) == 0x7F               # with the exponents given a NaN becomes a NaN code


def test_cpu_list_ops_equal_the_per_bag_ops_and_the_twin():
    from toad_amd import ops
    for dt in (torch.float32, torch.float16):
        x, offs = _data(seed=3)
        x = x.to(dt)
        bits = ops.bags_absmax(x, offs)
        assert bits.dtype == torch.uint32 and bits.shape == (len(ROWS),)
        want = [int(np.float32(np.abs(x[a:b].numpy().astype(np.float32)).max()).view(np.uint32)) if b > a else 0 for a, b in zip(offs, offs[1:])]
        assert bits.view(torch.int32).tolist() == want
        codes, exps = ops.bags_quantise_e4m3(x, offs)
        assert codes.dtype == torch.uint8 and codes.shape == x.shape and len(exps) == len(ROWS)
        dec16 = ops.bags_dequantise_e4m3(codes, offs, exps)
        dec32 = ops.bags_dequantise_e4m3(codes.view(torch.float8_e4m3fn), offs, exps, out_dtype=torch.float32)
        into = torch.full(x.shape, 7.0, dtype=torch.float16)
        assert ops.bags_dequantise_e4m3(codes, offs, exps, out=into) is into and torch.equal(into.view(torch.int16), dec16.view(torch.int16))
        for i, (a, b) in enumerate(zip(offs, offs[1:])):
            xa = x[a:b].numpy()
            e = R.e4m3_exponent(float(np.abs(xa).max())) if b > a else 0
            assert exps[i] == e, i
            one_codes, one_exp = ops.bag_quantise_e4m3(x[a:b].contiguous())
            assert one_exp == e and torch.equal(codes[a:b], one_codes)
            assert np.array_equal(codes[a:b].numpy(), R.quantise(xa, e))
            assert np.array_equal(dec16[a:b].numpy().view(np.uint16), R.decode_bits(codes[a:b].numpy(), e, np.float16).view(np.uint16))
            assert np.array_equal(dec32[a:b].numpy().view(np.uint32), R.decode_bits(codes[a:b].numpy(), e, np.float32).view(np.uint32))
            assert torch.equal(dec16[a:b].view(torch.int16), ops.bag_dequantise_e4m3(codes[a:b], e).view(torch.int16))
        given = [(-7 + i) for i in range(len(ROWS))]
        codes2, exps2 = ops.bags_quantise_e4m3(x, torch.tensor(offs), given)
        assert exps2 == given
        for i, (a, b) in enumerate(zip(offs, offs[1:])):
            assert np.array_equal(codes2[a:b].numpy(), R.quantise(x[a:b].numpy(), given[i]))
    # specials: -0.0, an Inf bag and a NaN bag
    x = torch.tensor([[-0.0, 0.0], [1.0, -math.inf], [math.nan, 2.0], [-3.0, 2.5]])
    got = [b & 0xFFFFFFFF for b in ops.bags_absmax(x, [0, 1, 2, 3, 3, 4]).view(torch.int32).tolist()]
    assert got[0] == 0 and got[1] == 0x7F800000 and got[2] > 0x7F800000 and got[3] == 0 and got[4] == 0x40400000
    assert ops.bags_absmax(torch.empty(0, 4), [0]).shape == (0,) and ops.bags_quantise_e4m3(torch.empty(0, 4), [0, 0])[1] == [0]


def _shard(rows=ROWS, k=K, seed=5):
    from toad_amd import ingest
    x, offs = _data(rows, k, seed)
    b = len(rows)
    label = torch.arange(b) % 18
    site = torch.arange(b) % 2
    sex = (torch.arange(b) % 2).float()
    return ingest.quantise_shard(x, offs, label, site, sex), x, offs


def test_shard_validation():
    from toad_amd import ingest
    shard, x, offs = _shard()
    assert isinstance(shard, ingest.E4M3Shard) and len(shard) == len(ROWS) and shard.rows == ROWS and shard.offsets == offs
    assert shard.codes.dtype == torch.uint8 and shard.label.dtype == torch.int64 and shard.site.dtype == torch.int64 and shard.sex.dtype == torch.float32
    b2 = shard.bag(2)
    assert isinstance(b2, ingest.E4M3Bag) and b2.exp == shard.exps[2] and torch.equal(b2.codes, shard.codes[3:20])
    recs = shard.records()
    assert len(recs) == len(ROWS) and recs[6][1:] == (6, 0, 0.0) and recs[5][1:] == (5, 1, 1.0) and recs[0][0].shape == (0, K)
    good = dict(codes=shard.codes, rows=shard.rows, exps=shard.exps, label=shard.label, site=shard.site, sex=shard.sex)
    assert ingest.E4M3Shard(**{**good, "codes": shard.codes.view(torch.float8_e4m3fn)}).codes.dtype == torch.uint8
    for bad, word in ((dict(codes=shard.codes.float()), "codes"), (dict(codes=shard.codes[0]), "codes"),
                      (dict(rows=ROWS[:-1] + [1]), "rows"), (dict(rows=ROWS[:1] + [-3] + ROWS[2:]), "bag 1:"), (dict(rows=ROWS[:2] + [17.0] + ROWS[3:]), "bag 2:"),
                      (dict(exps=shard.exps[:-1]), "exponents"), (dict(exps=shard.exps[:3] + [16] + shard.exps[4:]), "bag 3:"),
                      (dict(exps=shard.exps[:3] + [0.5] + shard.exps[4:]), "bag 3:"), (dict(label=shard.label[:-1]), "label"),
                      (dict(site=shard.site.reshape(3, 3)), "site"), (dict(sex=shard.sex[:2]), "sex"), (dict(label=shard.label.float()), "label"),
                      (dict(sex=shard.sex.long()), "sex")):
        with pytest.raises(ValueError, match=word):
            ingest.E4M3Shard(**{**good, **bad})
    # a list of bags gives the same shard as their concatenation; fp16 input; given exponents
    parts = [x[a:b] for a, b in zip(offs, offs[1:])]
    again = ingest.quantise_shard(parts, None, shard.label, shard.site, shard.sex)
    assert torch.equal(again.codes, shard.codes) and again.exps == shard.exps and again.rows == ROWS
    half = ingest.quantise_shard(x.half(), offs, shard.label, shard.site, shard.sex, exps=[0] * len(ROWS))
    assert half.exps == [0] * len(ROWS) and np.array_equal(half.codes.numpy(), R.quantise(x.half().numpy(), 0))
    for bad in (dict(bags=x, offsets=None), dict(bags=parts, offsets=offs), dict(bags=[], offsets=None), dict(bags=[x, x[:, :3]], offsets=None)):
        with pytest.raises(ValueError):
            ingest.quantise_shard(label=shard.label, site=shard.site, sex=shard.sex, **bad)


def test_file_round_trip_with_weights_only_and_malformed_dicts(tmp_path):
    from toad_amd import ingest
    shard, _, _ = _shard()
    path = str(tmp_path / "s.pt")
    assert ingest.save_shard_e4m3(path, shard) is shard
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(d) == ["e4m3_shard", "exp", "label", "rows", "sex", "site"]
    assert d["e4m3_shard"].dtype == torch.float8_e4m3fn and d["rows"].dtype == torch.int64 and d["exp"].dtype == torch.int32
    assert d["label"].dtype == torch.int64 and d["site"].dtype == torch.int64 and d["sex"].dtype == torch.float32
    assert torch.equal(d["e4m3_shard"].view(torch.uint8), shard.codes) and d["rows"].tolist() == ROWS and d["exp"].tolist() == shard.exps
    for src in (path, d, lambda: d, lambda: shard, shard):
        back = ingest._load_shard(src)
        assert torch.equal(back.codes, shard.codes) and back.rows == ROWS and back.exps == shard.exps
        assert torch.equal(back.label, shard.label) and torch.equal(back.site, shard.site) and torch.equal(back.sex, shard.sex)
    for bad in ({k: v for k, v in d.items() if k != "rows"}, {**d, "rows": d["rows"].tolist()}, {**d, "rows": d["rows"].to(torch.int32)},
                {**d, "exp": d["exp"].to(torch.int64)}, {**d, "exp": d["exp"][:-1]}, {**d, "label": [0] * len(ROWS)}, {**d, "sex": d["sex"][:-1]},
                {**d, "e4m3_shard": d["e4m3_shard"].view(torch.uint8)[:-1]}, {**d, "exp": torch.full((len(ROWS),), 16, dtype=torch.int32)},
                {"e4m3": d["e4m3_shard"], "exp": 0}):
        with pytest.raises(ValueError):
            ingest._load_shard(bad)
    with pytest.raises(ValueError):
        ingest._load_shard(lambda: torch.zeros(3, 4))
    with pytest.raises(ValueError):
        ingest.save_shard_e4m3(path, d)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_shard_prefetcher_on_cpu_equals_the_per_record_feed(tmp_path, dtype):
    from toad_amd import ingest
    s0, _, _ = _shard(seed=5)
    s1, _, _ = _shard(rows=[40, 0, 7, 100], k=96, seed=6)
    s2, _, _ = _shard(rows=[1], k=K, seed=7)
    path = str(tmp_path / "s1.pt")
    ingest.save_shard_e4m3(path, s1)
    d2 = {"e4m3_shard": s2.codes.view(torch.float8_e4m3fn), "rows": torch.tensor(s2.rows), "exp": torch.tensor(s2.exps, dtype=torch.int32),
          "label": s2.label, "site": s2.site, "sex": s2.sex}
    pf = ingest.ShardPrefetcher([s0, path, lambda: s0, d2], "cpu", depth=2, dtype=dtype)
    assert len(pf) == 4
    out = list(pf)
    assert len(out) == 4 and all(isinstance(b, ingest.BagBatch) for b in out)
    for batch, shard in zip(out, (s0, s1, s0, s2)):
        assert batch.bags.dtype == dtype and batch.bags.shape == shard.codes.shape and batch.offsets == shard.offsets and len(batch) == len(shard)
        assert torch.equal(batch.label, shard.label) and torch.equal(batch.site, shard.site) and torch.equal(batch.sex, shard.sex)
        assert batch.label.dtype == torch.int64 and batch.sex.dtype == torch.float32
        per_record = list(ingest.BagPrefetcher(shard.records(), "cpu", depth=3, dtype=dtype))
        slides = batch.slides()
        assert len(slides) == len(per_record) == len(shard)
        ib = torch.int16 if dtype == torch.float16 else torch.int32
        for i, ((bag, sex, label, site), (rbag, rlabel, rsite, rsex)) in enumerate(zip(slides, per_record)):      # mind the order of the two tuples
            assert bag.dtype == rbag.dtype == dtype and bag.shape == rbag.shape and torch.equal(bag.view(ib), rbag.view(ib)), i
            assert sex.shape == (1,) and label.shape == (1,) and site.shape == (1,)
            assert torch.equal(sex, rsex) and torch.equal(label, rlabel) and torch.equal(site, rsite)
            if bag.numel():                                                                # a view, not a copy
                assert bag.data_ptr() == batch.bags.data_ptr() + shard.offsets[i] * shard.codes.shape[1] * bag.element_size()
            ref = R.decode_bits(shard.codes[shard.offsets[i]:shard.offsets[i + 1]].numpy(), shard.exps[i], np.float16 if dtype == torch.float16 else np.float32)
            assert np.array_equal(bag.numpy().view(ref.dtype.str.replace("f", "u")), ref.view(ref.dtype.str.replace("f", "u")))
    assert list(ingest.ShardPrefetcher([], "cpu")) == []
    with pytest.raises(ValueError):
        ingest.ShardPrefetcher([s0], "cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        list(ingest.ShardPrefetcher([{"rows": 1}], "cpu"))


def test_bags_to_e4m3_tool_packs_shards(tmp_path):
    from toad_amd import ingest
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir()
    g = torch.Generator().manual_seed(9)
    names = [f"slide_{i:02d}" for i in range(5)]
    lens = [30, 7, 0, 55, 12]
    bags = {}
    for i, (name, n) in enumerate(zip(names, lens)):
        bags[name] = torch.randn(n, 32, generator=g) * (0.5 + i)
        torch.save(bags[name] if i != 1 else bags[name].half(), str(src / f"{name}.pt"))
    meta = tmp_path / "meta.csv"
    meta.write_text("slide_id,label,site,sex\n" + "".join(f"{name},{(3 * i) % 18},{i % 2},{float(i % 2)}\n" for i, name in reversed(list(enumerate(names)))))
    tool = os.path.join(REPO, "tools", "bags_to_e4m3.py")
    run = subprocess.run([sys.executable, tool, str(src), str(dst), "--shard", "2", "--meta", str(meta)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    files = sorted(os.listdir(dst))
    assert files == ["shard_00000.pt", "shard_00001.pt", "shard_00002.pt"], files
    seen = 0
    for f, want in zip(files, (names[:2], names[2:4], names[4:])):
        shard = ingest._load_shard(str(dst / f))
        assert shard.rows == [lens[names.index(n)] for n in want]
        for j, name in enumerate(want):
            i = names.index(name)
            x = bags[name] if i != 1 else bags[name].half()
            exp = R.e4m3_exponent(float(x.abs().max())) if x.numel() else 0
            assert shard.exps[j] == exp and np.array_equal(shard.bag(j).codes.numpy(), R.quantise(x.numpy(), exp))
            assert int(shard.label[j]) == (3 * i) % 18 and int(shard.site[j]) == i % 2 and float(shard.sex[j]) == float(i % 2)
            seen += 1
    assert seen == 5
    # a slide without a row in the CSV, and --shard without --meta, are refused
    meta.write_text("slide_id,label,site,sex\nslide_00,1,0,1.0\n")
    run = subprocess.run([sys.executable, tool, str(src), str(tmp_path / "d2"), "--shard", "2", "--meta", str(meta)], capture_output=True, text=True)
    assert run.returncode != 0 and "slide_01" in run.stderr
    run = subprocess.run([sys.executable, tool, str(src), str(tmp_path / "d3"), "--shard", "2"], capture_output=True, text=True)
    assert run.returncode != 0 and "--meta" in run.stderr
