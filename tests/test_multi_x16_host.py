"""CPU: fp16 bags on the ragged multi-slide route (toad_mil_multi_{step,fwd,bwd}_x16_f32, an additive extension of ABI 15). The entry points
exist in the header, the library and the ctypes table and validate like their *_f32 twins before any device access; ops._adjacent_rows joins
fp16 row ranges of one allocation; BagPrefetcher lands fp16 files in fp16 buffers; and the bit-image contract of the fp16 multi route
 holds over the row sweep of tests/test_relu_bits_plan.py without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

X16_SYMBOLS = ("toad_mil_multi_x16_ok", "toad_mil_multi_step_x16_f32", "toad_mil_multi_fwd_x16_f32", "toad_mil_multi_bwd_x16_f32")


def _lib():
    from toad_amd import _lib as L
    return L.load()


def test_x16_multi_symbols_are_declared_exported_and_bound():
    import os
    import re
    from toad_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toad_hip.h")).read()
    assert lib.toad_abi_version() == 15 and L.ABI_VERSION == 15 and re.search(r"#define\s+TOAD_ABI_VERSION\s+15\b", header)
    for name in X16_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/toad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is missing from the ctypes table"
    for twin in ("step", "fwd", "bwd"):                       # same argument lists as the fp32 calls
        assert L.SIGNATURES[f"toad_mil_multi_{twin}_x16_f32"] == L.SIGNATURES[f"toad_mil_multi_{twin}_f32"]


def test_multi_x16_ok_at_its_documented_bounds():
    """64 <= sum N_b <= 1,047,552: the one-slide rule (toad_mil_x16_ok) applied to the concatenation, up to the rows of one launch."""
    lib = _lib()
    for n, ok in ((-1, 0), (0, 0), (1, 0), (63, 0), (64, 1), (10000, 1), (524288, 1), (4092 * 256, 1), (4092 * 256 + 1, 0), ((1 << 20) - 1, 0),
                  (1 << 20, 0), (1 << 21, 0)):
        assert lib.toad_mil_multi_x16_ok(n) == ok, n
        if n <= 4092 * 256:
            assert lib.toad_mil_multi_x16_ok(n) == lib.toad_mil_x16_ok(n), n


def test_x16_multi_calls_report_argument_errors_like_their_f32_twins_without_a_gpu():
    lib = _lib()
    err = lambda: lib.toad_last_error().decode()              # noqa: E731
    one = ctypes.c_void_p(1 << 21)                            # non-null, aligned fake pointers: every check below comes before a device access
    odd = ctypes.c_void_p((1 << 21) + 4)
    big = 1 << 40
    p12 = (ctypes.c_void_p * 12)(*([1 << 21] * 12))
    g12 = (ctypes.c_void_p * 12)(*([1 << 21] * 12))
    offs = (ctypes.c_int64 * 4)(0, 100, 300, 301)
    bad0 = (ctypes.c_int64 * 4)(1, 100, 300, 301)
    empty = (ctypes.c_int64 * 4)(0, 100, 100, 301)
    tiny = (ctypes.c_int64 * 3)(0, 20, 63)                    # 63 rows in all: below what the fp16 kernels take

    def calls(sfx):
        step = lambda pr=p12, gr=g12, x=one, o=offs, b=3, ws=big, drop=0.0: getattr(lib, "toad_mil_multi_step" + sfx)(            # noqa: E731
            pr, gr, 0.0, x, o, b, one, one, one, 0.75, 0.25, 18, 384, drop, 0, one, None, None, one, ws, None, None)
        fwd = lambda pr=p12, x=one, o=offs, b=3, ab=big, sb=big, drop=0.0: getattr(lib, "toad_mil_multi_fwd" + sfx)(             # noqa: E731
            pr, x, o, b, one, 18, 384, drop, 0, one, ab, one, sb, None)
        bwd = lambda gr=g12, x=one, o=offs, b=3, ab=big, sb=big, dl=one: getattr(lib, "toad_mil_multi_bwd" + sfx)(               # noqa: E731
            p12, gr, 0.0, x, o, b, 18, 384, 0.0, 0, one, ab, dl, one, None, None, one, sb, None)
        return step, fwd, bwd

    seen = {}
    for sfx in ("_f32", "_x16_f32"):
        step, fwd, bwd = calls(sfx)
        name = "toad_mil_multi_%s" + sfx
        cases = [
            ("step null params", lambda: step(pr=None), -1, "null pointer"),
            ("step null bags", lambda: step(x=None), -1, "null pointer"),
            ("step null offsets", lambda: step(o=None), -1, "null pointer"),
            ("step B = 0", lambda: step(b=0), -1, "B must be in [1, 4096]"),
            ("step B = 4097", lambda: step(b=4097), -1, "B must be in [1, 4096]"),
            ("step offsets[0]", lambda: step(o=bad0), -1, "offsets[0] must be 0"),
            ("step empty slide", lambda: step(o=empty), -1, "slide 1 is empty"),
            ("step drop_p", lambda: step(drop=1.0), -1, "drop_p"),
            ("step unaligned", lambda: step(x=odd), -4, "16-byte aligned"),
            ("step workspace", lambda: step(ws=16), -3, "workspace too small"),
            ("fwd null params", lambda: fwd(pr=None), -1, "null pointer"),
            ("fwd null bags", lambda: fwd(x=None), -1, "null pointer"),
            ("fwd B = 0", lambda: fwd(b=0), -1, "B must be in [1, 4096]"),
            ("fwd offsets[0]", lambda: fwd(o=bad0), -1, "offsets[0] must be 0"),
            ("fwd empty slide", lambda: fwd(o=empty), -1, "slide 1 is empty"),
            ("fwd 2^20 rows", lambda: fwd(o=(ctypes.c_int64 * 2)(0, 1 << 20), b=1), -2, "unsupported shape"),
            ("fwd unaligned", lambda: fwd(x=odd), -4, "16-byte aligned"),
            ("fwd arena", lambda: fwd(ab=16), -3, "arena too small"),
            ("fwd scratch", lambda: fwd(sb=16), -3, "scratch too small"),
            ("bwd null dlogits", lambda: bwd(dl=None), -1, "null pointer"),
            ("bwd null bags", lambda: bwd(x=None), -1, "null pointer"),
            ("bwd B = 0", lambda: bwd(b=0), -1, "B must be in [1, 4096]"),
            ("bwd empty slide", lambda: bwd(o=empty), -1, "slide 1 is empty"),
            ("bwd unaligned", lambda: bwd(x=odd), -4, "16-byte aligned"),
            ("bwd arena", lambda: bwd(ab=16), -3, "arena too small"),
            ("bwd scratch", lambda: bwd(sb=16), -3, "scratch too small"),
        ]
        for what, call, rc, text in cases:
            got = call()
            msg = err()
            assert got == rc and text in msg, (sfx, what, got, msg)
            assert msg.startswith(name % what.split()[0] + ":"), (sfx, what, msg)
            seen.setdefault(what, []).append(msg.split(":", 1)[1])
    for what, msgs in seen.items():                           # the twin's message, word for word
        assert msgs[0] == msgs[1], (what, msgs)
    # what only the fp16 calls refuse: a total below 64 rows (callers up-cast such batches)
    step, fwd, bwd = calls("_x16_f32")
    for call in (lambda: step(o=tiny, b=2), lambda: fwd(o=tiny, b=2), lambda: bwd(o=tiny, b=2)):
        assert call() == -2 and "toad_mil_multi_x16_ok" in err()
    step, fwd, bwd = calls("_f32")
    assert fwd(o=tiny, b=2, ab=16) == -3                      # (the fp32 call takes the shape and goes on to its buffers)


def test_loader_names_a_missing_symbol_and_says_rebuild(monkeypatch):
    """An older library reports the same ABI version (the x16 multi calls are additive): the loader must say what is missing, not AttributeError."""
    from toad_amd import _lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setitem(L.SIGNATURES, "toad_symbol_of_a_newer_header", (ctypes.c_int, []))
    with pytest.raises(RuntimeError, match=r"toad_symbol_of_a_newer_header.*rebuild"):
        L.load()
    monkeypatch.delitem(L.SIGNATURES, "toad_symbol_of_a_newer_header")
    assert L.load().toad_abi_version() == 15


def test_adjacent_fp16_rows_are_their_own_concatenation():
    from toad_amd import ops
    buf = torch.randn(1000, 1024).half()
    a, b, c = buf[0:300], buf[300:500], buf[500:900]
    cat = ops._adjacent_rows([a, b, c])
    assert cat is not None and cat.dtype == torch.float16 and cat.shape == (900, 1024) and cat.data_ptr() == buf.data_ptr()
    assert torch.equal(cat, buf[:900])
    mid = ops._adjacent_rows([b, c])
    assert mid is not None and mid.data_ptr() == buf.data_ptr() + 300 * 1024 * 2 and torch.equal(mid, buf[300:900])
    assert ops._adjacent_rows([a, c]) is None                                  # a gap
    assert ops._adjacent_rows([b, a]) is None                                  # wrong order
    assert ops._adjacent_rows([a, buf[300:500].clone()]) is None               # another allocation
    both = torch.empty(600 * 1024 * 4, dtype=torch.uint8)                      # one allocation, fp16 rows followed at the right address by fp32 rows
    h = both[:200 * 1024 * 2].view(torch.float16).view(200, 1024)
    f = both[200 * 1024 * 2:200 * 1024 * 2 + 100 * 1024 * 4].view(torch.float32).view(100, 1024)
    assert f.data_ptr() == h.data_ptr() + h.numel() * 2
    assert ops._adjacent_rows([h, f]) is None and ops._adjacent_rows([f, h]) is None     # mixed dtypes are never adjacent
    x32 = buf.float()
    assert ops._adjacent_rows([x32[0:300], x32[300:500]]).data_ptr() == x32.data_ptr()   # fp32 as before


def test_concat_bags_keeps_an_all_fp16_list_and_up_casts_the_rest():
    from toad_amd import ops
    buf = torch.randn(400, 1024).half()
    x, off = ops._concat_bags([buf[0:100], buf[100:400]])
    assert x.dtype == torch.float16 and x.data_ptr() == buf.data_ptr() and off == [0, 100, 400]
    x, off = ops._concat_bags([buf[0:100], buf[100:400].clone()])                        # apart: one fp16 copy, still no up-cast
    assert x.dtype == torch.float16 and torch.equal(x, buf)
    x, _ = ops._concat_bags([buf[0:100], buf[100:400].float()])                          # mixed: fp32
    assert x.dtype == torch.float32 and torch.equal(x, buf.float())
    x, _ = ops._concat_bags([buf[0:100].bfloat16(), buf[100:400].bfloat16()])
    assert x.dtype == torch.float32
    x, _ = ops._concat_bags([buf[0:20], buf[20:63]])                                     # 63 rows: toad_mil_multi_x16_ok refuses, up-cast silently
    assert x.dtype == torch.float32 and torch.equal(x, buf[:63].float())
    x, off = ops._concat_bags(buf[:63], [0, 20, 63])
    assert x.dtype == torch.float32 and off == [0, 20, 63]
    x, _ = ops._concat_bags(buf, [0, 100, 400])
    assert x is buf


def test_fp16_landing_arenas_keep_fp16_files_as_they_are_cpu():
    """BagPrefetcher(dtype=torch.float16, arena_rows=R, arena_dtype=torch.float16): the lengths of the fp32 landing test
    (tests/test_ingest.py); values are the files', dtype fp16, the same buffer sharing, and the first four are their own concatenation."""
    from toad_amd import ops
    from toad_amd.ingest import BagPrefetcher
    lens = [300, 200, 400, 100, 1500, 64, 700]
    g = torch.Generator().manual_seed(5)
    bags = [torch.randn(n, 1024, generator=g).half() for n in lens]
    recs = [(b, i % 18, i % 2, float(i % 2)) for i, b in enumerate(bags)]
    out = list(BagPrefetcher(recs, "cpu", depth=3, workers=2, dtype=torch.float16, arena_rows=1000, arena_dtype=torch.float16))
    assert len(out) == len(lens)
    for i, (bag, label, site, sex) in enumerate(out):
        assert bag.dtype == torch.float16 and torch.equal(bag, bags[i]) and int(label) == i % 18 and int(site) == i % 2
    store = [o[0].untyped_storage().data_ptr() for o in out]
    assert store[0] == store[1] == store[2] == store[3] and store[4] not in (store[0], store[5]) and store[5] == store[6] != store[0]
    cat = ops._adjacent_rows([o[0] for o in out[:4]])
    assert cat is not None and cat.dtype == torch.float16 and cat.shape == (1000, 1024) and cat.data_ptr() == out[0][0].data_ptr()
    assert torch.equal(cat, torch.cat(bags[:4], 0))
    assert out[0][0].untyped_storage().nbytes() == 1000 * 1024 * 2            # half the landing buffer of the fp32 route
    assert ops._adjacent_rows([out[2][0], out[4][0]]) is None
    with pytest.raises(ValueError):                                            # the old refusal stands without the new keyword
        BagPrefetcher(recs, "cpu", dtype=torch.float16, arena_rows=1000)
    with pytest.raises(ValueError):                                            # fp16 buffers hand out fp16 bags: dtype must say so
        BagPrefetcher(recs, "cpu", arena_rows=1000, arena_dtype=torch.float16)
    with pytest.raises(ValueError):
        BagPrefetcher(recs, "cpu", dtype=torch.bfloat16, arena_rows=1000, arena_dtype=torch.bfloat16)
    # an fp32 file asked to land in fp16 buffers is down-cast: the caller's choice
    f32 = torch.randn(50, 1024, generator=g)
    (bag, _, _, _), = list(BagPrefetcher([(f32, 0, 0, 0.0)], "cpu", dtype=torch.float16, arena_rows=1000, arena_dtype=torch.float16))
    assert bag.dtype == torch.float16 and torch.equal(bag, f32.half())


def _sweep_ms(limit):
    """tests/test_relu_bits_plan.py::_sweep_ms up to `limit` rows: each tile's first row, its 128th and 129th, its last."""
    for t in range(1, 4201):
        r0 = (t - 1) * 256
        for m in (r0 + 1, r0 + 128, r0 + 129, r0 + 256):
            if m <= limit:
                yield m


def test_bit_image_contract_of_the_fp16_multi_route():
    """The fp16 multi-slide route has its own layer-1 rule (csrc/step.hip multi_forward_body / multi_backward_body): the A16 forward takes
    half-height tiles wherever the fp32 forward does, and the dgrad is ALWAYS handed the image - toad_relu_bits_plan describes it with
    TOAD_BITS_STEP_L1 | TOAD_BITS_MULTI | TOAD_BITS_A16. Over every total the route takes: the tiles the dgrad reads are tiles the forward
    wrote, and both maps are those of the fp32 multi-slide route (the same tile plan is what makes the two routes sum in the same order).
    At 10,000 rows the dgrad runs on half-height tiles and reads EVERY tile: the forward must have written every tile there (map all 2) -
    the one-slide x16 calls, whose A16 forward keeps 256-row tiles, leave tiles unwritten at that size and give their dgrad no image."""
    lib = _lib()
    A16, READER, SELF_MEASURE, STEP_L1, MULTI, APT, ROWS = 16, 1, 64, 256, 512, 32, 128
    limit = 4092 * 256                                         # the most rows toad_mil_multi_x16_ok takes
    assert lib.toad_mil_multi_x16_ok(limit) == 1 and lib.toad_mil_multi_x16_ok(limit + 1) == 0
    cap = 4200 * 2
    wbuf, rbuf, w32, r32 = (np.empty(cap, np.uint8) for _ in range(4))
    checked = halves = read_some = 0
    for m in _sweep_ms(limit):
        nt = ((m + 255) // 256) * 2
        rcw = lib.toad_relu_bits_plan(m, 512, 1024, STEP_L1 | MULTI | A16, wbuf.ctypes.data)
        rcr = lib.toad_relu_bits_plan(m, 512, 512, STEP_L1 | MULTI | A16 | READER, rbuf.ctypes.data)
        if not lib.toad_mil_multi_x16_ok(m):
            assert rcw == -2 and rcr == -2, m                  # below 64 rows: not a total of the fp16 route (callers up-cast)
            continue
        assert rcw == 0 and rcr == 0, m
        w, r = wbuf[:nt], rbuf[:nt]
        bad = (r != 0) & (w == 0)
        assert not bad.any(), f"sum N_b = {m}: the layer-1 dgrad reads tiles {np.nonzero(bad)[0][:8]} the fp16 forward left unwritten"
        assert lib.toad_relu_bits_plan(m, 512, 1024, STEP_L1 | MULTI | SELF_MEASURE, w32.ctypes.data) == 0
        assert lib.toad_relu_bits_plan(m, 512, 512, STEP_L1 | MULTI | READER, r32.ctypes.data) == 0
        assert np.array_equal(w, w32[:nt]) and np.array_equal(r, r32[:nt]), m      # the fp32 multi-slide route's plan
        checked += 1
        halves += bool((w == 2).any())
        read_some += bool(r.any())
        if (r == 2).any():
            assert (w == 2).all() and (r == 2).all(), m       # half-height dgrad: every tile read, so every tile written
    assert checked > 16000 and halves > 100 and read_some > 1000
    # 10,000 rows: half-height tiles on both sides of the multi route ...
    assert lib.toad_relu_bits_plan(10000, 512, 1024, STEP_L1 | MULTI | A16, wbuf.ctypes.data) == 0 and (wbuf[:80] == 2).all()
    assert lib.toad_relu_bits_plan(10000, 512, 512, STEP_L1 | MULTI | A16 | READER, rbuf.ctypes.data) == 0 and (rbuf[:80] == 2).all()
    # ... while the one-slide x16 calls leave tiles unwritten there and hand their dgrad the fp32 activations (unchanged)
    assert lib.toad_relu_bits_plan(10000, 512, 1024, STEP_L1 | A16, wbuf.ctypes.data) == 0 and (wbuf[:80] <= 1).all() and not wbuf[:80].all()
    assert lib.toad_relu_bits_plan(10000, 512, 512, STEP_L1 | A16 | READER, rbuf.ctypes.data) == 0 and not rbuf[:80].any()
    # what the flag goes with
    for fl in (MULTI, MULTI | A16, STEP_L1 | MULTI | APT, STEP_L1 | MULTI | ROWS):
        assert lib.toad_relu_bits_plan(10000, 512, 1024, fl, wbuf.ctypes.data) == -1, fl
    assert lib.toad_relu_bits_plan(limit + 1, 512, 1024, STEP_L1 | MULTI | A16, wbuf.ctypes.data) == -2
    assert lib.toad_relu_bits_plan(10000, 512, 1024, 1 << 12, wbuf.ctypes.data) == -1           # (still an unknown flag)
