"""What an fp16 cohort costs on the ragged multi-slide route: the native x16 calls against the up-cast + concatenation they replace.

  resident (per shape: 52 x 10,000, 10 x 50,000, 8 x 2,000 patches), the two arms ALTERNATED inside one process, device-event timing:
      arm A  what fp16 bags cost before the x16 multi-slide calls existed: `.float()` per bag + torch.cat + toad_mil_multi_step_f32, the
             up-cast and the copy INSIDE the clock (toad_amd/dp.py hip_batch_grad did exactly this);
      arm B  the same fp16 bags, back to back in one buffer, through toad_mil_multi_step_x16_f32 (ops.mil_multi_step: no copy, no up-cast);
      arm F  (context, not a claim) resident fp32 bags back to back through toad_mil_multi_step_f32.
    Arm A is reported as two interleaved halves (A1 = even rounds, A2 = odd rounds): their difference is the spread a difference between arms
    has to exceed to mean anything.
  one_slide: the one-slide x16 step (toad_mil_step_x16_f32) at 10,000 and 100,000 patches. Run the tool once on the shipped library and once with
      TOAD_HIP_LIB=<a library built from the parent's csrc/> (tools/ab/select_lib.py) for the before / after of the one-launch weight gradient.
  host_fed: 52 x 10,000-patch bags (--slides / --patches: another shape, 5 x 100,000 for one) from page-locked host memory through
      BagPrefetcher(depth=2, arena_rows=524288) into SlideShardedDP.step (one optimiser step per 52 slides). Three wires, alternated, three runs each:
      fp32 files landing in fp32 buffers, fp16 files and e4m3 files (8-bit codes, decoded behind each copy) landing in fp16 buffers: slides/s, link
      GB/s. Together with --resident the rows carry the ratio to the resident x16 call of the same shape. A fourth wire, "e4m3 shards": the same codes
      as ONE ingest.E4M3Shard per optimiser step (one copy, one list decode) through ShardPrefetcher(depth=2) into SlideShardedDP.step_batch.
  dequant: the e4m3 decode and quantise kernels alone at 524,288 x 1024 and 10,000 x 1024 (device events, four buffer sets in rotation): us and moved
      bytes/s; and the decode of one step's 520,000 rows as a share of that step's x16 multi-slide call - as one launch over all rows, as 52 per-bag
      launches, and as ONE list launch of 52 bags with an exponent each (ops.bags_dequantise_e4m3).
  launches: four calls of ONE arm (--arm A | B | ONE = the one-slide x16 step) at one shape, for a `rocprofv3 --kernel-trace --stats` run of
      its own: kernel names and counts per call show which weight-gradient and NT kernels the arm ran.

Prints one JSON line per result; --out FILE keeps them.
usage: x16_batch_bench.py [--resident] [--one-slide] [--host-fed] [--slides B --patches N] [--dequant] [--launches B,N --arm A|B|ONE] [--seconds S]
                          [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402

import tools.ab.select_lib as select_lib       # noqa: E402  (TOAD_HIP_LIB=<variant>: this process only)
from toad_amd import _lib                      # noqa: E402

X16_MULTI = ("toad_mil_multi_x16_ok", "toad_mil_multi_step_x16_f32", "toad_mil_multi_fwd_x16_f32", "toad_mil_multi_bwd_x16_f32")
if select_lib.TAG != "(shipped)":              # a variant built from older sources has no x16 multi-slide calls: bind what it has
    import ctypes
    _probe = ctypes.CDLL(_lib.LIB_PATH)
    for _n in X16_MULTI:
        if not hasattr(_probe, _n):
            _lib.SIGNATURES.pop(_n, None)
HAVE_X16_MULTI = all(n in _lib.SIGNATURES for n in X16_MULTI)

from toad_amd import TOAD_fc_mtl_concat, ops   # noqa: E402

C = 18
SHAPES = ((52, 10000), (10, 50000), (8, 2000))


def make_model():
    torch.manual_seed(0)
    m = TOAD_fc_mtl_concat(n_classes=C)
    m.relocate()
    m.train()
    return m


def grad_views(model):
    w = {k: v.detach() for k, v in model._weights().items()}
    return w, {k: torch.zeros_like(w[k]) for k in ops.STEP_SLOTS}


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(arms, seconds, rounds=8):
    """arms: {name: fn}. Warm-up of every arm, then `rounds` rounds of (arm 1, arm 2, ...) with device-event timing; every arm gets at least
    `seconds` of work in all. -> {name: [ms per call, one entry per round]}"""
    per = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per[name] = event_ms(fn, 3)
    iters = {name: max(1, int(seconds * 1e3 / rounds / per[name]) + 1) for name in arms}
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(event_ms(fn, iters[name]))
    return out, iters


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def resident(seconds):
    dev = torch.device("cuda:0")
    model = make_model()
    w, g = grad_views(model)
    res = []
    for B, n in SHAPES:
        pool16 = (torch.randn(B * n, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.7).half()
        bags16 = [pool16[i * n:(i + 1) * n] for i in range(B)]
        pool32 = pool16.float()
        bags32 = [pool32[i * n:(i + 1) * n] for i in range(B)]
        sex = (torch.arange(B, device=dev) % 2).float()
        label = torch.arange(B, device=dev) % C
        site = (torch.arange(B, device=dev) // 2) % 2

        def arm_a():
            up = [b.float() for b in bags16]                    # separate allocations, as the up-cast made them
            ops.mil_multi_step(w, g, 0.0, up, sex, label, site, 0.75 / B, 0.25 / B)      # -> torch.cat inside (not adjacent), then the fp32 call

        def arm_b():
            ops.mil_multi_step(w, g, 0.0, bags16, sex, label, site, 0.75 / B, 0.25 / B)

        def arm_f():
            ops.mil_multi_step(w, g, 0.0, bags32, sex, label, site, 0.75 / B, 0.25 / B)

        arms = {"A_upcast_cat_f32": arm_a, "F_resident_f32": arm_f}
        if HAVE_X16_MULTI:
            arms = {"A_upcast_cat_f32": arm_a, "B_x16": arm_b, "F_resident_f32": arm_f}
        t, iters = alternate(arms, seconds)
        a = t["A_upcast_cat_f32"]
        a1, a2 = median(a[0::2]), median(a[1::2])
        row = dict(kind="resident", lib=select_lib.TAG, slides=B, patches=n, rows=B * n, rounds=len(a), iters_per_round=iters,
                   ms={k: round(median(v), 4) for k, v in t.items()}, ms_min={k: round(min(v), 4) for k, v in t.items()},
                   ms_max={k: round(max(v), 4) for k, v in t.items()},
                   slides_per_s={k: round(B / median(v) * 1e3, 1) for k, v in t.items()},
                   arm_a_halves_ms=[round(a1, 4), round(a2, 4)], arm_a_spread=round(abs(a1 - a2) / median(a), 4))
        if HAVE_X16_MULTI:
            row["b_over_a"] = round(median(t["B_x16"]) / median(a), 4)
            row["b_not_slower_than_a_beyond_spread"] = bool(median(t["B_x16"]) <= median(a) * (1.0 + row["arm_a_spread"]))
        res.append(row)
        del pool16, pool32, bags16, bags32
        ops.release_workspaces()
        torch.cuda.empty_cache()
    return res


def one_slide(seconds):
    dev = torch.device("cuda:0")
    model = make_model()
    w, g = grad_views(model)
    sex, label, site = torch.ones(1, device=dev), torch.tensor([3], device=dev), torch.tensor([1], device=dev)
    res = []
    for n in (10000, 100000):
        x16 = (torch.randn(n, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(n)) * 0.7).half()
        x32 = x16.float()
        t, iters = alternate({"x16": lambda: ops.mil_step(w, g, 0.0, x16, sex, label, site),
                              "f32": lambda: ops.mil_step(w, g, 0.0, x32, sex, label, site)}, seconds)
        res.append(dict(kind="one_slide", lib=select_lib.TAG, patches=n, rounds=len(t["x16"]), iters_per_round=iters,
                        ms={k: round(median(v), 4) for k, v in t.items()}, ms_min={k: round(min(v), 4) for k, v in t.items()},
                        ms_max={k: round(max(v), 4) for k, v in t.items()}))
        del x16, x32
    return res


HAVE_E4M3 = "toad_bag_dequant_e4m3" in _lib.SIGNATURES
HAVE_E4M3_LIST = "toad_bags_dequant_e4m3" in _lib.SIGNATURES


def host_fed(steps=6, B=52, n=10000, arena_rows=524288, rounds=3):
    """Three wires - fp32 files into fp32 landing buffers, fp16 files and e4m3 files (ingest.E4M3Bag: the codes cross the link, the decode runs behind
    each copy) into fp16 ones - ALTERNATED, `rounds` runs of `steps` optimiser steps each. One row per wire with every run's figures, the medians, and
    for the e4m3 wire whether its median slides/s lies above the fp16 wire's maximum. The fourth wire, e4m3_shard, carries the e4m3 wire's codes as one
    ingest.E4M3Shard per step through ShardPrefetcher into step_batch; its row says whether its median lies above the e4m3 wire's maximum."""
    from toad_amd.dp import SlideShardedDP
    from toad_amd.ingest import BagPrefetcher, E4M3Bag, E4M3Shard, ShardPrefetcher
    dev = torch.device("cuda:0")
    arena_rows = max(arena_rows, n)
    g = torch.Generator().manual_seed(3)
    seedbags = [torch.randn(n, 1024, generator=g) * 0.7 for _ in range(min(B, 4))]       # the values do not move the clock: four bags, copied round
    legs = {}
    for wire, dt in (("fp32", torch.float32), ("fp16", torch.float16), ("e4m3", torch.uint8), ("e4m3_shard", torch.uint8)):
        if (wire != "fp32" and not HAVE_X16_MULTI) or (wire.startswith("e4m3") and not HAVE_E4M3) or (wire == "e4m3_shard" and not HAVE_E4M3_LIST):
            continue
        if wire.startswith("e4m3"):
            src = [ops.bag_quantise_e4m3(b) for b in seedbags]
        else:
            src = [(b.to(dt), None) for b in seedbags]
        host = []
        if wire == "e4m3_shard":                                 # one step's bags as ONE record in page-locked memory, cycled step after step
            hb = torch.empty((B * n, 1024), dtype=dt, pin_memory=True)
            for i in range(B):
                hb[i * n:(i + 1) * n].copy_(src[i % len(src)][0])
            host = E4M3Shard(hb, [n] * B, [src[i % len(src)][1] for i in range(B)], torch.arange(B) % C, torch.arange(B) % 2,
                             ((torch.arange(B) // 2) % 2).float())
        for i in range(B if wire != "e4m3_shard" else 0):        # one step's bags in page-locked memory, cycled step after step
            hb = torch.empty((n, 1024), dtype=dt, pin_memory=True)
            hb.copy_(src[i % len(src)][0])
            host.append(E4M3Bag(hb, src[i % len(src)][1]) if wire == "e4m3" else hb)
        land = torch.float32 if wire == "fp32" else torch.float16
        kw = dict(dtype=land, arena_rows=arena_rows, arena_dtype=land)
        dp = SlideShardedDP(make_model(), {"lr": 2e-4, "weight_decay": 1e-5}, batch_rows=arena_rows)
        legs[wire] = dict(host=host, kw=kw, dp=dp, nbytes=B * n * 1024 * torch.empty((), dtype=dt).element_size(), runs=[], timed={}, calls=0)

    def run(leg, k):
        if isinstance(leg["host"], E4M3Shard):
            for batch in ShardPrefetcher([leg["host"]] * k, dev, depth=2, workers=2, dtype=torch.float16):
                leg["dp"].step_batch(batch, B)
            return
        recs = [(leg["host"][i % B], i % C, i % 2, float((i // 2) % 2)) for i in range(k * B)]
        batch = []
        for bag, lb, st, sx in BagPrefetcher(recs, dev, depth=2, workers=2, **leg["kw"]):
            batch.append((bag, sx, lb, st))
            if len(batch) == B:
                leg["dp"].step(batch, B)
                batch = []

    for leg in legs.values():
        run(leg, 2)
    for _ in range(rounds):
        for leg in legs.values():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ops.enable_timing(True, level=1)
            run(leg, steps)
            leg["timed"] = {k: [v[0], round(v[1], 3)] for k, v in ops.collect_timing().items()}        # (collect_timing synchronises)
            leg["calls"] = ops.timing_call_count()
            ops.enable_timing(False)
            leg["runs"].append(time.perf_counter() - t0)
    res = []
    for wire, leg in legs.items():
        sps = [steps * B / s for s in leg["runs"]]
        res.append(dict(kind="host_fed", lib=select_lib.TAG, wire=wire, landing=str(leg["kw"]["arena_dtype"]), slides_per_step=B, patches=n, steps=steps,
                        runs=len(sps), slides_per_s=round(median(sps), 1), slides_per_s_runs=[round(v, 1) for v in sps],
                        ms_per_step=round(median(leg["runs"]) / steps * 1e3, 3), link_gbps=round(steps * leg["nbytes"] / median(leg["runs"]) / 1e9, 2),
                        wire_mb_per_step=round(leg["nbytes"] / 1e6, 1), library_calls=leg["calls"], timed_ops_calls_ms=leg["timed"]))
    by = {r["wire"]: r for r in res}
    if "e4m3" in by and "fp16" in by:
        by["e4m3"]["fp16_max_slides_per_s"] = max(by["fp16"]["slides_per_s_runs"])
        by["e4m3"]["median_above_fp16_max"] = bool(by["e4m3"]["slides_per_s"] > max(by["fp16"]["slides_per_s_runs"]))
    if "e4m3_shard" in by and "e4m3" in by:
        by["e4m3_shard"]["e4m3_max_slides_per_s"] = max(by["e4m3"]["slides_per_s_runs"])
        by["e4m3_shard"]["median_above_e4m3_max"] = bool(by["e4m3_shard"]["slides_per_s"] > max(by["e4m3"]["slides_per_s_runs"]))
    del legs
    ops.release_workspaces()
    torch.cuda.empty_cache()
    return res


def dequant(seconds, step_shape=(52, 10000)):
    """bag_dequantise_e4m3 (fp16 and fp32 output) and bag_quantise_e4m3 (fp32 and fp16 input) alone, device events, four buffer sets in rotation so no
    call finds its operands in a cache the previous call filled; then the decode of one step's rows as a share of that step's x16 multi-slide call."""
    dev = torch.device("cuda:0")
    res = []
    for n in (524288, 10000):
        g = torch.Generator(device=dev).manual_seed(n)
        x32 = [torch.randn(n, 1024, device=dev, generator=g) * 0.7 for _ in range(4)]
        x16 = [x.half() for x in x32]
        codes = [ops.bag_quantise_e4m3(x, 7)[0] for x in x32]
        o16, o32 = [torch.empty_like(x) for x in x16], [torch.empty_like(x) for x in x32]
        turn = [0]

        def rot(fn):
            def call():
                turn[0] = (turn[0] + 1) % 4
                fn(turn[0])
            return call
        arms = {"dequant_f16": (rot(lambda i: ops.bag_dequantise_e4m3(codes[i], 7, out=o16[i])), 3),
                "dequant_f32": (rot(lambda i: ops.bag_dequantise_e4m3(codes[i], 7, out=o32[i])), 5),
                "quant_f32": (rot(lambda i: ops.bag_quantise_e4m3(x32[i], 7)), 5),
                "quant_f16": (rot(lambda i: ops.bag_quantise_e4m3(x16[i], 7)), 3)}
        t, iters = alternate({k: v[0] for k, v in arms.items()}, seconds)
        for k, (_, bytes_per_elem) in arms.items():
            ms = median(t[k])
            res.append(dict(kind="dequant", lib=select_lib.TAG, op=k, rows=n, cols=1024, rounds=len(t[k]), iters_per_round=iters[k], us=round(ms * 1e3, 2),
                            us_min=round(min(t[k]) * 1e3, 2), us_max=round(max(t[k]) * 1e3, 2), bytes_moved=n * 1024 * bytes_per_elem,
                            tb_per_s=round(n * 1024 * bytes_per_elem / (ms * 1e-3) / 1e12, 3)))
        del x32, x16, codes, o16, o32
        torch.cuda.empty_cache()
    if HAVE_X16_MULTI:
        B, n = step_shape
        model = make_model()
        w, gr = grad_views(model)
        pool16 = (torch.randn(B * n, 1024, device=dev) * 0.7).half()
        bags16 = [pool16[i * n:(i + 1) * n] for i in range(B)]
        codes = ops.bag_quantise_e4m3(pool16, 7)[0]
        land = torch.empty_like(pool16)
        offs, exps = [i * n for i in range(B + 1)], [7] * B                # (one exponent so all three arms write the same bytes; the list kernel reads it per bag)
        sex = (torch.arange(B, device=dev) % 2).float()
        label = torch.arange(B, device=dev) % C
        site = (torch.arange(B, device=dev) // 2) % 2
        arms = {"x16_step": lambda: ops.mil_multi_step(w, gr, 0.0, bags16, sex, label, site, 0.75 / B, 0.25 / B),
                "decode_step_rows": lambda: ops.bag_dequantise_e4m3(codes, 7, out=land),
                "decode_per_bag": lambda: [ops.bag_dequantise_e4m3(codes[i * n:(i + 1) * n], 7, out=land[i * n:(i + 1) * n]) for i in range(B)]}
        if HAVE_E4M3_LIST:
            arms["decode_list"] = lambda: ops.bags_dequantise_e4m3(codes, offs, exps, out=land)
        t, iters = alternate(arms, seconds)
        ms = {k: round(median(v), 4) for k, v in t.items()}
        row = dict(kind="dequant_share", lib=select_lib.TAG, slides=B, patches=n, rows=B * n, ms=ms, iters_per_round=iters,
                   decode_share_of_x16_step=round(ms["decode_step_rows"] / ms["x16_step"], 4),
                   decode_per_bag_share_of_x16_step=round(ms["decode_per_bag"] / ms["x16_step"], 4))
        if HAVE_E4M3_LIST:
            one = t["decode_step_rows"]                                    # the single launch's interleaved halves: the spread a difference has to exceed
            h1, h2 = median(one[0::2]), median(one[1::2])
            row.update(ms_runs={k: [round(v, 4) for v in t[k]] for k in ("decode_step_rows", "decode_per_bag", "decode_list")},
                       single_launch_halves_ms=[round(h1, 4), round(h2, 4)], single_launch_spread_ms=round(abs(h1 - h2), 4),
                       list_over_single_launch=round(ms["decode_list"] / ms["decode_step_rows"], 4),
                       list_over_per_bag=round(ms["decode_list"] / ms["decode_per_bag"], 4),
                       list_faster_than_per_bag_beyond_spread=bool(ms["decode_per_bag"] - ms["decode_list"] > abs(h1 - h2)))
        res.append(row)
    return res


def launches(B, n, arm, calls=4):
    """`calls` calls of one arm at one shape, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    model = make_model()
    w, g = grad_views(model)
    pool16 = (torch.randn(B * n, 1024, device=dev) * 0.7).half()
    bags16 = [pool16[i * n:(i + 1) * n] for i in range(B)]
    sex = (torch.arange(B, device=dev) % 2).float()
    label = torch.arange(B, device=dev) % C
    site = (torch.arange(B, device=dev) // 2) % 2
    for _ in range(calls):
        if arm == "A":
            ops.mil_multi_step(w, g, 0.0, [b.float() for b in bags16], sex, label, site, 0.75 / B, 0.25 / B)
        elif arm == "B":
            ops.mil_multi_step(w, g, 0.0, bags16, sex, label, site, 0.75 / B, 0.25 / B)
        else:
            ops.mil_step(w, g, 0.0, bags16[0], sex[:1], label[:1], site[:1])
    torch.cuda.synchronize()
    what = {"A": "upcast + cat + toad_mil_multi_step_f32", "B": "toad_mil_multi_step_x16_f32", "ONE": f"toad_mil_step_x16_f32 at {n} patches"}[arm]
    return [dict(kind="launches", lib=select_lib.TAG, slides=B, patches=n, calls=calls, arm=arm, what=what)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--one-slide", action="store_true")
    ap.add_argument("--host-fed", action="store_true")
    ap.add_argument("--launches", default="")
    ap.add_argument("--arm", default="B", choices=("A", "B", "ONE"))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--dequant", action="store_true", help="time the e4m3 decode and quantise kernels alone")
    ap.add_argument("--slides", type=int, default=0, help="with --patches: the one shape of --resident and --host-fed (default: 52 x 10,000 host-fed)")
    ap.add_argument("--patches", type=int, default=0)
    a = ap.parse_args()
    if bool(a.slides) != bool(a.patches) or a.slides < 0 or a.patches < 0:
        ap.error("--slides and --patches go together")
    global SHAPES
    if a.slides:
        SHAPES = ((a.slides, a.patches),)
    res = []
    if a.launches:
        B, n = (int(v) for v in a.launches.split(","))
        res += launches(B, n, a.arm)
    elif a.dequant:
        res += dequant(a.seconds)
    else:
        every = not (a.resident or a.one_slide or a.host_fed)
        if a.resident or every:
            res += resident(a.seconds)
        if a.one_slide or every:
            res += one_slide(a.seconds)
        if a.host_fed or every:
            fed = host_fed(B=a.slides, n=a.patches) if a.slides else host_fed()
            x16 = [r["slides_per_s"].get("B_x16") for r in res if r["kind"] == "resident" and (r["slides"], r["patches"]) == (fed[0]["slides_per_step"], fed[0]["patches"])]
            for r in fed:                                        # the resident x16 call of the same shape in this process, where it was run
                if x16 and x16[0]:
                    r["resident_x16_slides_per_s"] = x16[0]
                    r["share_of_resident_x16"] = round(r["slides_per_s"] / x16[0], 4)
            res += fed
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
