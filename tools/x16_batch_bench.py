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
  host_fed: 52 x 10,000-patch bags from page-locked host memory through BagPrefetcher(depth=2, arena_rows=524288) into SlideShardedDP.step
      (one optimiser step per 52 slides), fp32 files landing in fp32 buffers against fp16 files landing in fp16 buffers: slides/s, link GB/s.
  launches: four calls of ONE arm (--arm A | B | ONE = the one-slide x16 step) at one shape, for a `rocprofv3 --kernel-trace --stats` run of
      its own: kernel names and counts per call show which weight-gradient and NT kernels the arm ran.

Prints one JSON line per result; --out FILE keeps them.
usage: x16_batch_bench.py [--resident] [--one-slide] [--host-fed] [--launches B,N --arm A|B|ONE] [--seconds S] [--out FILE]"""
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


def host_fed(steps=6, B=52, n=10000, arena_rows=524288):
    from toad_amd.dp import SlideShardedDP
    from toad_amd.ingest import BagPrefetcher
    dev = torch.device("cuda:0")
    res = []
    for wire, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
        if dt is torch.float16 and not HAVE_X16_MULTI:
            continue
        model = make_model()
        dp = SlideShardedDP(model, {"lr": 2e-4, "weight_decay": 1e-5}, batch_rows=arena_rows)
        g = torch.Generator().manual_seed(3)
        host = []
        for i in range(B):                                       # one step's bags in page-locked memory, cycled step after step
            hb = torch.empty((n, 1024), dtype=dt, pin_memory=True)
            hb.copy_((torch.randn(n, 1024, generator=g) * 0.7).to(dt))
            host.append(hb)
        nbytes = B * host[0].numel() * host[0].element_size()
        kw = dict(dtype=dt, arena_rows=arena_rows)
        if dt is torch.float16:
            kw["arena_dtype"] = torch.float16

        def run(k):
            recs = [(host[i % B], i % C, i % 2, float((i // 2) % 2)) for i in range(k * B)]
            batch = []
            for bag, lb, st, sx in BagPrefetcher(recs, dev, depth=2, workers=2, **kw):
                batch.append((bag, sx, lb, st))
                if len(batch) == B:
                    dp.step(batch, B)
                    batch = []
        run(2)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ops.enable_timing(True, level=1)
        run(steps)
        names = {k: v[0] for k, v in ops.collect_timing().items()}
        calls = ops.timing_call_count()
        ops.enable_timing(False)
        dt_s = time.perf_counter() - t0
        res.append(dict(kind="host_fed", lib=select_lib.TAG, wire=wire, landing=str(kw.get("arena_dtype", torch.float32)), slides_per_step=B, patches=n,
                        steps=steps, slides_per_s=round(steps * B / dt_s, 1), ms_per_step=round(dt_s / steps * 1e3, 3),
                        link_gbps=round(steps * nbytes / dt_s / 1e9, 2), library_calls=calls, timed_ops=names))
        del host, dp, model
        ops.release_workspaces()
        torch.cuda.empty_cache()
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
    a = ap.parse_args()
    res = []
    if a.launches:
        B, n = (int(v) for v in a.launches.split(","))
        res += launches(B, n, a.arm)
    else:
        every = not (a.resident or a.one_slide or a.host_fed)
        if a.resident or every:
            res += resident(a.seconds)
        if a.one_slide or every:
            res += one_slide(a.seconds)
        if a.host_fed or every:
            res += host_fed()
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
