"""What uint8 tiles cost on their way into the extractor: ResNet_Baseline.forward_u8 against the fp32 route and against the torch glue it replaces.

  resident: 512 tiles of 256 x 256 per call (bench_extract.py's chunk, `--config 5`), the arms ALTERNATED inside one process, device-event timing:
      arm A  forward on resident normalised fp32 NCHW tiles (what bench_extract.py measures);
      arm B  forward_u8 on resident uint8 NHWC tiles (the stem reads the bytes; no fp32 image);
      arm B16  arm B with out_dtype=torch.float16 (the bag rows stored as halves by the average pool);
      arm C  what uint8 tiles cost before forward_u8 existed: permute + float + sub + div in torch, then forward - all inside the clock.
    The tiles of arms A and C are the SAME pixels as arm B's (arm A's tensor is the normalised image of arm B's bytes). Arm A is reported as two
    interleaved halves (A1 = even rounds, A2 = odd rounds): their difference is the noise floor a difference between arms has to exceed.
  host_fed: the same 512-tile calls fed from page-locked host memory, the copies on a side stream into two device buffers (double-buffered) while the
      previous call computes:  arm D  fp32 NCHW tiles (786,432 B each) into forward;  arm E  uint8 tiles (196,608 B each) into forward_u8.
      tiles/s and link GB/s over `--calls` calls.
  launches: four calls of ONE arm (--arm A | B) for a `rocprofv3 --kernel-trace --stats` run of its own: the two stem instantiations' times.

Prints one JSON line per result; --out FILE keeps them.
usage: extract_u8_bench.py [--resident] [--host-fed] [--launches --arm A|B] [--tiles N] [--seconds S] [--calls K] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402

from toad_amd import ops                       # noqa: E402
from toad_amd.resnet_custom import IMAGENET_MEAN, IMAGENET_STD, resnet50_baseline      # noqa: E402


def make_model():
    torch.manual_seed(0)
    return resnet50_baseline().relocate().eval()               # random init, as bench_extract.py


def make_tiles(n, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    return torch.randint(0, 256, (n, 256, 256, 3), device=dev, dtype=torch.uint8, generator=g)


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(arms, seconds, rounds=8):
    """Warm-up of every arm, then `rounds` rounds of (arm 1, arm 2, ...) with device-event timing -> {name: [ms per call, one entry per round]}"""
    per = {}
    for name, fn in arms.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        per[name] = event_ms(fn, 2)
    iters = {name: max(1, int(seconds * 1e3 / rounds / per[name]) + 1) for name in arms}
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(event_ms(fn, iters[name]))
    return out, iters


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def resident(n, seconds):
    dev = torch.device("cuda:0")
    model = make_model()
    u8 = make_tiles(n, dev)
    f32 = ops.tiles_u8_to_f32(u8)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1) * 255.0
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1) * 255.0

    def arm_c():
        x = u8.permute(0, 3, 1, 2).float()
        x = x.sub_(mean).div_(std)
        return model(x.contiguous())

    same = bool(torch.equal(model.forward_u8(u8), model(f32)))
    same16 = bool(torch.equal(model.forward_u8(u8, out_dtype=torch.float16), model(f32).half()))
    arms = {"A_f32_resident": lambda: model(f32), "B_u8": lambda: model.forward_u8(u8),
            "B16_u8_fp16_rows": lambda: model.forward_u8(u8, out_dtype=torch.float16), "C_torch_glue_f32": arm_c}
    t, iters = alternate(arms, seconds)
    a = t["A_f32_resident"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    spread = abs(a1 - a2) / median(a)
    b = median(t["B_u8"])
    return [dict(kind="resident", tiles=n, tile="256x256", rounds=len(a), iters_per_round=iters,
                 ms={k: round(median(v), 4) for k, v in t.items()}, ms_min={k: round(min(v), 4) for k, v in t.items()},
                 ms_max={k: round(max(v), 4) for k, v in t.items()}, tiles_per_s={k: round(n / median(v) * 1e3, 1) for k, v in t.items()},
                 arm_a_halves_ms=[round(a1, 4), round(a2, 4)], arm_a_spread=round(spread, 4), b_over_a=round(b / median(a), 4),
                 c_over_a=round(median(t["C_torch_glue_f32"]) / median(a), 4), b_slower_than_a_beyond_spread=bool(b > median(a) * (1.0 + spread)),
                 u8_bitwise_f32=same, u8_fp16_bitwise_f32_half=same16)]


def host_fed(n, calls):
    dev = torch.device("cuda:0")
    model = make_model()
    u8 = make_tiles(n, dev)
    res = []
    for arm, src in (("D_f32_host", ops.tiles_u8_to_f32(u8).cpu()), ("E_u8_host", u8.cpu())):
        host = [torch.empty(src.shape, dtype=src.dtype, pin_memory=True) for _ in range(2)]
        for h in host:
            h.copy_(src)
        devb = [torch.empty(src.shape, dtype=src.dtype, device=dev) for _ in range(2)]
        fwd = model.forward if src.dtype == torch.float32 else model.forward_u8
        side = torch.cuda.Stream()
        main = torch.cuda.current_stream()

        def run(k):
            landed = [torch.cuda.Event(), torch.cuda.Event()]
            used = [torch.cuda.Event(), torch.cuda.Event()]
            for e in used:
                e.record(main)
            with torch.cuda.stream(side):
                devb[0].copy_(host[0], non_blocking=True)
                landed[0].record(side)
            for i in range(k):
                cur, nxt = i % 2, (i + 1) % 2
                if i + 1 < k:
                    with torch.cuda.stream(side):
                        side.wait_event(used[nxt])              # the call that read this buffer is done
                        devb[nxt].copy_(host[nxt], non_blocking=True)
                        landed[nxt].record(side)
                main.wait_event(landed[cur])
                fwd(devb[cur])
                used[cur].record(main)
            torch.cuda.synchronize()
        run(3)
        t0 = time.perf_counter()
        run(calls)
        dt = time.perf_counter() - t0
        nbytes = src.numel() * src.element_size()
        res.append(dict(kind="host_fed", arm=arm, tiles_per_call=n, calls=calls, bytes_per_tile=nbytes // n, tiles_per_s=round(calls * n / dt, 1),
                        ms_per_call=round(dt / calls * 1e3, 3), link_gbps=round(calls * nbytes / dt / 1e9, 2)))
        del host, devb
        torch.cuda.empty_cache()
    return res


def launches(n, arm, calls=4):
    """`calls` calls of one arm, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    model = make_model()
    u8 = make_tiles(n, dev)
    x = ops.tiles_u8_to_f32(u8) if arm == "A" else u8
    for _ in range(calls):
        (model if arm == "A" else model.forward_u8)(x)
    torch.cuda.synchronize()
    return [dict(kind="launches", tiles=n, calls=calls, arm=arm, what="forward (fp32 NCHW)" if arm == "A" else "forward_u8 (uint8 NHWC)")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--host-fed", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--arm", default="B", choices=("A", "B"))
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    if a.launches:
        res += launches(a.tiles, a.arm)
    else:
        every = not (a.resident or a.host_fed)
        if a.resident or every:
            res += resident(a.tiles, a.seconds)
        if a.host_fed or every:
            res += host_fed(a.tiles, a.calls)
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
