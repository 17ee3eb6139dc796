"""What reading tiles by origin costs: ResNet_Baseline.forward_u8_region against forward_u8 on the same tiles cut out beforehand. A sibling of
extract_u8_bench.py (its event timing, its alternation of the arms inside one process and its two interleaved halves of arm A as the noise figure).

  resident: 512 tiles of 256 x 256 per call, everything on the device before the clock starts:
      arm A  forward_u8 on the materialised tiles [512,256,256,3] (the existing route), reported as two interleaved halves A1 / A2;
      arm B  forward_u8_region on the region those tiles were cut from: a 16 x 32 grid of non-overlapping tiles, 4096 x 8192 pixels (the same bytes);
      arm C  forward_u8_region at stride 64: a 16 x 32 grid of overlapping tiles from a 1216 x 2240 region (the heat-map case; other pixels than A and B).
    The origins are a CPU tensor, checked and copied to the device inside the clock on every call of arms B and C.
  host_fed: 512 tiles per step from a region in page-locked host memory, the steps run one after another (nothing overlapped), wall-clock:
      arm D1  the host cuts the tiles with numpy into a page-locked [512,256,256,3] buffer, one H2D copy of it, forward_u8;
      arm D2  one H2D copy of the region, forward_u8_region.
    Per arm: tiles/s, link GB/s over the whole step, and the host seconds per step spent before the copy is issued (the cutting; for D2 nothing).
    --stride 64 runs the same pair on the overlapping grid, where the tiles are 12 times the region.
  launches: four calls of ONE resident arm (--arm A | B | C) for a `rocprofv3 --kernel-trace --stats` run of its own: the stem instantiations' times.

  --regions: the slide cut into 4 strips / 16 blocks, one forward_u8_region call per window against ONE forward_u8_regions call over all of them, and both
    against the whole region; see regions(). Appends to profiles/extract_regions_bench.jsonl unless --out names another file.

  --shrink 2: 512 footprints of 512 x 512 read box-filtered to 256 x 256 (forward_u8_region(shrink=2)) against today's 256-pixel call and against torch
    glue in front of forward_u8; see shrunk().

Prints one JSON line per result; --out FILE keeps them.
usage: extract_region_bench.py [--resident] [--host-fed] [--launches --arm A|B|C] [--shrink 2] [--regions] [--stride S] [--seconds S] [--steps K] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                   # noqa: E402

from extract_u8_bench import alternate, make_model, median      # noqa: E402

GRID = (16, 32)                                # 512 tiles
TILE = 256


def grid_region(stride, dev):
    """(region [Hr,Wr,3] of random bytes, origins [512,2] (x, y) as a CPU tensor) of the 16 x 32 grid at `stride` pixels."""
    gy, gx = GRID
    hr, wr = (gy - 1) * stride + TILE, (gx - 1) * stride + TILE
    g = torch.Generator(device=dev).manual_seed(1)
    region = torch.randint(0, 256, (hr, wr, 3), device=dev, dtype=torch.uint8, generator=g)
    origins = torch.tensor([(x * stride, y * stride) for y in range(gy) for x in range(gx)], dtype=torch.int32)
    return region, origins


def cut(region, origins):
    return torch.stack([region[y:y + TILE, x:x + TILE] for x, y in origins.tolist()])


def resident(seconds):
    dev = torch.device("cuda:0")
    model = make_model()
    region, origins = grid_region(TILE, dev)
    tiles = cut(region, origins)
    region64, origins64 = grid_region(64, dev)
    same = bool(torch.equal(model.forward_u8_region(region, origins), model.forward_u8(tiles)))
    same64 = bool(torch.equal(model.forward_u8_region(region64, origins64, out_dtype=torch.float16),
                              model.forward_u8(cut(region64, origins64), out_dtype=torch.float16)))
    arms = {"A_u8_tiles": lambda: model.forward_u8(tiles), "B_region_grid": lambda: model.forward_u8_region(region, origins),
            "C_region_stride64": lambda: model.forward_u8_region(region64, origins64)}
    t, iters = alternate(arms, seconds)
    a = t["A_u8_tiles"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    n = origins.shape[0]
    return [dict(kind="resident_region", tiles=n, tile="256x256", region=list(region.shape[:2]), region_stride64=list(region64.shape[:2]), rounds=len(a),
                 iters_per_round=iters, ms={k: round(median(v), 4) for k, v in t.items()}, ms_min={k: round(min(v), 4) for k, v in t.items()},
                 ms_max={k: round(max(v), 4) for k, v in t.items()}, tiles_per_s={k: round(n / median(v) * 1e3, 1) for k, v in t.items()},
                 arm_a_halves_ms=[round(a1, 4), round(a2, 4)], arm_a_spread=round(abs(a1 - a2) / median(a), 4),
                 b_over_a=round(median(t["B_region_grid"]) / median(a), 4), c_over_a=round(median(t["C_region_stride64"]) / median(a), 4),
                 b_within_1p02_a=bool(median(t["B_region_grid"]) <= 1.02 * median(a)), region_bitwise_tiles=same, region_stride64_fp16_bitwise_tiles=same64)]


def shrunk(seconds, shrink=2):
    """--shrink 2: a 40x scan read at the 20x-equivalent pitch. 512 footprints of 512 x 512 on the 16 x 32 grid of a resident 8192 x 16384 region:
      arm A  forward_u8_region on 512 tiles of 256 x 256 of a 4096 x 8192 region (arm B of --resident): the yardstick, two interleaved halves for its spread;
      arm S  forward_u8_region(tile=512, shrink=2): the box filter inside the stem's window loader;
      arm G  ops.box_tiles_u8 (torch integer ops) then forward_u8, the glue inside the clock.
    S is checked bitwise against G before anything is timed. The stem launches alone (ops.stem_pool_region_u8, the plane split and the output allocation
    included) are timed for A and S in the same alternation."""
    from toad_amd import ops
    dev = torch.device("cuda:0")
    model = make_model()
    foot = TILE * shrink
    region_a, origins_a = grid_region(TILE, dev)
    gy, gx = GRID
    g = torch.Generator(device=dev).manual_seed(2)
    region_s = torch.randint(0, 256, (gy * foot, gx * foot, 3), device=dev, dtype=torch.uint8, generator=g)
    origins_s = torch.tensor([(x * foot, y * foot) for y in range(gy) for x in range(gx)], dtype=torch.int32)

    def arm_g():
        return model.forward_u8(ops.box_tiles_u8(region_s, origins_s, foot, shrink))
    same = bool(torch.equal(model.forward_u8_region(region_s, origins_s, tile=foot, shrink=shrink), arm_g()))
    wf, bias = model._folded[0][0], model._folded[1][0]
    arms = {"A_region_256": lambda: model.forward_u8_region(region_a, origins_a),
            "S_region_512_shrink2": lambda: model.forward_u8_region(region_s, origins_s, tile=foot, shrink=shrink), "G_torch_box_then_u8": arm_g,
            "stem_A": lambda: ops.stem_pool_region_u8(region_a, origins_a, wf, bias, TILE),
            "stem_S": lambda: ops.stem_pool_region_u8(region_s, origins_s, wf, bias, foot, shrink=shrink)}
    t, iters = alternate(arms, seconds)
    a = t["A_region_256"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    spread = abs(a1 - a2) / median(a)
    s, gl = median(t["S_region_512_shrink2"]), median(t["G_torch_box_then_u8"])
    n = origins_s.shape[0]
    return [dict(kind="resident_shrink", shrink=shrink, tiles=n, footprint=f"{foot}x{foot}", network_tile="256x256", region=list(region_s.shape[:2]),
                 region_a=list(region_a.shape[:2]), rounds=len(a), iters_per_round=iters, ms={k: round(median(v), 4) for k, v in t.items()},
                 ms_min={k: round(min(v), 4) for k, v in t.items()}, ms_max={k: round(max(v), 4) for k, v in t.items()},
                 tiles_per_s={k: round(n / median(v) * 1e3, 1) for k, v in t.items()}, arm_a_halves_ms=[round(a1, 4), round(a2, 4)],
                 arm_a_spread=round(spread, 4), s_over_a=round(s / median(a), 4), s_over_g=round(s / gl, 4),
                 stem_s_over_stem_a=round(median(t["stem_S"]) / median(t["stem_A"]), 4), s_faster_than_g_beyond_spread=bool(s * (1.0 + spread) < gl),
                 s_bitwise_g=same)]


def regions(seconds):
    """--regions: a slide that arrives cut. The resident 4096 x 8192 region, 512 tiles of 256 x 256 on the 16 x 32 grid:
      arm A    forward_u8_region on the whole region (arm B of --resident): the yardstick, two interleaved halves for its spread;
      arm L1   forward_u8_regions with that one region;
      arm S4 / S16   one forward_u8_region call per 1024-row strip / per block of the 4 x 4 grid (128 / 32 tiles each), back to back in one bracket;
      arm L4 / L16   the same windows through ONE forward_u8_regions call.
    L1, L4, L16 are checked torch.equal to A before anything is timed; S4 / S16 have other abs-max scopes and need not equal A - whether they do is printed.
    The stem launches alone (ops.stem_pool_region_u8 / stem_pool_regions_u8 with one region, the plane split and the output allocation included) are timed
    in the same alternation. One JSON line per arm."""
    from toad_amd import ops
    dev = torch.device("cuda:0")
    model = make_model()
    region, origins = grid_region(TILE, dev)
    gy, gx = GRID
    xy = origins.tolist()

    def windows(ny, nx):
        """The ny x nx cut of the region: (views, per-window local origins, triples in the slide's row-major tile order)."""
        hy, wx = gy // ny * TILE, gx // nx * TILE
        views = [region[j * hy:(j + 1) * hy, i * wx:(i + 1) * wx] for j in range(ny) for i in range(nx)]
        local = [[] for _ in views]
        triples = []
        for x, y in xy:
            k = (y // hy) * nx + x // wx
            local[k].append((x % wx, y % hy))
            triples.append((x % wx, y % hy, k))
        return views, [torch.tensor(o, dtype=torch.int32) for o in local], torch.tensor(triples, dtype=torch.int32)
    v4, o4, t4 = windows(4, 1)
    v16, o16, t16 = windows(4, 4)
    t1 = torch.cat([origins, torch.zeros(origins.shape[0], 1, dtype=torch.int32)], dim=1)

    def per_window(views, local):
        return torch.cat([model.forward_u8_region(v, o) for v, o in zip(views, local)])
    want = model.forward_u8_region(region, origins)
    equal = {"L1": bool(torch.equal(model.forward_u8_regions([region], t1), want)), "L4": bool(torch.equal(model.forward_u8_regions(v4, t4), want)),
             "L16": bool(torch.equal(model.forward_u8_regions(v16, t16), want))}
    if not all(equal.values()):
        raise SystemExit(f"the list call is not bitwise the whole-region call: {equal}")
    # (S16's rows come block by block, not in the slide's order: compared as the set of rows of each tile)
    order16 = torch.argsort(t16[:, 2].to(torch.int64), stable=True).to(dev)
    equal["S4"] = bool(torch.equal(per_window(v4, o4), want))
    equal["S16"] = bool(torch.equal(per_window(v16, o16), want[order16]))
    wf, bias = model._folded[0][0], model._folded[1][0]
    arms = {"A": lambda: model.forward_u8_region(region, origins), "L1": lambda: model.forward_u8_regions([region], t1),
            "S4": lambda: [model.forward_u8_region(v, o) for v, o in zip(v4, o4)], "L4": lambda: model.forward_u8_regions(v4, t4),
            "S16": lambda: [model.forward_u8_region(v, o) for v, o in zip(v16, o16)], "L16": lambda: model.forward_u8_regions(v16, t16),
            "stem_region": lambda: ops.stem_pool_region_u8(region, origins, wf, bias, TILE),
            "stem_regions": lambda: ops.stem_pool_regions_u8([region], t1, wf, bias, TILE)}
    t, iters = alternate(arms, seconds)
    a = t["A"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    ma = median(a)
    spread = abs(a1 - a2) / ma
    n = origins.shape[0]
    res = []
    for arm, v in t.items():
        m = median(v)
        r = dict(kind="resident_regions", arm=arm, tiles=n, tile="256x256", region=list(region.shape[:2]), rounds=len(v), iters_per_round=iters, ms=round(m, 4),
                 ms_min=round(min(v), 4), ms_max=round(max(v), 4), tiles_per_s=round(n / m * 1e3, 1))
        if arm == "A":
            r.update(arm_a_halves_ms=[round(a1, 4), round(a2, 4)], arm_a_spread=round(spread, 4))
        elif arm == "stem_regions":
            r.update(over_stem_region=round(m / median(t["stem_region"]), 4))
        elif arm != "stem_region":
            r.update(over_a=round(m / ma, 4), bitwise_a=equal[arm])
        if arm == "L1":
            r.update(within_1p02_a=bool(m <= 1.02 * ma))
        if arm in ("L4", "L16"):
            s = median(t["S" + arm[1:]])
            r.update(over_s=round(m / s, 4), faster_than_s_beyond_spread=bool(m < s - spread * ma))
        res.append(r)
    return res


def host_fed(stride, steps):
    dev = torch.device("cuda:0")
    model = make_model()
    region_d, origins = grid_region(stride, dev)
    n = origins.shape[0]
    region_h = torch.empty(region_d.shape, dtype=torch.uint8, pin_memory=True)
    region_h.copy_(region_d)
    del region_d
    region_np = region_h.numpy()
    tiles_h = torch.empty((n, TILE, TILE, 3), dtype=torch.uint8, pin_memory=True)
    tiles_np = tiles_h.numpy()
    tiles_d = torch.empty(tiles_h.shape, dtype=torch.uint8, device=dev)
    region_dst = torch.empty(region_h.shape, dtype=torch.uint8, device=dev)
    xy = origins.tolist()

    def step_cut():
        t0 = time.perf_counter()
        for i, (x, y) in enumerate(xy):
            tiles_np[i] = region_np[y:y + TILE, x:x + TILE]
        host = time.perf_counter() - t0
        tiles_d.copy_(tiles_h, non_blocking=True)
        model.forward_u8(tiles_d)
        return host

    def step_region():
        region_dst.copy_(region_h, non_blocking=True)
        model.forward_u8_region(region_dst, origins)
        return 0.0

    res = []
    for arm, step, nbytes in (("D1_host_cuts_tiles", step_cut, tiles_h.numel()), ("D2_region_by_origin", step_region, region_h.numel())):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        host = 0.0
        t0 = time.perf_counter()
        for _ in range(steps):
            host += step()
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res.append(dict(kind="host_fed_region", arm=arm, stride=stride, tiles_per_step=n, steps=steps, h2d_bytes_per_step=nbytes,
                        tiles_per_s=round(steps * n / dt, 1), ms_per_step=round(dt / steps * 1e3, 3), link_gbps=round(steps * nbytes / dt / 1e9, 2),
                        host_s_per_step=round(host / steps, 5), host_cut_gbps=round(steps * nbytes / host / 1e9, 2) if host > 0 else None,
                        host_threads=torch.get_num_threads()))
    return res


def launches(arm, calls=4):
    """`calls` calls of one arm, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    model = make_model()
    region, origins = grid_region(64 if arm == "C" else TILE, dev)
    tiles = cut(region, origins) if arm == "A" else None
    for _ in range(calls):
        if arm == "A":
            model.forward_u8(tiles)
        else:
            model.forward_u8_region(region, origins)
    torch.cuda.synchronize()
    return [dict(kind="launches_region", tiles=origins.shape[0], calls=calls, arm=arm)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--host-fed", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--arm", default="B", choices=("A", "B", "C"))
    ap.add_argument("--stride", type=int, default=TILE)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shrink", type=int, default=1, choices=(1, 2))
    ap.add_argument("--regions", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    every = not (a.resident or a.host_fed or a.launches or a.shrink != 1 or a.regions)
    res = []
    if a.regions:
        res += regions(a.seconds)
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extract_regions_bench.jsonl")
    if a.shrink != 1:
        res += shrunk(a.seconds, a.shrink)
    if a.launches:
        res += launches(a.arm)
    if a.resident or every:
        res += resident(a.seconds)
    if a.host_fed or every:
        res += host_fed(a.stride, a.steps)
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
