"""What the segmented tissue selector costs (toad_amd.tissue.segmented_tissue_origins, csrc/tissue_seg.hip): its HIP launches, kernel by kernel, against
the same definition written in torch device ops, and - at CLAM's default level - against the per-pixel selector it stands next to. A sibling of
tissue_bench.py (its slides, its rotation, its event timing, the arms alternated inside one process, every arm warmed up).

  resident: a synthetic slide of 4096 x 8192 pixels (100.7 MB) on the device, FOUR in rotation (403 MB: every call finds its region evicted from the
  256 MB last-level cache - the HBM figure), 256 x 256 tiles at stride 256, median = 7, sat_thresh = 8, val_min = 0, at down = 1, 4 and 16:
      arm A   the launches of the selector, each timed on its own with device events - sat (region -> saturation plane), median (7 x 7 + histogram,
              with its 1 KB memset), cells (plane -> counts per cell), tiles (toad_tissue_tile_counts) - and all four in a row (A_total);
      arm B   the same definition in torch device ops: reshape-sum, integer divide, max / min, the rounded quotient, a replicate pad (clamped index
              gather: uint8), the 49 shifted views stacked, sort, the middle element, bincount, the compare and a reshape-sum per tile.
    B's median plane, histogram and tile counts are checked torch.equal to A's before anything is timed.
  against tissue_origins (down = 16 only): the four launches of the new selector without a histogram (an int sat_thresh needs none) against the two of
    tissue_tile_fraction, same slides, same process, alternated; the margin the comparison allows is the spread between the two interleaved halves of the
    new selector's rounds plus two launches of a kernel with nothing to do (plane_cells on a 4 x 4 plane), measured here as well.

  --strips (instead of the above; down = 1 and 16 unless --downs says otherwise): the saturation plane of that slide when it arrives in pieces
  (ops.regions_saturation, sat_plane_list_kernel), same slides, same rotation, same event timing, the arms alternated in one process:
      S0        ops.region_saturation on the whole slide into one plane
      S4 / S16  4 full-width strips / a 4 x 4 grid of blocks, one ops.region_saturation call each into its view of one plane
      L4 / L16  the same strips / blocks through ONE ops.regions_saturation call
      C4 / C16  the library entry toad_regions_saturation_u8 on a host array built once (no Python per window)
    every arm's plane is checked torch.equal to S0's before anything is timed. Pass: L4 < S4 and L16 < S16 by more than the spread between the two
    interleaved halves of S0's rounds; C / S0 and L / S0 are reported without a bar.

Prints one JSON line per result; --out FILE keeps them.
usage: tissue_seg_bench.py [--seconds S] [--downs 1,4,16] [--strips] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                   # noqa: E402

import tools.ab.select_lib                     # noqa: E402,F401  (TOAD_HIP_LIB=<variant.so> is honoured HERE, not by the product's loader)

from extract_u8_bench import alternate, median      # noqa: E402
from tissue_bench import HR, WR, TILE, Rotating, make_slide      # noqa: E402
from toad_amd import _lib, ops                                   # noqa: E402
from toad_amd.tissue import lattice_cell, tissue_tile_fraction   # noqa: E402

K, SAT, VMIN = 7, 8, 0
NX, NY = WR // TILE, HR // TILE


def hip_stages(region, down, want_hist=True):
    """Arm A: (median plane, hist or None, tile counts int32 [ny,nx]) - the launches of segmented_tissue_origins, no read-back."""
    sat = ops.region_saturation(region, down, VMIN)
    if want_hist:
        med, hist = ops.plane_median(sat, K, want_hist=True)
    else:
        med, hist = ops.plane_median(sat, K), None
    pt = TILE // down
    cell = lattice_cell(pt)
    cells = ops.plane_cells(med, cell, SAT)
    return med, hist, ops.tissue_tile_counts(cells, cell, (0, 0), (pt, pt), (pt, pt), (NX, NY))


def torch_stages(region, down):
    """Arm B: the same three results from torch device ops (int32 arithmetic)."""
    hp, wp = HR // down, WR // down
    box = region.view(hp, down, wp, down, 3).sum(dim=(1, 3), dtype=torch.int32) if down > 1 else region.to(torch.int32)
    mean = torch.div(box + down * down // 2, down * down, rounding_mode="floor")
    mx, mn = mean.amax(dim=2), mean.amin(dim=2)
    s = torch.div(255 * (mx - mn) + (mx >> 1), mx.clamp(min=1), rounding_mode="floor")
    s = torch.where((mx == 0) | (mx < VMIN), torch.zeros_like(s), s).to(torch.uint8)
    r = K // 2
    iy = torch.arange(-r, hp + r, device=region.device).clamp(0, hp - 1)
    ix = torch.arange(-r, wp + r, device=region.device).clamp(0, wp - 1)
    pad = s[iy][:, ix]                                                              # replicate border
    stack = torch.stack([pad[dy:dy + hp, dx:dx + wp] for dy in range(K) for dx in range(K)], dim=2)      # the 49-fold copy
    med = stack.sort(dim=2).values[:, :, (K * K) // 2].contiguous()
    hist = torch.bincount(med.flatten().to(torch.int32), minlength=256).to(torch.int32)
    pt = TILE // down
    counts = (med > SAT).view(NY, pt, NX, pt).sum(dim=(1, 3), dtype=torch.int32)
    return med, hist, counts


def one_down(slides, down, seconds):
    dev = slides[0].device
    hp, wp = HR // down, WR // down
    pt = TILE // down
    cell = lattice_cell(pt)
    same = True
    for s in slides[:2]:
        a, b = hip_stages(s, down), torch_stages(s, down)
        same = same and all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        del a, b
    print(json.dumps(dict(kind="tissue_seg_progress", down=down, hip_equals_torch=same)), flush=True)
    sats = [ops.region_saturation(s, down, VMIN) for s in slides]
    meds = [ops.plane_median(p, K) for p in sats]
    cells = [ops.plane_cells(m, cell, SAT) for m in meds]
    frac = float((meds[0] > SAT).sum()) / (hp * wp)
    arms = {"A_sat": Rotating(lambda s: ops.region_saturation(s, down, VMIN), slides),
            "A_median_hist": Rotating(lambda p: ops.plane_median(p, K, want_hist=True), sats),
            "A_cells": Rotating(lambda m: ops.plane_cells(m, cell, SAT), meds),
            "A_tiles": Rotating(lambda c: ops.tissue_tile_counts(c, cell, (0, 0), (pt, pt), (pt, pt), (NX, NY)), cells),
            "A_total": Rotating(lambda s: hip_stages(s, down), slides),
            "B_total": Rotating(lambda s: torch_stages(s, down), slides)}
    t, iters = alternate(arms, seconds, rounds=4 if down == 1 else 8)
    ms = {k: median(v) for k, v in t.items()}
    a = t["A_total"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    nbytes = 3 * HR * WR
    return dict(kind="tissue_seg", region=[HR, WR], down=down, median=K, sat_thresh=SAT, plane=[hp, wp], tile=TILE, cell_on_plane=cell,
                region_bytes=nbytes, slides_rotated=len(slides), tissue_fraction=round(frac, 4), rounds=len(a), iters_per_round=iters,
                ms={k: round(v, 5) for k, v in ms.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                ms_max={k: round(max(v), 5) for k, v in t.items()}, sat_region_tbps=round(nbytes / ms["A_sat"] / 1e9, 3),
                median_ns_per_output_pixel=round(ms["A_median_hist"] * 1e6 / (hp * wp), 5), arm_a_halves_ms=[round(a1, 5), round(a2, 5)],
                arm_a_spread=round(abs(a1 - a2) / ms["A_total"], 4), b_over_a=round(ms["B_total"] / ms["A_total"], 2),
                a_faster_than_b=bool(ms["A_total"] < ms["B_total"]), hip_equals_torch=same)


def against_tissue_origins(slides, seconds, down=16):
    """The whole new selector (device part, no histogram) against tissue_tile_fraction, and the margin: spread of the halves + two empty launches."""
    tiny = torch.zeros(4, 4, dtype=torch.uint8, device=slides[0].device)
    arms = {"new_selector": Rotating(lambda s: hip_stages(s, down, want_hist=False), slides),
            "tissue_tile_fraction": Rotating(lambda s: tissue_tile_fraction(s, TILE, None, (0, 0), SAT, VMIN), slides),
            "empty_launch": lambda: ops.plane_cells(tiny, 4, SAT)}
    t, iters = alternate(arms, seconds)
    ms = {k: median(v) for k, v in t.items()}
    a = t["new_selector"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    margin = abs(a1 - a2) + 2 * ms["empty_launch"]
    return dict(kind="tissue_seg_vs_origins", region=[HR, WR], down=down, median=K, tile=TILE, rounds=len(a), iters_per_round=iters,
                ms={k: round(v, 5) for k, v in ms.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                ms_max={k: round(max(v), 5) for k, v in t.items()}, new_halves_ms=[round(a1, 5), round(a2, 5)], margin_ms=round(margin, 5),
                new_minus_old_ms=round(ms["new_selector"] - ms["tissue_tile_fraction"], 5),
                new_within_old_plus_margin=bool(ms["new_selector"] <= ms["tissue_tile_fraction"] + margin))


def pieces(slide, plane, down, ny, nx):
    """The slide as ny x nx windows (cuts at multiples of 32, so every box lies in one window) and each window's rows and columns of `plane`."""
    hs, ws = HR // ny, WR // nx
    regions = [slide[j * hs:(j + 1) * hs, i * ws:(i + 1) * ws] for j in range(ny) for i in range(nx)]
    outs = [plane[j * hs // down:(j + 1) * hs // down, i * ws // down:(i + 1) * ws // down] for j in range(ny) for i in range(nx)]
    return regions, outs


def strips_one_down(slides, down, seconds):
    dev = slides[0].device
    hp, wp = HR // down, WR // down
    planes = [torch.empty((hp, wp), dtype=torch.uint8, device=dev) for _ in slides]
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    grids = {"4": (4, 1), "16": (4, 4)}
    work = {}
    for name, (ny, nx) in grids.items():
        per_slide = []
        for s, p in zip(slides, planes):
            regions, outs = pieces(s, p, down, ny, nx)
            host = (_lib.ToadSatWindow * len(regions))(*(_lib.ToadSatWindow(r.data_ptr(), r.stride(0), r.shape[0], r.shape[1], o.data_ptr(), o.stride(0))
                                                         for r, o in zip(regions, outs)))
            per_slide.append((regions, outs, host, p))
        work[name] = per_slide

    def arm_s(w):
        regions, outs, host, p = w
        for r, o in zip(regions, outs):
            ops.region_saturation(r, down, VMIN, out=o)
        return p

    def arm_l(w):
        regions, outs, host, p = w
        ops.regions_saturation(regions, down, VMIN, outs=outs)
        return p

    def arm_c(w):
        regions, outs, host, p = w
        _lib.check(lib.toad_regions_saturation_u8(host, len(regions), down, VMIN, stream), "toad_regions_saturation_u8")
        return p

    whole = list(zip(slides, planes))
    same = True
    for k, s in enumerate(slides):
        want = ops.region_saturation(s, down, VMIN)
        for name in grids:
            for arm in (arm_s, arm_l, arm_c):
                planes[k].fill_(0x7F)
                same = same and bool(torch.equal(arm(work[name][k]), want))
        del want
    print(json.dumps(dict(kind="tissue_strips_progress", down=down, every_arm_equals_whole_slide=same)), flush=True)
    arms = {"S0": Rotating(lambda w: ops.region_saturation(w[0], down, VMIN, out=w[1]), whole)}
    for name in grids:
        arms["S" + name] = Rotating(arm_s, work[name])
        arms["L" + name] = Rotating(arm_l, work[name])
        arms["C" + name] = Rotating(arm_c, work[name])
    t, iters = alternate(arms, seconds, rounds=8)
    ms = {k: median(v) for k, v in t.items()}
    a = t["S0"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    spread = abs(a1 - a2)
    return dict(kind="tissue_strips", region=[HR, WR], down=down, plane=[hp, wp], region_bytes=3 * HR * WR, slides_rotated=len(slides), rounds=len(a),
                iters_per_round=iters, ms={k: round(v, 5) for k, v in ms.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                ms_max={k: round(max(v), 5) for k, v in t.items()}, s0_halves_ms=[round(a1, 5), round(a2, 5)], s0_spread_ms=round(spread, 5),
                over_s0={k: round(ms[k] / ms["S0"], 4) for k in ms if k != "S0"},
                l4_below_s4_beyond_spread=bool(ms["L4"] < ms["S4"] - spread), l16_below_s16_beyond_spread=bool(ms["L16"] < ms["S16"] - spread),
                every_arm_equals_whole_slide=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--downs", default="")
    ap.add_argument("--strips", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    slides = [make_slide(s, dev) for s in range(4)]
    downs = [int(d) for d in (a.downs or ("1,16" if a.strips else "1,4,16")).split(",")]
    if a.strips:
        res = []
        for d in downs:
            res.append(strips_one_down(slides, d, a.seconds))
            print(json.dumps(res[-1]), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(json.dumps(r) for r in res) + "\n")
        return
    for d in downs:
        if TILE % (4 * d):
            raise SystemExit(f"down = {d}: the {TILE}-pixel tile is not a multiple of 4 * down")
    res = []
    for d in downs:
        res.append(one_down(slides, d, a.seconds))
        print(json.dumps(res[-1]), flush=True)
        torch.cuda.empty_cache()
    if 16 in downs:
        res.append(against_tissue_origins(slides, a.seconds))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in res) + "\n")


if __name__ == "__main__":
    main()
