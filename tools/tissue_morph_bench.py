"""What closing and the two area filters cost (the close / min_area / min_hole stages of toad_amd.tissue.segmented_tissue_origins, csrc/tissue_morph.hip):
their HIP launches, entry point by entry point, against the same definition written in torch device ops. A sibling of tissue_seg_bench.py (its slides with
holes added, its rotation, its event timing, the arms alternated inside one process, every arm warmed up).

  input: the synthetic slide of 4096 x 8192 pixels of tissue_bench.py with glass holes punched into it and pink specks strewn over it, FOUR in rotation;
  the median plane (median = 7, sat_thresh = 8) at down = 1, 4 and 16 is computed once per slide and is what both arms start from. close = 4,
  min_area = min_hole = 16384 / down^2 plane pixels.
      arm A   the new entry points, each timed on its own with device events - close (one kernel), components of the tissue (three launches: tiles in
              LDS, seams, roots and counts), select, components of the background, select - and all five in a row (A_total). The launches inside one
              components call are not separated: that takes a kernel trace.
      arm B   the same definition in torch device ops: max_pool2d for the dilation and, on the complement, the erosion; label propagation by a repeated
              3 x 3 (or, for the background, plus-shaped) minimum of int32 indices to a fixed point, tested every 16 sweeps; bincount for the areas.
    B's masks after every stage, and its labels and areas, are checked torch.equal to A's before anything is timed. B is seconds long at down = 1 (its sweep
    count grows with the diameter of the largest component), so it is timed as single calls.
  Also printed: the labelling's time per plane pixel, and at each down whether the five calls together cost no more than the median launch they follow plus
  the spread between the two interleaved halves of their own rounds.

Prints one JSON line per result; --out FILE keeps them.
usage: tissue_morph_bench.py [--seconds S] [--downs 1,4,16] [--torch-downs 1,4,16] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

import tools.ab.select_lib                     # noqa: E402,F401  (TOAD_HIP_LIB=<variant.so> is honoured HERE, not by the product's loader)

from extract_u8_bench import alternate, event_ms, median      # noqa: E402
from tissue_bench import HR, WR, Rotating, make_slide         # noqa: E402
from toad_amd import ops                                      # noqa: E402

K, SAT, VMIN, CLOSE, AREA = 7, 8, 0, 4, 16384
BIG = (1 << 31) - 1
BORDER = 1 << 30


def make_holey_slide(seed, dev):
    """make_slide(seed) with 48 glass discs (radii 4 .. 160 pixels) punched out and 48 pink discs (radii 3 .. 60) put on top, placed by `seed`."""
    img = make_slide(seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 100)
    glass = (torch.randint(230, 254, (HR, WR, 1), device=dev, generator=g) + torch.randint(0, 3, (HR, WR, 3), device=dev, generator=g)).to(torch.uint8)
    pink = torch.stack([torch.randint(180, 231, (HR, WR), device=dev, generator=g), torch.randint(80, 141, (HR, WR), device=dev, generator=g),
                        torch.randint(150, 201, (HR, WR), device=dev, generator=g)], dim=2).to(torch.uint8)
    y = torch.arange(HR, device=dev).view(HR, 1).float()
    x = torch.arange(WR, device=dev).view(1, WR).float()
    c = torch.rand(96, 3, generator=torch.Generator().manual_seed(seed + 200)).tolist()
    for i, (cx, cy, r) in enumerate(c):
        rad = (4 + 156 * r * r) if i < 48 else (3 + 57 * r * r)
        m = (x - cx * WR) ** 2 + (y - cy * HR) ** 2 <= rad * rad
        img = torch.where(m.unsqueeze(2), glass if i < 48 else pink, img)
    return img.contiguous()


def hip_stages(plane, down):
    """Arm A: (M1, labels, area, M2, labels, area, M3) as the device leaves them."""
    lim = AREA // (down * down)
    m1 = ops.plane_close(plane, CLOSE, SAT)
    l1, a1 = ops.plane_components(m1, 0, 0)
    m2 = ops.plane_area_select(l1, a1, 0, lim)
    l2, a2 = ops.plane_components(m2, 0, 1)
    m3 = ops.plane_area_select(l2, a2, 1, lim)
    return m1, l1, a1, m2, l2, a2, m3


def torch_close(m0, c):
    lo, hi = c // 2, c - 1 - c // 2
    f = m0.to(torch.float16)[None, None]
    d = F.max_pool2d(F.pad(f, (lo, hi, lo, hi), value=0.0), c, stride=1)
    e = 1.0 - F.max_pool2d(F.pad(1.0 - d, (lo, hi, lo, hi), value=0.0), c, stride=1)
    return e[0, 0] > 0.5


def torch_components(sel, conn8):
    """(labels int32 [Hp,Wp] with -1, area int32 [Hp * Wp], sweeps): minimum-index propagation to a fixed point."""
    hp, wp = sel.shape
    idx = torch.arange(hp * wp, device=sel.device, dtype=torch.int32).view(hp, wp)
    big = torch.full_like(idx, BIG)
    lab = torch.where(sel, idx, big)
    sweeps = 0
    while True:
        prev = lab
        for _ in range(16):
            p = F.pad(lab, (1, 1, 1, 1), value=BIG)
            if conn8:
                r = torch.minimum(torch.minimum(p[:, :-2], p[:, 1:-1]), p[:, 2:])
                n = torch.minimum(torch.minimum(r[:-2], r[1:-1]), r[2:])
            else:
                n = torch.minimum(torch.minimum(torch.minimum(p[1:-1, :-2], p[1:-1, 2:]), torch.minimum(p[:-2, 1:-1], p[2:, 1:-1])), lab)
            lab = torch.where(sel, n, big)
        sweeps += 16
        if torch.equal(lab, prev):
            break
    flat = lab[sel].to(torch.int64)
    area = torch.bincount(flat, minlength=hp * wp).to(torch.int32)
    edge = torch.zeros_like(sel)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    area[torch.unique(lab[sel & edge]).to(torch.int64)] += BORDER
    return torch.where(sel, lab, torch.full_like(lab, -1)), area, sweeps


def torch_select(labels, area, mode, limit):
    a = area[labels.clamp(min=0).to(torch.int64)]
    count, border = a & (BORDER - 1), (a & BORDER) != 0
    return ((labels >= 0) & (count >= limit)) if mode == 0 else ((labels < 0) | ((count < limit) & ~border))


def torch_stages(plane, down):
    lim = AREA // (down * down)
    m1 = torch_close(plane > SAT, CLOSE)
    l1, a1, s1 = torch_components(m1, True)
    m2 = torch_select(l1, a1, 0, lim)
    l2, a2, s2 = torch_components(~m2, False)
    m3 = torch_select(l2, a2, 1, lim)
    u8 = lambda m: m.to(torch.uint8) * 255                    # noqa: E731
    return (u8(m1), l1, a1, u8(m2), l2, a2, u8(m3)), s1 + s2


def one_down(slides, down, seconds, with_torch):
    hp, wp = HR // down, WR // down
    lim = AREA // (down * down)
    sats = [ops.region_saturation(s, down, VMIN) for s in slides]
    planes = [ops.plane_median(p, K) for p in sats]
    same, sweeps = None, None
    if with_torch:
        a = hip_stages(planes[0], down)
        b, sweeps = torch_stages(planes[0], down)
        same = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        del a, b
        print(json.dumps(dict(kind="tissue_morph_progress", down=down, hip_equals_torch=same, torch_sweeps=sweeps)), flush=True)
    st = [hip_stages(p, down) for p in planes]
    changed = [int((st[0][0] != (planes[0] > SAT).to(torch.uint8) * 255).sum()), int((st[0][3] != st[0][0]).sum()), int((st[0][6] != st[0][3]).sum())]
    arms = {"A_median": Rotating(lambda p: ops.plane_median(p, K), sats),
            "A_close": Rotating(lambda p: ops.plane_close(p, CLOSE, SAT), planes),
            "A_components_fg": Rotating(lambda s: ops.plane_components(s[0], 0, 0), st),
            "A_select_fg": Rotating(lambda s: ops.plane_area_select(s[1], s[2], 0, lim), st),
            "A_components_bg": Rotating(lambda s: ops.plane_components(s[3], 0, 1), st),
            "A_select_bg": Rotating(lambda s: ops.plane_area_select(s[4], s[5], 1, lim), st),
            "A_total": Rotating(lambda p: hip_stages(p, down), planes)}
    t, iters = alternate(arms, seconds, rounds=8)
    ms = {k: median(v) for k, v in t.items()}
    tot = t["A_total"]
    h1, h2 = median(tot[0::2]), median(tot[1::2])
    res = dict(kind="tissue_morph", region=[HR, WR], down=down, plane=[hp, wp], median=K, sat_thresh=SAT, close=CLOSE, min_area=lim, min_hole=lim,
               slides_rotated=len(slides), pixels_changed_by_stage=changed, rounds=len(tot), iters_per_round=iters,
               ms={k: round(v, 5) for k, v in ms.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
               ms_max={k: round(max(v), 5) for k, v in t.items()},
               labelling_ns_per_pixel={k: round(ms[k] * 1e6 / (hp * wp), 5) for k in ("A_components_fg", "A_components_bg")},
               arm_a_halves_ms=[round(h1, 5), round(h2, 5)], median_plus_spread_ms=round(ms["A_median"] + abs(h1 - h2), 5),
               stages_within_median_plus_spread=bool(ms["A_total"] <= ms["A_median"] + abs(h1 - h2)), hip_equals_torch=same)
    if with_torch:
        b = [event_ms(lambda: torch_stages(planes[i % len(planes)], down), 1) for i in range(3)]
        res.update(B_total_ms=[round(v, 3) for v in b], torch_sweeps=sweeps, b_over_a=round(median(b) / ms["A_total"], 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--downs", default="1,4,16")
    ap.add_argument("--torch-downs", default="1,4,16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    slides = [make_holey_slide(s, dev) for s in range(4)]
    tdowns = [int(d) for d in a.torch_downs.split(",") if d]
    res = []
    for d in [int(d) for d in a.downs.split(",")]:
        res.append(one_down(slides, d, a.seconds, d in tdowns))
        print(json.dumps(res[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in res) + "\n")


if __name__ == "__main__":
    main()
