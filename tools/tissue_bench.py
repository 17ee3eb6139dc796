"""What selecting the tissue tiles of a resident region costs: the two HIP launches of toad_amd.tissue against the same predicate and tile sums written in
torch device ops - what a user would write without them. A sibling of extract_region_bench.py (its event timing, its alternation of the arms inside one
process, warm-up of every arm).

  resident: a synthetic slide of 4096 x 8192 pixels (100.7 MB) on the device, 256 x 256 tiles at stride 256 (16 x 32 tiles, cell 64):
      arm A   tissue_tile_fraction: tissue_cells_kernel<64> + tissue_tile_counts_kernel, no read-back;
      arm B   amax / amin over the channel, the integer compare, a reshape-sum - several region-sized intermediates are written and read again.
    A region of 100.7 MB fits the 256 MB last-level cache, so each arm is timed twice: `_rot` calls walk round FOUR different slides (403 MB, every call
    finds its region evicted: the HBM figure, the one to quote) and `_same` calls repeat on one slide (the cache-resident figure). bytes/s = the region's
    3 Hr Wr bytes over the call's time: the bytes the selection NEEDS, for arm B too.
  launches: four calls of arm A (or B) on rotating slides, no warm-up, for a `rocprofv3 --kernel-trace --stats` run of its own.

Prints one JSON line per result; --out FILE keeps them.
usage: tissue_bench.py [--launches --arm A|B] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                   # noqa: E402

import tools.ab.select_lib                     # noqa: E402,F401  (TOAD_HIP_LIB=<variant.so> is honoured HERE, not by the product's loader)

from extract_u8_bench import alternate, median      # noqa: E402
from toad_amd.tissue import tissue_tile_fraction    # noqa: E402

HR, WR, TILE = 4096, 8192, 256
SAT, VMIN = 8, 0


def make_slide(seed, dev):
    """uint8 [HR,WR,3]: near-white glass (grey 230..253 plus a per-channel jitter of 0..2), pink ellipses (r 180..230, g 80..140, b 150..200) over about a
    third of the area, placed by `seed`."""
    g = torch.Generator(device=dev).manual_seed(seed)
    img = torch.randint(230, 254, (HR, WR, 1), device=dev, generator=g) + torch.randint(0, 3, (HR, WR, 3), device=dev, generator=g)
    pink = torch.stack([torch.randint(180, 231, (HR, WR), device=dev, generator=g), torch.randint(80, 141, (HR, WR), device=dev, generator=g),
                        torch.randint(150, 201, (HR, WR), device=dev, generator=g)], dim=2)
    y = torch.arange(HR, device=dev).view(HR, 1).float()
    x = torch.arange(WR, device=dev).view(1, WR).float()
    c = torch.rand(6, 4, generator=torch.Generator().manual_seed(seed))
    inside = torch.zeros(HR, WR, dtype=torch.bool, device=dev)
    for cx, cy, rx, ry in c.tolist():
        inside |= ((x - cx * WR) / ((0.08 + 0.12 * rx) * WR)) ** 2 + ((y - cy * HR) / ((0.1 + 0.2 * ry) * HR)) ** 2 <= 1.0
    return torch.where(inside.unsqueeze(2), pink, img).to(torch.uint8).contiguous()


def torch_counts(region):
    """Arm B: the predicate of include/toad_hip.h and the tile sums in torch ops (int32 arithmetic), int32 [ny,nx]."""
    mx, mn = region.amax(dim=2).to(torch.int32), region.amin(dim=2).to(torch.int32)
    mask = (mx >= VMIN) & (255 * (mx - mn) > SAT * mx)
    return mask.view(HR // TILE, TILE, WR // TILE, TILE).sum(dim=(1, 3), dtype=torch.int32)


def hip_counts(region):
    return tissue_tile_fraction(region, TILE, None, (0, 0), SAT, VMIN)[0]


class Rotating:
    def __init__(self, fn, slides):
        self.fn, self.slides, self.i = fn, slides, 0

    def __call__(self):
        self.i = (self.i + 1) % len(self.slides)
        return self.fn(self.slides[self.i])


def resident(seconds):
    dev = torch.device("cuda:0")
    slides = [make_slide(s, dev) for s in range(4)]
    same = all(bool(torch.equal(hip_counts(s), torch_counts(s))) for s in slides)
    frac = float(hip_counts(slides[0]).sum()) / (HR * WR)
    arms = {"A_hip_rot": Rotating(hip_counts, slides), "B_torch_rot": Rotating(torch_counts, slides),
            "A_hip_same": lambda: hip_counts(slides[0]), "B_torch_same": lambda: torch_counts(slides[0])}
    t, iters = alternate(arms, seconds)
    nbytes = 3 * HR * WR
    a = t["A_hip_rot"]
    a1, a2 = median(a[0::2]), median(a[1::2])
    return [dict(kind="resident_tissue", region=[HR, WR], tile=TILE, stride=TILE, cell=64, tiles=(HR // TILE) * (WR // TILE), region_bytes=nbytes,
                 slides_rotated=len(slides), tissue_fraction=round(frac, 4), rounds=len(a), iters_per_round=iters,
                 ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                 ms_max={k: round(max(v), 5) for k, v in t.items()}, region_tbps={k: round(nbytes / median(v) / 1e9, 3) for k, v in t.items()},
                 arm_a_halves_ms=[round(a1, 5), round(a2, 5)], arm_a_spread=round(abs(a1 - a2) / median(a), 4),
                 b_over_a_rot=round(median(t["B_torch_rot"]) / median(a), 2), b_over_a_same=round(median(t["B_torch_same"]) / median(t["A_hip_same"]), 2),
                 hip_equals_torch=same)]


def launches(arm, calls=4):
    """`calls` calls of one arm on rotating slides, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    slides = [make_slide(s, dev) for s in range(4)]
    torch.cuda.synchronize()
    for i in range(calls):
        (hip_counts if arm == "A" else torch_counts)(slides[i % 4])
    torch.cuda.synchronize()
    return [dict(kind="launches_tissue", calls=calls, arm=arm)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--arm", default="A", choices=("A", "B"))
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = launches(a.arm) if a.launches else resident(a.seconds)
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
