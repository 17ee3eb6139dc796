"""What rendering the attention heat map of a resident region costs: the two HIP launches of toad_amd.heatmap (ops.heat_cells + ops.region_heat_blend)
against the same integer definition written in torch device ops - what a user would write without them. A sibling of tissue_bench.py (its event timing,
its alternation of the arms inside one process, warm-up of every arm, its four slides in rotation).

  resident: a synthetic slide of 4096 x 8192 pixels (100.7 MB) on the device, 256 x 256 tiles at stride 64 (61 x 125 tiles, cell 64, up to 16 tiles over
  a cell), about half of the tiles present with seeded scores, alpha 102, the jet colours; at down = 1 and at down = 4:
      arm A   heat_cells_kernel + heat_blend_kernel<down> into a canvas allocated once;
      arm B   the cell sums as 16 shifted adds on the small tables, repeat_interleave of the cell colours, the box sum as a reshape-sum, the blend in
              int32 - several canvas-sized int32 intermediates are written and read again.
    Arm B's canvas is checked once to be bit-equal to arm A's. A region of 100.7 MB fits the 256 MB last-level cache, so each arm is timed twice: `_rot`
    calls walk round FOUR different slides (403 MB, every call finds its region evicted: the HBM figure, the one to quote) and `_same` calls repeat on
    one slide (the cache-resident figure). bytes/s = 3 Hr Wr read + 3 Ho Wo written over the call's time: the bytes the canvas NEEDS, for arm B too.
  launches: four calls of arm A (or B) on rotating slides, no warm-up, for a `rocprofv3 --kernel-trace --stats` run of its own.

Prints one JSON line per result; --out FILE keeps them.
usage: heatmap_bench.py [--launches --arm A|B --down D] [--seconds S] [--out FILE]"""
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
from toad_amd import ops                            # noqa: E402
from toad_amd.heatmap import jet_lut                # noqa: E402
from toad_amd.tissue import lattice, lattice_cell   # noqa: E402

STRIDE, ALPHA = 64, 102
CELL = lattice_cell(TILE, STRIDE)
NX, NY = lattice(HR, WR, TILE, STRIDE)
GY, GX = -(-HR // CELL), -(-WR // CELL)


def make_table(seed, dev):
    """int32 [NY,NX]: about half of the tiles present, q uniform in 0 .. 65535."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 65536, (NY, NX), generator=g, dtype=torch.int32)
    return torch.where(torch.rand(NY, NX, generator=g) < 0.5, q, torch.full_like(q, -1)).to(dev)


def hip_canvas(region, table, lut, down, out):
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    return ops.region_heat_blend(region, cells, CELL, lut, ALPHA, down, out=out)


def torch_canvas(region, table, lut, down):
    """Arm B: the definition of include/toad_hip.h in torch ops, uint8 [HR // down, WR // down, 3]."""
    ch, cs = TILE // CELL, STRIDE // CELL
    present = (table >= 0).to(torch.int64)
    q = table.clamp(min=0).to(torch.int64) * present
    n = torch.zeros(GY, GX, dtype=torch.int64, device=region.device)
    s = torch.zeros_like(n)
    for a in range(ch):
        for b in range(ch):
            n[a:a + NY * cs:cs, b:b + NX * cs:cs] += present
            s[a:a + NY * cs:cs, b:b + NX * cs:cs] += q
    idx = torch.where(n > 0, (2 * s + 257 * n) // (514 * n.clamp(min=1)), torch.full_like(n, -1))
    ho, wo, r = HR // down, WR // down, CELL // down
    col = lut.to(torch.int32)[idx.clamp(min=0)].repeat_interleave(r, dim=0).repeat_interleave(r, dim=1)[:ho, :wo]
    covered = (idx >= 0).repeat_interleave(r, dim=0).repeat_interleave(r, dim=1)[:ho, :wo].unsqueeze(2)
    if down == 1:
        m = region.to(torch.int32)
    else:
        m = (region[:ho * down, :wo * down].view(ho, down, wo, down, 3).sum(dim=(1, 3), dtype=torch.int32) + down * down // 2) // (down * down)
    return torch.where(covered, (ALPHA * col + (256 - ALPHA) * m + 128) >> 8, m).to(torch.uint8)


def setup(dev):
    slides = [make_slide(s, dev) for s in range(4)]
    return slides, make_table(11, dev), jet_lut(dev)


def resident(seconds):
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    res = []
    for down in (1, 4):
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        hip = lambda r: hip_canvas(r, table, lut, down, out)                   # noqa: E731
        tor = lambda r: torch_canvas(r, table, lut, down)                      # noqa: E731
        same = all(bool(torch.equal(hip(s), tor(s))) for s in slides)
        if not same:                                                           # a wrong arm must not produce a quoted ratio
            raise SystemExit(f"heatmap_bench: arm B's canvas differs from arm A's at down = {down}: nothing is timed")
        covered = float((ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR)) >= 0).float().mean())
        arms = {"A_hip_rot": Rotating(hip, slides), "B_torch_rot": Rotating(tor, slides),
                "A_hip_same": lambda: hip(slides[0]), "B_torch_same": lambda: tor(slides[0])}
        t, iters = alternate(arms, seconds)
        nbytes = 3 * HR * WR + 3 * (HR // down) * (WR // down)
        a = t["A_hip_rot"]
        a1, a2 = median(a[0::2]), median(a[1::2])
        res.append(dict(kind="resident_heatmap", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, tiles=NX * NY, down=down, alpha=ALPHA,
                        moved_bytes=nbytes, slides_rotated=len(slides), covered_cells=round(covered, 4), rounds=len(a), iters_per_round=iters,
                        ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                        ms_max={k: round(max(v), 5) for k, v in t.items()}, moved_tbps={k: round(nbytes / median(v) / 1e9, 3) for k, v in t.items()},
                        arm_a_halves_ms=[round(a1, 5), round(a2, 5)], arm_a_spread=round(abs(a1 - a2) / median(a), 4),
                        b_over_a_rot=round(median(t["B_torch_rot"]) / median(a), 2),
                        b_over_a_same=round(median(t["B_torch_same"]) / median(t["A_hip_same"]), 2), hip_equals_torch=same))
        del out
    return res


def launches(arm, down, calls=4):
    """`calls` calls of one arm on rotating slides, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for i in range(calls):
        hip_canvas(slides[i % 4], table, lut, down, out) if arm == "A" else torch_canvas(slides[i % 4], table, lut, down)
    torch.cuda.synchronize()
    return [dict(kind="launches_heatmap", calls=calls, arm=arm, down=down)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--arm", default="A", choices=("A", "B"))
    ap.add_argument("--down", type=int, default=1, choices=(1, 2, 4))
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = launches(a.arm, a.down) if a.launches else resident(a.seconds)
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
