"""What rendering the attention heat map of a resident region costs: the two HIP launches of toad_amd.heatmap (ops.heat_cells + ops.region_heat_blend)
against the same integer definition written in torch device ops - what a user would write without them. A sibling of tissue_bench.py (its event timing,
its alternation of the arms inside one process, warm-up of every arm, its four slides in rotation).

  resident: a synthetic slide of 4096 x 8192 pixels (100.7 MB) on the device, 256 x 256 tiles at stride 64 (61 x 125 tiles, cell 64, up to 16 tiles over
  a cell), about half of the tiles present with seeded scores, alpha 102, the jet colours; at down = 1 and at down = 4:
      arm A   heat_cells_kernel + heat_blend_px_kernel<down,0,false> (ops.region_heat_blend) into a canvas allocated once;
      arm B   the cell sums as 16 shifted adds on the small tables, a gather of the cell colours, the box sum as a reshape-sum, the blend in int32 -
              several canvas-sized intermediates are written and read again. One torch definition serves this arm and --px's.
    Arm B's canvas is checked once to be bit-equal to arm A's. A region of 100.7 MB fits the 256 MB last-level cache, so each arm is timed twice: `_rot`
    calls walk round FOUR different slides (403 MB, every call finds its region evicted: the HBM figure, the one to quote) and `_same` calls repeat on
    one slide (the cache-resident figure). bytes/s = 3 Hr Wr read + 3 Ho Wo written over the call's time: the bytes the canvas NEEDS, for arm B too.
  launches: four calls of arm A (or B) on rotating slides, no warm-up, for a `rocprofv3 --kernel-trace --stats` run of its own.
  px (--px): what the per-pixel variants of the pass (ops.region_heat_blend_px) cost over the flat one, at down = 1, 2 and 4. Same slides, table and
    canvas; the mask of each slide is the (plane, t) of tissue.segment_tissue at down 16, median 7, threshold 8. Arms, alternated in one process on the
    rotating slides:
      flat      arm A above, through ops.region_heat_blend;
      px_plain  ops.region_heat_blend_px without keywords: the flat kernel through the other entry point;
      px_smooth / px_mask / px_both   heat_cells_kernel + heat_blend_px_kernel<down> with smooth, with the mask, with both;
      B_torch   px_both's definition in torch ops (gathers of the four neighbours, int64 canvas-sized intermediates), checked bit-equal to px_both on
                every slide before anything is timed.
    All arms move the same 3 Hr Wr + 3 Ho Wo bytes (the mask plane is 1 / 768 of the region). px_over_flat = median over median; flat_spread = the flat
    arm's own interleaved-halves spread, the yardstick for "no cost".

  thumb (--thumb): what the overview canvas (ops.region_heat_thumb, heat_thumb_kernel<down>) costs at down = 8, 16 and 32. Same slides, table and colours;
    the cell table is built once per run (ops.heat_cells is not timed in any arm), the mask of each slide is the (plane, t) of tissue.segment_tissue at
    down 32, median 7, threshold 8. Arms, alternated in one process on the rotating slides:
      T_flat / T_both   ops.region_heat_thumb without keywords / with smooth and the mask, into a canvas allocated once;
      S                 the yardstick: ops.region_saturation at the same down (sat_plane_kernel<down>) - the same loads and the same reduction skeleton, a
                        third of the output bytes;
      P                 what was there before: ops.region_heat_blend_px at down = 4 with smooth and the mask into a canvas allocated once, then
                        avg_pool2d by down / 4 and a round in torch ops. TIMED ONLY: it rounds twice and samples the tent and the mask at down = 4, so it
                        is not bit-equal to T and is not checked against it.
    T_flat and T_both are checked bit-equal to the torch statement of the definition (torch_canvas) on every slide before anything is timed. t_over_s =
    median over median next to s_spread, S's own interleaved-halves spread; moved bytes = 3 Hr Wr read + 3 Ho Wo written.

  blur (--blur): what the Gaussian blur of the cell table (ops.heat_cells_blur, heat_cells_blur_kernel) costs. Tables of 64 x 128 cells (the 4096 x 8192
    slide at cell 64) and 1563 x 1563 cells (a 100k x 100k slide), about a third of the cells absent, Gaussian taps of radius 8 and 15. Arms, alternated in
    one process:
      A_hip     ops.heat_cells_blur;
      B_torch   the same definition in torch device ops: v p and p stacked, a float64 conv2d along x and one along y (sums below 2^53: exact), then
                (2 N + D) // (2 D) in int64 - checked torch.equal to A_hip before anything is timed;
      cells     the yardstick: the ops.heat_cells launch that builds a table of this size (256 x 256 tiles at stride 64).
    Then, on the rotating 4096 x 8192 slides at down = 1 and 16: heatmap.attention_canvas with blur=False and blur=True into a canvas allocated once (the
    whole call: host arithmetic, the index upload and the launches), and the launches alone (heat_cells [+ heat_cells_blur] + the blend) - canvas_blur
    is checked to differ from canvas_plain and launches_blur to equal canvas_blur bit for bit. Default output profiles/heatmap_blur_bench.jsonl.

  window (--window): what rendering a slide window by window (ops.region_heat_window, toad_region_heat_window_u8) costs. Same slides, table and colours;
    the cell table is built once per run, the mask of each slide is the (plane, t) of tissue.segment_tissue at down 16 (down = 1) or 32 (down = 16),
    median 7, threshold 8. Flat and with smooth + mask, at down = 1 and 16. Arms, alternated in one process on the rotating slides, each into a canvas
    allocated once:
      W0    the entry that was there before (ops.region_heat_blend_px / ops.region_heat_thumb), the whole slide;
      W1    ops.region_heat_window, the whole slide as window (0, 0): the same kernel with the two offsets zero;
      W4    the slide as 4 full-width strips of 1024 rows, W16 as a 4 x 4 grid of 1024 x 2048 blocks, through ops.region_heat_window: 4 and 16 launches.
    W1, W4 and W16 are checked torch.equal to W0 on every slide before anything is timed. w_over_w0 = median over median next to w0_spread, W0's own
    interleaved-halves spread: the margin for W1 / W0. W4 and W16 add launches and are reported without a bar. With TOAD_HIP_LIB=<a library built from
    the parent commit's sources> (tools/ab/select_lib.py), which does not export the window entry, only W0 is timed (kind ..._w0, lib = its tag): the
    same arm on the kernels as they were. --w0-only times W0 alone on this tree's library as well, so that the two processes run the same arms in the
    same order: those two are the lines to set side by side (W0 next to the window arms runs in another cache and clock state than W0 alone). Default
    output profiles/heatmap_window_bench.jsonl.

  pyramid (--pyramid): what several levels in ONE pass (ops.region_heat_pyramid, toad_region_heat_pyramid_u8) cost against one pass per level. The
    --window setup: same slides, table and colours, the cell table built once per run. Level sets (1, 4, 16), all six and (8, 16, 32), each flat and
    with smooth + mask; the mask of each slide is the (plane, t) of tissue.segment_tissue at down 16 for the first set and 32 for the others, median 7,
    threshold 8. Arms, alternated in one process on the rotating slides, each into canvases allocated once:
      P     ops.region_heat_pyramid: every level of the set from one read of the slide, one launch;
      S     ops.region_heat_window once per level, back to back in one bracket: one read and one launch per level;
      L1    ops.region_heat_window at down = 1 alone: P cannot be faster than this, its ratio carries no bar.
    P is checked torch.equal to S, level by level, on every slide before anything is timed. p_over_s = median over median next to s_spread, S's own
    interleaved-halves spread; p_faster_beyond_spread says whether P beats S by more than that. moved bytes = 3 Hr Wr read ONCE + every level's 3 Ho Wo
    written (S reads the region once per level: s_moved_bytes). Default output profiles/heatmap_pyramid_bench.jsonl.

  windows (--windows): what a LIST of windows in one call (ops.region_heat_windows, toad_region_heat_windows_u8) saves over one call per window. The
    --window setup: same slides, table, colours, masks, the cell table built once per run, flat and with smooth + mask, at down = 1 and 16. Arms,
    alternated in one process on the rotating slides, each into a canvas allocated once:
      W0        the entry that was there before, the whole slide;
      W4, W16   --window's: the 4 strips and the 4 x 4 block grid through ops.region_heat_window, 4 and 16 calls and launches;
      L4, L16   the same strips and blocks through ONE ops.region_heat_windows call: one launch;
      C4, C16   the library entry itself on a host array built once per slide: the launch without the Python wrapper's per-window checks and views.
    L4, L16, C4 and C16 are checked torch.equal to W0 on every slide before anything is timed. l_over_w = L4 / W4 and L16 / W16, median over median, next to
    w0_spread, W0's own interleaved-halves spread: l_faster_beyond_spread says whether the list beats the per-window calls by more than that. l_over_w0
    = L4 / W0 and L16 / W0, and c_over_w0 likewise, are reported without a bar. Default output profiles/heatmap_windows_bench.jsonl.

  pyramid windows (--pyramid-windows): what several levels for a LIST of windows in one call (ops.region_heat_pyramid_windows,
    toad_region_heat_pyramid_windows_u8) save over one pyramid call per window. The --window / --pyramid setup: same slides, table, colours and masks, the
    cell table built once per run; level sets (1, 4, 16) and all six, each flat and with smooth + mask. Arms, alternated in one process on the rotating
    slides, each into per-level canvases allocated once:
      P           ops.region_heat_pyramid on the whole slide: one launch;
      PW4, PW16   the 4 strips and the 4 x 4 block grid through one ops.region_heat_pyramid call each: 4 and 16 calls and launches;
      PL4, PL16   the same strips and blocks through ONE ops.region_heat_pyramid_windows call: one launch;
      CL4, CL16   the library entry itself on a host array built once per slide: the launch without the Python wrapper's per-window checks and views.
    PW, PL and CL are checked torch.equal to P, level by level, on every slide before anything is timed. pl_over_pw = PL4 / PW4 and PL16 / PW16, median
    over median, next to p_spread, P's own interleaved-halves spread: pl_faster_beyond_spread says whether the list beats the per-window calls by more
    than that. pl_over_p, cl_over_p and pw_over_p are reported without a bar. Default output profiles/heatmap_pyramid_windows_bench.jsonl.

Prints one JSON line per result; --out FILE keeps them.
usage: heatmap_bench.py [--launches --arm A|B --down D] [--px | --thumb | --blur | --window [--w0-only] | --windows | --pyramid | --pyramid-windows]
                        [--seconds S] [--out FILE]"""
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
from toad_amd.tissue import lattice, lattice_cell, segment_tissue   # noqa: E402

STRIDE, ALPHA = 64, 102
CELL = lattice_cell(TILE, STRIDE)
NX, NY = lattice(HR, WR, TILE, STRIDE)
GY, GX = -(-HR // CELL), -(-WR // CELL)


def make_table(seed, dev):
    """int32 [NY,NX]: about half of the tiles present, q uniform in 0 .. 65535."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 65536, (NY, NX), generator=g, dtype=torch.int32)
    return torch.where(torch.rand(NY, NX, generator=g) < 0.5, q, torch.full_like(q, -1)).to(dev)


MASK_DOWN = 16


def hip_canvas(region, table, lut, down, out, smooth=False, mask=None, px=True):
    """The two launches. px=False goes through ops.region_heat_blend, the entry point without the keywords."""
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    if not px:
        return ops.region_heat_blend(region, cells, CELL, lut, ALPHA, down, out=out)
    plane, t = mask if mask is not None else (None, 0)
    return ops.region_heat_blend_px(region, cells, CELL, lut, ALPHA, down, smooth=smooth, mask=plane, mask_down=MASK_DOWN if mask is not None else None,
                                    mask_thresh=t, out=out)


def torch_canvas(region, table, lut, down, smooth=False, mask=None, mask_down=MASK_DOWN):
    """The definition of include/toad_hip.h in torch ops, uint8 [HR // down, WR // down, 3]: the flat canvas without the keywords, the per-pixel one with."""
    dev = region.device
    ch, cs = TILE // CELL, STRIDE // CELL
    present = (table >= 0).to(torch.int64)
    q = table.clamp(min=0).to(torch.int64) * present
    n = torch.zeros(GY, GX, dtype=torch.int64, device=dev)
    s = torch.zeros_like(n)
    for a in range(ch):
        for b in range(ch):
            n[a:a + NY * cs:cs, b:b + NX * cs:cs] += present
            s[a:a + NY * cs:cs, b:b + NX * cs:cs] += q
    c = torch.where(n > 0, (2 * s + 257 * n) // (514 * n.clamp(min=1)), torch.full_like(n, -1))
    ho, wo = HR // down, WR // down
    oy, ox = torch.arange(ho, device=dev) * down, torch.arange(wo, device=dev) * down
    own = c[oy // CELL][:, ox // CELL]
    idx = own
    if smooth:
        def axis(n):
            p = 2 * down * torch.arange(n, device=dev) + down - CELL
            g0 = torch.div(p, 2 * CELL, rounding_mode="floor")
            f = p - 2 * CELL * g0
            return g0, 2 * CELL - f, f
        (gy0, wy0, wy1), (gx0, wx0, wx1) = axis(ho), axis(wo)
        acc = torch.zeros(ho, wo, dtype=torch.int64, device=dev)
        for gy, wy in ((gy0, wy0), (gy0 + 1, wy1)):
            for gx, wx in ((gx0, wx0), (gx0 + 1, wx1)):
                inside = ((gy >= 0) & (gy < GY))[:, None] & ((gx >= 0) & (gx < GX))[None, :]
                v = c[gy.clamp(0, GY - 1)][:, gx.clamp(0, GX - 1)]
                acc += wy[:, None] * wx[None, :] * torch.where(inside & (v >= 0), v, own)
        idx = (acc + 2 * CELL * CELL) >> (2 * (CELL.bit_length() - 1) + 2)
    blend = own >= 0
    if mask is not None:
        plane, t = mask
        hm, wm = plane.shape
        my, mx = oy // mask_down, ox // mask_down
        blend = blend & ((my < hm)[:, None] & (mx < wm)[None, :]) & (plane[my.clamp(max=hm - 1)][:, mx.clamp(max=wm - 1)] > t)
    col = lut.to(torch.int32)[idx.clamp(min=0)]
    if down == 1:
        m = region.to(torch.int32)
    else:
        m = (region[:ho * down, :wo * down].view(ho, down, wo, down, 3).sum(dim=(1, 3), dtype=torch.int32) + down * down // 2) // (down * down)
    return torch.where(blend.unsqueeze(2), (ALPHA * col + (256 - ALPHA) * m + 128) >> 8, m).to(torch.uint8)


def setup(dev):
    slides = [make_slide(s, dev) for s in range(4)]
    return slides, make_table(11, dev), jet_lut(dev)


def resident(seconds, px):
    """The resident figures (px=False) or the --px ones: the arms differ, the loop does not."""
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    masks = {s.data_ptr(): segment_tissue(s, MASK_DOWN, 7, 8) for s in slides} if px else {}
    res = []
    for down in (1, 2, 4) if px else (1, 4):
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        hip = lambda smooth=False, masked=False, px=True: (                                             # noqa: E731
            lambda r: hip_canvas(r, table, lut, down, out, smooth, masks[r.data_ptr()] if masked else None, px))
        flat, most = hip(px=False), hip(px, px, px)                                                     # most: px_both, or the flat arm again
        tor = lambda r: torch_canvas(r, table, lut, down, px, masks[r.data_ptr()] if px else None)      # noqa: E731
        same = all(bool(torch.equal(most(s), tor(s))) for s in slides)
        same_flat = all(bool(torch.equal(hip()(s).clone(), flat(s))) for s in slides)
        if not (same and same_flat):                                           # a wrong arm must not produce a quoted ratio
            raise SystemExit(f"heatmap_bench: the HIP canvas differs from its torch arm ({same}) or px without keywords from the flat pass ({same_flat}) "
                             f"at down = {down}, px = {px}: nothing is timed")
        if px:
            arms = {"flat": Rotating(flat, slides), "px_plain": Rotating(hip(), slides), "px_smooth": Rotating(hip(True), slides),
                    "px_mask": Rotating(hip(False, True), slides), "px_both": Rotating(most, slides), "B_torch": Rotating(tor, slides)}
        else:
            arms = {"A_hip_rot": Rotating(flat, slides), "B_torch_rot": Rotating(tor, slides),
                    "A_hip_same": lambda: flat(slides[0]), "B_torch_same": lambda: tor(slides[0])}
        t, iters = alternate(arms, seconds)
        nbytes = 3 * HR * WR + 3 * (HR // down) * (WR // down)
        a = t["flat" if px else "A_hip_rot"]
        a1, a2 = median(a[0::2]), median(a[1::2])
        halves, spread = [round(a1, 5), round(a2, 5)], round(abs(a1 - a2) / median(a), 4)
        rec = dict(kind="resident_heatmap_px" if px else "resident_heatmap", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, down=down, alpha=ALPHA,
                   moved_bytes=nbytes, slides_rotated=len(slides), rounds=len(a), iters_per_round=iters,
                   ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                   ms_max={k: round(max(v), 5) for k, v in t.items()}, moved_tbps={k: round(nbytes / median(v) / 1e9, 3) for k, v in t.items()})
        if px:
            changed = float((most(slides[0]).clone() != flat(slides[0])).any(dim=2).float().mean())
            rec.update(mask_down=MASK_DOWN, pixels_changed_vs_flat=round(changed, 4), flat_halves_ms=halves, flat_spread=spread,
                       px_over_flat={k: round(median(t[k]) / median(a), 4) for k in ("px_plain", "px_smooth", "px_mask", "px_both")},
                       torch_over_px_both=round(median(t["B_torch"]) / median(t["px_both"]), 2), px_equals_torch=same, px_plain_equals_flat=same_flat)
        else:
            covered = float((ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR)) >= 0).float().mean())
            rec.update(tiles=NX * NY, covered_cells=round(covered, 4), arm_a_halves_ms=halves, arm_a_spread=spread,
                       b_over_a_rot=round(median(t["B_torch_rot"]) / median(a), 2),
                       b_over_a_same=round(median(t["B_torch_same"]) / median(t["A_hip_same"]), 2), hip_equals_torch=same)
        res.append(rec)
        del out
    return res


THUMB_MASK_DOWN = 32


def thumb(seconds):
    """The --thumb figures: one record per down in ops.HEAT_THUMB_DOWNS."""
    import torch.nn.functional as F
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    masks = {s.data_ptr(): segment_tissue(s, THUMB_MASK_DOWN, 7, 8) for s in slides}
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    out4 = torch.empty((HR // 4, WR // 4, 3), dtype=torch.uint8, device=dev)
    res = []
    for down in ops.HEAT_THUMB_DOWNS:
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        plane = torch.empty((HR // down, WR // down), dtype=torch.uint8, device=dev)

        def t_flat(r):
            return ops.region_heat_thumb(r, cells, CELL, lut, ALPHA, down, out=out)

        def t_both(r):
            m, t = masks[r.data_ptr()]
            return ops.region_heat_thumb(r, cells, CELL, lut, ALPHA, down, smooth=True, mask=m, mask_down=THUMB_MASK_DOWN, mask_thresh=t, out=out)

        def sat(r):
            return ops.region_saturation(r, down, out=plane)

        def parent(r):
            m, t = masks[r.data_ptr()]
            c4 = ops.region_heat_blend_px(r, cells, CELL, lut, ALPHA, 4, smooth=True, mask=m, mask_down=THUMB_MASK_DOWN, mask_thresh=t, out=out4)
            return F.avg_pool2d(c4.permute(2, 0, 1).unsqueeze(0).float(), down // 4).add_(0.5).floor_().to(torch.uint8).squeeze(0).permute(1, 2, 0)

        same_flat = all(bool(torch.equal(t_flat(s), torch_canvas(s, table, lut, down))) for s in slides)
        same_both = all(bool(torch.equal(t_both(s), torch_canvas(s, table, lut, down, True, masks[s.data_ptr()], THUMB_MASK_DOWN))) for s in slides)
        if not (same_flat and same_both):                                      # a wrong arm must not produce a quoted ratio
            raise SystemExit(f"heatmap_bench: region_heat_thumb differs from the torch statement of the definition at down = {down} (flat {same_flat}, "
                             f"smooth + mask {same_both}): nothing is timed")
        changed = float((t_both(slides[0]).clone() != t_flat(slides[0])).any(dim=2).float().mean())
        p_differs = float((parent(slides[0]) != t_both(slides[0])).any(dim=2).float().mean())
        arms = {"T_flat": Rotating(t_flat, slides), "T_both": Rotating(t_both, slides), "S": Rotating(sat, slides), "P": Rotating(parent, slides)}
        t, iters = alternate(arms, seconds)
        nbytes = 3 * HR * WR + 3 * (HR // down) * (WR // down)
        sv = t["S"]
        s1, s2 = median(sv[0::2]), median(sv[1::2])
        spread = abs(s1 - s2) / median(sv)
        t_over_s = {k: round(median(t[k]) / median(sv), 4) for k in ("T_flat", "T_both")}
        res.append(dict(kind="resident_heatmap_thumb", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, down=down, alpha=ALPHA, mask_down=THUMB_MASK_DOWN,
                        moved_bytes=nbytes, slides_rotated=len(slides), rounds=len(sv), iters_per_round=iters,
                        ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                        ms_max={k: round(max(v), 5) for k, v in t.items()},
                        moved_tbps={k: round(nbytes / median(t[k]) / 1e9, 3) for k in ("T_flat", "T_both")},
                        s_read_tbps=round(3 * HR * WR / median(sv) / 1e9, 3), s_halves_ms=[round(s1, 5), round(s2, 5)], s_spread=round(spread, 4),
                        t_over_s=t_over_s, t_exceeds_s_beyond_spread={k: bool(v > 1.0 + spread) for k, v in t_over_s.items()},
                        p_over_t_both=round(median(t["P"]) / median(t["T_both"]), 3), thumb_equals_torch=same_flat and same_both,
                        pixels_changed_vs_flat=round(changed, 4), p_pixels_differing_from_t=round(p_differs, 4), p_is_bit_equal=False))
        del out, plane
    return res


BLUR_TABLES = ((GY, GX), (1563, 1563))
BLUR_RADII = (8, 15)


def torch_blur(cells, taps):
    """ops.heat_cells_blur in torch device ops: the definition of include/toad_hip.h, separably, in float64 (every sum is an integer below 2^53)."""
    import torch.nn.functional as F
    r = len(taps) - 1
    w = torch.tensor(list(taps[:0:-1]) + list(taps), dtype=torch.float64, device=cells.device)
    p = cells >= 0
    x = torch.stack([cells.clamp(0, 255) * p, p.to(cells.dtype)]).unsqueeze(1).to(torch.float64)      # [2,1,Gy,Gx]: v p and p
    x = F.conv2d(F.conv2d(x, w.view(1, 1, 1, -1), padding=(0, r)), w.view(1, 1, -1, 1), padding=(r, 0))
    n, d = x[0, 0].to(torch.int64), x[1, 0].to(torch.int64)
    return torch.where(p, (2 * n + d) // (2 * d).clamp(min=1), torch.full_like(n, -1)).to(torch.int32)


def blur(seconds):
    """The --blur figures: one record per (table, radius), then one per canvas down."""
    import numpy as np
    from toad_amd.heatmap import attention_canvas, gaussian_taps
    dev = torch.device("cuda:0")
    res = []
    for gy, gx in BLUR_TABLES:
        ny, nx = gy - TILE // CELL + 1, gx - TILE // CELL + 1
        g = torch.Generator().manual_seed(gy + gx)
        q = torch.randint(0, 65536, (ny, nx), generator=g, dtype=torch.int32)
        table = torch.where(torch.rand(ny, nx, generator=g) < 0.5, q, torch.full_like(q, -1)).to(dev)
        build = lambda: ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (nx, ny), (gy * CELL, gx * CELL))      # noqa: E731
        cells = build()
        hole = torch.rand(gy, gx, generator=g).to(dev) < 0.3        # coverage 4 x 4 at this stride leaves few cells absent: take a third out
        cells = torch.where(hole, torch.full_like(cells, -1), cells).contiguous()
        for radius in BLUR_RADII:
            taps = gaussian_taps(radius / 3.0, radius)
            same = bool(torch.equal(ops.heat_cells_blur(cells, taps), torch_blur(cells, taps)))
            if not same:                                                       # a wrong arm must not produce a quoted ratio
                raise SystemExit(f"heatmap_bench: heat_cells_blur differs from its torch arm on {gy} x {gx} cells at radius {radius}: nothing is timed")
            arms = {"A_hip": lambda: ops.heat_cells_blur(cells, taps), "B_torch": lambda: torch_blur(cells, taps), "cells": build}
            t, iters = alternate(arms, seconds)
            a = t["A_hip"]
            a1, a2 = median(a[0::2]), median(a[1::2])
            res.append(dict(kind="heat_cells_blur", table=[gy, gx], radius=radius, taps=list(taps), absent_cells=round(float((cells < 0).float().mean()), 4),
                            rounds=len(a), iters_per_round=iters, ms={k: round(median(v), 5) for k, v in t.items()},
                            ms_min={k: round(min(v), 5) for k, v in t.items()}, ms_max={k: round(max(v), 5) for k, v in t.items()},
                            a_halves_ms=[round(a1, 5), round(a2, 5)], a_spread=round(abs(a1 - a2) / median(a), 4),
                            a_over_cells=round(median(a) / median(t["cells"]), 3), b_over_a=round(median(t["B_torch"]) / median(a), 2),
                            cells_per_us_a=round(gy * gx / median(a) / 1e3, 1), hip_equals_torch=same))
    slides, table, lut = setup(dev)
    present = (table >= 0).cpu().numpy()
    jj, ii = np.nonzero(present)
    origins = np.stack([ii * STRIDE, jj * STRIDE], axis=1).astype(np.int64)
    scores = (table[table >= 0].float() / 65535).contiguous()
    lat = dict(tile=TILE, stride=STRIDE)
    taps = gaussian_taps((0.6 * TILE + 0.5) / CELL)
    for down in (1, 16):
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        blend = ops.region_heat_thumb if down in ops.HEAT_THUMB_DOWNS else ops.region_heat_blend_px

        def launches_only(r, blurred):
            c = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
            return blend(r, ops.heat_cells_blur(c, taps) if blurred else c, CELL, lut, ALPHA, down, out=out)

        plain = lambda r: attention_canvas(r, origins, scores, down=down, out=out, **lat)                   # noqa: E731
        blurred = lambda r: attention_canvas(r, origins, scores, down=down, out=out, blur=True, **lat)      # noqa: E731
        differs = float((blurred(slides[0]).clone() != plain(slides[0])).any(dim=2).float().mean())
        same = all(bool(torch.equal(blurred(s).clone(), launches_only(s, True))) and bool(torch.equal(plain(s).clone(), launches_only(s, False))) for s in slides)
        if not (same and differs > 0):
            raise SystemExit(f"heatmap_bench: attention_canvas and its launches disagree at down = {down} ({same}), or blur=True changed nothing: nothing is timed")
        arms = {"canvas_plain": Rotating(plain, slides), "canvas_blur": Rotating(blurred, slides),
                "launches_plain": Rotating(lambda r: launches_only(r, False), slides), "launches_blur": Rotating(lambda r: launches_only(r, True), slides)}
        t, iters = alternate(arms, seconds)
        a = t["launches_plain"]
        a1, a2 = median(a[0::2]), median(a[1::2])
        res.append(dict(kind="resident_heatmap_blur", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, down=down, alpha=ALPHA, taps=list(taps),
                        tiles_present=int(len(origins)), slides_rotated=len(slides), rounds=len(a), iters_per_round=iters,
                        ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                        ms_max={k: round(max(v), 5) for k, v in t.items()}, launches_plain_halves_ms=[round(a1, 5), round(a2, 5)],
                        launches_plain_spread=round(abs(a1 - a2) / median(a), 4),
                        blur_extra_ms={"canvas": round(median(t["canvas_blur"]) - median(t["canvas_plain"]), 5),
                                       "launches": round(median(t["launches_blur"]) - median(a), 5)},
                        blur_over_plain={"canvas": round(median(t["canvas_blur"]) / median(t["canvas_plain"]), 4),
                                         "launches": round(median(t["launches_blur"]) / median(a), 4)},
                        pixels_changed_by_blur=round(differs, 4), canvas_equals_launches=same))
        del out
    return res


def window(seconds, w0_only=False):
    """The --window figures: one record per (down, flat | smooth + mask)."""
    import ctypes
    from toad_amd import _lib
    name = "toad_region_heat_window_u8"
    parent = not hasattr(ctypes.CDLL(_lib.LIB_PATH), name)          # a library from before the entry: W0 alone
    if parent:
        if tools.ab.select_lib.TAG == "(shipped)":
            raise SystemExit(f"heatmap_bench: the shipped library does not export {name}: rebuild (python -m toad_amd.build --force)")
        del _lib.SIGNATURES[name]                                    # this process only: the loader binds every symbol it knows
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    strips = [(0, y, WR, HR // 4) for y in range(0, HR, HR // 4)]
    blocks = [(x, y, WR // 4, HR // 4) for y in range(0, HR, HR // 4) for x in range(0, WR, WR // 4)]
    res = []
    for down in (1, 16):
        md = MASK_DOWN if down == 1 else THUMB_MASK_DOWN
        masks = {s.data_ptr(): segment_tissue(s, md, 7, 8) for s in slides}
        whole = ops.region_heat_thumb if down in ops.HEAT_THUMB_DOWNS else ops.region_heat_blend_px
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        for both in (False, True):
            def kw(r):
                if not both:
                    return {}
                m, t = masks[r.data_ptr()]
                return dict(smooth=True, mask=m, mask_down=md, mask_thresh=t)

            def w0(r):
                return whole(r, cells, CELL, lut, ALPHA, down, out=out, **kw(r))

            def pieces(parts):
                def run(r):
                    k = kw(r)
                    for wx, wy, w, h in parts:
                        ops.region_heat_window(r[wy:wy + h, wx:wx + w], (wx, wy), cells, CELL, lut, ALPHA, down,
                                               out=out[wy // down:(wy + h) // down, wx // down:(wx + w) // down], **k)
                    return out
                return run

            arms = {"W0": Rotating(w0, slides)}
            if not parent and not w0_only:
                cand = {"W1": pieces([(0, 0, WR, HR)]), "W4": pieces(strips), "W16": pieces(blocks)}
                for s_ in slides:
                    want = w0(s_).clone()
                    for k, fn in cand.items():
                        out.fill_(0x7F)
                        if not torch.equal(fn(s_), want):                      # a wrong arm must not produce a quoted ratio
                            raise SystemExit(f"heatmap_bench: {k} differs from W0 at down = {down}, smooth + mask = {both}: nothing is timed")
                arms.update({k: Rotating(fn, slides) for k, fn in cand.items()})
            t, iters = alternate(arms, seconds)
            a = t["W0"]
            a1, a2 = median(a[0::2]), median(a[1::2])
            nbytes = 3 * HR * WR + 3 * (HR // down) * (WR // down)
            rec = dict(kind="resident_heatmap_window" + ("_w0" if parent or w0_only else ""), lib=tools.ab.select_lib.TAG, region=[HR, WR], tile=TILE, stride=STRIDE,
                       cell=CELL, down=down, alpha=ALPHA, smooth_and_mask=both, mask_down=md if both else None, moved_bytes=nbytes, slides_rotated=len(slides),
                       rounds=len(a), iters_per_round=iters, ms={k: round(median(v), 5) for k, v in t.items()},
                       ms_min={k: round(min(v), 5) for k, v in t.items()}, ms_max={k: round(max(v), 5) for k, v in t.items()},
                       moved_tbps={k: round(nbytes / median(v) / 1e9, 3) for k, v in t.items()}, w0_halves_ms=[round(a1, 5), round(a2, 5)],
                       w0_spread=round(abs(a1 - a2) / median(a), 4))
            if not parent and not w0_only:
                over = {k: round(median(t[k]) / median(a), 4) for k in ("W1", "W4", "W16")}
                rec.update(w_over_w0=over, w1_exceeds_w0_beyond_spread=bool(over["W1"] > 1.0 + rec["w0_spread"]), launches={"W0": 1, "W1": 1, "W4": 4, "W16": 16},
                           windows_equal_w0=True)
            res.append(rec)
        del out
    return res


def windows(seconds):
    """The --windows figures: one record per (down, flat | smooth + mask)."""
    from toad_amd import _lib
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    strips = [(0, y, WR, HR // 4) for y in range(0, HR, HR // 4)]
    blocks = [(x, y, WR // 4, HR // 4) for y in range(0, HR, HR // 4) for x in range(0, WR, WR // 4)]
    res = []
    for down in (1, 16):
        md = MASK_DOWN if down == 1 else THUMB_MASK_DOWN
        masks = {s.data_ptr(): segment_tissue(s, md, 7, 8) for s in slides}
        whole = ops.region_heat_thumb if down in ops.HEAT_THUMB_DOWNS else ops.region_heat_blend_px
        out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
        for both in (False, True):
            def kw(r):
                if not both:
                    return {}
                m, t = masks[r.data_ptr()]
                return dict(smooth=True, mask=m, mask_down=md, mask_thresh=t)

            def w0(r):
                return whole(r, cells, CELL, lut, ALPHA, down, out=out, **kw(r))

            def pieces(parts):
                def run(r):
                    k = kw(r)
                    for wx, wy, w, h in parts:
                        ops.region_heat_window(r[wy:wy + h, wx:wx + w], (wx, wy), cells, CELL, lut, ALPHA, down,
                                               out=out[wy // down:(wy + h) // down, wx // down:(wx + w) // down], **k)
                    return out
                return run

            def listed(parts):
                places = [(wx, wy) for wx, wy, _, _ in parts]
                outs = [out[wy // down:(wy + h) // down, wx // down:(wx + w) // down] for wx, wy, w, h in parts]

                def run(r):
                    ops.region_heat_windows([r[wy:wy + h, wx:wx + w] for wx, wy, w, h in parts], places, cells, CELL, lut, ALPHA, down, outs=outs, **kw(r))
                    return out
                return run

            def direct(parts):
                lib, win = _lib.load(), _lib.ToadHeatWindow
                hosts = {s_.data_ptr(): (win * len(parts))(*(win(s_[wy:wy + h, wx:wx + w].data_ptr(), s_.stride(0), h, w, wx, wy,
                                                                   out[wy // down:, wx // down:].data_ptr(), out.stride(0)) for wx, wy, w, h in parts))
                         for s_ in slides}

                def run(r):
                    m, t = masks[r.data_ptr()] if both else (None, 0)
                    plane = (m.data_ptr(), m.stride(0), m.shape[0], m.shape[1], md, t) if both else (None, 0, 0, 0, 0, 0)
                    _lib.check(lib.toad_region_heat_windows_u8(hosts[r.data_ptr()], len(parts), cells.data_ptr(), GY, GX, CELL, lut.data_ptr(), ALPHA, down, int(both),
                                                               *plane, ops._stream()), "toad_region_heat_windows_u8")
                    return out
                return run

            cand = {"W4": pieces(strips), "W16": pieces(blocks), "L4": listed(strips), "L16": listed(blocks), "C4": direct(strips), "C16": direct(blocks)}
            for s_ in slides:
                want = w0(s_).clone()
                for k, fn in cand.items():
                    out.fill_(0x7F)
                    if not torch.equal(fn(s_), want):                          # a wrong arm must not produce a quoted ratio
                        raise SystemExit(f"heatmap_bench: {k} differs from W0 at down = {down}, smooth + mask = {both}: nothing is timed")
            arms = {"W0": Rotating(w0, slides)}
            arms.update({k: Rotating(fn, slides) for k, fn in cand.items()})
            t, iters = alternate(arms, seconds)
            a = t["W0"]
            a1, a2 = median(a[0::2]), median(a[1::2])
            spread = abs(a1 - a2) / median(a)
            nbytes = 3 * HR * WR + 3 * (HR // down) * (WR // down)
            m = {k: median(v) for k, v in t.items()}
            l_over_w = {"L4": m["L4"] / m["W4"], "L16": m["L16"] / m["W16"]}
            res.append(dict(kind="resident_heatmap_windows", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, down=down, alpha=ALPHA, smooth_and_mask=both,
                            mask_down=md if both else None, moved_bytes=nbytes, slides_rotated=len(slides), rounds=len(a), iters_per_round=iters,
                            ms={k: round(v, 5) for k, v in m.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                            ms_max={k: round(max(v), 5) for k, v in t.items()}, moved_tbps={k: round(nbytes / v / 1e9, 3) for k, v in m.items()},
                            w0_halves_ms=[round(a1, 5), round(a2, 5)], w0_spread=round(spread, 4), l_over_w={k: round(v, 4) for k, v in l_over_w.items()},
                            l_faster_beyond_spread={k: bool(v < 1.0 - spread) for k, v in l_over_w.items()},
                            l_over_w0={k: round(m[k] / m["W0"], 4) for k in ("L4", "L16")}, c_over_w0={k: round(m[k] / m["W0"], 4) for k in ("C4", "C16")}, w_over_w0={k: round(m[k] / m["W0"], 4) for k in ("W4", "W16")},
                            launches={"W0": 1, "W4": 4, "W16": 16, "L4": 1, "L16": 1, "C4": 1, "C16": 1}, lists_equal_w0=True))
        del out
    return res


PYRAMID_SETS = ((1, 4, 16), (1, 2, 4, 8, 16, 32), (8, 16, 32))


def pyramid(seconds):
    """The --pyramid figures: one record per (level set, flat | smooth + mask)."""
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    out1 = torch.empty((HR, WR, 3), dtype=torch.uint8, device=dev)
    res = []
    for ds in PYRAMID_SETS:
        md = MASK_DOWN if max(ds) <= MASK_DOWN else THUMB_MASK_DOWN
        masks = {s.data_ptr(): segment_tissue(s, md, 7, 8) for s in slides}
        outs_p = [torch.empty((HR // d, WR // d, 3), dtype=torch.uint8, device=dev) for d in ds]
        outs_s = [torch.empty_like(o) for o in outs_p]
        for both in (False, True):
            def kw(r):
                if not both:
                    return {}
                m, t = masks[r.data_ptr()]
                return dict(smooth=True, mask=m, mask_down=md, mask_thresh=t)

            def arm_p(r):
                return ops.region_heat_pyramid(r, (0, 0), cells, CELL, lut, ALPHA, ds, outs=outs_p, **kw(r))

            def arm_s(r):
                k = kw(r)
                for d, o in zip(ds, outs_s):
                    ops.region_heat_window(r, (0, 0), cells, CELL, lut, ALPHA, d, out=o, **k)
                return outs_s

            def arm_l1(r):
                return ops.region_heat_window(r, (0, 0), cells, CELL, lut, ALPHA, 1, out=out1, **kw(r))

            for s_ in slides:
                for o in outs_p:
                    o.fill_(0x7F)
                got, want = arm_p(s_), arm_s(s_)
                if not all(torch.equal(g, w) for g, w in zip(got, want)):          # a wrong arm must not produce a quoted ratio
                    raise SystemExit(f"heatmap_bench: the pyramid differs from the per-level calls for levels {ds}, smooth + mask = {both}: nothing is timed")
            t, iters = alternate({"P": Rotating(arm_p, slides), "S": Rotating(arm_s, slides), "L1": Rotating(arm_l1, slides)}, seconds)
            sv = t["S"]
            s1, s2 = median(sv[0::2]), median(sv[1::2])
            spread = abs(s1 - s2) / median(sv)
            written = sum(3 * (HR // d) * (WR // d) for d in ds)
            nbytes, sbytes = 3 * HR * WR + written, len(ds) * 3 * HR * WR + written
            p_over_s = median(t["P"]) / median(sv)
            res.append(dict(kind="resident_heatmap_pyramid", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, levels=list(ds), alpha=ALPHA, smooth_and_mask=both,
                            mask_down=md if both else None, moved_bytes=nbytes, s_moved_bytes=sbytes, slides_rotated=len(slides), rounds=len(sv), iters_per_round=iters,
                            ms={k: round(median(v), 5) for k, v in t.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                            ms_max={k: round(max(v), 5) for k, v in t.items()}, p_moved_tbps=round(nbytes / median(t["P"]) / 1e9, 3),
                            s_moved_tbps=round(sbytes / median(sv) / 1e9, 3), s_halves_ms=[round(s1, 5), round(s2, 5)], s_spread=round(spread, 4),
                            p_over_s=round(p_over_s, 4), p_faster_beyond_spread=bool(p_over_s < 1.0 - spread), p_over_l1=round(median(t["P"]) / median(t["L1"]), 4),
                            launches={"P": 1, "S": len(ds), "L1": 1}, pyramid_equals_levels=True))
        del outs_p, outs_s
    return res


PYRAMID_WINDOWS_SETS = ((1, 4, 16), (1, 2, 4, 8, 16, 32))


def pyramid_windows(seconds):
    """The --pyramid-windows figures: one record per (level set, flat | smooth + mask)."""
    from toad_amd import _lib
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    cells = ops.heat_cells(table, CELL, (0, 0), (TILE, TILE), (STRIDE, STRIDE), (NX, NY), (HR, WR))
    strips = [(0, y, WR, HR // 4) for y in range(0, HR, HR // 4)]
    blocks = [(x, y, WR // 4, HR // 4) for y in range(0, HR, HR // 4) for x in range(0, WR, WR // 4)]
    res = []
    for ds in PYRAMID_WINDOWS_SETS:
        md = MASK_DOWN if max(ds) <= MASK_DOWN else THUMB_MASK_DOWN
        masks = {s.data_ptr(): segment_tissue(s, md, 7, 8) for s in slides}
        outs = [torch.empty((HR // d, WR // d, 3), dtype=torch.uint8, device=dev) for d in ds]
        bits = sum(ds)
        for both in (False, True):
            def kw(r):
                if not both:
                    return {}
                m, t = masks[r.data_ptr()]
                return dict(smooth=True, mask=m, mask_down=md, mask_thresh=t)

            def views(wx, wy, w, h):
                return [o[wy // d:(wy + h) // d, wx // d:(wx + w) // d] for d, o in zip(ds, outs)]

            def arm_p(r):
                return ops.region_heat_pyramid(r, (0, 0), cells, CELL, lut, ALPHA, ds, outs=outs, **kw(r))

            def pieces(parts):
                def run(r):
                    k = kw(r)
                    for wx, wy, w, h in parts:
                        ops.region_heat_pyramid(r[wy:wy + h, wx:wx + w], (wx, wy), cells, CELL, lut, ALPHA, ds, outs=views(wx, wy, w, h), **k)
                    return outs
                return run

            def listed(parts):
                places = [(wx, wy) for wx, wy, _, _ in parts]
                vs = [views(*p) for p in parts]

                def run(r):
                    ops.region_heat_pyramid_windows([r[wy:wy + h, wx:wx + w] for wx, wy, w, h in parts], places, cells, CELL, lut, ALPHA, ds, outs=vs, **kw(r))
                    return outs
                return run

            def direct(parts):
                lib, win = _lib.load(), _lib.ToadHeatPyramidWindow
                hosts = {}
                for s_ in slides:
                    host = (win * len(parts))()
                    for desc, (wx, wy, w, h) in zip(host, parts):
                        desc.region, desc.pitch, desc.Hr, desc.Wr, desc.wx, desc.wy = s_[wy:wy + h, wx:wx + w].data_ptr(), s_.stride(0), h, w, wx, wy
                        for d, o in zip(ds, outs):
                            desc.outs[d.bit_length() - 1], desc.out_pitches[d.bit_length() - 1] = o[wy // d:, wx // d:].data_ptr(), o.stride(0)
                    hosts[s_.data_ptr()] = host

                def run(r):
                    m, t = masks[r.data_ptr()] if both else (None, 0)
                    plane = (m.data_ptr(), m.stride(0), m.shape[0], m.shape[1], md, t) if both else (None, 0, 0, 0, 0, 0)
                    _lib.check(lib.toad_region_heat_pyramid_windows_u8(hosts[r.data_ptr()], len(parts), cells.data_ptr(), GY, GX, CELL, lut.data_ptr(), ALPHA, bits,
                                                                       int(both), *plane, ops._stream()), "toad_region_heat_pyramid_windows_u8")
                    return outs
                return run

            cand = {"PW4": pieces(strips), "PW16": pieces(blocks), "PL4": listed(strips), "PL16": listed(blocks), "CL4": direct(strips), "CL16": direct(blocks)}
            for s_ in slides:
                want = [o.clone() for o in arm_p(s_)]
                for k, fn in cand.items():
                    for o in outs:
                        o.fill_(0x7F)
                    if not all(torch.equal(g, w) for g, w in zip(fn(s_), want)):      # a wrong arm must not produce a quoted ratio
                        raise SystemExit(f"heatmap_bench: {k} differs from P for levels {ds}, smooth + mask = {both}: nothing is timed")
            arms = {"P": Rotating(arm_p, slides)}
            arms.update({k: Rotating(fn, slides) for k, fn in cand.items()})
            t, iters = alternate(arms, seconds)
            a = t["P"]
            a1, a2 = median(a[0::2]), median(a[1::2])
            spread = abs(a1 - a2) / median(a)
            nbytes = 3 * HR * WR + sum(3 * (HR // d) * (WR // d) for d in ds)
            m = {k: median(v) for k, v in t.items()}
            pl_over_pw = {"PL4": m["PL4"] / m["PW4"], "PL16": m["PL16"] / m["PW16"]}
            res.append(dict(kind="resident_heatmap_pyramid_windows", region=[HR, WR], tile=TILE, stride=STRIDE, cell=CELL, levels=list(ds), alpha=ALPHA,
                            smooth_and_mask=both, mask_down=md if both else None, moved_bytes=nbytes, slides_rotated=len(slides), rounds=len(a), iters_per_round=iters,
                            ms={k: round(v, 5) for k, v in m.items()}, ms_min={k: round(min(v), 5) for k, v in t.items()},
                            ms_max={k: round(max(v), 5) for k, v in t.items()}, moved_tbps={k: round(nbytes / v / 1e9, 3) for k, v in m.items()},
                            p_halves_ms=[round(a1, 5), round(a2, 5)], p_spread=round(spread, 4), pl_over_pw={k: round(v, 4) for k, v in pl_over_pw.items()},
                            pl_faster_beyond_spread={k: bool(v < 1.0 - spread) for k, v in pl_over_pw.items()},
                            pl_over_p={k: round(m[k] / m["P"], 4) for k in ("PL4", "PL16")}, cl_over_p={k: round(m[k] / m["P"], 4) for k in ("CL4", "CL16")},
                            pw_over_p={k: round(m[k] / m["P"], 4) for k in ("PW4", "PW16")},
                            launches={"P": 1, "PW4": 4, "PW16": 16, "PL4": 1, "PL16": 1, "CL4": 1, "CL16": 1}, lists_equal_p=True))
        del outs
    return res


def launches(arm, down, calls=4):
    """`calls` calls of one arm on rotating slides, no warm-up (run under rocprofv3 --kernel-trace --stats: every count divides by `calls`)."""
    dev = torch.device("cuda:0")
    slides, table, lut = setup(dev)
    out = torch.empty((HR // down, WR // down, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for i in range(calls):
        hip_canvas(slides[i % 4], table, lut, down, out, px=False) if arm == "A" else torch_canvas(slides[i % 4], table, lut, down)
    torch.cuda.synchronize()
    return [dict(kind="launches_heatmap", calls=calls, arm=arm, down=down)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--arm", default="A", choices=("A", "B"))
    ap.add_argument("--down", type=int, default=1, choices=(1, 2, 4))
    ap.add_argument("--px", action="store_true")
    ap.add_argument("--thumb", action="store_true")
    ap.add_argument("--blur", action="store_true")
    ap.add_argument("--window", action="store_true")
    ap.add_argument("--w0-only", action="store_true")
    ap.add_argument("--windows", action="store_true")
    ap.add_argument("--pyramid", action="store_true")
    ap.add_argument("--pyramid-windows", action="store_true")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.blur and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heatmap_blur_bench.jsonl")
    if a.window and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heatmap_window_bench.jsonl")
    if a.windows and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heatmap_windows_bench.jsonl")
    if a.pyramid and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heatmap_pyramid_bench.jsonl")
    if a.pyramid_windows and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heatmap_pyramid_windows_bench.jsonl")
    res = launches(a.arm, a.down) if a.launches else pyramid_windows(a.seconds) if a.pyramid_windows else windows(a.seconds) if a.windows else pyramid(a.seconds) if a.pyramid else window(a.seconds, a.w0_only) if a.window else blur(a.seconds) if a.blur else thumb(a.seconds) if a.thumb else resident(a.seconds, a.px)
    lines = [json.dumps(r) for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
