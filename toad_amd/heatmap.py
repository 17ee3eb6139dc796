"""Attention heat maps on the device: from the scores of the tiles of one decoded uint8 region to the canvas a pathologist looks at, rendered where the
region lies (csrc/heatmap.hip). The stage behind ``eval.region_tissue_attention_scores``; the mirror image of ``toad_amd.tissue``.

CLAM draws its heat maps on the host: ``overlay[y:y+h, x:x+w] += score; counter[...] += 1``, divide, colour-map, ``addWeighted``. The same here, defined in
integers so that the canvas has one right answer:

* a score becomes ``q = round(clamp((s - lo) / (hi - lo), 0, 1) * 65535)``, and a NaN score makes its tile absent;
* a ``cell x cell`` cell (``tissue.lattice_cell``) covered by ``n`` present tiles whose ``q`` sum to ``S`` gets the colour index
  ``(2 S + 257 n) // (514 n)``, which is ``255 mean(q) / 65535`` rounded half up; a cell no present tile covers gets none;
* the canvas is the region box-filtered by ``down`` in 1, 2, 4 (mean rounded half up, partial boxes at the right and the bottom edge dropped), and on the
  cells with a colour ``(alpha lut[idx][c] + (256 - alpha) m + 128) >> 8`` with an integer ``alpha`` in [0, 256].

Conventions as in ``toad_amd.tissue``: ``tile`` = int or (H, W), ``stride`` = int or (sy, sx), ``origin`` = (x, y) of the lattice's first tile.
Gaussian smoothing, CLAM's vis-level pyramid and saving images are not done here."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .tissue import _lattice_args, lattice, lattice_cell


_JET = {}


def jet_lut(device) -> torch.Tensor:
    """The default colours, uint8 [256,3] on ``device``: an integer "jet" - channel k of entry i is ``clamp(765 - |8 i - 510 k|, 0, 510) // 2`` with
    k = 3, 2, 1 for r, g, b - from (0, 0, 127) over blue, cyan, green, yellow and red to (127, 0, 0). No matplotlib. Built and uploaded once per
    device; the tensor is shared between calls and must not be written to."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    lut = _JET.get(device)
    if lut is None:
        i = np.arange(256, dtype=np.int64)[:, None]
        k = np.array([3, 2, 1], dtype=np.int64)[None, :]
        lut = _JET[device] = torch.from_numpy((np.clip(765 - np.abs(8 * i - 510 * k), 0, 510) // 2).astype(np.uint8)).to(device)
    return lut


def quantise_scores(scores: torch.Tensor, score_range=(0, 1)) -> torch.Tensor:
    """int32 [B] on the scores' device: ``round(clamp((s - lo) / (hi - lo), 0, 1) * 65535)``, and -1 (absent) for a NaN score. The default range skips
    the subtraction and the division: exactly ``torch.round(s.clamp(0, 1) * 65535)``, what the percentile scores of ``eval`` need. Torch ops only."""
    lo, hi = score_range
    if not hi > lo:
        raise ValueError(f"score_range must be (lo, hi) with lo < hi, got {score_range!r}")
    s = scores.reshape(-1).to(torch.float32)
    if (lo, hi) != (0, 1):
        s = (s - lo) / (hi - lo)
    q = torch.round(s.clamp(0, 1) * 65535)
    return torch.where(torch.isnan(q), torch.full_like(q, -1), q).to(torch.int32)


def tile_table(origins, scores_q: torch.Tensor, tile, stride, origin, n) -> torch.Tensor:
    """The tile table of the heat-map kernels, int32 [ny,nx] on the device of ``scores_q``: -1 everywhere except at the tiles of ``origins`` ([B,2] of
    (x, y) on the host, as ``tissue.tissue_origins`` returns them), which take their ``scores_q``. Host arithmetic maps each (x, y) to its lattice index
    j nx + i and raises ValueError for an origin off the lattice, outside it or given twice; then one index upload and one scatter, deterministic
    because no index repeats. n = (nx, ny)."""
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    nx, ny = n
    o = np.asarray(origins)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError(f"origins must be [B,2] integers (x, y), got shape {o.shape} dtype {o.dtype}")
    o = o.astype(np.int64)
    if scores_q.dim() != 1 or scores_q.shape[0] != o.shape[0] or scores_q.dtype != torch.int32:
        raise ValueError(f"scores_q must be int32 [{o.shape[0]}], one per origin, got {scores_q.dtype} {tuple(scores_q.shape)}")
    dx, dy = o[:, 0] - x0, o[:, 1] - y0
    i, j = dx // sx, dy // sy
    for name, bad in (("off the lattice", (dx % sx != 0) | (dy % sy != 0)), ("outside the lattice", (i < 0) | (i >= nx) | (j < 0) | (j >= ny))):
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise ValueError(f"origins[{b}] = (x={int(o[b, 0])}, y={int(o[b, 1])}) is {name}: origin ({x0}, {y0}), stride (sy, sx) = ({sy}, {sx}), "
                             f"{nx} x {ny} tiles (nx x ny)")
    idx = j * nx + i
    uniq, first = np.unique(idx, return_index=True)
    if uniq.size != idx.size:
        b = int(np.setdiff1d(np.arange(idx.size), first)[0])
        raise ValueError(f"origins[{b}] = (x={int(o[b, 0])}, y={int(o[b, 1])}) is given twice: a tile has one score")
    table = torch.full((ny * nx,), -1, dtype=torch.int32, device=scores_q.device)
    if idx.size:
        table[torch.from_numpy(idx).to(scores_q.device)] = scores_q
    return table.view(ny, nx)


def _alpha_arg(alpha) -> int:
    if isinstance(alpha, float) and 0.0 <= alpha <= 1.0:
        return int(round(256 * alpha))
    if isinstance(alpha, int) and not isinstance(alpha, bool) and 0 <= alpha <= 256:
        return alpha
    raise ValueError(f"alpha must be an int in [0, 256] or a float in [0, 1] (meaning round(256 alpha)), got {alpha!r}")


def attention_canvas(region: torch.Tensor, origins, scores: torch.Tensor, tile=256, stride=None, origin=(0, 0), alpha=102, down: int = 1, lut=None,
                     score_range=(0, 1), out=None) -> torch.Tensor:
    """The heat map of one decoded uint8 region [Hr,Wr,3]: uint8 [Hr // down, Wr // down, 3] ON THE DEVICE. ``origins`` [B,2] of (x, y) on the host are
    tiles of the lattice (tile, stride, origin) inside the region - ``tissue.tissue_origins`` with the same arguments gives such - and ``scores`` their B
    scores on the device, in that order. The definition is the module's. ``alpha`` an int in [0, 256] or a float in [0, 1] (the default 102 is CLAM's
    0.4), ``lut`` uint8 [256,3] on the device (default ``jet_lut``), ``out`` as in ``ops.region_heat_blend``.

    Two launches and a few small torch ops, no synchronisation. Empty ``origins`` give the box-filtered region."""
    _, hr, wr = ops._region_pitch(region, "attention_canvas")
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    a = _alpha_arg(alpha)
    if not isinstance(scores, torch.Tensor) or scores.device != region.device:
        raise ValueError(f"attention_canvas: scores must be a tensor on the region's device ({region.device}), got "
                         f"{scores.device if isinstance(scores, torch.Tensor) else type(scores).__name__}")
    nx, ny = lattice(hr, wr, (h, w), (sy, sx), (x0, y0))
    table = tile_table(origins, quantise_scores(scores, score_range), (h, w), (sy, sx), (x0, y0), (nx, ny))
    if table.numel() and len(origins):
        cells = ops.heat_cells(table, cell, (x0, y0), (h, w), (sy, sx), (nx, ny), (hr, wr))
    else:
        cells = torch.full((-(-hr // cell), -(-wr // cell)), -1, dtype=torch.int32, device=region.device)
    return ops.region_heat_blend(region, cells, cell, jet_lut(region.device) if lut is None else lut, a, down, out=out)
