"""Evaluation over the drop-in model: checkpoint loading, per-slide summary, top-k / AUC metrics, heat-map scores.

Reference: ``utils/eval_utils_mtl_concat.py`` — ``initiate_model`` (:19-32), ``eval`` (:34-46), ``accuracy``
(:49-63), ``summary`` (:65-177); ``attention_only`` scoring is ``models/model_toad.py:93-94`` as used by the
reference's heat-map scripts. Names, argument meaning and result keys follow the reference so that its
``eval_mtl_concat.py`` reads the same dictionaries; the forward pass is the HIP path (``TOAD_fc_mtl_concat``),
the metrics are host-side numpy / scikit-learn exactly like the reference's.

What differs from the reference: per-slide probabilities are collected on the device and read back once
(the reference synchronises 4+ times per slide through ``.item()`` / ``.cpu()``), and ``summary`` does not
raise ``NameError`` for ``n_classes == 2`` (the reference's ``topk`` is only bound for ``n_classes > 2``,
``eval_utils:125-131,174`` — here the top-k block is simply skipped, as the reference intends).
"""
from __future__ import annotations

import inspect
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from .model_toad import TOAD_fc_mtl_concat
from .train import AccuracyLogger, _to_device


def initiate_model(args, ckpt_path: Optional[str] = None) -> TOAD_fc_mtl_concat:
    """``eval_utils:19-32``: build from ``args.drop_out`` / ``args.n_classes``, relocate, load (non-strict), eval()."""
    model = TOAD_fc_mtl_concat(dropout=args.drop_out, n_classes=args.n_classes)
    model.relocate()
    if ckpt_path is not None:
        ckpt = torch.load(ckpt_path, map_location="cpu")
        # non-strict like the reference (eval_utils:28-29), but never silently partial: DataParallel-era keys
        # (``attention_net.module.*``) are renamed by the model's loader, and anything still missing is an error
        res = model.load_state_dict(ckpt, strict=False)
        if res.missing_keys:
            raise RuntimeError(f"{ckpt_path}: checkpoint lacks {len(res.missing_keys)} model tensors "
                               f"(e.g. {res.missing_keys[:3]}); refusing to evaluate a partly random model")
        if res.unexpected_keys:
            import warnings
            warnings.warn(f"{ckpt_path}: ignoring {len(res.unexpected_keys)} unexpected keys, e.g. {res.unexpected_keys[:3]}")
    model.eval()
    return model


def accuracy(output: torch.Tensor, target: torch.Tensor, topk: Sequence[int] = (1,)):
    """Top-k accuracy over rows of ``output`` (``eval_utils:49-63``); returns one 1-element tensor per k."""
    with torch.no_grad():
        maxk = max(topk)
        n = target.size(0)
        pred = output.topk(maxk, 1, True, True)[1].t()                    # [maxk, n]
        hit = pred.eq(target.view(1, -1).expand_as(pred))
        return [hit[:k].reshape(-1).float().sum(0, keepdim=True) * (1.0 / n) for k in topk]


def _cls_auc(labels: np.ndarray, probs: np.ndarray, n_classes: int, micro_average: bool):
    """``eval_utils:133-158``: (-1, []) for a single class present; binary -> AUC of column 1;
    multi-class -> per-class one-vs-rest AUCs (nan for absent classes) and their nan-mean, or the micro average."""
    from sklearn.metrics import auc, roc_auc_score, roc_curve
    from sklearn.preprocessing import label_binarize
    if len(np.unique(labels)) == 1:
        return -1, []
    if n_classes == 2:
        return float(roc_auc_score(labels, probs[:, 1])), []
    binary = label_binarize(labels, classes=list(range(n_classes)))
    aucs = []
    for c in range(n_classes):
        if c in labels:
            fpr, tpr, _ = roc_curve(binary[:, c], probs[:, c])
            aucs.append(float(auc(fpr, tpr)))
        else:
            aucs.append(float("nan"))
    if micro_average:
        valid = np.where(np.any(binary, axis=0))[0]
        fpr, tpr, _ = roc_curve(binary[:, valid].ravel(), probs[:, valid].ravel())
        return float(auc(fpr, tpr)), aucs
    return float(np.nanmean(np.array(aucs))), aucs


def forward_grouped(model, batches: Iterable, group_rows: int = 0):
    """Yield ``(batch, result_dict)`` in loader order for an iterable of ``(data, label, site, sex)`` device batches.
    Consecutive slides are collected until their patch counts reach ``group_rows`` and forwarded with ONE pass of the
    trunk GEMMs (``TOAD_fc_mtl_concat.forward_many``): a 256-patch slide costs as many kernel launches as a 100k-patch one,
    so the reference's per-slide loop (eval_utils_mtl_concat.py:88-91, core_utils_mtl_concat.py:281-284) is launch-bound on
    small bags. A slide that alone reaches ``group_rows`` goes through ``model(data, sex)``. DEFAULT ``group_rows = 0``: no grouping - the
    reference's one ``model(data, sex)`` per slide, whose numbers do not depend on which neighbours the loader put next to a slide.
    Grouping is opt-in (e.g. 131072: 17.6k instead of 6.7k slides/s on 128..4096-patch bags): the GEMM operand scales are taken per
    256-row block of the CONCATENATED bags, so grouped results agree with the per-slide ones to fp32 round-off (2e-5), not bitwise,
    and the group holds its bags plus their concatenation on the device."""
    pending, rows = [], 0

    def flush():
        if len(pending) == 1:
            b = pending[0]
            yield b, model(b[0], b[3])
        elif pending:
            for b, r in zip(pending, model.forward_many([b[0] for b in pending], [b[3] for b in pending])):
                yield b, r

    for b in batches:
        n = int(b[0].shape[0])
        if group_rows <= 0 or n == 0 or n >= group_rows or not hasattr(model, "forward_many"):
            yield from flush(); pending, rows = [], 0
            yield b, model(b[0], b[3])
            continue
        if rows + n > group_rows and pending:
            yield from flush(); pending, rows = [], 0
        pending.append(b); rows += n
    yield from flush()


@torch.no_grad()
def summary(model, loader: Iterable, args, slide_ids: Optional[Sequence] = None, group_rows: int = 0) -> Dict[str, object]:
    """Forward every slide once and tabulate (``eval_utils:65-177``).

    ``slide_ids`` defaults to ``loader.dataset.slide_data['slide_id']`` like the reference; pass a list when the
    loader is a plain iterable. ``group_rows`` > 0: consecutive slides are forwarded together (``forward_grouped``) until
    their patch counts add up to it; 0 keeps the reference's one ``model(data, sex)`` per slide. Returns the reference's keys: ``patient_results, cls_test_error, cls_auc,
    cls_aucs, site_test_error, site_auc, loggers, df`` and ``top{k}_acc``.
    """
    import pandas as pd
    device = next(model.parameters()).device
    n_classes = args.n_classes
    model.eval()
    cls_logger, site_logger = AccuracyLogger(n_classes, device), AccuracyLogger(2, device)
    if slide_ids is None:
        slide_ids = loader.dataset.slide_data["slide_id"]
    ids = list(slide_ids)
    probs, site_probs, labels, sites, sexes, y_hats, s_hats = [], [], [], [], [], [], []
    for (data, label, site, sex), res in forward_grouped(model, (_to_device(b, device) for b in loader), group_rows):
        cls_logger.log(res["Y_hat"], label)
        site_logger.log(res["site_hat"], site)
        probs.append(res["Y_prob"]); site_probs.append(res["site_prob"])
        labels.append(label.reshape(-1)); sites.append(site.reshape(-1)); sexes.append(sex.reshape(-1))
        y_hats.append(res["Y_hat"].reshape(-1)); s_hats.append(res["site_hat"].reshape(-1))
    n = len(probs)
    if n == 0:
        raise ValueError("summary: empty loader")
    # the loop's only host read-backs
    all_cls_probs = torch.cat(probs).double().cpu().numpy()
    all_site_probs = torch.cat(site_probs).double().cpu().numpy()
    all_cls_labels = torch.cat(labels).double().cpu().numpy()
    all_site_labels = torch.cat(sites).double().cpu().numpy()
    all_sexes = torch.cat(sexes).double().cpu().numpy()
    y_hat = torch.cat(y_hats).cpu().numpy(); s_hat = torch.cat(s_hats).cpu().numpy()
    cls_test_error = float(np.mean(y_hat != all_cls_labels))                # mean of calculate_error per slide
    site_test_error = float(np.mean(s_hat != all_site_labels))

    patient_results = {}
    for i in range(n):
        sid = ids[i]
        patient_results[sid] = {"slide_id": np.array(sid), "cls_prob": all_cls_probs[i:i + 1].astype(np.float32),
                                "cls_label": int(all_cls_labels[i]), "site_prob": all_site_probs[i:i + 1].astype(np.float32),
                                "site_label": int(all_site_labels[i])}

    topk, topk_accs = (), []
    if n_classes > 2:
        topk = (1, 3, 5) if n_classes > 5 else (1, 3)
        topk_accs = accuracy(torch.from_numpy(all_cls_probs), torch.from_numpy(all_cls_labels), topk=topk)

    cls_auc, cls_aucs = _cls_auc(all_cls_labels, all_cls_probs, n_classes, bool(getattr(args, "micro_average", False)))
    if len(np.unique(all_site_labels)) == 1:
        site_auc = -1
    else:
        from sklearn.metrics import roc_auc_score
        site_auc = float(roc_auc_score(all_site_labels, all_site_probs[:, 1]))

    table = {"slide_id": ids[:n], "sex": all_sexes, "Y": all_cls_labels, "Y_hat": np.argmax(all_cls_probs, axis=1),
             "site": all_site_labels, "site_hat": np.argmax(all_site_probs, axis=1)}
    for c in range(n_classes):
        table["p_{}".format(c)] = all_cls_probs[:, c]
    table["site_p"] = all_site_probs[:, 1]
    out = {"patient_results": patient_results, "cls_test_error": cls_test_error, "cls_auc": cls_auc, "cls_aucs": cls_aucs,
           "site_test_error": site_test_error, "site_auc": site_auc, "loggers": (cls_logger, site_logger),
           "df": pd.DataFrame(table)}
    for k, a in zip(topk, topk_accs):
        out["top{}_acc".format(k)] = a.item()
    return out


def eval(loader: Iterable, args, ckpt_path: Optional[str], slide_ids: Optional[Sequence] = None):   # noqa: A001 (reference name)
    """``eval_utils:34-46``: model from checkpoint + ``summary``. Takes the loader (the reference builds it from
    its dataset with ``get_simple_loader``: sequential, batch size 1)."""
    model = initiate_model(args, ckpt_path)
    return model, summary(model, loader, args, slide_ids=slide_ids)


@torch.no_grad()
def attention_heatmap_scores(model: TOAD_fc_mtl_concat, data: torch.Tensor, percentile: bool = False) -> torch.Tensor:
    """Raw task-0 attention score per patch: ``model(data, sex, attention_only=True)`` (``model_toad.py:93-94``),
    which runs the trunk GEMMs and the fused gate/score kernel and skips pooling and heads. With ``percentile``
    the scores are converted to their rank in [0, 1] on the device (what the heat-map colour scale consumes)."""
    sex = torch.zeros(1, device=data.device)
    a = model(data, sex, attention_only=True)
    if not percentile:
        return a
    order = torch.argsort(a)
    ranks = torch.empty_like(a)
    ranks[order] = torch.arange(a.numel(), device=a.device, dtype=a.dtype)
    return ranks / max(a.numel() - 1, 1)


def region_attention_scores(extractor, model: TOAD_fc_mtl_concat, region: torch.Tensor, origins, tile=256, bag_dtype: torch.dtype = torch.float16,
                            percentile: bool = False, shrink=1) -> torch.Tensor:
    """Heat-map scores of the tiles at ``origins`` of one decoded uint8 region [Hr,Wr,3], in the order of ``origins``, with no tile tensor at any point:
    ``extractor.forward_u8_region`` reads the tiles where they lie (overlapping ones - a heat-map stride below the tile size - included) and writes its
    rows chunk by chunk into one [B,1024] bag of ``bag_dtype``; ``attention_heatmap_scores(model, bag, percentile)`` scores that bag. Equal to scoring
    ``extractor.forward_u8(stacked tiles, out_dtype=bag_dtype)``. Putting the B scores on a canvas: ``heatmap.attention_canvas``, or
    ``region_tissue_attention_heatmap`` for selection, scores and canvas in one call.

    ``shrink`` = 2 (a 40x scan): ``tile`` is the footprint in region pixels and the extractor reads it box-filtered to ``tile / 2``
    (``forward_u8_region(..., shrink=2)``); equal to scoring ``extractor.forward_u8(ops.box_tiles_u8(region, origins, tile, 2), out_dtype=bag_dtype)``."""
    bag = extractor.forward_u8_region(region, origins, tile=tile, out_dtype=bag_dtype, shrink=shrink)
    return attention_heatmap_scores(model, bag, percentile)


_SEGMENT_KEYS = ("down", "median", "sat_thresh", "val_min", "close", "min_area", "min_hole")


def _segment_down(segment: dict):
    """The ``down`` a segment dict selects with: its own, or the default of ``tissue.segmented_tissue_origins``."""
    from .tissue import segmented_tissue_origins
    return segment.get("down", inspect.signature(segmented_tissue_origins).parameters["down"].default)


def _select_origins(region, tile, stride, min_fraction, sat_thresh, val_min, segment, return_mask=False):
    """The tissue tiles' origins; with ``return_mask`` (a ``segment`` dict only) -> (origins, (plane, t, mask_down)), the mask they were counted on."""
    from .tissue import segmented_tissue_origins, tissue_origins
    if return_mask and segment is None:
        raise ValueError("tissue_mask=True needs a segment dict: only tissue.segmented_tissue_origins leaves a mask plane on the device")
    if segment is None:
        return tissue_origins(region, tile=tile, stride=stride, min_fraction=min_fraction, sat_thresh=sat_thresh, val_min=val_min)
    if not isinstance(segment, dict) or any(k not in _SEGMENT_KEYS for k in segment):
        bad = segment if not isinstance(segment, dict) else sorted(k for k in segment if k not in _SEGMENT_KEYS)
        raise ValueError(f"segment must be None or a dict with keys among {_SEGMENT_KEYS}, got {bad!r}")
    kw = dict(sat_thresh=sat_thresh, val_min=val_min)
    kw.update(segment)
    if not return_mask:
        return segmented_tissue_origins(region, tile=tile, stride=stride, min_fraction=min_fraction, **kw)
    kw["down"] = _segment_down(kw)
    origins, (plane, t) = segmented_tissue_origins(region, tile=tile, stride=stride, min_fraction=min_fraction, return_mask=True, **kw)
    return origins, (plane, t, kw["down"])


def region_tissue_attention_scores(extractor, model: TOAD_fc_mtl_concat, region: torch.Tensor, tile=256, stride=None, min_fraction: float = 0.25,
                                   sat_thresh: int = 8, val_min: int = 0, bag_dtype: torch.dtype = torch.float16, percentile: bool = False,
                                   segment: Optional[dict] = None, shrink=1):
    """``(origins, scores)`` of the tissue tiles of one decoded uint8 region [Hr,Wr,3]: ``tissue.tissue_origins`` picks the lattice tiles that hold tissue
    from the pixels (two launches and one small read-back, on the region where it lies), ``region_attention_scores`` scores exactly those. ``origins`` is
    the int64 [B,2] host array of (x, y), row-major over the lattice; ``scores`` its B scores on the device. A region without a tissue tile returns an
    empty [0,2] array and an empty score tensor, and the extractor is not called. Selection arguments and their defaults: ``tissue.tissue_origins``.

    ``segment``: None selects with ``tissue_origins``; a dict of ``tissue.segmented_tissue_origins`` keywords - any of ``down``, ``median``,
    ``sat_thresh``, ``val_min``, ``close``, ``min_area``, ``min_hole`` - selects with that function instead (CLAM's median-filtered saturation of a box-filtered level, ``sat_thresh`` an int
    or ``"otsu"``). Keys it does not give take this call's ``sat_thresh`` / ``val_min`` and that function's ``down`` / ``median`` defaults.

    ``shrink``: ``region_attention_scores`` - it goes to the extractor only; the selection works on ``tile``, the footprint, as it does without it."""
    return _tissue_scores(extractor, model, region, tile, stride, min_fraction, sat_thresh, val_min, bag_dtype, percentile, segment, shrink=shrink)[:2]


def _tissue_scores(extractor, model, region, tile, stride, min_fraction, sat_thresh, val_min, bag_dtype, percentile, segment, return_mask=False, shrink=1):
    """``region_tissue_attention_scores`` -> (origins, scores, mask): mask = None, or with ``return_mask`` the (plane, t, mask_down) of the selection."""
    origins, mask = _select_origins(region, tile, stride, min_fraction, sat_thresh, val_min, segment, return_mask), None
    if return_mask:
        origins, mask = origins
    if origins.shape[0] == 0:
        return origins, torch.empty(0, dtype=torch.float32, device=region.device), mask
    return origins, region_attention_scores(extractor, model, region, origins, tile=tile, bag_dtype=bag_dtype, percentile=percentile, shrink=shrink), mask


def region_tissue_attention_heatmap(extractor, model: TOAD_fc_mtl_concat, region: torch.Tensor, tile=256, stride=None, min_fraction: float = 0.25,
                                    sat_thresh: int = 8, val_min: int = 0, bag_dtype: torch.dtype = torch.float16, alpha=102, down: int = 1, lut=None,
                                    out=None, segment: Optional[dict] = None, smooth: bool = False, tissue_mask: bool = False, thresh=None,
                                    binarize: bool = False, blur=False, shrink=1):
    """``(origins, scores, canvas)`` of one decoded uint8 region [Hr,Wr,3]: ``region_tissue_attention_scores(..., percentile=True)`` selects and scores the
    tissue tiles, ``heatmap.attention_canvas`` renders those percentile scores onto the region on the same lattice, on the device - uint8
    [Hr // down, Wr // down, 3]; the tiles that were not selected keep the (box-filtered) pixels of the region. ``alpha``, ``down``, ``lut`` and ``out``:
    ``heatmap.attention_canvas``. ``segment``: as for ``region_tissue_attention_scores`` - None or a dict that selects the tiles with
    ``tissue.segmented_tissue_origins``.

    ``smooth``, ``thresh``, ``binarize``: ``heatmap.attention_canvas`` (the colour index interpolated between cell centres; tiles below a percentile
    score dropped; present tiles saturated). ``tissue_mask=True`` (CLAM's ``segment=True``) colours only the tissue pixels of a selected tile: it needs
    a ``segment`` dict, whose mask plane - the one the tiles were counted on, nothing is recomputed - goes to the renderer with its threshold and its
    ``down``; the canvas ``down`` must be one of 1 .. 32 and that ``down`` a multiple of it (ValueError otherwise, before anything is launched).

    ``down`` in 8, 16, 32 gives the slide overview in one pass (``ops.region_heat_thumb``; the lattice's cell must be at least ``down``). With the CLAM
    default segment ``down = 16`` masked canvases at 8 and 16 work; one at 32 needs ``segment=dict(down=32)``.

    ``blur`` (CLAM's ``blur``): ``heatmap.attention_canvas`` - False, True for CLAM's Gaussian width ``0.6 tile + 0.5`` pixels, a sigma in pixels, or the
    integer taps; the cell table is smoothed by ``ops.heat_cells_blur`` before it is rendered, and a bad value raises ValueError before the selection runs.

    ``shrink``: ``region_attention_scores`` - the extractor reads each ``tile`` footprint box-filtered by it (2 for a 40x scan); selection and canvas keep
    working on ``tile`` and ``stride`` in region pixels. A bad value, or a footprint it does not divide, raises ValueError before the selection runs.

    Not done here: a sigma per axis for tiles that are not square, radii above 16 cells (``blur=True`` on lattices whose cell is 16 or less), CLAM's
    second blur of the coloured image and saving the image. ``down`` may be a sequence of distinct levels from 1 .. 32: ``canvas`` is then a dict
    ``{down: tensor}`` and ``out`` a dict of that kind or None; one selection, one scoring, one cell table and one read of the region
    (``heatmap.attention_pyramid``), each level byte for byte the call with that ``down``; the lattice's cell must be at least the largest level and,
    with ``tissue_mask=True``, the segment ``down`` a multiple of it (ValueError otherwise, before anything is launched). A slide
    that arrives strip by strip: ``slide_attention_heatmap`` (no seams, one colour scale); ``segment=`` and ``tissue_mask=`` there select on the slide's plane, put together from the strips."""
    from .heatmap import attention_canvas, attention_pyramid, blur_taps
    from .tissue import _lattice_args, lattice_cell
    levels = None                                                   # a sequence of levels: one scoring, one cell table, one read of the region
    if isinstance(down, (tuple, list)):
        from .ops import heat_downs_arg
        levels = heat_downs_arg("region_tissue_attention_heatmap", down)
        h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, (0, 0))
        cell = lattice_cell((h, w), (sy, sx), (x0, y0))
        if max(levels) > cell:
            raise ValueError(f"region_tissue_attention_heatmap: down = {max(levels)}, the largest level, exceeds the lattice's cell = {cell}: a canvas box "
                             "must lie in one cell")
        if out is not None and (not isinstance(out, dict) or set(out) != set(levels)):
            raise ValueError(f"region_tissue_attention_heatmap: with down = {levels} out must be None or a dict with one canvas per level")
    if shrink != 1:                                                 # refuse a bad shrink before the selection runs; the extractor checks it again
        from .ops import shrunk_tile
        shrunk_tile(tile, shrink)
    if blur is not None and blur is not False:                      # refuse a bad blur before the extractor runs; attention_canvas parses it again
        h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, (0, 0))
        blur_taps(blur, (h, w), lattice_cell((h, w), (sy, sx), (x0, y0)))
    if tissue_mask and isinstance(segment, dict):                   # (without a dict _select_origins refuses)
        seg_down = _segment_down(segment)
        if levels is not None:
            if not isinstance(seg_down, int) or seg_down % max(levels):
                raise ValueError(f"tissue_mask=True: the segment down = {seg_down!r} must be a multiple of the largest canvas down = {max(levels)} (a canvas "
                                 "box must lie in one mask pixel)")
        elif down not in (1, 2, 4, 8, 16, 32) or not isinstance(seg_down, int) or seg_down % down:
            raise ValueError(f"tissue_mask=True: the segment down = {seg_down!r} must be a multiple of the canvas down = {down!r} (a canvas box must lie "
                             "in one mask pixel)")
    origins, scores, mask = _tissue_scores(extractor, model, region, tile, stride, min_fraction, sat_thresh, val_min, bag_dtype, True, segment,
                                           return_mask=tissue_mask, shrink=shrink)
    if levels is not None:
        canvases = attention_pyramid(region, origins, scores, tile=tile, stride=stride, alpha=alpha, downs=levels, lut=lut,
                                     outs=None if out is None else [out[d] for d in levels], smooth=smooth, mask=mask, thresh=thresh, binarize=binarize, blur=blur)
        return origins, scores, dict(zip(levels, canvases))
    return origins, scores, attention_canvas(region, origins, scores, tile=tile, stride=stride, alpha=alpha, down=down, lut=lut, out=out, smooth=smooth,
                                             mask=mask, thresh=thresh, binarize=binarize, blur=blur)


def strip_triples(parts):
    """The arguments of ONE ``forward_u8_regions`` call for the strips that own tiles: ``parts`` = [(region, local origins [B_k,2] = (x, y) in the strip's
    coordinates), ...], only strips with at least one tile, in the walk's order -> (regions, triples int64 [sum B_k, 3] = (x, y, k)), k the position in
    ``parts``. A strip without a tile must not be in the list: the call requires a tile to fit every region, and a remainder strip may be shorter."""
    regions, triples = [], []
    for k, (region, local) in enumerate(parts):
        local = np.asarray(local, dtype=np.int64)
        if local.ndim != 2 or local.shape[1] != 2 or local.shape[0] == 0:
            raise ValueError(f"strip_triples: part {k} must bring [B,2] origins with B >= 1, got shape {local.shape}")
        regions.append(region)
        triples.append(np.concatenate([local, np.full((local.shape[0], 1), k, dtype=np.int64)], axis=1))
    return regions, (np.concatenate(triples, axis=0) if triples else np.zeros((0, 3), dtype=np.int64))


def slide_attention_heatmap(extractor, model: TOAD_fc_mtl_concat, strips, slide_hw, tile=256, stride=None, origin=(0, 0), origins=None,
                            min_fraction: float = 0.25, sat_thresh: int = 8, val_min: int = 0, bag_dtype: torch.dtype = torch.float16, alpha=102,
                            down: int = 1, lut=None, out=None, smooth: bool = False, mask=None, thresh=None, binarize: bool = False, blur=False, shrink=1,
                            batch_render: bool = False, batch_levels: bool = False, segment: Optional[dict] = None, tissue_mask: bool = False,
                            batch_extract: bool = False):
    """``(origins, scores, canvas)`` of a slide of ``slide_hw`` = (Hs, Ws) pixels that arrives from the decoder strip by strip: what
    ``region_tissue_attention_heatmap`` gives for one region, with no seam where two strips meet. ``strips`` is a sequence of ``(region, y_k)`` - a
    decoded uint8 [H_k,Ws,3] full-width strip on the device and the slide row of its first row - sorted, each abutting or overlapping the one before,
    covering rows 0 .. Hs (``heatmap.strip_plan``; its ValueErrors come before anything is launched). Strips must overlap by at least tile - stride
    rows, so that every lattice tile row lies whole in one strip. The sequence is read once for its shapes and then walked twice:

    1. per strip, the tissue tiles the strip owns (``tissue.tissue_origins`` on the strip with the strip's local lattice origin; or, with ``origins``
       [B,2] of (x, y) in SLIDE coordinates, the caller's tiles whose lattice row the strip owns, in the order given) go through
       ``extractor.forward_u8_region`` on that strip; the rows are put into one bag, strips in order, row-major inside a strip - the slide's row-major
       lattice order. ``attention_heatmap_scores(model, bag, percentile=True)`` runs ONCE over that bag, so the ranks - the colour scale - are the
       slide's, and ``heatmap.slide_cells`` builds the slide's cell table from them (``thresh``, ``binarize``, ``blur`` as in ``attention_canvas``).
    2. per strip, ``heatmap.window_canvas`` renders the strip's rows from max(y_k, the end of the previous strip) on into its rows of ONE uint8
       [Hs // down, Ws // down, 3] canvas (or ``out``), against the slide's table: the tent and the blur see the neighbouring strip's cells.

    ``origins`` returned are slide coordinates, int64 [B,2] on the host. ``mask`` is a SLIDE-wide ``(plane, t, mask_down)``, for example
    ``tissue.segment_tissue`` of the slide's overview level; ``alpha``, ``down`` (1 .. 32), ``lut``, ``smooth``: ``attention_canvas``; ``shrink``:
    ``region_attention_scores``. A slide without a tissue tile gives empty origins, empty scores and the box-filtered slide; neither the extractor nor
    the model is called. With the same tiles the canvas is byte for byte ``attention_canvas`` of the whole slide.

    ``down`` may be a sequence of distinct levels from 1 .. 32: ``canvas`` is then a dict ``{down: tensor}`` and ``out`` such a dict or None. Still one
    scoring and one cell table, and pass 2 is ONE walk over the strips - ``heatmap.window_pyramid`` renders every level of a strip from one read of
    it; render starts are multiples of max(4, the largest level), and each level is byte for byte the call with that ``down``.

    ``batch_render=True`` (an int ``down`` only) makes pass 2 ONE ``heatmap.windows_canvas`` call over all strips - each strip's rendered rows as a view,
    its rows of the one canvas as ``out`` - and so one launch instead of one per strip; the strips are resident by then, and the bytes are the same.
    With ``False`` every call is what it was. With a sequence of levels it is a ValueError: that is ``batch_levels``.

    ``batch_levels=True`` (a sequence ``down`` only) makes pass 2 ONE ``heatmap.windows_pyramid`` call over all strips - each strip's rendered rows as
    the region, its rows of every level's slide canvas as its ``outs`` - and so one launch per ``ops.HEAT_PYR_LIST_MAX`` strips and one read of every
    strip; the dict ``{down: canvas}`` is byte for byte what the walk gives. With an int ``down`` it is a ValueError: that is ``batch_render``.

    ``segment``: None selects per strip with ``tissue_origins``, as above; a dict of the keys ``region_tissue_attention_heatmap`` takes (``down``,
    ``median``, ``sat_thresh``, ``val_min``, ``close``, ``min_area``, ``min_hole``; the same defaults) selects with CLAM's recipe ON THE WHOLE SLIDE:
    before pass 1 the strips are read once, in one launch, for the slide's saturation plane (``tissue.slide_saturation`` - only that step touches the
    pixels, and a plane put together from strips is the plane of the slide), and ``tissue.segmented_slide_origins`` runs the median, Otsu, the closing,
    the component filters and the tile sums once on it - they see across the seams, and there is one read-back for the slide. The tiles then take the
    ``origins=`` route: each strip extracts the lattice rows it owns, with one percentile ranking. Every plane row of the segment ``down`` must lie whole
    in one strip (``tissue.plane_strip_plan``: strips meet at multiples of it or overlap enough). ``tissue_mask=True`` (CLAM's ``segment=True``) hands
    that selection's ``(plane, t, segment down)`` to pass 2 as ``mask``; the segment ``down`` must be a multiple of the canvas ``down`` (of the
    largest level). ValueError before anything is launched: ``segment`` together with ``origins``, ``tissue_mask=True`` without a ``segment`` dict or
    together with ``mask``, the multiple rule, and what ``plane_strip_plan`` and the segmented lattice rule (multiples of 4 * segment ``down``) refuse.
    With ``segment=None`` and ``tissue_mask=False`` every path, message and byte is what it was.

    ``batch_extract=True`` keeps pass 1's selection (per strip with ``tissue_origins``, the caller's ``origins=``, or ``segment=``) but takes the bag from
    ONE ``extractor.forward_u8_regions`` call: the strips' tiles in the order above, as triples (x, y local to the strip, k) - ``strip_triples``. Only the
    strips that own a tile are regions of that call, numbered k = 0, 1, ... in the strips' order: a strip that owns no lattice row or no tissue tile - a
    last strip shorter than the tile, which only renders the slide's last rows - is skipped exactly as the per-strip walk skips it (the list call
    requires a tile to fit every region it is given). The extractor scales every layer by an abs-max over the tiles of a call, so with per-strip calls a bag row depends on how the decoder cut the
    slide; with the one call - chunked like the whole-slide call - it does not: with the same tiles ``scores`` is ``torch.equal`` to
    ``attention_heatmap_scores(model, extractor.forward_u8_region(whole_slide, origins, ...), percentile=True)``. More strips than
    ``ops.TILE_REGIONS_MAX`` is a ValueError before anything is launched - the limit counts ALL strips given, since which of them own a tile is known
    only after the selection has run on the device - and a non-bool too. Independent of ``batch_render`` / ``batch_levels``; with
    ``False`` every path, message and byte is what it was.

    Not done here: blocks that are not full-width strips (``heatmap.window_canvas`` renders any window and ``ops.regions_saturation`` takes any
    windows; this walk does not), and the "not done" list of ``region_tissue_attention_heatmap`` except seams."""
    from .heatmap import slide_cells, strip_plan, window_canvas, window_pyramid, windows_canvas, windows_pyramid
    from .heatmap import blur_taps
    from .tissue import _lattice_args, lattice_cell, segmented_slide_origins, tissue_origins
    hs, ws = slide_hw
    h, w, sy, sx, x0, y0 = _lattice_args(tile, stride, origin)
    if shrink != 1:                                                 # refuse what the second pass would refuse before the extractor runs
        from .ops import shrunk_tile
        shrunk_tile(tile, shrink)
    cell = lattice_cell((h, w), (sy, sx), (x0, y0))
    if not isinstance(batch_render, bool):
        raise ValueError(f"slide_attention_heatmap: batch_render must be a bool, got {batch_render!r}")
    if not isinstance(batch_levels, bool):
        raise ValueError(f"slide_attention_heatmap: batch_levels must be a bool, got {batch_levels!r}")
    if not isinstance(batch_extract, bool):
        raise ValueError(f"slide_attention_heatmap: batch_extract must be a bool, got {batch_extract!r}")
    if batch_extract:
        from .ops import TILE_REGIONS_MAX
        if len(strips) > TILE_REGIONS_MAX:
            raise ValueError(f"slide_attention_heatmap: batch_extract=True takes at most {TILE_REGIONS_MAX} strips (ops.TILE_REGIONS_MAX, the regions of one "
                             f"extractor call), got {len(strips)}")
    levels = None                                                   # a sequence of levels: pass 2 renders them all in one walk over the strips
    if batch_levels and not isinstance(down, (tuple, list)):
        raise ValueError("slide_attention_heatmap: batch_levels=True takes a sequence of levels, not one down (one canvas for a list of windows: "
                         "batch_render=True)")
    if isinstance(down, (tuple, list)):
        if batch_render:
            raise ValueError("slide_attention_heatmap: batch_render=True takes one down, not a sequence of levels (pyramid levels for a list of windows: "
                             "batch_levels=True)")
        from .ops import heat_downs_arg
        levels = heat_downs_arg("slide_attention_heatmap", down)
        if cell < max(levels):
            raise ValueError(f"slide_attention_heatmap: down = {max(levels)}, the largest level, exceeds the lattice's cell = {cell}: a canvas box must "
                             "lie in one cell")
        if out is not None and (not isinstance(out, dict) or set(out) != set(levels)):
            raise ValueError(f"slide_attention_heatmap: with down = {levels} out must be None or a dict with one canvas per level")
    elif down in (8, 16, 32) and cell < down:
        raise ValueError(f"slide_attention_heatmap: down = {down} exceeds the lattice's cell = {cell}: a canvas box must lie in one cell")
    blur_taps(blur, (h, w), cell)
    seg_kw = None
    if tissue_mask and not isinstance(segment, dict):
        raise ValueError("tissue_mask=True needs a segment dict: only tissue.segmented_tissue_origins leaves a mask plane on the device")
    if segment is not None:
        if not isinstance(segment, dict) or any(k not in _SEGMENT_KEYS for k in segment):
            bad = segment if not isinstance(segment, dict) else sorted(k for k in segment if k not in _SEGMENT_KEYS)
            raise ValueError(f"segment must be None or a dict with keys among {_SEGMENT_KEYS}, got {bad!r}")
        if origins is not None:
            raise ValueError("slide_attention_heatmap: segment selects the tiles, origins gives them: pass one of the two")
        if tissue_mask and mask is not None:
            raise ValueError("slide_attention_heatmap: tissue_mask=True renders with the selection's own mask plane: pass that or mask, not both")
        seg_kw = dict(sat_thresh=sat_thresh, val_min=val_min)
        seg_kw.update(segment)
        seg_kw["down"] = seg_down = _segment_down(seg_kw)
        if tissue_mask:
            if levels is not None:
                if not isinstance(seg_down, int) or seg_down % max(levels):
                    raise ValueError(f"tissue_mask=True: the segment down = {seg_down!r} must be a multiple of the largest canvas down = {max(levels)} (a canvas "
                                     "box must lie in one mask pixel)")
            elif down not in (1, 2, 4, 8, 16, 32) or not isinstance(seg_down, int) or seg_down % down:
                raise ValueError(f"tissue_mask=True: the segment down = {seg_down!r} must be a multiple of the canvas down = {down!r} (a canvas box must lie "
                                 "in one mask pixel)")
    shapes = []
    for k, (region, y) in enumerate(strips):
        if region.dim() != 3 or region.shape[1] != ws or region.shape[2] != 3:
            raise ValueError(f"slide_attention_heatmap: strip {k} must be a full-width uint8 [H_k,{ws},3] region, got {tuple(region.shape)}")
        shapes.append((y, region.shape[0]))
    plan = strip_plan((hs, ws), shapes, (h, w), (sy, sx), (x0, y0), down)
    device = strips[0][0].device
    given = None
    if seg_kw is not None:                                          # one selection on the slide's plane: one read of the strips, one read-back
        given, (plane, t) = segmented_slide_origins(strips, (hs, ws), tile=(h, w), stride=(sy, sx), min_fraction=min_fraction, origin=(x0, y0),
                                                    return_mask=True, **seg_kw)
        rows = (given[:, 1] - y0) // sy
        if tissue_mask and plane is not None:
            mask = (plane, t, seg_kw["down"])
    elif origins is not None:
        given = np.asarray(origins)
        if given.ndim != 2 or given.shape[1] != 2 or given.dtype.kind not in "iu":
            raise ValueError(f"slide_attention_heatmap: origins must be [B,2] integers (x, y) in slide coordinates, got shape {given.shape} dtype {given.dtype}")
        given = given.astype(np.int64)
        rows = (given[:, 1] - y0) // sy
        off = (rows < 0) | (rows >= plan[-1]["rows"][1]) | ((given[:, 1] - y0) % sy != 0) | ((given[:, 0] - x0) % sx != 0)
        if off.any():                                                # (outside the lattice along x, or given twice: slide_cells, after the first pass)
            bad = given[off][0]
            raise ValueError(f"slide_attention_heatmap: origin (x={int(bad[0])}, y={int(bad[1])}) is off the lattice or in none of the slide's lattice rows")
    kept, bags, parts = [], [], []
    for (region, y), p in zip(strips, plan):                        # pass 1: the tiles each strip owns -> bag rows
        j0, j1 = p["rows"]
        if j1 == j0:
            continue
        if given is None:
            local = tissue_origins(region, tile=(h, w), stride=(sy, sx), min_fraction=min_fraction, sat_thresh=sat_thresh, val_min=val_min, origin=p["origin"])
        else:
            local = given[(rows >= j0) & (rows < j1)] - np.array([0, y], dtype=np.int64)
        if local.shape[0] == 0:
            continue
        kept.append(local + np.array([0, y], dtype=np.int64))
        if batch_extract:                                           # the strip's tiles go into the one call behind the loop
            parts.append((region, local))
        else:
            bags.append(extractor.forward_u8_region(region, local, tile=(h, w), out_dtype=bag_dtype, shrink=shrink))
    if parts:                                                       # ONE extractor call: its abs-max scopes are those of the whole slide's call
        regions, triples = strip_triples(parts)
        bags.append(extractor.forward_u8_regions(regions, triples, tile=(h, w), out_dtype=bag_dtype, shrink=shrink))
    if kept:
        found = np.concatenate(kept, axis=0)
        scores = attention_heatmap_scores(model, bags[0] if len(bags) == 1 else torch.cat(bags, dim=0), percentile=True)
    else:
        found, scores = np.zeros((0, 2), dtype=np.int64), torch.empty(0, dtype=torch.float32, device=device)
    cells, cell = slide_cells((hs, ws), found, scores, (h, w), (sy, sx), (x0, y0), thresh=thresh, binarize=binarize, blur=blur,
                              name="slide_attention_heatmap")
    if levels is not None:
        canvases = {}
        for d in levels:
            c = torch.empty((hs // d, ws // d, 3), dtype=torch.uint8, device=device) if out is None else out[d]
            if not isinstance(c, torch.Tensor) or tuple(c.shape) != (hs // d, ws // d, 3):
                raise ValueError(f"slide_attention_heatmap: out[{d}] must be a uint8 [{hs // d},{ws // d},3] tensor on the strips' device")
            canvases[d] = c
        if batch_levels:                                            # pass 2 in one call: every strip's own rows of every level's canvas
            spans = [p["render"] for p in plan]
            windows_pyramid([region[r0 - y:r1 - y] for (region, y), (r0, r1) in zip(strips, spans)], [(0, r0) for r0, _ in spans], cells, cell, alpha=alpha,
                            downs=levels, lut=lut, outs=[[canvases[d][r0 // d:r0 // d + (r1 - r0) // d] for d in levels] for r0, r1 in spans], smooth=smooth,
                            mask=mask)
            return found, scores, canvases
        for (region, y), p in zip(strips, plan):                  # pass 2: each strip's own rows of every level's canvas, one read of the strip
            r0, r1 = p["render"]
            window_pyramid(region[r0 - y:r1 - y], (0, r0), cells, cell, alpha=alpha, downs=levels, lut=lut,
                           outs=[canvases[d][r0 // d:r0 // d + (r1 - r0) // d] for d in levels], smooth=smooth, mask=mask)
        return found, scores, canvases
    ho, wo = hs // down, ws // down
    if out is None:
        out = torch.empty((ho, wo, 3), dtype=torch.uint8, device=device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (ho, wo, 3):
        raise ValueError(f"slide_attention_heatmap: out must be a uint8 [{ho},{wo},3] tensor on the strips' device")
    if batch_render:                                                # pass 2 in one call: every strip's own rows of the one canvas
        spans = [p["render"] for p in plan]
        windows_canvas([region[r0 - y:r1 - y] for (region, y), (r0, r1) in zip(strips, spans)], [(0, r0) for r0, _ in spans], cells, cell, alpha=alpha,
                       down=down, lut=lut, outs=[out[r0 // down:r0 // down + (r1 - r0) // down] for r0, r1 in spans], smooth=smooth, mask=mask)
        return found, scores, out
    for (region, y), p in zip(strips, plan):                        # pass 2: each strip's own rows of the one canvas
        r0, r1 = p["render"]
        n = (r1 - r0) // down
        window_canvas(region[r0 - y:r1 - y], (0, r0), cells, cell, alpha=alpha, down=down, lut=lut, out=out[r0 // down:r0 // down + n], smooth=smooth, mask=mask)
    return found, scores, out
