"""Drop-in for the reference's ``models/resnet_custom.py``: the truncated ResNet-50 that turns 256x256 tiles into the
1024-d patch embeddings of a bag, running on the HIP kernels (``toad_resnet50_trunc_fwd_f32``).

Same classes, constructor arguments, module tree and state-dict keys as the reference (``Bottleneck_Baseline``
:19-56, ``ResNet_Baseline`` :58-108, ``resnet50_baseline`` :111-119), so torchvision ResNet-50 checkpoints load exactly
like they do there (``load_state_dict(..., strict=False)``, :121-124). The ``nn.Conv2d`` / ``nn.BatchNorm2d`` children
are parameter containers only: ``forward`` folds eval-mode BatchNorm into the convolution weights once (fp64 on the
device), lays each convolution out as the [Cout, kh*kw*Cin] operand of the NHWC GEMM, and hands the whole network
to one C-ABI call. There is no CPU path and no train-mode BatchNorm: the reference only ever runs the extractor under
``eval()`` to write the ``.pt`` bags (it is never optimised), and this module refuses anything else loudly.

``pretrained=True`` needs the network in the reference too (model_zoo download, :122); here it raises with that
explanation — load a local checkpoint with ``load_state_dict`` instead.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib
from .ops import (IMAGENET_MEAN, IMAGENET_STD, TILE_REGIONS_MAX, _row_pitch, check_origins, check_region_origins, check_shrink, norm_constants_u8,
                  region_layout_ok, region_table, shrunk_tile, tile_shape)

__all__ = ["Bottleneck_Baseline", "ResNet_Baseline", "resnet50_baseline", "IMAGENET_MEAN", "IMAGENET_STD"]

STEM_K = 192            # 4 x 4 space-to-depth taps x 12 channels (147 real taps + zero slots)
MAX_TILES_PER_CALL = 512     # at 256x256 tiles. 32-bit byte offsets inside the kernels: B*(H/4)*(W/4)*128*4 < 2^31 (layer2.0 conv2 input)


def max_tiles_per_call(h: int, w: int) -> int:
    """Tiles per C call for H x W tiles: the kernels' 32-bit offsets bound B * H * W, so the cap scales with the tile area
    (512 at the reference's 256 x 256; 128 at 512 x 512; more for smaller tiles, bounded by the workspace to 4096)."""
    return max(1, min(4096, (MAX_TILES_PER_CALL * 256 * 256) // max(h * w, 1)))


class Bottleneck_Baseline(nn.Module):
    """Parameter container of one bottleneck block, children named and shaped as in the reference (resnet_custom.py:19-33):
    conv1 1x1 -> bn1 -> conv2 3x3 (carries the stride) -> bn2 -> conv3 1x1 (x4 channels) -> bn3, optional downsample."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        out = planes * self.expansion
        for i, (cin, cout, k, s) in enumerate(((inplanes, planes, 1, 1), (planes, planes, 3, stride), (planes, out, 1, 1)), start=1):
            self.add_module(f"conv{i}", nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=k // 2, bias=False))
            self.add_module(f"bn{i}", nn.BatchNorm2d(cout))
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        raise RuntimeError("Bottleneck_Baseline runs only inside ResNet_Baseline.forward (one fused HIP call)")


def _fold(conv: nn.Conv2d, bn: nn.BatchNorm2d, stem: bool):
    """eval-mode BN folded into the convolution: W' = W * g/sqrt(var+eps), b' = beta - mean * g/sqrt(var+eps)."""
    w = conv.weight.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    w = w * scale.view(-1, 1, 1, 1)
    if stem:                                            # space-to-depth operand of toad_stem_conv_s2d_f32: [64, 4(qy), 4(qx), 2(ry), 2(rx), 3(c)]
        w8 = torch.zeros(w.shape[0], 3, 8, 8, dtype=torch.float64, device=w.device)
        w8[:, :, 1:, 1:] = w                            # slot (2q + r) holds tap 2q + r - 1; slot 0 (tap -1) stays zero
        w2 = w8.view(w.shape[0], 3, 4, 2, 4, 2).permute(0, 2, 4, 3, 5, 1).reshape(w.shape[0], STEM_K)
    else:                                               # (ky, kx, c) order = the NHWC gather's column order
        w2 = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return w2.float().contiguous(), shift.float().contiguous()


class ResNet_Baseline(nn.Module):
    def __init__(self, block, layers):
        super().__init__()
        self.inplanes = 64
        if block is not Bottleneck_Baseline or list(layers[:3]) != [3, 4, 6]:
            raise NotImplementedError("the HIP extractor implements resnet50_baseline: Bottleneck_Baseline, layers [3, 4, 6, (3)]")
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        for m in self.modules():                                            # reference init, :70-75
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._folded = None           # (weights, biases, ctypes arrays), built lazily on the device
        self._folded_sig = None
        self._ws: Optional[torch.Tensor] = None

    def _make_layer(self, block, planes, blocks, stride=1):
        """`blocks` bottlenecks; the first one carries the stride and, when the shape changes, the 1x1 projection of the skip."""
        width = planes * block.expansion
        proj = None
        if stride != 1 or self.inplanes != width:
            proj = nn.Sequential(nn.Conv2d(self.inplanes, width, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(width))
        stack = [block(self.inplanes, planes, stride, proj)] + [block(width, planes) for _ in range(blocks - 1)]
        self.inplanes = width
        return nn.Sequential(*stack)

    # ---- folded-weight cache ------------------------------------------------------------------------------------
    def refold(self) -> None:
        """Drop the folded weights (call after changing parameters in place; load_state_dict / .to() do it themselves)."""
        self._folded = None

    def load_state_dict(self, *args, **kwargs):
        self._folded = None
        return super().load_state_dict(*args, **kwargs)

    def _param_signature(self):
        """(storage address, in-place version) of every parameter and BN statistic: changes whenever weights are loaded
        (also as a child of a parent module, which bypasses this class's load_state_dict), moved, or edited in place."""
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        self._ws = None
        return super()._apply(fn, *args, **kwargs)

    def _conv_bn_pairs(self):
        yield self.conv1, self.bn1, True
        for layer in (self.layer1, self.layer2, self.layer3):
            for blk in layer:
                yield blk.conv1, blk.bn1, False
                yield blk.conv2, blk.bn2, False
                yield blk.conv3, blk.bn3, False
                if blk.downsample is not None:
                    yield blk.downsample[0], blk.downsample[1], False

    def _fold_all(self):
        ws: List[torch.Tensor] = []
        bs: List[torch.Tensor] = []
        for conv, bn, stem in self._conv_bn_pairs():
            w, b = _fold(conv, bn, stem)
            ws.append(w); bs.append(b)
        assert len(ws) == 43
        wp = (ctypes.c_void_p * 43)(*[t.data_ptr() for t in ws])
        bp = (ctypes.c_void_p * 43)(*[t.data_ptr() for t in bs])
        self._folded = (ws, bs, wp, bp)
        self._folded_sig = self._param_signature()

    def relocate(self):
        if not torch.cuda.is_available():
            raise RuntimeError("toad_amd.resnet_custom needs a HIP device (no CPU fallback)")
        return self.to(torch.device("cuda", torch.cuda.current_device()))

    # ---- forward ------------------------------------------------------------------------------------------------
    def _ready(self, x: torch.Tensor, problem: Optional[str]) -> None:
        """The refusals every forward makes, in their order: training mode, the ``problem`` its own checks found with the input (or None), a model
        on another device."""
        if self.training:
            raise RuntimeError("the HIP extractor is inference-only: call .eval() (the reference never trains it)")
        if problem is not None:
            raise RuntimeError(problem)
        if self.conv1.weight.device != x.device:
            raise RuntimeError("model and input are on different devices; call model.relocate()")

    def _chunked(self, out: torch.Tensor, H: int, W: int, ws_bytes, call) -> torch.Tensor:
        """Fill the [B,1024] ``out``, at most max_tiles_per_call(H, W) tiles per library call. Folds the weights if they are stale, then
        ``call(b0, nb, wp, bp, o32, o16, tail)`` launches rows [b0, b0 + nb): ``wp`` / ``bp`` are the folded weight / bias pointers, the rows'
        destination is ``o32`` for an fp32 ``out`` and ``o16`` for an fp16 one (the other is None), and ``tail`` is the end of every entry's
        argument list (nb, H, W, workspace, its bytes, stream). ``ws_bytes(nb, H, W)`` sizes the workspace, which the model keeps and only grows."""
        if self._folded is None or self._folded_sig != self._param_signature():
            self._fold_all()
        _, _, wp, bp = self._folded
        B, dev = out.shape[0], out.device
        half = out.dtype == torch.float16
        stream = torch.cuda.current_stream(dev).cuda_stream
        cap = max_tiles_per_call(H, W)
        for b0 in range(0, B, cap):
            nb = min(cap, B - b0)
            need = ws_bytes(nb, H, W)
            if need == 0:
                raise RuntimeError(f"unsupported tile shape {H}x{W}")
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            o = out[b0:b0 + nb].data_ptr()
            call(b0, nb, wp, bp, None if half else o, o if half else None, (nb, H, W, self._ws.data_ptr(), self._ws.numel(), stream))
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B,3,H,W] fp32 NCHW on the HIP device -> [B,1024] (ResNet_Baseline.forward, :95-108)."""
        self._ready(x, None if x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 else
                    "expected a float32 [B,3,H,W] tensor on the HIP device (no CPU fallback)")
        lib = _lib.load()
        x = x.contiguous()
        B, _, H, W = x.shape

        def call(b0, nb, wp, bp, o32, _, tail):
            _lib.check(lib.toad_resnet50_trunc_fwd_f32(x[b0:b0 + nb].data_ptr(), wp, bp, o32, *tail), "toad_resnet50_trunc_fwd_f32")
        return self._chunked(torch.empty(B, 1024, device=x.device, dtype=torch.float32), H, W, lib.toad_resnet50_trunc_ws_bytes, call)

    def forward_u8(self, tiles: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """[B,H,W,3] uint8 RGB tiles on the HIP device, as an image decoder hands them over -> [B,1024] bag rows, fp32 or fp16.

        ToTensor + Normalize(mean, std) happen on the device in one rounding, x = fmaf(u, 1/(255 std_c), -mean_c/std_c); the result is bitwise
        ``forward`` of that fp32 NCHW tensor (``out_dtype=torch.float16``: bitwise ``forward(...).half()``, stored by the last kernel). 256-wide tiles with
        H % 4 == 0 never exist as an fp32 image: the stem kernel reads the bytes. Other shapes are converted into a staging image inside the workspace."""
        self._ready(tiles, (
            f"forward_u8 expects uint8 tiles, got {tiles.dtype} (normalised float32 [B,3,H,W] tiles go to forward)" if tiles.dtype != torch.uint8 else
            f"forward_u8 expects channels-last [B,H,W,3] tiles, got {tuple(tiles.shape)}" if tiles.dim() != 4 or tiles.shape[3] != 3 else
            f"out_dtype must be torch.float32 or torch.float16, got {out_dtype}" if out_dtype not in (torch.float32, torch.float16) else
            "expected a uint8 [B,H,W,3] tensor on the HIP device (no CPU fallback)" if not tiles.is_cuda else None))
        norm = norm_constants_u8(mean, std)
        lib = _lib.load()
        tiles = tiles.contiguous()
        B, H, W, _ = tiles.shape
        if W == 256 and H >= 4 and H % 4 == 0 and tiles.data_ptr() % 2:
            tiles = tiles.clone()                       # the stem reads 2-byte aligned words: one copy of a source at an odd address

        def call(b0, nb, wp, bp, o32, o16, tail):
            _lib.check(lib.toad_resnet50_trunc_fwd_u8(tiles[b0:b0 + nb].data_ptr(), norm, wp, bp, o32, o16, *tail), "toad_resnet50_trunc_fwd_u8")
        return self._chunked(torch.empty(B, 1024, device=tiles.device, dtype=out_dtype), H, W, lib.toad_resnet50_trunc_u8_ws_bytes, call)

    def forward_u8_region(self, region: torch.Tensor, origins, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, out_dtype: torch.dtype = torch.float32,
                          shrink=1) -> torch.Tensor:
        """Tiles read by origin from one decoded region -> [B,1024] bag rows, fp32 or fp16; no tile copy exists at any point.

        ``region``: uint8 [Hr,Wr,3] RGB on the HIP device with stride(2) == 1, stride(1) == 3 and any row pitch stride(0) >= 3 Wr (a column crop of a
        wider image is read in place; any base address). ``origins``: [B,2] integers (x, y), the top-left pixel of each tile in region coordinates, given
        on the HOST (CPU tensor, numpy array or list) - every tile must lie inside the region, which is checked here before anything is launched
        (``ValueError`` naming the first offender); duplicates, overlaps and any order are fine. ``tile``: an int or (H, W). Padding is the tile's, not the
        region's: the result is bitwise ``forward_u8(torch.stack([region[y:y+H, x:x+W] for x, y in origins]), mean, std, out_dtype)``. More than
        ``max_tiles_per_call`` origins are run in chunks that write into the one [B,1024] result.

        ``shrink`` = 2 reads a 40x scan at the 20x-equivalent pitch (CLAM's ``custom_downsample = 2``): ``tile`` stays the FOOTPRINT in region pixels - the
        origins, the tissue lattice and the heat-map lattice need no translation - ``shrink`` must divide both of its sides, and the network sees
        ``tile / shrink``, each pixel the mean, rounded half up, of its 2 x 2 box. Bitwise ``forward_u8(ops.box_tiles_u8(region, origins, tile, shrink), mean,
        std, out_dtype)``; on the 256-wide route (a (2 H, 512) footprint) the stem sums the boxes while it loads its window and neither those tiles nor a
        float image exist. A shrink other than 1 or 2, or one that does not divide the footprint, is a ``ValueError`` before anything else is looked at."""
        check_shrink(shrink)
        if shrink != 1:
            shrunk_tile(tile, shrink)
        self._ready(region, (
            f"forward_u8_region expects a uint8 region, got {region.dtype}" if region.dtype != torch.uint8 else
            f"forward_u8_region expects a channels-last [Hr,Wr,3] region, got {tuple(region.shape)}" if region.dim() != 3 or region.shape[2] != 3 else
            f"out_dtype must be torch.float32 or torch.float16, got {out_dtype}" if out_dtype not in (torch.float32, torch.float16) else
            "expected a uint8 [Hr,Wr,3] tensor on the HIP device (no CPU fallback)" if not region.is_cuda else
            f"forward_u8_region expects a region with stride(2) == 1, stride(1) == 3 and a row pitch stride(0) >= 3 Wr (rows are read in "
            f"place, there is no hidden copy), got strides {tuple(region.stride())} for shape {tuple(region.shape)}" if not region_layout_ok(region) else None))
        (FH, FW), (H, W) = shrunk_tile(tile, shrink)        # the footprint the origins are checked for, the tile the network and the chunking see
        Hr, Wr = region.shape[0], region.shape[1]
        org = check_origins(origins, Hr, Wr, FH, FW)
        B = org.shape[0]
        norm = norm_constants_u8(mean, std)
        out = torch.empty(B, 1024, device=region.device, dtype=out_dtype)
        if B == 0:
            return out
        lib = _lib.load()
        pitch = _row_pitch(region, 3 * Wr)
        org = org.to(region.device)                         # int32 [B,2]: the one small copy of the call

        def call(b0, nb, wp, bp, o32, o16, tail):           # the origins are sliced, never the region
            if shrink == 1:
                _lib.check(lib.toad_resnet50_trunc_fwd_u8_region(region.data_ptr(), pitch, Hr, Wr, org[b0:b0 + nb].data_ptr(), norm, wp, bp, o32, o16, *tail),
                           "toad_resnet50_trunc_fwd_u8_region")
            else:
                _lib.check(lib.toad_resnet50_trunc_fwd_u8_region_box(region.data_ptr(), pitch, Hr, Wr, org[b0:b0 + nb].data_ptr(), norm, wp, bp, o32, o16,
                                                                     *tail[:3], shrink, *tail[3:]), "toad_resnet50_trunc_fwd_u8_region_box")
        return self._chunked(out, H, W, lib.toad_resnet50_trunc_u8_ws_bytes, call)

    def forward_u8_regions(self, regions, origins, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, out_dtype: torch.dtype = torch.float32,
                           shrink=1) -> torch.Tensor:
        """``forward_u8_region`` for a slide that arrives as a LIST of regions (strips, blocks, any windows) -> [B,1024] bag rows, fp32 or fp16.

        ``regions``: a list or tuple of 1 .. ``ops.TILE_REGIONS_MAX`` uint8 [Hr,Wr,3] tensors on one HIP device, each laid out as ``forward_u8_region`` wants
        its region, each with its own extent, pitch and base address; the same tensor or overlapping views of one image may appear several times.
        ``origins``: [B,3] integers (x, y, k) on the HOST - the top-left pixel of tile b in the coordinates of ``regions[k]``; every k and every tile is
        checked here before anything is launched (``ops.check_region_origins``). The result is bitwise
        ``forward_u8(torch.stack([regions[k][y:y+H, x:x+W] for x, y, k in origins]), mean, std, out_dtype)`` - with ``shrink = 2`` ``forward_u8`` of the
        box-filtered footprints, as ``forward_u8_region`` defines them. The network scales every layer by an abs-max over the tiles of a call, so a bag row
        depends on the tiles that share its call: this call makes the cut of the slide invisible - the same tiles in the same order give the bits of
        ``forward_u8_region`` on the whole slide. More than ``max_tiles_per_call`` triples run in chunks exactly as there: the triples are sliced, never
        the regions, and every chunk gets the same list. Refusals in ``forward_u8_region``'s order - shrink, the model and the regions (RuntimeError, the
        first offending region named), then the origins - with one addition in front of the model's: ``regions`` not being a list or tuple (TypeError) and
        their count (ValueError), because every later check, the model's device test included, looks at ``regions[0]``."""
        check_shrink(shrink)
        if shrink != 1:
            shrunk_tile(tile, shrink)
        if isinstance(regions, torch.Tensor) or not isinstance(regions, (list, tuple)):
            raise TypeError(f"forward_u8_regions expects a list or tuple of uint8 [Hr,Wr,3] regions (one region: forward_u8_region), got {type(regions).__name__}")
        n = len(regions)
        if n < 1 or n > TILE_REGIONS_MAX:
            raise ValueError(f"forward_u8_regions: {n} regions: one call takes 1 .. {TILE_REGIONS_MAX} (ops.TILE_REGIONS_MAX); more regions per call are not built")

        def problem(k, r):
            return (f"forward_u8_regions expects uint8 [Hr,Wr,3] tensors, got {type(r).__name__} as regions[{k}]" if not isinstance(r, torch.Tensor) else
                    f"forward_u8_regions expects uint8 regions, got {r.dtype} as regions[{k}]" if r.dtype != torch.uint8 else
                    f"forward_u8_regions expects channels-last [Hr,Wr,3] regions, got {tuple(r.shape)} as regions[{k}]" if r.dim() != 3 or r.shape[2] != 3 else
                    f"out_dtype must be torch.float32 or torch.float16, got {out_dtype}" if out_dtype not in (torch.float32, torch.float16) else
                    f"expected uint8 [Hr,Wr,3] tensors on the HIP device (no CPU fallback), got regions[{k}] on {r.device}" if not r.is_cuda else
                    f"forward_u8_regions expects regions with stride(2) == 1, stride(1) == 3 and a row pitch stride(0) >= 3 Wr (rows are read in place, "
                    f"there is no hidden copy), got strides {tuple(r.stride())} for shape {tuple(r.shape)} as regions[{k}]" if not region_layout_ok(r) else
                    f"regions[{k}] is on {r.device}, regions[0] on {regions[0].device}: all regions of a call must be on one device"
                    if r.device != regions[0].device else None)
        found = next((p for p in (problem(k, r) for k, r in enumerate(regions)) if p is not None), None)
        self._ready(regions[0], found)
        (FH, FW), (H, W) = shrunk_tile(tile, shrink)        # the footprint the triples are checked for, the tile the network and the chunking see
        org = check_region_origins(origins, [(r.shape[0], r.shape[1]) for r in regions], FH, FW)
        B = org.shape[0]
        norm = norm_constants_u8(mean, std)
        dev = regions[0].device
        out = torch.empty(B, 1024, device=dev, dtype=out_dtype)
        if B == 0:
            return out
        lib = _lib.load()
        arr, _ = region_table(regions)                      # the HOST descriptor table: every chunk gets the same one
        org = org.to(dev)                                   # int32 [B,3]: the one small copy of the call

        def call(b0, nb, wp, bp, o32, o16, tail):           # the triples are sliced, never the regions
            _lib.check(lib.toad_resnet50_trunc_fwd_u8_regions(arr, n, org[b0:b0 + nb].data_ptr(), norm, wp, bp, o32, o16, *tail[:3], shrink, *tail[3:]),
                       "toad_resnet50_trunc_fwd_u8_regions")
        return self._chunked(out, H, W, lib.toad_resnet50_trunc_u8_ws_bytes, call)


def resnet50_baseline(pretrained: bool = False) -> ResNet_Baseline:
    """Constructs the modified (truncated) ResNet-50 (reference :111-119)."""
    model = ResNet_Baseline(Bottleneck_Baseline, [3, 4, 6, 3])
    if pretrained:
        raise RuntimeError("pretrained=True downloads ImageNet weights in the reference (model_zoo, :122); there is no network here - "
                           "load a local torchvision resnet50 checkpoint with model.load_state_dict(sd, strict=False)")
    return model
