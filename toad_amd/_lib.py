"""ctypes binding of libtoad_hip.so (the C ABI declared in include/toad_hip.h).

There is no CPU fallback: if the shared library is missing or a symbol is absent the import
fails loudly, and every op refuses non-CUDA tensors.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtoad_hip.so")      # the one library the product loads (A/B builds: tools/ab/select_lib.py rebinds this in the TOOL's process)
ABI_VERSION = 15

P, I64, I, F, SZ, U64 = c_void_p, c_int64, c_int, c_float, c_size_t, c_uint64


class ToadHeatWindow(ctypes.Structure):
    """One window of toad_region_heat_windows_u8's HOST array (include/toad_hip.h): region and out are device addresses."""
    _fields_ = [("region", c_void_p), ("pitch", c_int64), ("Hr", c_int), ("Wr", c_int), ("wx", c_int), ("wy", c_int), ("out", c_void_p),
                ("out_pitch", c_int64)]


class ToadHeatPyramidWindow(ctypes.Structure):
    """One window of toad_region_heat_pyramid_windows_u8's HOST array (include/toad_hip.h): region and outs[k] are device addresses, outs and out_pitches
    indexed by k = log2(down); a level that is empty for the window keeps a null address."""
    _fields_ = [("region", c_void_p), ("pitch", c_int64), ("Hr", c_int), ("Wr", c_int), ("wx", c_int), ("wy", c_int), ("outs", c_void_p * 6),
                ("out_pitches", c_int64 * 6)]


class ToadSatWindow(ctypes.Structure):
    """One window of toad_regions_saturation_u8's HOST array (include/toad_hip.h): region and plane are device addresses."""
    _fields_ = [("region", c_void_p), ("pitch", c_int64), ("Hr", c_int), ("Wr", c_int), ("plane", c_void_p), ("plane_pitch", c_int64)]


class ToadTileRegion(ctypes.Structure):
    """One region of the HOST array of the toad_*_regions_* extractor calls (include/toad_hip.h): region is a device address. 24 bytes."""
    _fields_ = [("region", c_void_p), ("pitch", c_int64), ("Hr", c_int), ("Wr", c_int)]


class ToadWgradJob(ctypes.Structure):
    """One job of toad_linear_wgrad_batch_f32's HOST array (include/toad_hip.h): every pointer is a device address."""
    _fields_ = [("dY", c_void_p), ("dy_amax", c_void_p), ("X", c_void_p), ("x_amax", c_void_p), ("dW", c_void_p), ("db", c_void_p),
                ("N", c_int64), ("K", c_int64), ("ws", c_void_p)]


# name -> (restype, argtypes); mirrors include/toad_hip.h one to one
SIGNATURES = {
    "toad_abi_version": (I, []),
    "toad_last_error": (c_char_p, []),
    "toad_fallback_launches": (I64, []),
    "toad_amax_floats": (SZ, [I64]),
    "toad_absmax_rows256_f32": (I, [P, I64, I64, P, P]),
    "toad_linear_h2_ok": (I, [I64, I64, I64]),
    "toad_linear_ws_bytes": (SZ, [I64, I64, I64]),
    "toad_relu_bits_bytes": (SZ, [I64, I64]),
    "toad_relu_bits_plan": (I, [I64, I64, I64, I, P]),
    "toad_nt_plan": (I, [I64, I64, I64, I, P]),
    "toad_linear_act_fwd_f32": (I, [P, P, P, P, I64, I64, I64, I, F, U64, P, P, P, P, SZ, P]),
    "toad_linear_dgrad_f32": (I, [P, P, P, P, F, P, I64, I64, I64, P, P, P, I, P, P, P, P, SZ, P]),
    "toad_dropout_mask_f32": (I, [P, I64, F, U64, P]),
    "toad_linear_wgrad_ws_bytes": (SZ, [I64, I64, I64]),
    "toad_linear_wgrad_f32": (I, [P, P, P, P, I64, I64, I64, F, P, P, P, SZ, P]),
    "toad_transpose_f32": (I, [P, P, I64, I64, P]),
    "toad_gated_pool_ws_bytes": (SZ, [I64, I, I, I]),
    "toad_gated_pool_fwd_f32": (I, [P, P, I64, P, P, P, P, P, P, P, SZ, I64, I, I, I, F, U64, U64, P]),
    "toad_gated_pool_bwd_ws_bytes": (SZ, [I64, I, I, I]),
    "toad_gated_pool_bwd_f32": (I, [P, P, I64, P, P, P, P, P, P, P, P, P, I64, P, P, P, F, P, P, SZ, I64, I, I, I, F, U64, U64, P]),
    "toad_heads_fwd_f32": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "toad_heads_bwd_f32": (I, [P, P, P, P, P, P, P, P, P, P, P, P, F, I, I, P]),
    "toad_heads_ce_fused_f32": (I, [P, P, P, P, P, P, P, P, F, F, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, F, I, I, P]),
    "toad_sgd_step_f32": (I, [P, P, P, I64, F, F, F, I64, P]),
    "toad_mtl_ce_fwd_bwd_f32": (I, [P, P, P, P, F, F, P, P, P, I, P]),
    "toad_adam_step_f32": (I, [P, P, P, P, I64, F, F, F, F, F, I64, P]),
    "toad_linear_act_res_fwd_f32": (I, [P, P, P, P, P, I64, I64, I64, I, P, SZ, P]),
    "toad_conv_nhwc_f32": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, P, SZ, P]),
    "toad_im2col_nhwc_f32": (I, [P, P, I, I, I, I, I, I, I, I, P]),
    "toad_im2col_stem_nchw_f32": (I, [P, P, I, I, I, P]),
    "toad_stem_s2d_nchw_f32": (I, [P, P, I, I, I, P]),
    "toad_stem_conv_s2d_f32": (I, [P, P, P, P, I, I, I, I, P, SZ, P]),
    "toad_stem_conv_pool_s2d_f32": (I, [P, P, P, P, I, I, I, P, SZ, P]),
    "toad_stem_pool_nchw_f32": (I, [P, P, P, P, I, I, I, P, SZ, P]),
    "toad_maxpool3x3s2_nhwc_f32": (I, [P, P, I, I, I, I, P]),
    "toad_avgpool_nhwc_f32": (I, [P, P, I, I, I, P]),
    "toad_resnet50_trunc_ws_bytes": (SZ, [I, I, I]),
    "toad_resnet50_trunc_fwd_f32": (I, [P, P, P, P, I, I, I, P, SZ, P]),
    "toad_mil_buffer_align": (SZ, [I64]),
    "toad_mil_arena_bytes": (SZ, [I64, I, I]),
    "toad_mil_arena_layout": (I, [I64, I, I, P]),
    "toad_mil_scratch_bytes": (SZ, [I64, I, I]),
    "toad_mil_fwd_f32": (I, [P, P, P, I64, I, I, F, U64, P, I, P, SZ, P, SZ, P]),
    "toad_mil_bwd_f32": (I, [P, P, F, P, I64, I, I, F, U64, P, SZ, P, P, P, P, P, P, P, SZ, P]),
    "toad_mil_step_ws_bytes": (SZ, [I64, I, I]),
    "toad_mil_step_f32": (I, [P, P, F, P, P, P, P, F, F, I64, I, I, F, U64, P, P, P, P, P, SZ, P, P]),
    "toad_mil_x16_ok": (I, [I64]),
    "toad_mil_fwd_x16_f32": (I, [P, P, P, I64, I, I, F, U64, I, P, SZ, P, SZ, P]),
    "toad_mil_bwd_x16_f32": (I, [P, P, F, P, I64, I, I, F, U64, P, SZ, P, P, P, P, P, P, SZ, P]),
    "toad_mil_step_x16_f32": (I, [P, P, F, P, P, P, P, F, F, I64, I, I, F, U64, P, P, P, P, SZ, P, P]),
    "toad_bag_planes_bytes": (SZ, [I64, I64]),
    "toad_bag_prepare_f32": (I, [P, I64, I64, P, P, P]),
    "toad_linear_wgrad_xp_f32": (I, [P, P, P, P, P, I64, I64, I64, F, P, P, SZ, P]),
    "toad_mil_fwd_xp_f32": (I, [P, P, P, P, I64, I, I, F, U64, I, P, SZ, P, SZ, P]),
    "toad_mil_bwd_xp_f32": (I, [P, P, F, P, P, I64, I, I, F, U64, P, SZ, P, P, P, P, P, P, SZ, P]),
    "toad_mil_multi_ws_bytes": (SZ, [I64, I, I, I]),
    "toad_mil_multi_step_f32": (I, [P, P, F, P, P, I, P, P, P, F, F, I, I, F, U64, P, P, P, P, SZ, P, P]),
    "toad_mil_step_xp_f32": (I, [P, P, F, P, P, P, P, P, F, F, I64, I, I, F, U64, P, P, P, P, SZ, P, P]),
    "toad_mil_multi_arena_bytes": (SZ, [I64, I, I, I]),
    "toad_mil_multi_arena_layout": (I, [I64, I, I, I, P]),
    "toad_mil_multi_scratch_bytes": (SZ, [I64, I, I, I]),
    "toad_mil_multi_fwd_f32": (I, [P, P, P, I, P, I, I, F, U64, P, SZ, P, SZ, P]),
    "toad_mil_multi_bwd_f32": (I, [P, P, F, P, P, I, I, I, F, U64, P, SZ, P, P, P, P, P, SZ, P]),
    # fp16 bags on the ragged multi-slide route: an additive extension of ABI 15 (the version number does not change)
    "toad_mil_multi_x16_ok": (I, [I64]),
    "toad_mil_multi_step_x16_f32": (I, [P, P, F, P, P, I, P, P, P, F, F, I, I, F, U64, P, P, P, P, SZ, P, P]),
    "toad_mil_multi_fwd_x16_f32": (I, [P, P, P, I, P, I, I, F, U64, P, SZ, P, SZ, P]),
    "toad_mil_multi_bwd_x16_f32": (I, [P, P, F, P, P, I, I, I, F, U64, P, SZ, P, P, P, P, P, SZ, P]),
    # uint8 NHWC tiles into the extractor: additive to ABI 15 as well
    "toad_tiles_u8_nhwc_to_nchw_f32": (I, [P, P, P, I, I, I, P]),
    "toad_stem_pool_nhwc_u8": (I, [P, P, P, P, P, I, I, I, P, SZ, P]),
    "toad_resnet50_trunc_u8_ws_bytes": (SZ, [I, I, I]),
    "toad_resnet50_trunc_fwd_u8": (I, [P, P, P, P, P, P, I, I, I, P, SZ, P]),
    # ... and tiles read by origin from one decoded uint8 region: additive to ABI 15 too
    "toad_tiles_u8_region_to_nchw_f32": (I, [P, I64, I, I, P, P, P, I, I, I, P]),
    "toad_stem_pool_region_u8": (I, [P, I64, I, I, P, P, P, P, P, I, I, I, P, SZ, P]),
    "toad_resnet50_trunc_fwd_u8_region": (I, [P, I64, I, I, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    # ... with a 2 x 2 box filter in front of the tile (shrink, after H and W; 1 = the calls above): additive to ABI 15
    "toad_tiles_u8_region_box_to_nchw_f32": (I, [P, I64, I, I, P, P, P, I, I, I, I, P]),
    "toad_stem_pool_region_box_u8": (I, [P, I64, I, I, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "toad_resnet50_trunc_fwd_u8_region_box": (I, [P, I64, I, I, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    # ... and the same three for a list of regions (regions: a HOST array of n ToadTileRegion; tiles: device int32 [B][3] = (x, y, k)): additive to ABI 15
    "toad_tiles_u8_regions_to_nchw_f32": (I, [ctypes.POINTER(ToadTileRegion), I, P, P, P, I, I, I, I, P]),
    "toad_stem_pool_regions_u8": (I, [ctypes.POINTER(ToadTileRegion), I, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "toad_resnet50_trunc_fwd_u8_regions": (I, [ctypes.POINTER(ToadTileRegion), I, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    # ... and the stage in front of them, tissue-pixel counts per cell and per lattice tile of a region: additive to ABI 15
    "toad_region_tissue_cells_u8": (I, [P, I64, I, I, I, I, I, P, P]),
    "toad_tissue_tile_counts": (I, [P, I, I, I, I, I, I, I, I, I, I, I, P, P]),
    # ... and the stage behind them, the tiles' scores rendered onto the region as a heat map: additive to ABI 15
    "toad_heat_cells": (I, [P, I, I, I, I, I, I, I, I, I, I, I, P, P]),
    "toad_region_heat_blend_u8": (I, [P, I64, I, I, P, I, I, I, P, I, I, P, I64, P]),
    # ... and the same canvas with the colour index (bilinear tent) and the alpha (tissue mask) per pixel: additive to ABI 15
    "toad_region_heat_blend_px_u8": (I, [P, I64, I, I, P, I, I, I, P, I, I, I, P, I64, I, I, I, I, P, I64, P]),
    # ... and that canvas at overview scale, down in 8, 16, 32, in one pass: additive to ABI 15
    "toad_region_heat_thumb_u8": (I, [P, I64, I, I, P, I, I, I, P, I, I, I, P, I64, I, I, I, I, P, I64, P]),
    # ... and any of these canvases for a window (wx, wy after Hr, Wr) of the image that the cell table and the mask plane describe: additive to ABI 15
    "toad_region_heat_window_u8": (I, [P, I64, I, I, I, I, P, I, I, I, P, I, I, I, P, I64, I, I, I, I, P, I64, P]),
    # ... and a list of such windows of one image in one call (windows: a HOST array of n ToadHeatWindow): additive to ABI 15
    "toad_region_heat_windows_u8": (I, [ctypes.POINTER(ToadHeatWindow), I, P, I, I, I, P, I, I, I, P, I64, I, I, I, I, P]),
    # ... and several levels of that pyramid from one read of the window (levels: a bit set; outs, out_pitches: HOST arrays of 6): additive to ABI 15
    "toad_region_heat_pyramid_u8": (I, [P, I64, I, I, I, I, P, I, I, I, P, I, ctypes.c_uint, I, P, I64, I, I, I, I, P, P, P]),
    # ... and those levels for a list of windows of one image in one call (windows: a HOST array of n ToadHeatPyramidWindow): additive to ABI 15
    "toad_region_heat_pyramid_windows_u8": (I, [ctypes.POINTER(ToadHeatPyramidWindow), I, P, I, I, I, P, I, ctypes.c_uint, I, P, I64, I, I, I, I, P]),
    # ... and the Gaussian blur of the cell table in front of any of these canvases (the taps are a HOST array): additive to ABI 15
    "toad_heat_cells_blur": (I, [P, I, I, P, I, P, P]),
    # ... and the second tissue selector, CLAM's recipe in integers (saturation plane, median, histogram, cells): additive to ABI 15
    "toad_region_saturation_u8": (I, [P, I64, I, I, I, I, P, I64, P]),
    "toad_plane_median_u8": (I, [P, I64, I, I, I, P, I64, P, P]),
    "toad_plane_cells_u8": (I, [P, I64, I, I, I, I, P, P]),
    # ... and its saturation plane for a list of windows in one call (windows: a HOST array of n ToadSatWindow): additive to ABI 15
    "toad_regions_saturation_u8": (I, [ctypes.POINTER(ToadSatWindow), I, I, I, P]),
    # ... and what follows its threshold, closing and the component / hole area filters (csrc/tissue_morph.hip): additive to ABI 15
    "toad_plane_close_u8": (I, [P, I64, I, I, I, I, P, I64, P]),
    "toad_plane_components_u8": (I, [P, I64, I, I, I, I, P, P, P]),
    "toad_plane_area_select_u8": (I, [P, P, I, I, I, I, P, I64, P]),
    # ... and bags as 8-bit e4m3 codes with one exponent, decoded behind their copy and quantised where they are made (csrc/bag_e4m3.hip): additive to ABI 15
    "toad_bag_dequant_e4m3": (I, [P, P, I, I64, I, P]),
    "toad_bag_quant_e4m3": (I, [P, I, P, I64, I, P]),
    # ... and a list of such bags, back to back with one exponent each, in one call (row_offsets, exps: HOST arrays): additive to ABI 15
    "toad_bags_dequant_e4m3": (I, [P, P, I, I64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), I, P]),
    "toad_bags_quant_e4m3": (I, [P, I, P, I64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), I, P]),
    "toad_bags_absmax_bits": (I, [P, I, P, I64, ctypes.POINTER(ctypes.c_int64), I, P]),
    # ... and the batched weight-gradient launch of the whole-slide calls on operands of the caller's choice (jobs: a HOST array of n ToadWgradJob;
    # a test/debug helper like toad_dropout_mask_f32): additive to ABI 15
    "toad_linear_wgrad_batch_f32": (I, [ctypes.POINTER(ToadWgradJob), I, I64, F, I, SZ, P]),
}

_lib = None


def load() -> ctypes.CDLL:
    """dlopen libtoad_hip.so and bind every declared symbol (raises if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first (python -m toad_amd.build). "
            "toad_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # (additions inside one ABI version - the x16 multi-slide calls of ABI 15 - cannot be told apart by toad_abi_version)
            raise RuntimeError(f"{LIB_PATH} does not export {name}: it was built from older sources; rebuild "
                               "(python -m toad_amd.build --force)") from None
        fn.restype = res
        fn.argtypes = args
    got = lib.toad_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"libtoad_hip.so ABI version {got} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().toad_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
