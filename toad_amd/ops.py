"""Thin tensor-level wrappers over the C ABI (pointers + sizes + the current HIP stream).

PyTorch is used for device memory and streams only; all arithmetic happens in libtoad_hip.so.
Shape/dtype/device/contiguity are validated here (the checks PyTorch's own ops would do for the
reference), the C side validates again and reports through toad_last_error().
"""
from __future__ import annotations

import ctypes
import numbers
from typing import Optional, Tuple

import torch

from . import _lib

ACT_NONE, ACT_RELU = 0, 1

# ---- optional per-op HIP-event timing (used by bench.py for the roofline figures) -------------
# Events are recorded on the stream the kernels are launched on (the current torch stream), so the
# elapsed time is device time of exactly the launches made by that C-ABI call.
_TIMING = None
_TIMING_LEVEL = 2          # 1: only the fused pool forward is bracketed (2 events per slide); 2: pool + the eight GEMM calls (18)
_EVENT_POOL = []           # events created AND recorded once ahead of time, so a timed region pays no event creation
_TIMING_STRIDE = 1         # whole-slide calls: bracket every k-th call only (an event packet costs ~5 us of stream time: 2 % of a 10k-patch step)
_TIMING_CALLS = 0


def enable_timing(on: bool = True, level: int = 2, prealloc: int = 0, stride: int = 1) -> None:
    """Switch per-op HIP-event timing on / off. Event packets are not free (18 per slide cost ~0.1 ms of stream time), so a
    throughput measurement uses level 1 (two events around the dominant kernel) and a separate instrumented loop level 2.
    `prealloc` events are created and materialised now, outside any timed region. `stride`: the whole-slide calls (mil_step,
    mil_multi_step) record their events on every stride-th call only (the first one included)."""
    global _TIMING, _TIMING_LEVEL, _TIMING_STRIDE, _TIMING_CALLS
    _TIMING = {} if on else None
    _TIMING_LEVEL = level
    _TIMING_STRIDE = max(1, int(stride))
    _TIMING_CALLS = 0
    if on and prealloc > 0 and torch.cuda.is_available():
        for _ in range(prealloc):
            e = torch.cuda.Event(enable_timing=True)
            e.record()                     # materialises the underlying hipEvent_t
            _EVENT_POOL.append(e)
        torch.cuda.synchronize()


def _timing_due() -> bool:
    global _TIMING_CALLS
    _TIMING_CALLS += 1
    return (_TIMING_CALLS - 1) % _TIMING_STRIDE == 0


def timing_call_count() -> int:
    """Whole-slide calls made since enable_timing (bracketed or not)."""
    return _TIMING_CALLS


def _take_event():
    if _EVENT_POOL:
        return _EVENT_POOL.pop()
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def collect_timing():
    """-> {op name: (calls, total milliseconds)}; synchronises the device."""
    if _TIMING is None:
        return {}
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in _TIMING.items()}


class _timed:
    __slots__ = ("name", "e0")

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _TIMING is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if _TIMING is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMING.setdefault(self.name, []).append((self.e0, e1))


def _chk(t: Optional[torch.Tensor], name: str, dtype=torch.float32, allow_none: bool = False):
    if t is None:
        if allow_none:
            return
        raise ValueError(f"{name} is None")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor: toad_amd has no CPU path (got {t.device})")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Per-op workspaces are scratch: one growing buffer per (device, stream) instead of one allocation per call. Work on a
# stream is ordered, so consecutive ops of that stream can share it; different streams (two models training side by side)
# get different buffers.
_WS_CACHE = {}


def _ws(nbytes: int, device, slot: str = "op") -> torch.Tensor:
    nbytes = max(int(nbytes), 16)
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(), slot)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes + (nbytes >> 3), dtype=torch.uint8, device=device)      # 12 % headroom: bags vary in length
        _WS_CACHE[key] = buf
    return buf


def release_workspaces() -> None:
    """Drop every cached workspace (they are re-created on demand)."""
    _WS_CACHE.clear()


def amax_floats(rows: int) -> int:
    return int(_lib.load().toad_amax_floats(int(rows)))


def absmax_rows256(x: torch.Tensor) -> torch.Tensor:
    """abs-max array of x [M,K]: one float per block of 256 rows (the operand scales of the fp16 two-piece GEMMs)."""
    _chk(x, "x")
    m, k = x.shape
    out = torch.empty((amax_floats(m),), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().toad_absmax_rows256_f32(_p(x), m, k, _p(out), _stream()), "toad_absmax_rows256_f32")
    return out


def h2_ok(m: int, n: int, k: int) -> bool:
    """True when the persistent fp16 two-piece kernel serves an [m,k] x [n,k]^T product."""
    return bool(_lib.load().toad_linear_h2_ok(int(m), int(n), int(k)))


def x16_ok(n: int) -> bool:
    """True when a [n, 1024] fp16 bag can go through the whole-slide fp16 entry points (toad_mil_*_x16_f32)."""
    return bool(_lib.load().toad_mil_x16_ok(int(n)))


def relu_bits_bytes(m: int, n: int) -> int:
    return int(_lib.load().toad_relu_bits_bytes(int(m), int(n)))


# ---- ONE arithmetic (round 6) -------------------------------------------------------------------------------------------------------------
# The fp16 two-piece GEMMs take reductions in whole 32-deep stages, 16-byte output rows and operands they can address with 32-bit row offsets
# (toad_linear_h2_ok). Every shape TOAD itself builds qualifies; a standalone Attn_Net_Gated of another (L, D) (models/model_toad.py:19 takes any)
# used to fall through to the exact-fp32 MFMA kernels inside the library (a 5x lower ceiling and another rounding). The per-op wrappers below
# ZERO-PAD such operands instead - padded products are exactly zero, padded output columns are sliced off - and cut operands of 2^32 bytes and
# more into row chunks, so every public Python entry point runs on the two-piece kernels (tests/test_gpu_h2.py counts the library's fallback
# launches: toad_fallback_launches). The exact-fp32 kernels remain in the library only for raw C-ABI callers that pass such shapes unpadded.
_K_STAGE = 32
_CHUNK_ROWS = 4092 * 256                        # csrc/step.hip kChunkRows: rows of one NT launch on a 1024-wide fp32 operand (32-bit byte offsets)
_CHUNK_SEED_STEP = 0xD1B54A32D192ED03          # csrc/step.hip kChunkSeedStep: train-mode dropout stream of row chunk j = seed + j * this
_M64 = 0xFFFFFFFFFFFFFFFF


def _pad_cols(t: Optional[torch.Tensor], to: int) -> Optional[torch.Tensor]:
    """t [..., c] -> [..., to] with zero columns appended (a copy; only shapes outside the kernels' envelope pay it)."""
    if t is None or t.shape[-1] == to:
        return t
    return torch.nn.functional.pad(t, (0, to - t.shape[-1])).contiguous()


def _up(v: int, q: int) -> int:
    return (v + q - 1) // q * q


def _row_chunks(m: int, row_bytes: int):
    """Row ranges of one NT launch each. By ROWS, with the fixed step of the whole-slide calls (csrc/step.hip nt_rows: one launch up to
    _CHUNK_ROWS rows, then chunks of _CHUNK_ROWS), whatever the operand's width up to 1024 floats: the forward of a layer and the dgrad that
    reads its one-bit ReLU image have operands of different widths and must still cut the rows at the same places, since a launch reads the
    image by ITS OWN tile plan (toad_relu_bits_plan). Only rows wider than 1024 floats take a smaller step (32-bit byte offsets)."""
    step = _CHUNK_ROWS if _CHUNK_ROWS * row_bytes < (1 << 32) else max(256, ((1 << 32) - 1) // row_bytes // 256 * 256)
    if m <= step:
        return [(0, m)]
    return [(r0, min(m, r0 + step)) for r0 in range(0, m, step)]


def _bits_chunks_ok(m: int, row_bytes: int) -> bool:
    """True when an operand of this width is cut like every operand of at most 1024 floats per row - the only geometry in which a one-bit ReLU
    image is produced (linear_act_fwd) or consumed (linear_dgrad); any other cut masks with the fp32 activations."""
    return _row_chunks(m, row_bytes) == _row_chunks(m, 4)


def linear_act_fwd(x, w, b, act: int, out: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0,
                   x_amax: Optional[torch.Tensor] = None, want_amax: bool = False, want_bits: bool = False,
                   bits_out: Optional[torch.Tensor] = None):
    """Y = dropout_p(act(X W^T + b)); X [M,K], W [N,K], b [N] or None. drop_p = 0 disables dropout.
    x_amax: abs-max array of X (else measured inside). want_amax: also return the abs-max array of Y -> (Y, y_amax).
    want_bits (act = RELU, h2_ok shapes): also return the one-bit image of Y for the dgrad of this layer -> (Y, y_amax, bits); bits is None
    where no image is produced (an output width that is not a multiple of 4, rows wider than 1024 floats cut into chunks).
    bits_out (implies want_bits): uint8 destination of the image, at least relu_bits_bytes(M, N) bytes; row chunks write their slices of it.
    Shapes outside the two-piece kernels' envelope are zero-padded (K to a multiple of 32, N to a multiple of 4) and operands of more than
    _CHUNK_ROWS rows run as row chunks (_row_chunks). Train-mode dropout then draws chunk j's masks from drop_seed + j * kChunkSeedStep at the
    chunk-local element index: for operands of at most 1024 floats per row these are the chunks, and therefore the masks, of the whole-slide
    calls (csrc/step.hip nt_rows); wider rows are cut into shorter chunks and draw other masks."""
    _chk(x, "x"); _chk(w, "w"); _chk(b, "b", allow_none=True); _chk(x_amax, "x_amax", allow_none=True)
    _chk(bits_out, "bits_out", dtype=torch.uint8, allow_none=True)
    want_bits = want_bits or bits_out is not None
    m, k = x.shape
    n, k2 = w.shape
    if k != k2 or (b is not None and b.numel() != n):
        raise ValueError(f"linear_act_fwd: shape mismatch x{tuple(x.shape)} w{tuple(w.shape)}")
    kp, np_ = _up(k, _K_STAGE), _up(n, 4)
    chunks = _row_chunks(m, kp * 4)
    if kp != k or np_ != n or len(chunks) > 1:
        if drop_p > 0 and np_ != n:
            raise NotImplementedError("linear_act_fwd: dropout with an output width that is not a multiple of 4")
        xp, wp = _pad_cols(x, kp), _pad_cols(w, kp)
        if np_ != n:
            wp = torch.nn.functional.pad(wp, (0, 0, 0, np_ - n)).contiguous()
            bp = None if b is None else torch.nn.functional.pad(b, (0, np_ - n)).contiguous()
        else:
            bp = b
        yp = out if (out is not None and np_ == n) else torch.empty((m, np_), dtype=torch.float32, device=x.device)
        # the image: one buffer, every chunk writes the blocks of its rows (chunks start at multiples of 256 rows). Only in the chunk geometry
        # the dgrad of the layer will use as well (_bits_chunks_ok), and only where the kernel that writes it runs
        bits = None
        if want_bits and np_ == n and _bits_chunks_ok(m, kp * 4) and all(h2_ok(r1 - r0, n, kp) for r0, r1 in chunks):
            nbits = relu_bits_bytes(m, n)
            if bits_out is not None and bits_out.numel() < nbits:
                raise ValueError(f"linear_act_fwd: bits_out needs {nbits} bytes")
            bits = bits_out[:nbits] if bits_out is not None else torch.empty((nbits,), dtype=torch.uint8, device=x.device)
        per_blk = relu_bits_bytes(256, n)
        amaxs = []
        for j, (r0, r1) in enumerate(chunks):
            b0, b1 = r0 // 256, (r1 + 255) // 256
            xa = None if x_amax is None else x_amax[b0:b1].contiguous()
            res = linear_act_fwd(xp[r0:r1], wp, bp, act, out=yp[r0:r1], drop_p=drop_p, drop_seed=(drop_seed + j * _CHUNK_SEED_STEP) & _M64,
                                 x_amax=xa, want_amax=want_amax or want_bits, bits_out=None if bits is None else bits[b0 * per_blk:b1 * per_blk])
            if want_amax or want_bits:
                amaxs.append(res[1])
        y = yp if np_ == n else yp[:, :n].contiguous()
        if out is not None and y is not out:
            out.copy_(y); y = out
        if want_bits:
            return y, torch.cat(amaxs), bits
        return (y, torch.cat(amaxs)) if want_amax else y
    y = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=x.device)
    _chk(y, "out")
    lib = _lib.load()
    y_amax = torch.empty((amax_floats(m),), dtype=torch.float32, device=x.device) if (want_amax or want_bits) else None
    bits = None
    if want_bits and h2_ok(m, n, k):
        nbits = relu_bits_bytes(m, n)
        if bits_out is not None and bits_out.numel() < nbits:
            raise ValueError(f"linear_act_fwd: bits_out needs {nbits} bytes")
        bits = bits_out[:nbits] if bits_out is not None else torch.empty((nbits,), dtype=torch.uint8, device=x.device)
    ws = _ws(lib.toad_linear_ws_bytes(m, n, k), x.device)
    with _timed("gemm_fwd"):
        _lib.check(lib.toad_linear_act_fwd_f32(_p(x), _p(w), _p(b), _p(y), m, k, n, act, float(drop_p), int(drop_seed),
                                               _p(x_amax), _p(y_amax), _p(bits), _p(ws), ws.numel(), _stream()), "toad_linear_act_fwd_f32")
    if want_bits:
        return y, y_amax, bits
    return (y, y_amax) if want_amax else y


def transpose(w: torch.Tensor) -> torch.Tensor:
    _chk(w, "w")
    r, c = w.shape
    out = torch.empty((c, r), dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().toad_transpose_f32(_p(w), _p(out), r, c, _stream()), "toad_transpose_f32")
    return out


def linear_dgrad(dy, wt, addend=None, relu_src=None, out: Optional[torch.Tensor] = None, mask_scale: float = 1.0,
                 pool=None, dy_amax: Optional[torch.Tensor] = None, want_amax: bool = False, relu_bits: Optional[torch.Tensor] = None):
    """dX = (dY W + addend + pool) * (relu_src > 0) * mask_scale; dY [M,N], wt = W^T [K,N].
    pool = (A_raw [M,T], stats [T,2], dM [T,K]): the attention-pooling gradient sum_t softmax(A_raw)[:,t] dM[t,:], recomputed in
    the epilogue instead of read from an [M,K] buffer (needs h2_ok(M, K, N)). relu_bits: the one-bit image of relu_src
    (linear_act_fwd(..., want_bits=True) of the same layer)."""
    _chk(dy, "dy"); _chk(wt, "wt"); _chk(addend, "addend", allow_none=True); _chk(relu_src, "relu_src", allow_none=True)
    _chk(relu_bits, "relu_bits", dtype=torch.uint8, allow_none=True)
    _chk(dy_amax, "dy_amax", allow_none=True)
    m, n = dy.shape
    k, n2 = wt.shape
    if n != n2:
        raise ValueError("linear_dgrad: shape mismatch")
    np_, kp = _up(n, _K_STAGE), _up(k, 4)
    chunks = _row_chunks(m, np_ * 4)
    if np_ != n or kp != k or len(chunks) > 1:               # outside the two-piece kernels' envelope: zero padding / row chunks (see linear_act_fwd)
        dyp, wtp = _pad_cols(dy, np_), _pad_cols(wt, np_)
        if kp != k:
            wtp = torch.nn.functional.pad(wtp, (0, 0, 0, kp - k)).contiguous()
            if relu_bits is not None:
                raise NotImplementedError("linear_dgrad: a bit image with an output width that is not a multiple of 4")
        addp, srcp = _pad_cols(addend, kp), _pad_cols(relu_src, kp)
        poolp = None if pool is None else (pool[0], pool[1], _pad_cols(pool[2], kp))
        dxp = out if (out is not None and kp == k) else torch.empty((m, kp), dtype=torch.float32, device=dy.device)
        if not _bits_chunks_ok(m, np_ * 4):                # not the chunks the forward of the layer wrote its image in: mask with relu_src alone
            relu_bits = None
        amaxs = []
        for (r0, r1) in chunks:
            b0, b1 = r0 // 256, (r1 + 255) // 256
            bits_c = None
            if relu_bits is not None:
                per_blk = relu_bits.numel() // max(amax_floats(m), 1)
                bits_c = relu_bits[b0 * per_blk:b1 * per_blk]
            res = linear_dgrad(dyp[r0:r1], wtp, None if addp is None else addp[r0:r1], None if srcp is None else srcp[r0:r1], out=dxp[r0:r1],
                               mask_scale=mask_scale, pool=None if poolp is None else (poolp[0][r0:r1], poolp[1], poolp[2]),
                               dy_amax=None if dy_amax is None else dy_amax[b0:b1].contiguous(), want_amax=want_amax, relu_bits=bits_c)
            if want_amax:
                amaxs.append(res[1])
        dxr = dxp if kp == k else dxp[:, :k].contiguous()
        if out is not None and dxr is not out:
            out.copy_(dxr); dxr = out
        return (dxr, torch.cat(amaxs)) if want_amax else dxr
    dx = out if out is not None else torch.empty((m, k), dtype=torch.float32, device=dy.device)
    _chk(dx, "out")
    for t, nm in ((addend, "addend"), (relu_src, "relu_src"), (dx, "out")):
        if t is not None and tuple(t.shape) != (m, k):
            raise ValueError(f"linear_dgrad: {nm} must be [{m},{k}]")
    pa = ps = pd = None
    pt = 0
    if pool is not None:
        pa, ps, pd = pool
        _chk(pa, "pool A_raw"); _chk(ps, "pool stats"); _chk(pd, "pool dM")
        pt = pa.shape[1]
        if pa.shape[0] != m or tuple(ps.shape) != (pt, 2) or tuple(pd.shape) != (pt, k):
            raise ValueError("linear_dgrad: pooling-addend shapes must be A_raw [M,T], stats [T,2], dM [T,K]")
    lib = _lib.load()
    dx_amax = torch.empty((amax_floats(m),), dtype=torch.float32, device=dy.device) if want_amax else None
    ws = _ws(lib.toad_linear_ws_bytes(m, k, n), dy.device)
    with _timed("gemm_dgrad"):
        _lib.check(lib.toad_linear_dgrad_f32(_p(dy), _p(wt), _p(addend), _p(relu_src), float(mask_scale), _p(dx), m, n, k,
                                             _p(pa), _p(ps), _p(pd), pt, _p(dy_amax), _p(dx_amax), _p(relu_bits), _p(ws), ws.numel(),
                                             _stream()), "toad_linear_dgrad_f32")
    return (dx, dx_amax) if want_amax else dx


def linear_wgrad(dy, x, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                 beta: float = 0.0, want_db: bool = True, dy_amax: Optional[torch.Tensor] = None,
                 x_amax: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dW = beta*dW + dY^T X; db = beta*db + colsum(dY). dy_amax / x_amax: abs-max arrays of the operands (else measured).
    ``x`` may be a PreparedBag (plane-tiled input operand: toad_linear_wgrad_xp_f32)."""
    prepared = getattr(x, "is_prepared_bag", False)
    _chk(dy, "dy"); _chk(dy_amax, "dy_amax", allow_none=True)
    if not prepared:
        _chk(x, "x"); _chk(x_amax, "x_amax", allow_none=True)
    m, n = dy.shape
    m2, k = x.shape
    if m != m2:
        raise ValueError("linear_wgrad: shape mismatch")
    if not prepared and (n % 4 or k % 4):                    # 16-byte rows for the TN kernels: zero columns, sliced off the result
        np_, kp = _up(n, 4), _up(k, 4)
        dwp, dbp = linear_wgrad(_pad_cols(dy, np_), _pad_cols(x, kp), None, None, 0.0, want_db or db is not None, dy_amax, x_amax)
        dwn = dwp[:n, :k]
        if dw is None:
            dw = dwn.contiguous()
        else:
            dw.mul_(beta).add_(dwn) if beta != 0.0 else dw.copy_(dwn)
        if dbp is not None:
            if db is None:
                db = dbp[:n].contiguous()
            else:
                db.mul_(beta).add_(dbp[:n]) if beta != 0.0 else db.copy_(dbp[:n])
        return dw, db
    if dw is None:
        dw = torch.empty((n, k), dtype=torch.float32, device=dy.device); beta = 0.0
    if db is None and want_db:
        db = torch.empty((n,), dtype=torch.float32, device=dy.device)
    _chk(dw, "dw"); _chk(db, "db", allow_none=True)
    lib = _lib.load()
    nbytes = lib.toad_linear_wgrad_ws_bytes(m, n, k)
    ws = _ws(nbytes, dy.device, "wgrad")
    with _timed("gemm_wgrad"):
        if prepared:
            _lib.check(lib.toad_linear_wgrad_xp_f32(_p(dy), _p(x.planes), _p(x.amax), _p(dw), _p(db), m, n, k, float(beta), _p(dy_amax),
                                                    _p(ws), ws.numel(), _stream()), "toad_linear_wgrad_xp_f32")
        else:
            _lib.check(lib.toad_linear_wgrad_f32(_p(dy), _p(x), _p(dw), _p(db), m, n, k, float(beta), _p(dy_amax), _p(x_amax),
                                                 _p(ws), ws.numel(), _stream()), "toad_linear_wgrad_f32")
    return dw, db


def linear_wgrad_batch_ws_bytes(m: int, shapes) -> int:
    """Bytes of ONE job's workspace for linear_wgrad_batch over m rows; shapes = [(N, K)] of all its jobs. The launch runs at most one item per
    workgroup, so it cuts the rows into at most 256 // (tiles of all jobs) splits of whole 32-row stages; the per-op sizes alone can be too small
    for that (a 300-row call of the model's three products: 10 splits against the per-op plans' 5)."""
    lib = _lib.load()
    tiles = sum(((n + 255) // 256) * ((k + 255) // 256) for n, k in shapes)
    splits = max(min(256 // max(tiles, 1), (m + 31) // 32), 1)
    return max(max(int(lib.toad_linear_wgrad_ws_bytes(m, n, k)) for n, k in shapes),
               splits * max(n * k + n for n, k in shapes) * 4 + (2 * amax_floats(m) + 64) * 4)


def linear_wgrad_batch(jobs, outs=None, beta: float = 0.0, want_db: bool = True, ws=None):
    """Two or three weight gradients over the same M rows in the ONE batched launch the whole-slide calls use (toad_linear_wgrad_batch_f32; a
    test/debug entry: those calls hand the launch operands that other kernels produced). jobs: [(dy [M,N], x [M,K], dy_amax, x_amax)]; the x of
    the last of three may be float16 (its x_amax is ignored). outs: [(dw, db | None)] destinations per job (else allocated, beta = 0).
    Returns [(dw, db)]. ws: one uint8 workspace per job (the library is told the smallest of their sizes); else job i's is the cached buffer
    of slot "wgrad_batch{i}" (linear_wgrad_batch_ws_bytes)."""
    lib = _lib.load()
    n_jobs = len(jobs)
    if n_jobs < 1:
        raise ValueError("linear_wgrad_batch: no jobs")
    m = jobs[0][0].shape[0]
    x16 = jobs[-1][1].dtype == torch.float16
    res, shapes = [], []
    for i, (dy, x, dy_amax, x_amax) in enumerate(jobs):
        half = x16 and i == n_jobs - 1
        _chk(dy, "dy"); _chk(x, "x", dtype=torch.float16 if half else torch.float32)
        _chk(dy_amax, "dy_amax"); _chk(x_amax, "x_amax", allow_none=half)
        if dy.shape[0] != m or x.shape[0] != m:
            raise ValueError("linear_wgrad_batch: every operand must have the same number of rows")
        n, k = dy.shape[1], x.shape[1]
        shapes.append((n, k))
        if outs is None:
            dw = torch.empty((n, k), dtype=torch.float32, device=dy.device)
            db = torch.empty((n,), dtype=torch.float32, device=dy.device) if want_db else None
        else:
            dw, db = outs[i]
            _chk(dw, "dw"); _chk(db, "db", allow_none=True)
            if tuple(dw.shape) != (n, k) or (db is not None and db.numel() != n):
                raise ValueError("linear_wgrad_batch: destination shapes must be dw [N,K], db [N]")
        res.append((dw, db))
    if outs is None:
        beta = 0.0
    if ws is None:
        each = linear_wgrad_batch_ws_bytes(m, shapes)
        wss = [_ws(each, jobs[0][0].device, f"wgrad_batch{i}") for i in range(n_jobs)]
    else:
        wss = list(ws)
        for t in wss:
            _chk(t, "ws", dtype=torch.uint8)
        if len(wss) != n_jobs:
            raise ValueError("linear_wgrad_batch: one workspace per job")
        each = min(t.numel() for t in wss)
    arr = (_lib.ToadWgradJob * n_jobs)()
    for i, ((dy, x, dy_amax, x_amax), (dw, db), (n, k), wsi) in enumerate(zip(jobs, res, shapes, wss)):
        arr[i] = _lib.ToadWgradJob(_p(dy), _p(dy_amax), _p(x), _p(x_amax), _p(dw), _p(db), n, k, _p(wsi))
    with _timed("gemm_wgrad_batch"):
        _lib.check(lib.toad_linear_wgrad_batch_f32(arr, n_jobs, m, float(beta), 1 if x16 else 0, each, _stream()), "toad_linear_wgrad_batch_f32")
    return res


def dropout_mask(n: int, drop_p: float, drop_seed: int, device) -> torch.Tensor:
    """The multiplier (0 or 1/(1-p)) the kernels apply to flat element e under ``drop_seed`` (never stored by them)."""
    out = torch.empty((n,), dtype=torch.float32, device=device)
    _lib.check(_lib.load().toad_dropout_mask_f32(_p(out), n, float(drop_p), int(drop_seed), _stream()), "toad_dropout_mask_f32")
    return out


def gated_pool_fwd(p: torch.Tensor, d: int, h: Optional[torch.Tensor], wc, bc, drop_p: float = 0.0, seed_a: int = 0, seed_b: int = 0):
    """p = [N, 2D] stacked pre-activations (Pa | Pb). Returns (A_raw [N,T], M [T,L], stats [T,2]);
    with h=None only A_raw is computed (attention_only)."""
    _chk(p, "p"); _chk(h, "h", allow_none=True); _chk(wc, "wc"); _chk(bc, "bc")
    n, ldp = p.shape
    t = wc.shape[0]
    if ldp != 2 * d or wc.shape[1] != d or bc.numel() != t:
        raise ValueError("gated_pool_fwd: shape mismatch")
    lib = _lib.load()
    a_raw = torch.empty((n, t), dtype=torch.float32, device=p.device)
    pb_ptr = p.data_ptr() + 4 * d
    if h is None:
        _lib.check(lib.toad_gated_pool_fwd_f32(_p(p), pb_ptr, ldp, None, _p(wc), _p(bc), _p(a_raw), None, None, None, 0,
                                               n, 512, d, t, float(drop_p), int(seed_a), int(seed_b), _stream()),
                   "toad_gated_pool_fwd_f32")
        return a_raw, None, None
    l = h.shape[1]
    if h.shape[0] != n:
        raise ValueError("gated_pool_fwd: h rows != p rows")
    m = torch.empty((t, l), dtype=torch.float32, device=p.device)
    stats = torch.empty((t, 2), dtype=torch.float32, device=p.device)
    ws = _ws(lib.toad_gated_pool_ws_bytes(n, l, d, t), p.device, "pool")
    with _timed("pool_fwd"):
        _lib.check(lib.toad_gated_pool_fwd_f32(_p(p), pb_ptr, ldp, _p(h), _p(wc), _p(bc), _p(a_raw), _p(m), _p(stats),
                                               _p(ws), ws.numel(), n, l, d, t, float(drop_p), int(seed_a), int(seed_b),
                                               _stream()), "toad_gated_pool_fwd_f32")
    return a_raw, m, stats


def gated_pool_bwd(p, d: int, h, wc, a_raw, stats, m, dm, da_ext=None, dwc=None, dbc=None, beta: float = 0.0,
                   dp: Optional[torch.Tensor] = None, dh: Optional[torch.Tensor] = None,
                   drop_p: float = 0.0, seed_a: int = 0, seed_b: int = 0, want_dh: bool = True, want_amax: bool = False):
    """Returns (dP [N,2D], dH_pool [N,L] | None, dWc [T,D], dbc [T]) (+ the abs-max array of dP with want_amax).
    want_dh=False skips the [N,L] pooling gradient (linear_dgrad(pool=...) recomputes it in its epilogue)."""
    for t_, nm in ((p, "p"), (h, "h"), (wc, "wc"), (a_raw, "a_raw"), (stats, "stats"), (m, "m"), (dm, "dm")):
        _chk(t_, nm)
    _chk(da_ext, "da_ext", allow_none=True)
    n, ldp = p.shape
    l = h.shape[1]
    t = wc.shape[0]
    if ldp != 2 * d or tuple(a_raw.shape) != (n, t) or tuple(dm.shape) != (t, l) or tuple(m.shape) != (t, l):
        raise ValueError("gated_pool_bwd: shape mismatch")
    if dp is None:
        dp = torch.empty_like(p)
    if dh is None and want_dh:
        dh = torch.empty_like(h)
    if dwc is None:
        dwc = torch.empty_like(wc); dbc = torch.empty((t,), dtype=torch.float32, device=p.device); beta = 0.0
    _chk(dp, "dp"); _chk(dh, "dh", allow_none=True); _chk(dwc, "dwc"); _chk(dbc, "dbc")
    lib = _lib.load()
    dp_amax = torch.empty((amax_floats(n),), dtype=torch.float32, device=p.device) if want_amax else None
    ws = _ws(lib.toad_gated_pool_bwd_ws_bytes(n, l, d, t), p.device, "pool")
    with _timed("pool_bwd"):
        _lib.check(lib.toad_gated_pool_bwd_f32(_p(p), p.data_ptr() + 4 * d, ldp, _p(h), _p(wc), _p(a_raw), _p(stats), _p(m),
                                               _p(dm), _p(da_ext), _p(dp), dp.data_ptr() + 4 * d, ldp, _p(dh), _p(dwc),
                                               _p(dbc), float(beta), _p(dp_amax), _p(ws), ws.numel(), n, l, d, t, float(drop_p),
                                               int(seed_a), int(seed_b), _stream()),
                   "toad_gated_pool_bwd_f32")
    if want_amax:
        return dp, dh, dwc, dbc, dp_amax
    return dp, dh, dwc, dbc


# ---- scores only, over a column block of the stacked pre-activations (standalone Attn_Net_Gated of any shape) -------------------------
# The pool kernels' covering instantiation takes D <= 512 (multiple of 4) and n_tasks <= 4. The scores are linear in the gate columns and
# independent per task, so any (D, n_tasks) is a sum over column blocks of <= 512 and a concatenation over task blocks of <= 4
# (toad_amd.model_toad._ScoresFn drives the blocks). ``p`` is the [N, 2*dtot] stacked pre-activation matrix; the block is columns
# [d0, d0 + wc.shape[1]) of its tanh half and of its sigmoid half.
def gate_scores_block_fwd(p: torch.Tensor, dtot: int, d0: int, wc: torch.Tensor, bc: torch.Tensor, drop_p: float = 0.0, seed_a: int = 0, seed_b: int = 0):
    """A_block [N, T_blk] = (tanh(Pa[:, blk]) * sigmoid(Pb[:, blk])) wc^T + bc for one (task block, column block)."""
    _chk(p, "p"); _chk(wc, "wc"); _chk(bc, "bc")
    n, ldp = p.shape
    t, d = wc.shape
    if ldp != 2 * dtot or d0 % 4 or d % 4 or dtot % 4 or d0 + d > dtot or d > 512 or t > 4 or bc.numel() != t:
        raise ValueError("gate_scores_block_fwd: bad block")
    a_raw = torch.empty((n, t), dtype=torch.float32, device=p.device)
    _lib.check(_lib.load().toad_gated_pool_fwd_f32(p.data_ptr() + 4 * d0, p.data_ptr() + 4 * (dtot + d0), ldp, None, _p(wc), _p(bc), _p(a_raw), None, None,
                                                   None, 0, n, 8, d, t, float(drop_p), int(seed_a), int(seed_b), _stream()), "toad_gated_pool_fwd_f32")
    return a_raw


def gate_scores_block_bwd(p: torch.Tensor, dtot: int, d0: int, wc: torch.Tensor, da: torch.Tensor, drop_p: float = 0.0, seed_a: int = 0, seed_b: int = 0):
    """Backward of gate_scores_block_fwd for the external gradient ``da`` [N, T_blk]: returns (dPa_blk [N, d], dPb_blk [N, d], dWc_blk, dbc_blk).
    The pooled backward is reused with softmax weights of zero (stats = (0, inf)) and a zero pooled gradient: dS = dA exactly; its H operand is
    then multiplied by zeros only, so an 8-column dummy stands in for it (no limit on the layer's L)."""
    _chk(p, "p"); _chk(wc, "wc"); _chk(da, "da")
    n, ldp = p.shape
    t, d = wc.shape
    if ldp != 2 * dtot or d0 % 4 or d % 4 or dtot % 4 or d0 + d > dtot or d > 512 or t > 4 or tuple(da.shape) != (n, t):
        raise ValueError("gate_scores_block_bwd: bad block")
    dev = p.device
    lib = _lib.load()
    h = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    zeros_tl = torch.zeros((t, 8), dtype=torch.float32, device=dev)
    a0 = torch.zeros((n, t), dtype=torch.float32, device=dev)
    stats = torch.tensor([[0.0, float("inf")]] * t, dtype=torch.float32, device=dev)
    dp = torch.empty((n, 2 * d), dtype=torch.float32, device=dev)
    dwc = torch.empty_like(wc); dbc = torch.empty((t,), dtype=torch.float32, device=dev)
    ws = _ws(lib.toad_gated_pool_bwd_ws_bytes(n, 8, d, t), dev, "pool")
    _lib.check(lib.toad_gated_pool_bwd_f32(p.data_ptr() + 4 * d0, p.data_ptr() + 4 * (dtot + d0), ldp, _p(h), _p(wc), _p(a0), _p(stats), _p(zeros_tl), _p(zeros_tl),
                                           _p(da), _p(dp), dp.data_ptr() + 4 * d, 2 * d, None, _p(dwc), _p(dbc), 0.0, None, _p(ws), ws.numel(), n, 8, d, t,
                                           float(drop_p), int(seed_a), int(seed_b), _stream()), "toad_gated_pool_bwd_f32")
    return dp[:, :d], dp[:, d:], dwc, dbc


def heads_fwd(m, sex, wcls, bcls, wsite, bsite):
    """Returns (Mcat [2,L+1], logits [1,C], Y_prob, Y_hat [1,1] int64, site_logits [1,2], site_prob, site_hat)."""
    for t_, nm in ((m, "m"), (sex, "sex"), (wcls, "wcls"), (bcls, "bcls"), (wsite, "wsite"), (bsite, "bsite")):
        _chk(t_, nm)
    l = m.shape[1]
    c = wcls.shape[0]
    if m.shape[0] != 2 or wcls.shape[1] != l + 1 or tuple(wsite.shape) != (2, l + 1) or sex.numel() != 1:
        raise ValueError("heads_fwd: shape mismatch")
    dev = m.device
    mcat = torch.empty((2, l + 1), dtype=torch.float32, device=dev)
    logits = torch.empty((1, c), dtype=torch.float32, device=dev)
    y_prob = torch.empty((1, c), dtype=torch.float32, device=dev)
    y_hat = torch.empty((1, 1), dtype=torch.int64, device=dev)
    site_logits = torch.empty((1, 2), dtype=torch.float32, device=dev)
    site_prob = torch.empty((1, 2), dtype=torch.float32, device=dev)
    site_hat = torch.empty((1, 1), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().toad_heads_fwd_f32(_p(m), _p(sex), _p(wcls), _p(bcls), _p(wsite), _p(bsite), _p(mcat), _p(logits),
                                              _p(y_prob), _p(y_hat), _p(site_logits), _p(site_prob), _p(site_hat), l, c,
                                              _stream()), "toad_heads_fwd_f32")
    return mcat, logits, y_prob, y_hat, site_logits, site_prob, site_hat


def heads_bwd(mcat, dlogits, dsite, wcls, wsite, dmcat_ext=None, grads=None, beta: float = 0.0, want_dsex: bool = False):
    """Returns (dWcls, dbcls, dWsite, dbsite, dM [2,L]) (+ dsex [1] with want_dsex: the gradient of the `sex` scalar
    appended to both pooled rows, models/model_toad.py:99). grads = optional tuple of 4 destination tensors."""
    for t_, nm in ((mcat, "mcat"), (dlogits, "dlogits"), (dsite, "dsite"), (wcls, "wcls"), (wsite, "wsite")):
        _chk(t_, nm)
    _chk(dmcat_ext, "dmcat_ext", allow_none=True)
    l = mcat.shape[1] - 1
    c = wcls.shape[0]
    dev = mcat.device
    if dlogits.numel() != c or dsite.numel() != 2:
        raise ValueError("heads_bwd: shape mismatch")
    if grads is None:
        grads = (torch.empty_like(wcls), torch.empty((c,), dtype=torch.float32, device=dev),
                 torch.empty_like(wsite), torch.empty((2,), dtype=torch.float32, device=dev))
        beta = 0.0
    dwcls, dbcls, dwsite, dbsite = grads
    for t_, nm in ((dwcls, "dwcls"), (dbcls, "dbcls"), (dwsite, "dwsite"), (dbsite, "dbsite")):
        _chk(t_, nm)
    dm = torch.empty((2, l), dtype=torch.float32, device=dev)
    dsex = torch.empty((1,), dtype=torch.float32, device=dev) if want_dsex else None
    _lib.check(_lib.load().toad_heads_bwd_f32(_p(mcat), _p(dlogits), _p(dsite), _p(wcls), _p(wsite), _p(dmcat_ext),
                                              _p(dwcls), _p(dbcls), _p(dwsite), _p(dbsite), _p(dm), _p(dsex), float(beta), l, c,
                                              _stream()), "toad_heads_bwd_f32")
    if want_dsex:
        return dwcls, dbcls, dwsite, dbsite, dm, dsex
    return dwcls, dbcls, dwsite, dbsite, dm


def mtl_ce_fwd_bwd(logits, site_logits, label, site, w_cls: float = 0.75, w_site: float = 0.25):
    """Weighted two-task CE and its gradient. Returns (loss_vec[3] = loss, cls_loss, site_loss; dlogits; dsite)."""
    _chk(logits, "logits"); _chk(site_logits, "site_logits")
    _chk(label, "label", dtype=torch.int64); _chk(site, "site", dtype=torch.int64)
    c = logits.numel()
    dev = logits.device
    loss = torch.empty((3,), dtype=torch.float32, device=dev)
    dlogits = torch.empty((1, c), dtype=torch.float32, device=dev)
    dsite = torch.empty((1, 2), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().toad_mtl_ce_fwd_bwd_f32(_p(logits), _p(site_logits), _p(label), _p(site), float(w_cls),
                                                   float(w_site), _p(loss), _p(dlogits), _p(dsite), c, _stream()),
               "toad_mtl_ce_fwd_bwd_f32")
    return loss, dlogits, dsite


# ---- whole per-slide step in one C call (toad_mil_step_f32) -------------------------------------------
STEP_SLOTS = ("w1", "b1", "w2", "b2", "wab", "bab", "wc", "bc", "wcls", "bcls", "wsite", "bsite")
_GEMM_EVENT_NAMES = ("gemm_fwd", "gemm_fwd", "gemm_fwd", "gemm_wgrad", "gemm_dgrad", "gemm_wgrad", "gemm_dgrad", "gemm_wgrad")


def _slot_ptrs(slots, label: str = "", check: bool = True):
    """The STEP_SLOTS tensors of a weight or gradient dict as the pointer array the whole-slide entries take, each checked like any operand
    (``label`` prefixes the slot name in the message). The backward calls pass check=False for the weights: the forward that filled their
    arena has checked them."""
    ts = [slots[k] for k in STEP_SLOTS]
    if check:
        for k, t in zip(STEP_SLOTS, ts):
            _chk(t, label + k)
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# The bag kinds of the whole-slide calls and the suffix of their entry points, toad_mil_<family><suffix>_f32. The multi-slide families take the
# first two.
KIND_F32, KIND_F16, KIND_PREPARED = 0, 1, 2
_KIND_SUFFIX = ("", "_x16", "_xp")

# The argument list of each family's fp32 entry. The kinds differ in two places only: "bag" is one pointer for an fp32 / fp16 tensor and
# (planes, amax) for a PreparedBag, and the argument marked "*" exists in the fp32 list alone.
_MIL_FIELDS = {
    "step": "w g beta bag sex label site w_cls w_site n c d drop_p seed *x_amax loss logits slog ws ws_bytes events stream",
    "fwd": "w bag sex n c d drop_p seed *x_amax attention_only arena arena_bytes scratch scratch_bytes stream",
    "bwd": "w g beta bag n c d drop_p seed arena arena_bytes dlogits dsite da_ext dmcat_ext *dx dsex scratch scratch_bytes stream",
    "multi_step": "w g beta bag offsets b sex label site w_cls w_site c d drop_p seed loss logits slog ws ws_bytes events stream",
    "multi_fwd": "w bag offsets b sex c d drop_p seed arena arena_bytes scratch scratch_bytes stream",
    "multi_bwd": "w g beta bag offsets b c d drop_p seed arena arena_bytes dlogits dsite da_ext dmcat_ext scratch scratch_bytes stream",
}
_MIL_FIELDS = {family: tuple(fields.split()) for family, fields in _MIL_FIELDS.items()}
# family -> (position of the bag, position of the fp32-only argument | None)
_MIL_SPLICE = {family: (f.index("bag"), next((i for i, name in enumerate(f) if name[0] == "*"), None)) for family, f in _MIL_FIELDS.items()}
_NO_DX = "mil_bwd: no gradient with respect to an fp16 / prepared bag (pass the float32 bag if the bag itself is trained)"


def _mil_args(family: str, kind: int, vals: tuple):
    """(entry name, its argument tuple) from one value per _MIL_FIELDS[family] field, ``bag`` being the pointer tuple of _bag_kind. Pure: it
    touches neither a tensor nor the library."""
    ib, ix = _MIL_SPLICE[family]
    if kind != KIND_F32 and ix is not None:
        if family == "bwd" and vals[ix] is not None:
            raise ValueError(_NO_DX)
        vals = vals[:ix] + vals[ix + 1:]
    return f"toad_mil_{family}{_KIND_SUFFIX[kind]}_f32", vals[:ib] + vals[ib] + vals[ib + 1:]


def _mil_call(lib, family: str, kind: int, vals: tuple) -> None:
    name, args = _mil_args(family, kind, vals)
    _lib.check(getattr(lib, name)(*args), name)


class PreparedBag:
    """A slide's bag in the form the first Linear and its weight gradient consume directly (toad_bag_prepare_f32, ABI 9): the two
    fp16 pieces of every element, plane-tiled in the GEMMs' LDS stage order, plus the bag's abs-max array. Same 4 bytes per
    element as the fp32 bag it was made from (which the caller may drop). Made once per slide - at ingest - because a bag is an
    input that stays the same across epochs (datasets/dataset_mtl_concat.py:369-373). Quacks like the [N, 1024] tensor it stands
    for where the host code only asks for shape / device; it is not differentiable."""

    is_prepared_bag = True
    requires_grad = False
    is_cuda = True
    dtype = torch.float32            # the values it represents (fp32 precision)

    def __init__(self, planes: torch.Tensor, amax: torch.Tensor, n: int, k: int):
        self.planes, self.amax, self.shape = planes, amax, torch.Size((n, k))

    @property
    def device(self):
        return self.planes.device

    def dim(self) -> int:
        return 2

    def contiguous(self):
        return self

    def to(self, *args, **kwargs):           # already resident in its final form (train._to_device calls data.to(device))
        dev = kwargs.get("device", args[0] if args and isinstance(args[0], (str, torch.device)) else None)
        if dev is not None and torch.device(dev).type == "cuda" and torch.device(dev).index not in (None, self.planes.device.index):
            raise RuntimeError(f"PreparedBag lives on {self.planes.device}; prepare it on the device that trains on it")
        if dev is not None and torch.device(dev).type != "cuda":
            raise RuntimeError("PreparedBag is a device-side format (toad_amd has no CPU path)")
        return self

    def nbytes(self) -> int:
        return self.planes.numel() + 4 * self.amax.numel()


def prepare_bag(x: torch.Tensor, out: Optional[PreparedBag] = None) -> PreparedBag:
    """fp32 (or fp16 / bf16: up-cast first) bag [N, K] on the device -> PreparedBag. One pass for the abs-max array, one for the
    split (reads the bag twice, writes it once: ~0.2 ms per 100,000 x 1024 bag, off the training stream when done at ingest).
    ``out``: a PreparedBag of the same shape whose buffers are overwritten (a double-buffered ingest loop allocates two and
    alternates; the caller orders the overwrite behind the last step that read them)."""
    if x.dtype != torch.float32:
        x = x.float()
    x = x.contiguous()
    _chk(x, "bag")
    n, k = x.shape
    if n == 0 or k % 8 != 0:
        raise ValueError("prepare_bag: needs a non-empty [N, K] bag with K a multiple of 8")
    lib = _lib.load()
    if out is not None:
        if tuple(out.shape) != (n, k) or out.planes.device != x.device:
            raise ValueError("prepare_bag: `out` must be a PreparedBag of the same shape on the same device")
        planes, amax = out.planes, out.amax
    else:
        planes = torch.empty(int(lib.toad_bag_planes_bytes(n, k)), dtype=torch.uint8, device=x.device)
        amax = torch.empty(amax_floats(n), dtype=torch.float32, device=x.device)
    _lib.check(lib.toad_bag_prepare_f32(_p(x), n, k, _p(planes), _p(amax), _stream()), "toad_bag_prepare_f32")
    return out if out is not None else PreparedBag(planes, amax, n, k)


def _bag_kind(bag, name: str = "bag"):
    """The bag of a whole-slide call (or the concatenated ``bags`` of a multi-slide one), checked -> (kind, what stands in the bag position of
    the argument list): fp32, fp16 (features stored in half precision: toad_mil_*_x16_f32) or a PreparedBag (toad_mil_*_xp_f32)."""
    if getattr(bag, "is_prepared_bag", False):
        _chk(bag.planes, name + " planes", dtype=torch.uint8); _chk(bag.amax, name + " amax")
        return KIND_PREPARED, (bag.planes.data_ptr(), bag.amax.data_ptr())
    kind = KIND_F16 if bag.dtype == torch.float16 else KIND_F32
    _chk(bag, name, dtype=torch.float16 if kind else torch.float32)
    return kind, (bag.data_ptr(),)


def _step_events():
    """The events of a bracketed whole-slide step -> (event objects, the 18-slot array the library records into), or (None, None) when timing
    is off or this call is not due (stride). Level 1 fills the pool-forward pair only."""
    if _TIMING is None or not _timing_due():
        return None, None
    nev = 18 if _TIMING_LEVEL >= 2 else 2
    evs = [_take_event() for _ in range(nev)]
    return evs, (ctypes.c_void_p * 18)(*([e.cuda_event for e in evs] + [None] * (18 - nev)))


def _file_events(evs, whole: Optional[str] = None) -> None:
    """File the pairs the library recorded: pool forward, then the eight GEMM calls; ``whole`` names a bucket for the whole call, from the first
    GEMM's start to the deferred weight-gradient reduction's end (the weight split launch in front of the first GEMM, ~6 us, is outside it;
    no extra event packets on the stream)."""
    if evs is None:
        return
    _TIMING.setdefault("pool_fwd", []).append((evs[0], evs[1]))
    if len(evs) == 18:
        for i, name in enumerate(_GEMM_EVENT_NAMES):
            _TIMING.setdefault(name, []).append((evs[2 + 2 * i], evs[3 + 2 * i]))
        if whole is not None:
            _TIMING.setdefault(whole, []).append((evs[2], evs[17]))


def _step_dims(w, bag):
    c = w["wcls"].shape[0]
    d = w["wc"].shape[1]
    if bag.shape[1] != 1024 or w["w1"].shape != (512, 1024) or w["wab"].shape != (2 * d, 512):
        raise ValueError("whole-slide calls need the TOAD trunk shapes (1024 -> 512 -> 2 x 384|256)")
    return bag.shape[0], c, d


def mil_step(w, grads, beta: float, bag, sex, label, site, w_cls: float = 0.75, w_site: float = 0.25,
             drop_p: float = 0.0, seed: int = 0, want_logits: bool = False, x_amax: Optional[torch.Tensor] = None):
    """forward + weighted CE + backward for one slide in ONE library call. ``w`` / ``grads`` map the STEP_SLOTS
    to tensors (grads = beta*grads + gradient). Returns (loss[3], logits [1,C] | None, site_logits [1,2] | None)."""
    kind, bagp = _bag_kind(bag)
    _chk(sex, "sex"); _chk(label, "label", dtype=torch.int64); _chk(site, "site", dtype=torch.int64)
    _chk(x_amax, "x_amax", allow_none=True)
    wp, gp = _slot_ptrs(w), _slot_ptrs(grads, "grad ")
    n, c, d = _step_dims(w, bag)
    lib = _lib.load()
    dev = bag.device
    ws = _ws(lib.toad_mil_step_ws_bytes(n, c, d), dev, "step")
    loss = torch.empty((3,), dtype=torch.float32, device=dev)
    logits = torch.empty((1, c), dtype=torch.float32, device=dev) if want_logits else None
    slog = torch.empty((1, 2), dtype=torch.float32, device=dev) if want_logits else None
    evs, events = _step_events()
    _mil_call(lib, "step", kind, (wp, gp, float(beta), bagp, _p(sex), _p(label), _p(site), float(w_cls), float(w_site), n, c, d, float(drop_p),
                                  int(seed), _p(x_amax), _p(loss), _p(logits), _p(slog), _p(ws), ws.numel(), events, _stream()))
    _file_events(evs)
    return loss, logits, slog


def _adjacent_rows(bags):
    """Bags that already lie back to back in ONE allocation (an ingest buffer filled slide after slide, or views cut from a concatenated
    tensor) are their own concatenation: return it as a view, or None. Saves the copy of every bag row that torch.cat would make."""
    first = bags[0]
    if first.dtype not in (torch.float32, torch.float16) or first.dim() != 2:
        return None
    esz = first.element_size()                   # fp16 landing buffers (BagPrefetcher(arena_dtype=torch.float16)) are joined like fp32 ones
    store = first.untyped_storage().data_ptr()
    nxt, rows = first.data_ptr() + first.numel() * esz, first.shape[0]
    for b in bags[1:]:
        if b.dtype != first.dtype or b.dim() != 2 or b.shape[1] != first.shape[1] or not b.is_contiguous() \
                or b.untyped_storage().data_ptr() != store or b.data_ptr() != nxt:
            return None
        nxt += b.numel() * esz
        rows += b.shape[0]
    return torch.as_strided(first, (rows, first.shape[1]), (first.shape[1], 1))


def mil_multi_step(w, grads, beta: float, bags, sex, label, site, w_cls: float = 0.75, w_site: float = 0.25,
                   drop_p: float = 0.0, seed: int = 0, want_logits: bool = False, offsets=None):
    """forward + weighted CE + backward for a BATCH of slides in ONE library call (toad_mil_multi_step_f32): the trunk / attention GEMMs
    run once over the concatenated bags, pooling + heads + loss per slide. ``bags``: a list of fp32 [N_b, 1024] device tensors
    (concatenated here), or ONE already concatenated [sum N_b, 1024] tensor together with ``offsets`` (list of B + 1 row offsets).
    fp16 bags - a list that is fp16 throughout, or an fp16 concatenation - run as stored (toad_mil_multi_step_x16_f32: no up-cast, no fp32
    copy); mixed lists and totals toad_mil_multi_x16_ok refuses are up-cast.
    ``sex`` [B] float32, ``label`` / ``site`` [B] int64 device tensors. grads = beta*grads + sum over the batch.
    Returns (loss [B,3], logits [B,C] | None, site_logits [B,2] | None)."""
    xcat, offsets = _concat_bags(bags, offsets)
    nb = len(offsets) - 1
    kind, bagp = _bag_kind(xcat, "bags")
    _chk(sex, "sex"); _chk(label, "label", dtype=torch.int64); _chk(site, "site", dtype=torch.int64)
    if xcat.dim() != 2 or xcat.shape[0] != offsets[-1] or sex.numel() != nb or label.numel() != nb or site.numel() != nb:
        raise ValueError("mil_multi_step: one sex / label / site entry per slide and offsets[-1] == rows of the concatenation")
    wp, gp = _slot_ptrs(w), _slot_ptrs(grads, "grad ")
    n, c, d = _step_dims(w, xcat)
    lib = _lib.load()
    dev = xcat.device
    nbytes = int(lib.toad_mil_multi_ws_bytes(n, nb, c, d))
    if nbytes == 0:
        raise ValueError(f"mil_multi_step: unsupported batch (rows {n}, slides {nb})")
    ws = _ws(nbytes, dev, "step")
    loss = torch.empty((nb, 3), dtype=torch.float32, device=dev)
    logits = torch.empty((nb, c), dtype=torch.float32, device=dev) if want_logits else None
    slog = torch.empty((nb, 2), dtype=torch.float32, device=dev) if want_logits else None
    offs = (ctypes.c_int64 * (nb + 1))(*offsets)
    evs, events = _step_events()                             # same 18-event layout as mil_step
    _mil_call(lib, "multi_step", kind, (wp, gp, float(beta), bagp, offs, nb, _p(sex), _p(label), _p(site), float(w_cls), float(w_site), c, d,
                                        float(drop_p), int(seed), _p(loss), _p(logits), _p(slog), _p(ws), ws.numel(), events, _stream()))
    _file_events(evs, "mil_multi_step" + _KIND_SUFFIX[kind])
    return loss, logits, slog


# ---- model(data, sex) and loss.backward() as one C call each (toad_mil_fwd_f32 / toad_mil_bwd_f32) ---------------------
ARENA_SLOTS = ("h1", "h", "p", "a_raw", "stats", "m", "mcat", "logits", "y_prob", "y_hat", "site_logits", "site_prob", "site_hat",
               "x_amax", "h1_amax", "h_amax", "h1_bits", "h_bits")


class MilArena:
    """The forward arena of one slide: saved activations + outputs, as typed views of ONE allocation."""

    def __init__(self, n: int, c: int, d: int, device, cached: bool = False):
        """``cached``: carve the arena out of the per-(device, stream) workspace cache instead of a fresh allocation - for forwards
        whose activations nobody will read back (no_grad / eval): the caller must CLONE the outputs it keeps, since the next
        cached forward overwrites them (a view of a fresh arena would pin ~7 KB per patch for as long as any output lives)."""
        self.n, self.c, self.d = n, c, d
        self._carve("toad_mil_arena", ARENA_SLOTS, (n, c, d), device, cached)

    def _carve(self, query: str, slots, shape, device, cached: bool) -> None:
        """Allocate the buffer the library lays out for ``shape`` ((N, C, D), or (sum N_b, B, C, D) for a batch) and note where its slots lie."""
        lay = _ARENA_LAYOUTS.get(shape)                       # (three library queries, cached per shape: this runs once per forward)
        if lay is None:
            lay = _remember(_ARENA_LAYOUTS, shape, _arena_layout(query, slots, shape))
        nbytes, align, self.off = lay
        self.buf = _ws(nbytes, device, "eval_arena")[:nbytes] if cached else torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.base = (-self.buf.data_ptr()) % align

    def view(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        nbytes = _ELEM_BYTES[dtype]
        for s_ in shape:
            nbytes *= int(s_)
        o = self.base + self.off[name]
        return self.buf[o:o + nbytes].view(dtype).view(*shape)


_ELEM_BYTES = {torch.float32: 4, torch.int64: 8, torch.uint8: 1, torch.float16: 2, torch.int32: 4}
_ARENA_LAYOUTS = {}
_SCRATCH_BYTES = {}


def _remember(cache: dict, key, value):
    """File a library query's answer under its shape key. The caches are bounded: past 4096 shapes one is dropped whole."""
    if len(cache) > 4096:
        cache.clear()
    cache[key] = value
    return value


def _arena_layout(query: str, slots, shape):
    """(arena bytes, base alignment, slot -> offset from the aligned base) of <query>_bytes / <query>_layout for one shape."""
    lib = _lib.load()
    nbytes = int(getattr(lib, query + "_bytes")(*shape))
    if nbytes == 0 and len(shape) == 4:                       # a batch the library does not take (one slide's shape: the layout call reports it)
        raise ValueError("unsupported batch (rows {}, slides {}, C={}, D={})".format(*shape))
    offs = (ctypes.c_int64 * len(slots))()
    _lib.check(getattr(lib, query + "_layout")(*shape, offs), query + "_layout")
    return nbytes, int(lib.toad_mil_buffer_align(shape[0])), {k: int(o) for k, o in zip(slots, offs)}


def _scratch_bytes(*shape) -> int:
    """toad_mil_scratch_bytes(N, C, D), or toad_mil_multi_scratch_bytes(sum N_b, B, C, D), cached per shape."""
    b = _SCRATCH_BYTES.get(shape)
    if b is None:
        lib = _lib.load()
        b = _remember(_SCRATCH_BYTES, shape, int((lib.toad_mil_multi_scratch_bytes if len(shape) == 4 else lib.toad_mil_scratch_bytes)(*shape)))
    return b


def mil_fwd(w, bag, sex, drop_p: float = 0.0, seed: int = 0, attention_only: bool = False,
            x_amax: Optional[torch.Tensor] = None, cached_arena: bool = False) -> MilArena:
    """models/model_toad.py:90-116 for one bag in ONE library call; returns the arena (outputs + what backward needs).
    ``cached_arena``: forward-only use (see MilArena): clone what you keep."""
    kind, bagp = _bag_kind(bag)
    _chk(sex, "sex", allow_none=attention_only); _chk(x_amax, "x_amax", allow_none=True)
    wp = _slot_ptrs(w)
    n, c, d = _step_dims(w, bag)
    lib = _lib.load()
    arena = MilArena(n, c, d, bag.device, cached=cached_arena)
    scratch = _ws(_scratch_bytes(n, c, d), bag.device, "mil")
    with _timed("mil_fwd"):
        _mil_call(lib, "fwd", kind, (wp, bagp, _p(sex), n, c, d, float(drop_p), int(seed), _p(x_amax), 1 if attention_only else 0,
                                     _p(arena.buf), arena.buf.numel(), _p(scratch), scratch.numel(), _stream()))
    return arena


def mil_bwd(w, grads, beta: float, bag, arena: MilArena, dlogits, dsite, da_ext=None, dmcat_ext=None, drop_p: float = 0.0,
            seed: int = 0, need_dx: bool = False, need_dsex: bool = False):
    """Backward of mil_fwd in ONE library call: grads[slot] = beta*grads[slot] + gradient. Returns (dX | None, dsex | None)."""
    kind, bagp = _bag_kind(bag)
    if kind != KIND_F32 and need_dx:
        raise ValueError(_NO_DX)
    _chk(dlogits, "dlogits"); _chk(dsite, "dsite")
    _chk(da_ext, "da_ext", allow_none=True); _chk(dmcat_ext, "dmcat_ext", allow_none=True)
    wp, gp = _slot_ptrs(w, check=False), _slot_ptrs(grads, "grad ")
    n, c, d = arena.n, arena.c, arena.d
    if dlogits.numel() != c or dsite.numel() != 2 or bag.shape[0] != n:
        raise ValueError("mil_bwd: shape mismatch")
    if da_ext is not None and tuple(da_ext.shape) != (n, 2):
        raise ValueError("mil_bwd: da_ext must be [N,2]")
    if dmcat_ext is not None and tuple(dmcat_ext.shape) != (2, 513):
        raise ValueError("mil_bwd: dmcat_ext must be [2,513]")
    lib = _lib.load()
    dev = bag.device
    dx = torch.empty_like(bag) if need_dx else None
    dsex = torch.empty((1,), dtype=torch.float32, device=dev) if need_dsex else None
    scratch = _ws(_scratch_bytes(n, c, d), dev, "mil")
    buf = arena.buf
    with _timed("mil_bwd"):
        _mil_call(lib, "bwd", kind, (wp, gp, float(beta), bagp, n, c, d, float(drop_p), int(seed), _p(buf), buf.numel(), _p(dlogits), _p(dsite),
                                     _p(da_ext), _p(dmcat_ext), _p(dx), _p(dsex), _p(scratch), scratch.numel(), _stream()))
    return dx, dsex


# ---- a batch of slides: forward and backward as one C call each (toad_mil_multi_fwd_f32 / toad_mil_multi_bwd_f32, ABI 14) ------------------
MULTI_ARENA_SLOTS = ("h1", "h", "p", "a_raw", "mcat", "logits", "y_prob", "y_hat", "site_logits", "site_prob", "site_hat")
MULTI_MAX_SLIDES = 4096                    # csrc/step.hip multi_batch_ok
MULTI_MAX_ROWS = (1 << 20) - 1             # sum N_b: the concatenation is ONE launch of the NT kernels (32-bit row offsets, h2_nt_ok)


class MilMultiArena(MilArena):
    """The forward arena of a batch of slides (toad_mil_multi_arena_layout): saved activations of the concatenation, per-slide pooling
    records, the device copy of the offsets and the dense per-slide outputs, as typed views of ONE allocation. Keeps the concatenated bag
    (fp32, or fp16 as stored: half the bytes held between forward and backward) and the offsets the forward ran on (the backward needs both)."""

    def __init__(self, xcat: torch.Tensor, offsets, c: int, d: int, cached: bool = False):
        n, nb = int(xcat.shape[0]), len(offsets) - 1
        self.n, self.c, self.d, self.b = n, c, d, nb
        self.xcat, self.offsets = xcat, tuple(offsets)
        self._carve("toad_mil_multi_arena", MULTI_ARENA_SLOTS, (n, nb, c, d), xcat.device, cached)

    def outputs(self):
        """Dense per-slide outputs (views of the arena): logits [B,C], site_logits [B,2], a_raw [sum N_b,2], features [B,2,513],
        y_prob [B,C], y_hat [B,1], site_prob [B,2], site_hat [B,1]."""
        v, nb, c = self.view, self.b, self.c
        return dict(logits=v("logits", (nb, c)), site_logits=v("site_logits", (nb, 2)), a_raw=v("a_raw", (self.n, 2)), features=v("mcat", (nb, 2, 513)),
                    y_prob=v("y_prob", (nb, c)), y_hat=v("y_hat", (nb, 1), torch.int64), site_prob=v("site_prob", (nb, 2)),
                    site_hat=v("site_hat", (nb, 1), torch.int64))


def _concat_bags(bags, offsets=None):
    """(xcat, offsets): a list of [N_b, 1024] bags concatenated once (bags already back to back in one allocation are taken as they are), or
    an already concatenated tensor with its B + 1 row offsets. A list whose bags are ALL fp16 stays fp16 (the x16 multi-slide calls read it as
    stored) when the library takes the total (toad_mil_multi_x16_ok); any other list is up-cast to fp32, and so is an fp16 total it refuses."""
    if offsets is None:
        half = all(b.dtype == torch.float16 for b in bags) and multi_x16_ok(sum(int(b.shape[0]) for b in bags))
        bags = [(b if half or b.dtype == torch.float32 else b.float()).contiguous() for b in bags]
        offsets = [0]
        for b in bags:
            offsets.append(offsets[-1] + int(b.shape[0]))
        xcat = bags[0] if len(bags) == 1 else _adjacent_rows(bags)
        return (torch.cat(bags, 0) if xcat is None else xcat), offsets
    xcat, offsets = bags, [int(o) for o in offsets]
    if xcat.dtype == torch.float16 and not multi_x16_ok(int(xcat.shape[0])):
        xcat = xcat.float()
    return xcat, offsets


def multi_x16_ok(rows: int) -> bool:
    """The ragged multi-slide calls take fp16 bags of this many concatenated rows as stored (toad_mil_multi_x16_ok); others are up-cast."""
    return bool(_lib.load().toad_mil_multi_x16_ok(int(rows)))


def _multi_scratch(n: int, nb: int, c: int, d: int, dev) -> torch.Tensor:
    nbytes = _scratch_bytes(n, nb, c, d)
    if nbytes == 0:
        raise ValueError(f"unsupported batch (rows {n}, slides {nb}, C={c}, D={d})")
    return _ws(nbytes, dev, "mil")


def mil_multi_fwd(w, bags_or_xcat, sex, drop_p: float = 0.0, seed: int = 0, offsets=None, cached_arena: bool = False):
    """models/model_toad.py:90-116 for a BATCH of slides in ONE library call (toad_mil_multi_fwd_f32): the trunk / attention GEMMs run once over
    the concatenated bags, pooling and heads per slide. ``bags``: a list of fp32 [N_b, 1024] device tensors (concatenated here, once), or ONE
    concatenated tensor with ``offsets`` (B + 1 row offsets); fp16 bags as for mil_multi_step (toad_mil_multi_fwd_x16_f32: the arena then keeps
    the fp16 concatenation for the backward); ``sex`` [B] float32 on the device. Returns (arena, outputs): the MilMultiArena the backward needs
    and MilMultiArena.outputs(). Dropout masks are those of mil_multi_step for the same (drop_p, seed). ``cached_arena``: forward-only use (see
    MilArena): clone what you keep."""
    xcat, offsets = _concat_bags(bags_or_xcat, offsets)
    nb = len(offsets) - 1
    kind, bagp = _bag_kind(xcat, "bags")
    _chk(sex, "sex")
    if xcat.dim() != 2 or nb < 1 or xcat.shape[0] != offsets[-1] or sex.numel() != nb:
        raise ValueError("mil_multi_fwd: one sex entry per slide and offsets[-1] == rows of the concatenation")
    wp = _slot_ptrs(w)
    n, c, d = _step_dims(w, xcat)
    lib = _lib.load()
    arena = MilMultiArena(xcat, offsets, c, d, cached=cached_arena)
    scratch = _multi_scratch(n, nb, c, d, xcat.device)
    offs = (ctypes.c_int64 * (nb + 1))(*offsets)
    with _timed("mil_multi_fwd" + _KIND_SUFFIX[kind]):
        _mil_call(lib, "multi_fwd", kind, (wp, bagp, offs, nb, _p(sex), c, d, float(drop_p), int(seed), _p(arena.buf), arena.buf.numel(),
                                           _p(scratch), scratch.numel(), _stream()))
    return arena, arena.outputs()


def mil_multi_bwd(w, grads, beta: float, xcat, offsets, arena: MilMultiArena, dlogits, dsite, da_ext=None, dmcat_ext=None, drop_p: float = 0.0,
                  seed: int = 0):
    """Backward of mil_multi_fwd in ONE library call (toad_mil_multi_bwd_f32): grads[slot] = beta*grads[slot] + the gradient summed over the batch,
    from dlogits [B,C], dsite [B,2] and optionally da_ext [sum N_b,2] (through the raw scores) and dmcat_ext [B,2,513] (through the features).
    ``xcat`` / ``offsets`` as for mil_multi_fwd (None: the ones the forward ran on, kept by the arena); the same (drop_p, seed) as the forward."""
    if xcat is None:
        xcat, offsets = arena.xcat, list(arena.offsets)
    else:
        xcat, offsets = _concat_bags(xcat, offsets)
    nb = len(offsets) - 1
    if tuple(offsets) != arena.offsets or xcat.shape[0] != arena.n:
        raise ValueError("mil_multi_bwd: the offsets / bags must be those of the forward that filled the arena")
    kind, bagp = _bag_kind(xcat, "bags")
    _chk(dlogits, "dlogits"); _chk(dsite, "dsite")
    _chk(da_ext, "da_ext", allow_none=True); _chk(dmcat_ext, "dmcat_ext", allow_none=True)
    wp, gp = _slot_ptrs(w, check=False), _slot_ptrs(grads, "grad ")
    n, c, d = arena.n, arena.c, arena.d
    if tuple(dlogits.shape) != (nb, c) or tuple(dsite.shape) != (nb, 2):
        raise ValueError(f"mil_multi_bwd: dlogits must be [{nb},{c}] and dsite [{nb},2]")
    if da_ext is not None and tuple(da_ext.shape) != (n, 2):
        raise ValueError(f"mil_multi_bwd: da_ext must be [{n},2]")
    if dmcat_ext is not None and tuple(dmcat_ext.shape) != (nb, 2, 513):
        raise ValueError(f"mil_multi_bwd: dmcat_ext must be [{nb},2,513]")
    lib = _lib.load()
    scratch = _multi_scratch(n, nb, c, d, xcat.device)
    offs = (ctypes.c_int64 * (nb + 1))(*offsets)
    with _timed("mil_multi_bwd" + _KIND_SUFFIX[kind]):
        _mil_call(lib, "multi_bwd", kind, (wp, gp, float(beta), bagp, offs, nb, c, d, float(drop_p), int(seed), _p(arena.buf), arena.buf.numel(),
                                           _p(dlogits), _p(dsite), _p(da_ext), _p(dmcat_ext), _p(scratch), scratch.numel(), _stream()))


# ---- feature-extractor pieces (conv.hip) --------------------------------------------------------------------------
def linear_act_res_fwd(x, w, b, residual, act: int) -> torch.Tensor:
    """Y = act(X W^T + b + residual): a convolution-as-GEMM with folded BN, the bottleneck's skip add and ReLU."""
    _chk(x, "x"); _chk(w, "w"); _chk(b, "b", allow_none=True); _chk(residual, "residual", allow_none=True)
    m, k = x.shape
    n, k2 = w.shape
    if k != k2 or (b is not None and b.numel() != n) or (residual is not None and tuple(residual.shape) != (m, n)):
        raise ValueError(f"linear_act_res_fwd: shape mismatch x{tuple(x.shape)} w{tuple(w.shape)}")
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(m, n, k), x.device)
    _lib.check(lib.toad_linear_act_res_fwd_f32(_p(x), _p(w), _p(b), _p(residual), _p(y), m, k, n, act, _p(ws), ws.numel(),
                                               _stream()), "toad_linear_act_res_fwd_f32")
    return y


def conv_nhwc(x: torch.Tensor, wf: torch.Tensor, b, residual, kh: int, kw: int, stride: int, pad: int, act: int) -> torch.Tensor:
    """Implicit-GEMM convolution: x [B,H,W,Cin] NHWC, wf [Cout, kh*kw*Cin] in (ky,kx,c) order -> [B,Ho,Wo,Cout]."""
    _chk(x, "x"); _chk(wf, "wf"); _chk(b, "b", allow_none=True); _chk(residual, "residual", allow_none=True)
    bb, h, w, c = x.shape
    cout = wf.shape[0]
    if wf.shape[1] != kh * kw * c:
        raise ValueError("conv_nhwc: weight shape mismatch")
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((bb, ho, wo, cout), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(bb * ho * wo, cout, kh * kw * c), x.device)
    _lib.check(lib.toad_conv_nhwc_f32(_p(x), _p(wf), _p(b), _p(residual), _p(y), bb, h, w, c, kh, kw, stride, pad, cout, act,
                                      _p(ws), ws.numel(), _stream()), "toad_conv_nhwc_f32")
    return y


def im2col_nhwc(x: torch.Tensor, kh: int, kw: int, stride: int, pad: int) -> torch.Tensor:
    """x [B,H,W,C] -> cols [B*Ho*Wo, kh*kw*C], column order (ky, kx, c)."""
    _chk(x, "x")
    b, h, w, c = x.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    cols = torch.empty((b * ho * wo, kh * kw * c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().toad_im2col_nhwc_f32(_p(x), _p(cols), b, h, w, c, kh, kw, stride, pad, _stream()), "toad_im2col_nhwc_f32")
    return cols


def im2col_stem_nchw(x: torch.Tensor) -> torch.Tensor:
    """x [B,3,H,W] -> cols [B*Ho*Wo, 160] for the 7x7/2 pad-3 stem, column order (c, ky, kx), columns 147.. zero."""
    _chk(x, "x")
    b, c, h, w = x.shape
    if c != 3:
        raise ValueError("im2col_stem_nchw: expected 3 channels")
    ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    cols = torch.empty((b * ho * wo, 160), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().toad_im2col_stem_nchw_f32(_p(x), _p(cols), b, h, w, _stream()), "toad_im2col_stem_nchw_f32")
    return cols


def stem_conv(x: torch.Tensor, wf: torch.Tensor, b, act: int) -> torch.Tensor:
    """7x7/2 pad-3 stem on NCHW tiles via the space-to-depth image: x [B,3,H,W], wf [64,192] -> [B,Ho,Wo,64] NHWC."""
    _chk(x, "x"); _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    bb, c, h, w = x.shape
    if c != 3 or tuple(wf.shape) != (64, 192):
        raise ValueError("stem_conv: expected [B,3,H,W] tiles and a [64,192] space-to-depth weight")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xs = torch.empty((bb, ho + 3, wo + 3, 12), dtype=torch.float32, device=x.device)
    y = torch.empty((bb, ho, wo, 64), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.toad_stem_s2d_nchw_f32(_p(x), _p(xs), bb, h, w, _stream()), "toad_stem_s2d_nchw_f32")
    ws = _ws(lib.toad_linear_ws_bytes(bb * ho * wo, 64, 192), x.device)
    _lib.check(lib.toad_stem_conv_s2d_f32(_p(xs), _p(wf), _p(b), _p(y), bb, ho, wo, act, _p(ws), ws.numel(), _stream()), "toad_stem_conv_s2d_f32")
    return y


def stem_conv_pool(x: torch.Tensor, wf: torch.Tensor, b) -> torch.Tensor:
    """Stem + ReLU + 3x3/2 max-pool as one kernel (tiles 256 wide: Wo == 128, Ho even): x [B,3,H,W] -> [B,Ho/2,Wo/2,64] NHWC,
    bit-identical to maxpool3x3s2_nhwc(stem_conv(x, wf, b, ACT_RELU))."""
    _chk(x, "x"); _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    bb, c, h, w = x.shape
    if c != 3 or tuple(wf.shape) != (64, 192):
        raise ValueError("stem_conv_pool: expected [B,3,H,W] tiles and a [64,192] space-to-depth weight")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xs = torch.empty((bb, ho + 3, wo + 3, 12), dtype=torch.float32, device=x.device)
    y = torch.empty((bb, ho // 2, wo // 2, 64), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.toad_stem_s2d_nchw_f32(_p(x), _p(xs), bb, h, w, _stream()), "toad_stem_s2d_nchw_f32")
    ws = _ws(lib.toad_linear_ws_bytes(bb * ho * wo, 64, 192), x.device)
    _lib.check(lib.toad_stem_conv_pool_s2d_f32(_p(xs), _p(wf), _p(b), _p(y), bb, ho, wo, _p(ws), ws.numel(), _stream()), "toad_stem_conv_pool_s2d_f32")
    return y


def stem_pool_nchw(x: torch.Tensor, wf: torch.Tensor, b) -> torch.Tensor:
    """Stem + ReLU + 3x3/2 max-pool straight from NCHW tiles (W == 256, H % 4 == 0): x [B,3,H,W] -> [B,H/4,64,64] NHWC; the values of
    maxpool3x3s2_nhwc(stem_conv(x, wf, b, ACT_RELU)) to fp32 round-off (per-tile operand scales)."""
    _chk(x, "x"); _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    bb, c, h, w = x.shape
    if c != 3 or tuple(wf.shape) != (64, 192):
        raise ValueError("stem_pool_nchw: expected [B,3,H,W] tiles and a [64,192] space-to-depth weight")
    y = torch.empty((bb, h // 4, w // 4, 64), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(bb * (h // 2) * (w // 2), 64, 192), x.device)
    _lib.check(lib.toad_stem_pool_nchw_f32(_p(x), _p(wf), _p(b), _p(y), bb, h, w, _p(ws), ws.numel(), _stream()), "toad_stem_pool_nchw_f32")
    return y


IMAGENET_MEAN = (0.485, 0.456, 0.406)      # the statistics of the weights the reference loads (models/resnet_custom.py:121-124)
IMAGENET_STD = (0.229, 0.224, 0.225)


def norm_constants_u8(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The `norm` argument of the uint8 calls: ctypes float[6] = a_c = 1/(255 std_c) then b_c = -mean_c/std_c, each computed in double precision and
    rounded once to fp32. The device value of a byte u is fmaf(u, a_c, b_c)."""
    import ctypes
    import math
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must have three entries (R, G, B)")
    if any(v == 0.0 or not math.isfinite(v) for v in std) or not all(math.isfinite(v) for v in mean):
        raise ValueError(f"mean / std must be finite and std non-zero (got mean={mean}, std={std})")
    vals = [1.0 / (255.0 * sd) for sd in std] + [-m / sd for m, sd in zip(mean, std)]
    arr = (ctypes.c_float * 6)(*vals)                    # c_float rounds the double to nearest fp32
    if not all(math.isfinite(v) for v in arr):
        raise ValueError(f"1/(255 std) or -mean/std is not finite in fp32 (mean={mean}, std={std})")
    return arr


def _chk_tiles_u8(tiles: torch.Tensor, name: str):
    _chk(tiles, "tiles", dtype=torch.uint8)
    if tiles.dim() != 4 or tiles.shape[3] != 3:
        raise ValueError(f"{name}: expected uint8 [B,H,W,3] tiles (RGB, channels last), got {tuple(tiles.shape)}")


def tiles_u8_to_f32(tiles: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """ToTensor + Normalize(mean, std) on the device in one rounding: uint8 [B,H,W,3] (any alignment) -> fp32 [B,3,H,W],
    out[b,c,y,x] = fmaf(tiles[b,y,x,c], 1/(255 std_c), -mean_c/std_c)."""
    _chk_tiles_u8(tiles, "tiles_u8_to_f32")
    norm = norm_constants_u8(mean, std)
    b, h, w, _ = tiles.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=tiles.device)
    _lib.check(_lib.load().toad_tiles_u8_nhwc_to_nchw_f32(_p(tiles), norm, _p(out), b, h, w, _stream()), "toad_tiles_u8_nhwc_to_nchw_f32")
    return out


def stem_pool_nhwc_u8(tiles: torch.Tensor, wf: torch.Tensor, b, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """stem_pool_nchw straight from uint8 tiles [B,H,256,3] (H % 4 == 0): bitwise stem_pool_nchw(tiles_u8_to_f32(tiles, mean, std), wf, b), without the
    fp32 image. A source at an odd address is copied once (the kernel reads 2-byte aligned words)."""
    _chk_tiles_u8(tiles, "stem_pool_nhwc_u8"); _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    if tuple(wf.shape) != (64, 192):
        raise ValueError("stem_pool_nhwc_u8: expected a [64,192] space-to-depth weight")
    norm = norm_constants_u8(mean, std)
    bb, h, w, _ = tiles.shape
    if tiles.data_ptr() % 2:
        tiles = tiles.clone()
    y = torch.empty((bb, h // 4, w // 4, 64), dtype=torch.float32, device=tiles.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(bb * (h // 2) * (w // 2), 64, 192), tiles.device)
    _lib.check(lib.toad_stem_pool_nhwc_u8(_p(tiles), norm, _p(wf), _p(b), _p(y), bb, h, w, _p(ws), ws.numel(), _stream()), "toad_stem_pool_nhwc_u8")
    return y


def tile_shape(tile):
    """`tile` of the region calls, an int or (H, W) -> (H, W)."""
    h, w = (tile, tile) if isinstance(tile, int) else tuple(tile)
    if not (isinstance(h, int) and isinstance(w, int)) or h < 1 or w < 1:
        raise ValueError(f"tile must be a positive int or (H, W), got {tile!r}")
    return h, w


def check_origins(origins, hr: int, wr: int, h: int, w: int) -> torch.Tensor:
    """The `origins` argument of the region calls, checked on the HOST: [B,2] integers (x, y), the top-left pixel of each tile in region coordinates, as a
    CPU tensor, a numpy array or a list -> a contiguous int32 CPU tensor. Every tile must lie inside the hr x wr region: the kernels read where the origins
    point, so an origin out of range is an out-of-bounds read. A device tensor is refused for that reason - its values cannot be checked without a
    synchronisation. Raises before anything is launched."""
    if isinstance(origins, torch.Tensor) and origins.device.type != "cpu":
        raise ValueError("origins must be given on the host (a CPU tensor, a numpy array or a list): their bounds are checked before the launch, and "
                         f"device values cannot be read without a synchronisation (got a tensor on {origins.device})")
    o = torch.as_tensor(origins)
    if o.is_floating_point() or o.is_complex() or o.dtype == torch.bool:
        raise TypeError(f"origins must be integers (pixel coordinates), got {o.dtype}")
    if o.dim() != 2 or o.shape[1] != 2:
        raise ValueError(f"origins must be [B,2] = (x, y) per tile, got {tuple(o.shape)}")
    o = o.to(torch.int64)
    bad = (o[:, 0] < 0) | (o[:, 0] + w > wr) | (o[:, 1] < 0) | (o[:, 1] + h > hr)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"origins[{i}] = (x={int(o[i, 0])}, y={int(o[i, 1])}): a {h} x {w} (H x W) tile there does not lie inside the {hr} x {wr} region")
    return o.to(torch.int32).contiguous()


def region_layout_ok(region: torch.Tensor) -> bool:
    """[Hr,Wr,3] with stride(2) == 1, stride(1) == 3 and a row pitch stride(0) >= 3 Wr (any pitch: a column crop of a wider image is taken as it is)."""
    return region.dim() == 3 and region.shape[2] == 3 and region.shape[0] >= 1 and region.shape[1] >= 1 and region.stride(2) == 1 and region.stride(1) == 3 \
        and (region.stride(0) >= 3 * region.shape[1] or region.shape[0] == 1)


# the row pitch in bytes of a uint8 view whose rows hold row_bytes bytes; the stride of a single row says nothing, so it counts as at least one row
def _row_pitch(t: torch.Tensor, row_bytes: int) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), row_bytes)


def _region_pitch(region: torch.Tensor, name: str):
    """The device / dtype / layout checks every region call makes -> (pitch in bytes, Hr, Wr)."""
    if not isinstance(region, torch.Tensor) or not region.is_cuda:
        raise RuntimeError(f"{name}: region must be a CUDA(HIP) tensor: toad_amd has no CPU path")
    if region.dtype != torch.uint8:
        raise TypeError(f"{name}: region must be torch.uint8, got {region.dtype}")
    if not region_layout_ok(region):
        raise ValueError(f"{name}: expected a uint8 [Hr,Wr,3] region (RGB, channels last) with stride(2) == 1, stride(1) == 3 and a row pitch >= 3 Wr, got "
                         f"shape {tuple(region.shape)} strides {tuple(region.stride())}")
    hr, wr = region.shape[0], region.shape[1]
    return _row_pitch(region, 3 * wr), hr, wr


SHRINKS = (1, 2)      # the box filters the region calls can put in front of the network: a tile is a (shrink H, shrink W) footprint of the region


def check_shrink(shrink):
    if not isinstance(shrink, int) or isinstance(shrink, bool) or shrink not in SHRINKS:
        raise ValueError(f"shrink must be one of {SHRINKS} (the footprint is box-filtered by that factor; larger factors are not built), got {shrink!r}")


def shrunk_tile(tile, shrink=1):
    """`tile` (the FOOTPRINT in region pixels, an int or (H, W)) and `shrink` of the region calls -> (footprint, network tile), each (H, W). shrink is 1 or
    2 and must divide both sides of the footprint: ValueError otherwise, before anything else is looked at."""
    check_shrink(shrink)
    fh, fw = tile_shape(tile)
    if fh % shrink or fw % shrink:
        raise ValueError(f"shrink = {shrink} does not divide the {fh} x {fw} (H x W) footprint: tile stays the footprint in region pixels, the network "
                         f"sees tile / shrink")
    return (fh, fw), (fh // shrink, fw // shrink)


def box_tiles_u8(region: torch.Tensor, origins, tile, shrink=1) -> torch.Tensor:
    """The box-filtered tiles of the region calls, MATERIALISED with torch integer ops - the stated reference of `shrink`, for tests and benchmarks, on no
    product path. region uint8 [Hr,Wr,3] on any device, origins [B,2] = (x, y) on the host, tile = the footprint -> uint8 [B, H/shrink, W/shrink, 3] with

        t[iy, ix, c] = (sum of region[y + s iy + dy, x + s ix + dx, c] over dy, dx in 0 .. s-1, + s*s/2) // (s*s)

    the mean rounded half up (the box filter of every `down` in this package)."""
    (fh, fw), (h, w) = shrunk_tile(tile, shrink)
    if not isinstance(region, torch.Tensor) or region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] != 3:
        raise ValueError("box_tiles_u8: expected a uint8 [Hr,Wr,3] region")
    o = check_origins(origins, region.shape[0], region.shape[1], fh, fw)
    if o.shape[0] == 0:
        return torch.empty((0, h, w, 3), dtype=torch.uint8, device=region.device)
    t = torch.stack([region[y:y + fh, x:x + fw] for x, y in o.tolist()])
    if shrink == 1:
        return t
    s = t.view(-1, h, shrink, w, shrink, 3).to(torch.int32).sum(dim=(2, 4))
    return ((s + shrink * shrink // 2) // (shrink * shrink)).to(torch.uint8)


def _region_args(region: torch.Tensor, origins, tile, name: str, shrink=1):
    """-> (pitch, Hr, Wr, H, W, origins on the device); H, W = the NETWORK tile, the origins are checked for the footprint (shrink H, shrink W)."""
    check_shrink(shrink)
    pitch, hr, wr = _region_pitch(region, name)
    (fh, fw), (h, w) = shrunk_tile(tile, shrink)
    o = check_origins(origins, hr, wr, fh, fw)
    if o.shape[0] == 0:
        raise ValueError(f"{name}: no origins")
    return pitch, hr, wr, h, w, o.to(region.device)


def tiles_u8_region_to_f32(region: torch.Tensor, origins, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, shrink=1) -> torch.Tensor:
    """tiles_u8_to_f32 with the tiles read by origin from one decoded uint8 region [Hr,Wr,3] (any row pitch, any alignment): bitwise
    tiles_u8_to_f32(torch.stack([region[y:y+H, x:x+W] for x, y in origins]), mean, std), and no such stack exists. origins: check_origins.
    shrink = 2: `tile` is the footprint, the result [B,3,H/2,W/2] is bitwise tiles_u8_to_f32(box_tiles_u8(region, origins, tile, 2), mean, std)."""
    pitch, hr, wr, h, w, o = _region_args(region, origins, tile, "tiles_u8_region_to_f32", shrink)
    norm = norm_constants_u8(mean, std)
    out = torch.empty((o.shape[0], 3, h, w), dtype=torch.float32, device=region.device)
    if shrink == 1:
        _lib.check(_lib.load().toad_tiles_u8_region_to_nchw_f32(_p(region), pitch, hr, wr, _p(o), norm, _p(out), o.shape[0], h, w, _stream()),
                   "toad_tiles_u8_region_to_nchw_f32")
    else:
        _lib.check(_lib.load().toad_tiles_u8_region_box_to_nchw_f32(_p(region), pitch, hr, wr, _p(o), norm, _p(out), o.shape[0], h, w, shrink, _stream()),
                   "toad_tiles_u8_region_box_to_nchw_f32")
    return out


def stem_pool_region_u8(region: torch.Tensor, origins, wf: torch.Tensor, b, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, shrink=1) -> torch.Tensor:
    """stem_pool_nhwc_u8 with the tiles (H, 256), H % 4 == 0, read by origin from one decoded uint8 region: bitwise stem_pool_nhwc_u8 on the stacked
    tiles. Padding is the tile's, not the region's; the region is read in place whatever its address and pitch.
    shrink = 2: `tile` is the footprint (2 H, 512), box-filtered while the window is loaded: bitwise stem_pool_nhwc_u8(box_tiles_u8(region, origins, tile, 2))."""
    pitch, hr, wr, h, w, o = _region_args(region, origins, tile, "stem_pool_region_u8", shrink)
    _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    if tuple(wf.shape) != (64, 192):
        raise ValueError("stem_pool_region_u8: expected a [64,192] space-to-depth weight")
    norm = norm_constants_u8(mean, std)
    bb = o.shape[0]
    y = torch.empty((bb, h // 4, w // 4, 64), dtype=torch.float32, device=region.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(bb * (h // 2) * (w // 2), 64, 192), region.device)
    if shrink == 1:
        _lib.check(lib.toad_stem_pool_region_u8(_p(region), pitch, hr, wr, _p(o), norm, _p(wf), _p(b), _p(y), bb, h, w, _p(ws), ws.numel(), _stream()),
                   "toad_stem_pool_region_u8")
    else:
        _lib.check(lib.toad_stem_pool_region_box_u8(_p(region), pitch, hr, wr, _p(o), norm, _p(wf), _p(b), _p(y), bb, h, w, shrink, _p(ws), ws.numel(),
                                                    _stream()), "toad_stem_pool_region_box_u8")
    return y


TILE_REGIONS_MAX = 128                 # the regions one extractor call takes (include/toad_hip.h: TOAD_TILE_REGIONS_MAX)


def check_region_origins(origins, shapes, h: int, w: int) -> torch.Tensor:
    """The `origins` argument of the region-LIST calls, checked on the HOST: [B,3] integers (x, y, k), the top-left pixel of each tile in the coordinates of
    region k, as a CPU tensor, a numpy array or a list -> a contiguous int32 CPU tensor. ``shapes`` = [(Hr, Wr), ...], one per region; every k must name one
    of them and every h x w tile (the footprint, for a shrink) must lie inside ITS region: the kernels read where the triples point. A device tensor is
    refused, as by check_origins. Raises before anything is launched."""
    if isinstance(origins, torch.Tensor) and origins.device.type != "cpu":
        raise ValueError("origins must be given on the host (a CPU tensor, a numpy array or a list): their bounds are checked before the launch, and "
                         f"device values cannot be read without a synchronisation (got a tensor on {origins.device})")
    o = torch.as_tensor(origins)
    if o.is_floating_point() or o.is_complex() or o.dtype == torch.bool:
        raise TypeError(f"origins must be integers (pixel coordinates and a region index), got {o.dtype}")
    if o.dim() != 2 or o.shape[1] != 3:
        raise ValueError(f"origins must be [B,3] = (x, y, k) per tile - k the index of the tile's region in the list - got {tuple(o.shape)}")
    shapes = [(int(hr), int(wr)) for hr, wr in shapes]
    n = len(shapes)
    o = o.to(torch.int64)
    if o.shape[0] == 0:
        return o.to(torch.int32).contiguous()
    bad_k = (o[:, 2] < 0) | (o[:, 2] >= n)
    ext = torch.tensor(shapes if n else [(0, 0)], dtype=torch.int64)[o[:, 2].clamp(0, max(n - 1, 0))]        # [B,2] = (Hr, Wr) of each tile's region
    bad = bad_k | (o[:, 0] < 0) | (o[:, 0] + w > ext[:, 1]) | (o[:, 1] < 0) | (o[:, 1] + h > ext[:, 0])
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        x, y, k = (int(v) for v in o[i])
        if bool(bad_k[i]):
            raise ValueError(f"origins[{i}] = (x={x}, y={y}, k={k}): k must name one of the {n} regions (0 .. {n - 1})")
        raise ValueError(f"origins[{i}] = (x={x}, y={y}, k={k}): a {h} x {w} (H x W) tile there does not lie inside region {k}, which is "
                         f"{shapes[k][0]} x {shapes[k][1]}")
    return o.to(torch.int32).contiguous()


def region_list_arg(regions, name: str):
    """The `regions` argument of the region-LIST calls: a sequence of 1 .. TILE_REGIONS_MAX uint8 [Hr,Wr,3] device tensors on ONE device, each with its own
    extent, pitch and base address (_region_pitch's checks per region; the error names the region) -> (ctypes array of ToadTileRegion, shapes, device).
    The same tensor, or overlapping views of one image, may appear several times."""
    if isinstance(regions, torch.Tensor) or not isinstance(regions, (list, tuple)):
        raise TypeError(f"{name}: regions must be a list or tuple of uint8 [Hr,Wr,3] tensors (one region: the *_region call), got {type(regions).__name__}")
    n = len(regions)
    if n < 1 or n > TILE_REGIONS_MAX:
        raise ValueError(f"{name}: {n} regions: one call takes 1 .. {TILE_REGIONS_MAX} (TILE_REGIONS_MAX); more regions per call are not built")
    for k, r in enumerate(regions):
        _region_pitch(r, f"{name}: regions[{k}]")
        if r.device != regions[0].device:
            raise ValueError(f"{name}: regions[{k}] is on {r.device}, regions[0] on {regions[0].device}: all regions of a call must be on one device")
    arr, shapes = region_table(regions)
    return arr, shapes, regions[0].device


def region_table(regions):
    """The HOST descriptor table of the region-LIST calls for regions that have passed their checks (region_list_arg; ResNet_Baseline.forward_u8_regions,
    which refuses with its own exceptions) -> (ctypes array of ToadTileRegion, [(Hr, Wr), ...])."""
    arr = (_lib.ToadTileRegion * len(regions))()
    for k, r in enumerate(regions):
        arr[k].region, arr[k].pitch, arr[k].Hr, arr[k].Wr = r.data_ptr(), _row_pitch(r, 3 * r.shape[1]), r.shape[0], r.shape[1]
    return arr, [(r.shape[0], r.shape[1]) for r in regions]


def _regions_args(regions, origins, tile, name: str, shrink=1):
    """-> (descriptor array, n, H, W, triples on the device); H, W = the NETWORK tile, the triples are checked for the footprint (shrink H, shrink W)."""
    check_shrink(shrink)
    arr, shapes, dev = region_list_arg(regions, name)
    (fh, fw), (h, w) = shrunk_tile(tile, shrink)
    o = check_region_origins(origins, shapes, fh, fw)
    if o.shape[0] == 0:
        raise ValueError(f"{name}: no origins")
    return arr, len(shapes), h, w, o.to(dev)


def tiles_u8_regions_to_f32(regions, origins, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, shrink=1) -> torch.Tensor:
    """tiles_u8_region_to_f32 for a LIST of regions: origins [B,3] = (x, y, k) on the host (check_region_origins), tile b read from regions[k] - bitwise
    tiles_u8_to_f32(torch.stack([regions[k][y:y+H, x:x+W] for x, y, k in origins]), mean, std); shrink = 2: of the box-filtered footprints."""
    arr, n, h, w, o = _regions_args(regions, origins, tile, "tiles_u8_regions_to_f32", shrink)
    norm = norm_constants_u8(mean, std)
    out = torch.empty((o.shape[0], 3, h, w), dtype=torch.float32, device=o.device)
    _lib.check(_lib.load().toad_tiles_u8_regions_to_nchw_f32(arr, n, _p(o), norm, _p(out), o.shape[0], h, w, shrink, _stream()), "toad_tiles_u8_regions_to_nchw_f32")
    return out


def stem_pool_regions_u8(regions, origins, wf: torch.Tensor, b, tile=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, shrink=1) -> torch.Tensor:
    """stem_pool_region_u8 for a LIST of regions: origins [B,3] = (x, y, k) on the host, tile b (H, 256), H % 4 == 0, read from regions[k] - bitwise
    stem_pool_nhwc_u8 on the stacked tiles (shrink = 2: on the box-filtered (2 H, 512) footprints). Padding is the tile's; every region is read in place
    whatever its address and pitch."""
    arr, n, h, w, o = _regions_args(regions, origins, tile, "stem_pool_regions_u8", shrink)
    _chk(wf, "wf"); _chk(b, "b", allow_none=True)
    if tuple(wf.shape) != (64, 192):
        raise ValueError("stem_pool_regions_u8: expected a [64,192] space-to-depth weight")
    norm = norm_constants_u8(mean, std)
    bb = o.shape[0]
    y = torch.empty((bb, h // 4, w // 4, 64), dtype=torch.float32, device=o.device)
    lib = _lib.load()
    ws = _ws(lib.toad_linear_ws_bytes(bb * (h // 2) * (w // 2), 64, 192), o.device)
    _lib.check(lib.toad_stem_pool_regions_u8(arr, n, _p(o), norm, _p(wf), _p(b), _p(y), bb, h, w, shrink, _p(ws), ws.numel(), _stream()),
               "toad_stem_pool_regions_u8")
    return y


TISSUE_CELLS = (64, 32, 16, 8, 4)      # the cell sizes of csrc/tissue.hip


def _cell_arg(name: str, cell):
    if cell not in TISSUE_CELLS:
        raise ValueError(f"{name}: cell must be one of {TISSUE_CELLS}, got {cell!r}")


def _u8_arg(name: str, arg: str, v):
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= 255:
        raise ValueError(f"{name}: {arg} must be an int in [0, 255] (the 8-bit scale), got {v!r}")


def region_tissue_cells(region: torch.Tensor, cell: int, sat_thresh: int, val_min: int) -> torch.Tensor:
    """Tissue pixels per cell x cell cell of one decoded uint8 region [Hr,Wr,3] (any row pitch, any alignment; read in place): int32 [Gy,Gx] on the device,
    Gy = ceil(Hr / cell), Gx = ceil(Wr / cell), cells anchored at the region's (0, 0), partial edge cells counting the pixels that exist. A pixel is tissue
    iff mx >= val_min and 255 (mx - mn) > sat_thresh mx, mx / mn = max / min of (r, g, b): HSV saturation above sat_thresh on the 8-bit scale in exact
    integers - not OpenCV's rounded S channel. cell in TISSUE_CELLS; sat_thresh, val_min ints in [0, 255]. One launch, no synchronisation."""
    name = "region_tissue_cells"
    pitch, hr, wr = _region_pitch(region, name)
    _cell_arg(name, cell)
    _u8_arg(name, "sat_thresh", sat_thresh)
    _u8_arg(name, "val_min", val_min)
    counts = torch.empty((-(-hr // cell), -(-wr // cell)), dtype=torch.int32, device=region.device)
    _lib.check(_lib.load().toad_region_tissue_cells_u8(_p(region), pitch, hr, wr, cell, sat_thresh, val_min, _p(counts), _stream()),
               "toad_region_tissue_cells_u8")
    return counts


def tissue_tile_counts(cells: torch.Tensor, cell: int, origin, tile, stride, n) -> torch.Tensor:
    """Tissue pixels per tile of a lattice, from the cell counts of region_tissue_cells(region, cell, ...): int32 [ny,nx] on the device. origin = (x0, y0)
    of tile (0, 0), tile = (H, W), stride = (sy, sx), n = (nx, ny); tile (j, i) has its top-left pixel at (x0 + i sx, y0 + j sy). All six lattice numbers
    must be multiples of `cell` (a tile is then an exact union of whole cells) and every tile must lie inside the region the cells were counted on
    (toad_amd.tissue.lattice gives the largest such extent). One launch, no synchronisation."""
    _chk(cells, "cells", dtype=torch.int32)
    if cells.dim() != 2:
        raise ValueError(f"tissue_tile_counts: expected int32 [Gy,Gx] cell counts, got {tuple(cells.shape)}")
    (x0, y0), (h, w), (sy, sx), (nx, ny) = origin, tile, stride, n
    if nx < 1 or ny < 1:
        raise ValueError(f"tissue_tile_counts: an empty lattice (nx = {nx}, ny = {ny})")
    out = torch.empty((ny, nx), dtype=torch.int32, device=cells.device)
    _lib.check(_lib.load().toad_tissue_tile_counts(_p(cells), cells.shape[0], cells.shape[1], cell, x0, y0, h, w, sx, sy, nx, ny, _p(out), _stream()),
               "toad_tissue_tile_counts")
    return out


SEG_DOWNS = (1, 2, 4, 8, 16, 32)       # the box filters of csrc/tissue_seg.hip
SEG_MEDIANS = (1, 3, 5, 7)             # ... and its median windows


def _plane_pitch(plane: torch.Tensor, name: str):
    """The device / dtype / layout checks of the plane calls -> (pitch in bytes, Hp, Wp). A plane is uint8 [Hp,Wp] with stride(1) == 1 and any row pitch
    >= Wp (a window of a wider plane is taken as it is); either extent may be 0."""
    if not isinstance(plane, torch.Tensor) or not plane.is_cuda:
        raise RuntimeError(f"{name}: plane must be a CUDA(HIP) tensor: toad_amd has no CPU path")
    if plane.dtype != torch.uint8:
        raise TypeError(f"{name}: plane must be torch.uint8, got {plane.dtype}")
    if plane.dim() != 2:
        raise ValueError(f"{name}: expected a uint8 [Hp,Wp] plane, got shape {tuple(plane.shape)}")
    hp, wp = plane.shape
    if hp and wp and not ((plane.stride(1) == 1 or wp == 1) and (plane.stride(0) >= wp or hp == 1)):
        raise ValueError(f"{name}: expected a uint8 [Hp,Wp] plane with stride(1) == 1 and a row pitch >= Wp, got shape {tuple(plane.shape)} strides "
                         f"{tuple(plane.stride())}")
    return _row_pitch(plane, wp), hp, wp


def region_saturation(region: torch.Tensor, down: int, val_min: int = 0, out=None) -> torch.Tensor:
    """The saturation plane of one decoded uint8 region [Hr,Wr,3] (any row pitch, any alignment; read in place): uint8 [Hr // down, Wr // down] on the
    device. Per channel m = the down x down box mean rounded half up, (sum + down^2 / 2) // down^2 (partial boxes at the right and the bottom edge are
    dropped); with mx / mn = max / min of the mean pixel, S = (255 (mx - mn) + (mx >> 1)) // mx - 255 (mx - mn) / mx rounded half up - and S = 0 where
    mx == 0 or mx < val_min. Exact integers; not claimed to be bit-equal to OpenCV's COLOR_RGB2HSV. down in SEG_DOWNS, val_min an int in [0, 255]. `out`
    may be a uint8 [Hp,Wp] view with stride(1) == 1 and any pitch >= Wp. One launch, no synchronisation; an empty plane launches nothing."""
    name = "region_saturation"
    pitch, hr, wr = _region_pitch(region, name)
    if down not in SEG_DOWNS:
        raise ValueError(f"{name}: down must be one of {SEG_DOWNS}, got {down!r}")
    _u8_arg(name, "val_min", val_min)
    hp, wp = hr // down, wr // down
    if out is None:
        out = torch.empty((hp, wp), dtype=torch.uint8, device=region.device)
    else:
        if not isinstance(out, torch.Tensor) or out.device != region.device or tuple(out.shape) != (hp, wp):
            raise ValueError(f"{name}: out must be a uint8 [{hp},{wp}] tensor on the region's device")
        _plane_pitch(out, name)
        if out.untyped_storage().data_ptr() == region.untyped_storage().data_ptr():
            raise ValueError(f"{name}: out must not share storage with region (the plane is written while the region is read)")
    if hp == 0 or wp == 0:
        return out
    _lib.check(_lib.load().toad_region_saturation_u8(_p(region), pitch, hr, wr, down, val_min, _p(out), _row_pitch(out, wp), _stream()),
               "toad_region_saturation_u8")
    return out


SAT_LIST_MAX = 32                      # the windows one launch of regions_saturation takes (csrc/tissue_seg.hip): a longer list is more launches in the one call


def regions_saturation(regions, down: int, val_min: int = 0, outs=None) -> tuple:
    """region_saturation for a LIST of windows in ONE library call and one launch per SAT_LIST_MAX windows (toad_regions_saturation_u8;
    include/toad_hip.h): a tuple of uint8 [Hr_k // down, Wr_k // down] planes, each byte for byte what region_saturation gives for ``regions[k]`` with
    the same ``down`` and ``val_min``. ``regions`` is a sequence of uint8 [Hr,Wr,3] views on one device, of any extents, pitches and alignment - the
    strips or blocks a slide arrives in, or buffers of their own. ``outs`` is None or one uint8 [Hr_k // down, Wr_k // down] view per region with
    stride(1) == 1 and any pitch, for example each strip's rows of the slide's one plane (``tissue.slide_saturation``); no plane may share storage with
    its own region, and planes that overlap each other are the caller's business. The checks are region_saturation's, per region, with ValueErrors
    that name the window's index, all before the library is called. A window without a plane row or column is returned empty and the others are still
    written. No synchronisation, no copy to the device: the descriptors travel in the kernel argument. An empty list returns () and, like a list whose
    planes are all empty, launches nothing."""
    name = "regions_saturation"
    if isinstance(regions, (str, bytes, torch.Tensor)) or not hasattr(regions, "__len__") or not hasattr(regions, "__iter__"):
        raise ValueError(f"{name}: regions must be a sequence with one entry per window, got {type(regions).__name__}")
    regions = tuple(regions)
    n = len(regions)
    if outs is not None:
        if isinstance(outs, torch.Tensor) or not hasattr(outs, "__len__") or len(outs) != n:
            raise ValueError(f"{name}: outs must be None or a sequence of {n} planes, one per window")
        outs = tuple(outs)
    if down not in SEG_DOWNS:
        raise ValueError(f"{name}: down must be one of {SEG_DOWNS}, got {down!r}")
    _u8_arg(name, "val_min", val_min)
    planes, live = [], []
    for k, region in enumerate(regions):
        who = f"{name}: window {k}"
        pitch, hr, wr = _region_pitch(region, who)
        if region.device != regions[0].device:
            raise ValueError(f"{who}: every region must be on one device ({regions[0].device}), got {region.device}")
        hp, wp = hr // down, wr // down
        if outs is None:
            out = torch.empty((hp, wp), dtype=torch.uint8, device=region.device)
        else:
            out = outs[k]
            if not isinstance(out, torch.Tensor) or out.device != region.device or tuple(out.shape) != (hp, wp):
                raise ValueError(f"{who}: outs[{k}] must be a uint8 [{hp},{wp}] tensor on the region's device")
            _plane_pitch(out, who)
            if out.untyped_storage().data_ptr() == region.untyped_storage().data_ptr():
                raise ValueError(f"{who}: outs[{k}] must not share storage with region (the plane is written while the region is read)")
        planes.append(out)
        if hp and wp:
            live.append((region.data_ptr(), pitch, hr, wr, out.data_ptr(), _row_pitch(out, wp)))
    if live:
        host = (_lib.ToadSatWindow * len(live))(*(_lib.ToadSatWindow(*w) for w in live))
        _lib.check(_lib.load().toad_regions_saturation_u8(host, len(live), down, val_min, _stream()), "toad_regions_saturation_u8")
    return tuple(planes)


def plane_median(plane: torch.Tensor, k: int, want_hist: bool = False):
    """The k x k median of a uint8 [Hp,Wp] plane (stride(1) == 1, any pitch >= Wp, any alignment): a new contiguous uint8 [Hp,Wp] on the device. The
    output is the (k k) // 2-th of the sorted k k values of the window around each pixel, coordinates clamped to the plane (replicate border, as
    cv2.medianBlur); k in SEG_MEDIANS, k = 1 the identity; planes smaller than the window are fine. With want_hist -> (median, hist): hist int32 [256] on
    the device, hist[v] = the pixels of the median plane equal to v (integer atomics: the same on every run). One launch (and one 1 KB memset with
    want_hist), no synchronisation; an empty plane launches nothing and has a zero histogram."""
    name = "plane_median"
    pitch, hp, wp = _plane_pitch(plane, name)
    if k not in SEG_MEDIANS:
        raise ValueError(f"{name}: k must be one of {SEG_MEDIANS}, got {k!r}")
    out = torch.empty((hp, wp), dtype=torch.uint8, device=plane.device)
    if hp == 0 or wp == 0:
        return (out, torch.zeros(256, dtype=torch.int32, device=plane.device)) if want_hist else out
    hist = torch.empty(256, dtype=torch.int32, device=plane.device) if want_hist else None
    _lib.check(_lib.load().toad_plane_median_u8(_p(plane), pitch, hp, wp, k, _p(out), wp, _p(hist), _stream()), "toad_plane_median_u8")
    return (out, hist) if want_hist else out


def plane_cells(plane: torch.Tensor, cell: int, thresh: int) -> torch.Tensor:
    """Pixels > thresh per cell x cell cell of a uint8 [Hp,Wp] plane (stride(1) == 1, any pitch >= Wp, any alignment): int32 [Gy,Gx] on the device,
    Gy = ceil(Hp / cell), Gx = ceil(Wp / cell), cells anchored at (0, 0), partial edge cells counting the pixels that exist. cell in TISSUE_CELLS, thresh
    an int in [0, 255]. tissue_tile_counts sums these over a lattice given in plane units. One launch, no synchronisation."""
    name = "plane_cells"
    pitch, hp, wp = _plane_pitch(plane, name)
    _cell_arg(name, cell)
    _u8_arg(name, "thresh", thresh)
    counts = torch.empty((-(-hp // cell), -(-wp // cell)), dtype=torch.int32, device=plane.device)
    if hp == 0 or wp == 0:
        return counts
    _lib.check(_lib.load().toad_plane_cells_u8(_p(plane), pitch, hp, wp, cell, thresh, _p(counts), _stream()), "toad_plane_cells_u8")
    return counts


SEG_CLOSES = tuple(range(9))           # the closing windows of csrc/tissue_morph.hip (0 and 1: the identity)


def plane_close(plane: torch.Tensor, close: int, thresh: int) -> torch.Tensor:
    """The morphological closing of the mask plane > thresh of a uint8 [Hp,Wp] plane (stride(1) == 1, any pitch >= Wp, any alignment): a new contiguous
    uint8 [Hp,Wp] on the device, 255 where the closed mask is set and 0 elsewhere. close = c in SEG_CLOSES; with lo = c // 2 and hi = c - 1 - c // 2 the
    mask is dilated - OR over -lo <= dy, dx <= hi, the window clipped to the plane - and the result eroded - AND over the same offsets, clipped the same
    way: cv2.morphologyEx(m, MORPH_CLOSE, np.ones((c, c))) as OpenCV defines it, not claimed bit-equal to OpenCV. c = 0 or 1 binarises only. One launch,
    no synchronisation; an empty plane launches nothing."""
    name = "plane_close"
    pitch, hp, wp = _plane_pitch(plane, name)
    if not isinstance(close, int) or isinstance(close, bool) or close not in SEG_CLOSES:
        raise ValueError(f"{name}: close must be one of {SEG_CLOSES}, got {close!r}")
    _u8_arg(name, "thresh", thresh)
    out = torch.empty((hp, wp), dtype=torch.uint8, device=plane.device)
    if hp == 0 or wp == 0:
        return out
    _lib.check(_lib.load().toad_plane_close_u8(_p(plane), pitch, hp, wp, thresh, close, _p(out), wp, _stream()), "toad_plane_close_u8")
    return out


def plane_components(plane: torch.Tensor, thresh: int, background: int = 0, workspace: bool = False):
    """(labels, area): the connected components of the selected pixels, (plane > thresh) != background, of a uint8 [Hp,Wp] plane (stride(1) == 1, any pitch
    >= Wp, any alignment). background = 0 labels the pixels above the threshold with connectivity 8, background = 1 the others with connectivity 4.
    labels int32 [Hp,Wp]: -1 on unselected pixels, otherwise the smallest y * Wp + x of the pixel's component - canonical, the same on every run. area int32
    [Hp * Wp]: at a component's label its pixel count, plus 2^30 iff it touches row 0, row Hp - 1, column 0 or column Wp - 1; 0 elsewhere. Hp * Wp < 2^30.
    With `workspace` both are views of per-stream scratch (``_ws``), valid until the next such call on the stream. Three launches (two where the plane is
    one 64 x 16 tile), no synchronisation; an empty plane launches nothing."""
    name = "plane_components"
    pitch, hp, wp = _plane_pitch(plane, name)
    _u8_arg(name, "thresh", thresh)
    if not isinstance(background, int) or isinstance(background, bool) or background not in (0, 1):
        raise ValueError(f"{name}: background must be 0 or 1, got {background!r}")
    if hp * wp >= 1 << 30:
        raise ValueError(f"{name}: plane too large: Hp * Wp = {hp * wp} must stay below 2^30")
    n = hp * wp
    if workspace and n:
        labels = _ws(4 * n, plane.device, "cc_labels")[:4 * n].view(torch.int32).view(hp, wp)
        area = _ws(4 * n, plane.device, "cc_area")[:4 * n].view(torch.int32)
    else:
        labels = torch.empty((hp, wp), dtype=torch.int32, device=plane.device)
        area = torch.empty((n,), dtype=torch.int32, device=plane.device)
    if n == 0:
        return labels, area
    _lib.check(_lib.load().toad_plane_components_u8(_p(plane), pitch, hp, wp, thresh, background, _p(labels), _p(area), _stream()),
               "toad_plane_components_u8")
    return labels, area


def plane_area_select(labels: torch.Tensor, area: torch.Tensor, mode: int, limit: int) -> torch.Tensor:
    """A mask from the (labels, area) of plane_components: a new contiguous uint8 [Hp,Wp] on the device, 255 or 0. With count = area[label] & (2^30 - 1):
    mode 0 (drop small components) sets a pixel iff label >= 0 and count >= limit; mode 1 (fill small holes; labels of the background) iff label < 0, or
    count < limit and the component does not touch the plane's border. limit a non-negative int. One launch, no synchronisation."""
    name = "plane_area_select"
    for t, what in ((labels, "labels"), (area, "area")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: {what} must be a CUDA(HIP) tensor: toad_amd has no CPU path")
        if t.dtype != torch.int32:
            raise TypeError(f"{name}: {what} must be torch.int32, got {t.dtype}")
    if labels.dim() != 2 or area.dim() != 1 or area.numel() != labels.numel() or not labels.is_contiguous() or not area.is_contiguous():
        raise ValueError(f"{name}: expected contiguous labels int32 [Hp,Wp] and area int32 [Hp * Wp], got shapes {tuple(labels.shape)} and {tuple(area.shape)}")
    if not isinstance(mode, int) or isinstance(mode, bool) or mode not in (0, 1):
        raise ValueError(f"{name}: mode must be 0 (drop small components) or 1 (fill small holes), got {mode!r}")
    if not isinstance(limit, int) or isinstance(limit, bool) or limit < 0:
        raise ValueError(f"{name}: limit must be a non-negative int, got {limit!r}")
    hp, wp = labels.shape
    out = torch.empty((hp, wp), dtype=torch.uint8, device=labels.device)
    if hp == 0 or wp == 0:
        return out
    _lib.check(_lib.load().toad_plane_area_select_u8(_p(labels), _p(area), hp, wp, mode, min(limit, 1 << 30), _p(out), wp, _stream()),
               "toad_plane_area_select_u8")
    return out


HEAT_DOWNS = (1, 2, 4)                 # the box filters of csrc/heatmap.hip
HEAT_THUMB_DOWNS = (8, 16, 32)         # ... and those of its overview canvas (region_heat_thumb), which must not exceed the cell


def heat_cells(tile_q: torch.Tensor, cell: int, origin, tile, stride, n, region_hw) -> torch.Tensor:
    """The heat-map value of every cell x cell cell of an (Hr, Wr) = region_hw region: int32 [Gy,Gx] on the device, Gy = ceil(Hr / cell), Gx = ceil(Wr /
    cell). tile_q int32 [ny,nx] holds -1 for an absent tile and otherwise its score quantised to 0 .. 65535 (toad_amd.heatmap); the lattice arguments are
    those of tissue_tile_counts. With n the present tiles that cover a cell and S the sum of their q the value is (2 S + 257 n) // (514 n) - that is
    255 mean(q) / 65535 rounded half up, in 0 .. 255 - and -1 where no present tile covers the cell. One launch, no synchronisation."""
    _chk(tile_q, "tile_q", dtype=torch.int32)
    (x0, y0), (h, w), (sy, sx), (nx, ny), (hr, wr) = origin, tile, stride, n, region_hw
    if tile_q.dim() != 2 or tuple(tile_q.shape) != (ny, nx) or nx < 1 or ny < 1:
        raise ValueError(f"heat_cells: expected a non-empty int32 [ny,nx] = [{ny},{nx}] tile table, got {tuple(tile_q.shape)}")
    if hr < 1 or wr < 1:
        raise ValueError(f"heat_cells: bad region shape (Hr, Wr) = {region_hw!r}")
    _cell_arg("heat_cells", cell)
    cells = torch.empty((-(-hr // cell), -(-wr // cell)), dtype=torch.int32, device=tile_q.device)
    _lib.check(_lib.load().toad_heat_cells(_p(tile_q), nx, ny, cell, x0, y0, h, w, sx, sy, cells.shape[0], cells.shape[1], _p(cells), _stream()),
               "toad_heat_cells")
    return cells


HEAT_BLUR_RADIUS = 16                  # the widest half-kernel of heat_cells_blur, in cells
HEAT_BLUR_SUM = 1024                   # ... and the largest sum of its full 1-D kernel: 2 N + D then fits in int32


def heat_blur_taps(name: str, taps) -> tuple:
    """The half-kernel of heat_cells_blur as a tuple of Python ints, or ValueError: r + 1 ints with 1 <= r <= HEAT_BLUR_RADIUS, taps[0] >= 1, every tap >= 0
    and taps[0] + 2 sum(taps[1:]) <= HEAT_BLUR_SUM."""
    if isinstance(taps, (str, bytes, torch.Tensor)) or not hasattr(taps, "__len__") or not hasattr(taps, "__iter__"):
        raise ValueError(f"{name}: taps must be a sequence of ints w[0 .. r] on the host (the half of a symmetric kernel), got {type(taps).__name__}")
    w = tuple(taps)
    if any(isinstance(t, bool) or not isinstance(t, numbers.Integral) for t in w):
        raise ValueError(f"{name}: taps must be ints, got {w!r}")
    w = tuple(int(t) for t in w)
    if not 1 <= len(w) - 1 <= HEAT_BLUR_RADIUS:
        raise ValueError(f"{name}: the radius len(taps) - 1 = {len(w) - 1} must lie in 1 .. {HEAT_BLUR_RADIUS} cells")
    if w[0] < 1 or min(w) < 0:
        raise ValueError(f"{name}: taps[0] must be >= 1 and every tap >= 0, got {w!r}")
    if w[0] + 2 * sum(w[1:]) > HEAT_BLUR_SUM:
        raise ValueError(f"{name}: taps[0] + 2 sum(taps[1:]) = {w[0] + 2 * sum(w[1:])} exceeds {HEAT_BLUR_SUM} (2 N + D must fit in int32)")
    return w


def heat_cells_blur(cells: torch.Tensor, taps) -> torch.Tensor:
    """The cell table of heat_cells smoothed by the symmetric separable integer kernel w[|dy|] w[|dx|], w = taps (heat_blur_taps; heatmap.gaussian_taps gives
    Gaussian ones): a new int32 [Gy,Gx] on the device. A cell without a value (-1) keeps none; elsewhere, over the cells of the (2 r + 1)^2 window that lie
    inside the table and hold a value v (above 255 reads as 255), N = sum w w min(v, 255), D = sum w w and the result is (2 N + D) // (2 D) - a
    normalised convolution in integers (include/toad_hip.h): absent cells carry no weight, a constant field is reproduced, (k, 0, ..) is the identity.
    The taps travel as kernel arguments. One launch, no synchronisation; an empty table launches nothing."""
    name = "heat_cells_blur"
    _chk(cells, "cells", dtype=torch.int32)
    if cells.dim() != 2 or cells.numel() >= 1 << 31:
        raise ValueError(f"{name}: expected an int32 [Gy,Gx] table of fewer than 2^31 cells, got {tuple(cells.shape)}")
    w = heat_blur_taps(name, taps)
    out = torch.empty_like(cells)
    if cells.numel() == 0:
        return out
    _lib.check(_lib.load().toad_heat_cells_blur(_p(cells), cells.shape[0], cells.shape[1], (ctypes.c_int * len(w))(*w), len(w) - 1, _p(out), _stream()),
               "toad_heat_cells_blur")
    return out


def _heat_window_arg(name: str, window, down, cell, hr, wr, cells):
    """The window rules of region_heat_window -> (wx, wy): two non-negative ints, multiples of max(4, down), wx + Wr < 2^30, the window inside the table."""
    if (not isinstance(window, (tuple, list)) or len(window) != 2
            or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in window)):
        raise ValueError(f"{name}: window must be (wx, wy), two ints, got {window!r}")
    wx, wy = int(window[0]), int(window[1])
    align = max(4, down)
    if wx < 0 or wy < 0 or wx % align or wy % align:
        raise ValueError(f"{name}: window (wx, wy) = ({wx}, {wy}) must be non-negative multiples of max(4, down) = {align}: a lane's 4 x 4 block and a canvas "
                         "box must lie in one cell and in one mask pixel")
    if wx + wr >= 1 << 30:
        raise ValueError(f"{name}: wx + Wr = {wx + wr} must stay below 2^30")
    if cells.dim() != 2 or -(-(wy + hr) // cell) > cells.shape[0] or -(-(wx + wr) // cell) > cells.shape[1]:
        raise ValueError(f"{name}: the window ends at cell row {-(-(wy + hr) // cell)} and cell column {-(-(wx + wr) // cell)}, beyond the int32 [Gy,Gx] = "
                         f"{list(cells.shape)} cells")
    return wx, wy


def _heat_shared_args(name: str, cells, cell, alpha, down, downs):
    """What the canvas calls check of the arguments that do not belong to one region: cell, down (one of ``downs``, not above the cell), alpha, cells."""
    _cell_arg(name, cell)
    if down not in downs:
        raise ValueError(f"{name}: down must be one of {downs}, got {down!r}")
    if down > cell:                                                  # (the overview canvas only: HEAT_DOWNS divide every cell)
        raise ValueError(f"{name}: down = {down} exceeds cell = {cell}: a canvas box must lie in one cell")
    if not isinstance(alpha, int) or isinstance(alpha, bool) or not 0 <= alpha <= 256:
        raise ValueError(f"{name}: alpha must be an int in [0, 256], got {alpha!r}")
    _chk(cells, "cells", dtype=torch.int32)


def _heat_lut_arg(name: str, lut, device):
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or not lut.is_contiguous() or lut.device != device:
        raise ValueError(f"{name}: lut must be a contiguous uint8 [256,3] tensor on the region's device")


def _heat_out_arg(name: str, region, out, ho, wo, what: str = "out"):
    """The canvas of one region: a new [ho,wo,3] tensor, or the caller's view after its checks."""
    if out is None:
        return torch.empty((ho, wo, 3), dtype=torch.uint8, device=region.device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != region.device or tuple(out.shape) != (ho, wo, 3):
        raise ValueError(f"{name}: {what} must be a uint8 [{ho},{wo},3] tensor on the region's device")
    if ho and wo and not region_layout_ok(out):
        raise ValueError(f"{name}: {what} must have strides (pitch, 3, 1) with pitch >= 3 Wo, got {tuple(out.stride())}")
    if out.untyped_storage().data_ptr() == region.untyped_storage().data_ptr():
        raise ValueError(f"{name}: {what} must not share storage with region (the canvas is written while the region is read)")
    return out


def _heat_blend_args(name: str, region, cells, cell, lut, alpha, down, out, window=None):
    """The checks region_heat_blend, region_heat_blend_px, region_heat_thumb and region_heat_window share -> (pitch, Hr, Wr, Ho, Wo, out, window)."""
    pitch, hr, wr = _region_pitch(region, name)
    windowed = name == "region_heat_window"
    downs = HEAT_THUMB_DOWNS if name == "region_heat_thumb" else HEAT_DOWNS + HEAT_THUMB_DOWNS if windowed else HEAT_DOWNS
    _heat_shared_args(name, cells, cell, alpha, down, downs)
    if windowed:
        window = _heat_window_arg(name, window, down, cell, hr, wr, cells)
    elif tuple(cells.shape) != (-(-hr // cell), -(-wr // cell)):
        raise ValueError(f"{name}: expected int32 [Gy,Gx] = [{-(-hr // cell)},{-(-wr // cell)}] cells, got {tuple(cells.shape)}")
    _heat_lut_arg(name, lut, region.device)
    ho, wo = hr // down, wr // down
    return pitch, hr, wr, ho, wo, _heat_out_arg(name, region, out, ho, wo), window


def _heat_px_args(name: str, device, alpha, down, smooth, mask, mask_down, mask_thresh, extent=None):
    """The smooth and mask checks of the per-pixel calls -> (alpha, mask, the library's (mask_pitch, Hm, Wm, mask_down, mask_thresh)). ``extent`` =
    (Hr, Wr) where the plane must be exactly the region's, None where it is the image's, of any extent (the window calls)."""
    if not isinstance(smooth, (bool, int)) or smooth not in (0, 1):
        raise ValueError(f"{name}: smooth must be False or True, got {smooth!r}")
    mp, hm, wm, md = 0, 0, 0, 0
    if mask is None:
        if mask_down is not None:
            raise ValueError(f"{name}: mask_down = {mask_down!r} without a mask")
    else:
        mp, hm, wm = _plane_pitch(mask, name)
        if mask.device != device:
            raise ValueError(f"{name}: mask must be on the region's device ({device}), got {mask.device}")
        if mask_down not in SEG_DOWNS or isinstance(mask_down, bool) or mask_down % down:
            raise ValueError(f"{name}: mask_down must be one of {SEG_DOWNS} and a multiple of down = {down}, got {mask_down!r}")
        _u8_arg(name, "mask_thresh", mask_thresh)
        if extent is not None and (hm, wm) != (extent[0] // mask_down, extent[1] // mask_down):
            raise ValueError(f"{name}: expected a uint8 [Hr // mask_down, Wr // mask_down] = [{extent[0] // mask_down},{extent[1] // mask_down}] mask, got "
                             f"{tuple(mask.shape)}")
        md = mask_down
        if hm == 0 or wm == 0:                                       # an empty plane has no address and no tissue: the box-filtered region
            mask, alpha, mp, hm, wm, md = None, 0, 0, 0, 0, 0
    return alpha, mask, (mp, hm, wm, md, mask_thresh if mask is not None else 0)


def _heat_blend(name: str, region, cells, cell, lut, alpha, down, smooth, mask, mask_down, mask_thresh, out, window=None):
    """The body of region_heat_blend, region_heat_blend_px, region_heat_thumb and region_heat_window: the px checks, then toad_<name>_u8 (the first two
    launch the same kernel; the flat one takes no smooth and no mask arguments; the window one takes (wx, wy) and a mask plane of any extent)."""
    pitch, hr, wr, ho, wo, out, window = _heat_blend_args(name, region, cells, cell, lut, alpha, down, out, window)
    alpha, mask, plane = _heat_px_args(name, region.device, alpha, down, smooth, mask, mask_down, mask_thresh, None if window is not None else (hr, wr))
    if ho == 0 or wo == 0:
        return out
    px = () if name == "region_heat_blend" else (int(smooth), _p(mask), *plane)
    entry = f"toad_{name}_u8"
    _lib.check(getattr(_lib.load(), entry)(_p(region), pitch, hr, wr, *(window or ()), _p(cells), cells.shape[0], cells.shape[1], cell, _p(lut), alpha, down, *px, _p(out),
                                           _row_pitch(out, 3 * wo), _stream()), entry)
    return out


def region_heat_blend(region: torch.Tensor, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, down: int, out=None) -> torch.Tensor:
    """The heat-map canvas of one decoded uint8 region [Hr,Wr,3] (any row pitch, any alignment; read in place): uint8 [Hr // down, Wr // down, 3] on the
    device. Per channel m = the down x down box mean rounded half up (partial boxes at the right and the bottom edge are dropped); the output is m where
    the box's cell has cells = -1 and (alpha lut[cells][c] + (256 - alpha) m + 128) >> 8 elsewhere. cells int32 [ceil(Hr / cell), ceil(Wr / cell)] with
    values -1 .. 255 (heat_cells), lut uint8 [256,3], alpha an int in [0, 256], down in HEAT_DOWNS. `out` may be a [Ho,Wo,3] uint8 view with strides
    (pitch, 3, 1), a window of a larger canvas; it must not share storage with region. One launch, no synchronisation; an empty canvas launches nothing."""
    return _heat_blend("region_heat_blend", region, cells, cell, lut, alpha, down, False, None, None, 0, out)


def region_heat_blend_px(region: torch.Tensor, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, down: int, smooth: bool = False, mask=None,
                         mask_down=None, mask_thresh: int = 0, out=None) -> torch.Tensor:
    """region_heat_blend with the colour index and the alpha decided per canvas pixel (toad_region_heat_blend_px_u8; the definition is in
    include/toad_hip.h and toad_amd.heatmap). ``smooth``: the index of a pixel is the bilinear tent between the centres of the four nearest cells, a
    neighbour outside the table or without a value counting as the pixel's own cell; coverage edges stay sharp. ``mask``: a uint8 [Hr // mask_down,
    Wr // mask_down] plane on the region's device (stride(1) == 1, any pitch, any alignment), ``mask_down`` in SEG_DOWNS and a multiple of ``down``,
    ``mask_thresh`` an int in [0, 255]: only pixels whose mask pixel is > mask_thresh are blended, the others - the pixels of the partial boxes the plane
    dropped among them - keep the box-filtered region. The (plane, t) pair of ``tissue.segment_tissue`` and its ``down`` are such a mask. With
    smooth=False and mask=None this is region_heat_blend: the same kernel. One launch, no synchronisation; an empty canvas launches nothing."""
    return _heat_blend("region_heat_blend_px", region, cells, cell, lut, alpha, down, smooth, mask, mask_down, mask_thresh, out)


def region_heat_thumb(region: torch.Tensor, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, down: int, smooth: bool = False, mask=None,
                      mask_down=None, mask_thresh: int = 0, out=None) -> torch.Tensor:
    """region_heat_blend_px at overview scale (toad_region_heat_thumb_u8): ``down`` in HEAT_THUMB_DOWNS = 8, 16, 32, the same definition and the same
    arguments, uint8 [Hr // down, Wr // down, 3] in ONE pass over the region - no full-size canvas in between, no second rounding. ``down`` must not
    exceed ``cell`` (a canvas box must lie in one cell: ValueError before any launch), and ``mask_down`` is a multiple of ``down``, so it lies in
    down .. 32. One launch, no synchronisation; an empty canvas launches nothing."""
    return _heat_blend("region_heat_thumb", region, cells, cell, lut, alpha, down, smooth, mask, mask_down, mask_thresh, out)


def region_heat_window(region: torch.Tensor, window, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, down: int, smooth: bool = False,
                       mask=None, mask_down=None, mask_thresh: int = 0, out=None) -> torch.Tensor:
    """The canvas of a WINDOW of a larger image (toad_region_heat_window_u8; the definition is in include/toad_hip.h): ``region`` [Hr,Wr,3] is the window
    whose pixel (0, 0) is pixel ``window`` = (wx, wy) of the image - "the slide" - that ``cells`` int32 [Gy,Gx] and the ``mask`` plane describe. The uint8
    [Hr // down, Wr // down, 3] written is byte for byte rows wy // down .. and columns wx // down .. of the slide's canvas under region_heat_blend_px
    (``down`` in 1, 2, 4) or region_heat_thumb (``down`` in 8, 16, 32, not above ``cell``): a tent neighbour inside the table contributes its value also
    where it lies outside the window, so canvases put together from strips or blocks show no seams. wx and wy are non-negative multiples of
    max(4, down), wx + Wr < 2^30, and the table holds the window: ceil((wy + Hr) / cell) <= Gy, ceil((wx + Wr) / cell) <= Gx. ``mask`` is the slide's
    plane, uint8 of any extent (a pixel outside it is not tissue), ``mask_down`` and ``mask_thresh`` as for region_heat_blend_px. ``out`` may be a view
    into the slide's canvas at any pitch. ValueError for anything else, before the library is called. One launch, no synchronisation; a canvas with no
    rows or no columns launches nothing."""
    return _heat_blend("region_heat_window", region, cells, cell, lut, alpha, down, smooth, mask, mask_down, mask_thresh, out, window)


HEAT_LIST_MAX = 32                     # the windows one launch of region_heat_windows takes (csrc/heatmap.hip): a longer list is more launches in the one call


def region_heat_windows(regions, windows, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, down: int, smooth: bool = False, mask=None,
                        mask_down=None, mask_thresh: int = 0, outs=None) -> tuple:
    """region_heat_window for a LIST of windows of one slide in ONE library call and one launch per HEAT_LIST_MAX windows
    (toad_region_heat_windows_u8; include/toad_hip.h): a tuple of uint8 [Hr_k // down, Wr_k // down, 3] canvases, each byte for byte what
    region_heat_window gives for ``regions[k]`` at ``windows[k]`` = (wx, wy) with the same other arguments. ``regions`` is a sequence of uint8 [Hr,Wr,3]
    views on one device, of any extents, pitches and alignment - blocks or strips of one resident slide, or buffers of their own; ``cells``, ``cell``,
    ``lut``, ``alpha``, ``down``, ``smooth`` and the ``mask`` plane are the slide's and shared. ``outs`` is None or one view per window, for example each
    window's rows and columns of the slide's canvas; no canvas may share storage with its own region, and canvases that overlap each other are the
    caller's business. The checks are region_heat_window's, per window, with ValueErrors that name the window's index, all before the library is
    called. A window without a canvas row or column is returned empty and the others are still rendered. No synchronisation, no copy to the device:
    the descriptors travel in the kernel argument. An empty list, or one whose canvases are all empty, launches nothing."""
    name = "region_heat_windows"
    for arg, what in ((regions, "regions"), (windows, "windows")):
        if isinstance(arg, (str, bytes, torch.Tensor)) or not hasattr(arg, "__len__") or not hasattr(arg, "__iter__"):
            raise ValueError(f"{name}: {what} must be a sequence with one entry per window, got {type(arg).__name__}")
    regions, windows = tuple(regions), tuple(windows)
    n = len(regions)
    if len(windows) != n:
        raise ValueError(f"{name}: {n} regions but {len(windows)} windows: one (wx, wy) per region")
    if outs is not None:
        if isinstance(outs, torch.Tensor) or not hasattr(outs, "__len__") or len(outs) != n:
            raise ValueError(f"{name}: outs must be None or a sequence of {n} canvases, one per window")
        outs = tuple(outs)
    _heat_shared_args(name, cells, cell, alpha, down, HEAT_DOWNS + HEAT_THUMB_DOWNS)
    device = regions[0].device if n and isinstance(regions[0], torch.Tensor) else cells.device
    _heat_lut_arg(name, lut, device)
    alpha, mask, plane = _heat_px_args(name, device, alpha, down, smooth, mask, mask_down, mask_thresh)
    canvases, live = [], []
    for k, (region, window) in enumerate(zip(regions, windows)):
        who = f"{name}: window {k}"
        pitch, hr, wr = _region_pitch(region, who)
        if region.device != device:
            raise ValueError(f"{who}: every region must be on one device ({device}), got {region.device}")
        wx, wy = _heat_window_arg(who, window, down, cell, hr, wr, cells)
        ho, wo = hr // down, wr // down
        out = _heat_out_arg(who, region, None if outs is None else outs[k], ho, wo, what=f"outs[{k}]")
        canvases.append(out)
        if ho and wo:
            live.append((region, pitch, hr, wr, wx, wy, out, _row_pitch(out, 3 * wo)))
    if live:
        lib = _lib.load()
        host = (_lib.ToadHeatWindow * len(live))(*(_lib.ToadHeatWindow(r.data_ptr(), rp, hr, wr, wx, wy, o.data_ptr(), op) for r, rp, hr, wr, wx, wy, o, op in live))
        _lib.check(lib.toad_region_heat_windows_u8(host, len(live), _p(cells), cells.shape[0], cells.shape[1], cell, _p(lut), alpha, down, int(smooth), _p(mask),
                                                   *plane, _stream()), "toad_region_heat_windows_u8")
    return tuple(canvases)


def heat_downs_arg(name: str, downs) -> tuple:
    """The ``downs`` of the pyramid calls as a tuple of Python ints, or ValueError: a non-empty sequence of distinct values from 1, 2, 4, 8, 16, 32."""
    legal = HEAT_DOWNS + HEAT_THUMB_DOWNS
    if isinstance(downs, (str, bytes, torch.Tensor)) or not hasattr(downs, "__len__") or not hasattr(downs, "__iter__"):
        raise ValueError(f"{name}: downs must be a non-empty sequence of distinct values from {legal}, got {downs!r}")
    ds = tuple(downs)
    if not ds or any(isinstance(d, bool) or not isinstance(d, numbers.Integral) or d not in legal for d in ds) or len(set(ds)) != len(ds):
        raise ValueError(f"{name}: downs must be a non-empty sequence of distinct values from {legal}, got {downs!r}")
    return tuple(int(d) for d in ds)


def region_heat_pyramid(region: torch.Tensor, window, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, downs, smooth: bool = False,
                        mask=None, mask_down=None, mask_thresh: int = 0, outs=None) -> tuple:
    """Several levels of region_heat_window from ONE read of the window (toad_region_heat_pyramid_u8; include/toad_hip.h): a tuple of uint8
    [Hr // down, Wr // down, 3] canvases in the order of ``downs``, each byte for byte what region_heat_window gives for that ``down`` with the same other
    arguments. ``downs`` is a non-empty sequence of distinct values from 1, 2, 4, 8, 16, 32; with D = max(downs) the rules are region_heat_window's at
    ``down`` = D: D <= ``cell``, ``window`` = (wx, wy) non-negative multiples of max(4, D), wx + Wr < 2^30, the table holds the window, ``mask_down`` a
    multiple of D. Each level keeps its own extent: the rows and columns a coarse level drops are still rendered at the finer ones, and an empty level
    is returned empty. ``outs`` is None or one view per level, each as ``out`` of region_heat_window; no two of them may share storage, and none may
    share storage with the region. ``smooth`` at ``cell`` = 4 with more than one level is not done (ValueError). ValueError for anything else, before the
    library is called. One launch for any number of levels (one level: region_heat_window's kernel), no synchronisation; a call in which every level is
    empty launches nothing."""
    name = "region_heat_pyramid"
    ds = heat_downs_arg(name, downs)
    top = max(ds)
    pitch, hr, wr = _region_pitch(region, name)
    _cell_arg(name, cell)
    if top > cell:
        raise ValueError(f"{name}: down = {top}, the largest level, exceeds cell = {cell}: a canvas box must lie in one cell")
    if not isinstance(alpha, int) or isinstance(alpha, bool) or not 0 <= alpha <= 256:
        raise ValueError(f"{name}: alpha must be an int in [0, 256], got {alpha!r}")
    _chk(cells, "cells", dtype=torch.int32)
    wx, wy = _heat_window_arg(name, window, top, cell, hr, wr, cells)
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or not lut.is_contiguous() or lut.device != region.device:
        raise ValueError(f"{name}: lut must be a contiguous uint8 [256,3] tensor on the region's device")
    if not isinstance(smooth, (bool, int)) or smooth not in (0, 1):
        raise ValueError(f"{name}: smooth must be False or True, got {smooth!r}")
    if smooth and cell == 4 and len(ds) > 1:
        raise ValueError(f"{name}: smooth at cell = 4 is not done for more than one level (render those levels one by one with region_heat_window)")
    mp, hm, wm, md = 0, 0, 0, 0
    if mask is None:
        if mask_down is not None:
            raise ValueError(f"{name}: mask_down = {mask_down!r} without a mask")
    else:
        mp, hm, wm = _plane_pitch(mask, name)
        if mask.device != region.device:
            raise ValueError(f"{name}: mask must be on the region's device ({region.device}), got {mask.device}")
        if mask_down not in SEG_DOWNS or isinstance(mask_down, bool) or mask_down % top:
            raise ValueError(f"{name}: mask_down must be one of {SEG_DOWNS} and a multiple of down = {top}, the largest level, got {mask_down!r}")
        _u8_arg(name, "mask_thresh", mask_thresh)
        md = mask_down
        if hm == 0 or wm == 0:                                       # an empty plane has no address and no tissue: the box-filtered region
            mask, alpha, mp, hm, wm, md = None, 0, 0, 0, 0, 0
    shapes = [(hr // d, wr // d) for d in ds]
    if outs is None:
        outs = tuple(torch.empty((ho, wo, 3), dtype=torch.uint8, device=region.device) for ho, wo in shapes)
    else:
        if isinstance(outs, torch.Tensor) or not hasattr(outs, "__len__") or len(outs) != len(ds):
            raise ValueError(f"{name}: outs must be None or a sequence of {len(ds)} canvases, one per level of downs = {ds}")
        outs = tuple(outs)
        for k, (d, out, (ho, wo)) in enumerate(zip(ds, outs, shapes)):
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != region.device or tuple(out.shape) != (ho, wo, 3):
                raise ValueError(f"{name}: outs[{k}] (down = {d}) must be a uint8 [{ho},{wo},3] tensor on the region's device")
            if ho and wo and not region_layout_ok(out):
                raise ValueError(f"{name}: outs[{k}] (down = {d}) must have strides (pitch, 3, 1) with pitch >= 3 Wo, got {tuple(out.stride())}")
        for k, (d, out, (ho, wo)) in enumerate(zip(ds, outs, shapes)):
            if out.untyped_storage().data_ptr() == region.untyped_storage().data_ptr():
                raise ValueError(f"{name}: outs[{k}] (down = {d}) must not share storage with region (the canvas is written while the region is read)")
            for j in range(k):
                if out.untyped_storage().data_ptr() == outs[j].untyped_storage().data_ptr() and ho and wo and shapes[j][0] and shapes[j][1]:
                    raise ValueError(f"{name}: outs[{j}] and outs[{k}] must not share storage (every canvas is written in the same launch)")
    levels = 0
    ptrs, pitches = (ctypes.c_void_p * 6)(), (ctypes.c_int64 * 6)()
    for d, out, (ho, wo) in zip(ds, outs, shapes):
        if ho == 0 or wo == 0:
            continue
        k = d.bit_length() - 1
        levels |= 1 << k
        ptrs[k], pitches[k] = out.data_ptr(), _row_pitch(out, 3 * wo)
    if levels == 0:
        return outs
    _lib.check(_lib.load().toad_region_heat_pyramid_u8(_p(region), pitch, hr, wr, wx, wy, _p(cells), cells.shape[0], cells.shape[1], cell, _p(lut), alpha, levels,
                                                       int(smooth), _p(mask), mp, hm, wm, md, mask_thresh if mask is not None else 0, ptrs, pitches, _stream()),
               "toad_region_heat_pyramid_u8")
    return outs


HEAT_PYR_LIST_MAX = 16                 # the windows one launch of region_heat_pyramid_windows takes (csrc/heatmap.hip): a longer list is more launches in the one call


def region_heat_pyramid_windows(regions, windows, cells: torch.Tensor, cell: int, lut: torch.Tensor, alpha: int, downs, smooth: bool = False, mask=None,
                                mask_down=None, mask_thresh: int = 0, outs=None) -> tuple:
    """region_heat_pyramid for a LIST of windows of one slide in ONE library call and one launch per HEAT_PYR_LIST_MAX windows
    (toad_region_heat_pyramid_windows_u8; include/toad_hip.h): a tuple with one tuple of canvases per window, in the order of ``downs``, canvas j of
    window k being uint8 [Hr_k // downs[j], Wr_k // downs[j], 3] and byte for byte what region_heat_pyramid gives for ``regions[k]`` at ``windows[k]`` =
    (wx, wy) with the same other arguments. ``regions`` and ``windows`` are region_heat_windows's - views of any extents, pitches and alignment on one
    device and their places, here multiples of max(4, max(downs)); ``cells``, ``cell``, ``lut``, ``alpha``, ``downs``, ``smooth`` and the ``mask`` plane
    are the slide's and shared, under region_heat_pyramid's rules. ``outs`` is None or one sequence per window of one view per level, for example each
    window's rows and columns of per-level slide canvases: within one window no two levels may share storage and none may share storage with its
    region; across windows the canvases may be views of one canvas, and overlap between windows is the caller's business. The checks are
    region_heat_pyramid's, per window, with ValueErrors that name the window's index, all before the library is called. A level that is empty for a
    window is returned empty there, and the window's other levels and the other windows are still rendered. No synchronisation, no copy to the
    device: the descriptors travel in the kernel argument. An empty list, or one whose canvases are all empty, launches nothing."""
    name = "region_heat_pyramid_windows"
    ds = heat_downs_arg(name, downs)
    top = max(ds)
    for arg, what in ((regions, "regions"), (windows, "windows")):
        if isinstance(arg, (str, bytes, torch.Tensor)) or not hasattr(arg, "__len__") or not hasattr(arg, "__iter__"):
            raise ValueError(f"{name}: {what} must be a sequence with one entry per window, got {type(arg).__name__}")
    regions, windows = tuple(regions), tuple(windows)
    n = len(regions)
    if len(windows) != n:
        raise ValueError(f"{name}: {n} regions but {len(windows)} windows: one (wx, wy) per region")
    if outs is not None:
        if isinstance(outs, torch.Tensor) or not hasattr(outs, "__len__") or len(outs) != n:
            raise ValueError(f"{name}: outs must be None or a sequence of {n} sequences of {len(ds)} canvases, one per window and level of downs = {ds}")
        outs = tuple(outs)
    _cell_arg(name, cell)
    if top > cell:
        raise ValueError(f"{name}: down = {top}, the largest level, exceeds cell = {cell}: a canvas box must lie in one cell")
    if not isinstance(alpha, int) or isinstance(alpha, bool) or not 0 <= alpha <= 256:
        raise ValueError(f"{name}: alpha must be an int in [0, 256], got {alpha!r}")
    _chk(cells, "cells", dtype=torch.int32)
    device = regions[0].device if n and isinstance(regions[0], torch.Tensor) else cells.device
    _heat_lut_arg(name, lut, device)
    alpha, mask, plane = _heat_px_args(name, device, alpha, top, smooth, mask, mask_down, mask_thresh)
    if smooth and cell == 4 and len(ds) > 1:
        raise ValueError(f"{name}: smooth at cell = 4 is not done for more than one level (render those levels one by one with region_heat_windows)")
    result, live = [], []
    for k, (region, window) in enumerate(zip(regions, windows)):
        who = f"{name}: window {k}"
        pitch, hr, wr = _region_pitch(region, who)
        if region.device != device:
            raise ValueError(f"{who}: every region must be on one device ({device}), got {region.device}")
        wx, wy = _heat_window_arg(who, window, top, cell, hr, wr, cells)
        given = None
        if outs is not None:
            given = outs[k]
            if isinstance(given, torch.Tensor) or not hasattr(given, "__len__") or len(given) != len(ds):
                raise ValueError(f"{who}: outs[{k}] must be a sequence of {len(ds)} canvases, one per level of downs = {ds}")
            given = tuple(given)
        shapes = [(hr // d, wr // d) for d in ds]
        canvases = tuple(_heat_out_arg(who, region, None if given is None else given[j], ho, wo, what=f"outs[{k}][{j}] (down = {d})")
                         for j, (d, (ho, wo)) in enumerate(zip(ds, shapes)))
        if given is not None:
            for j, (ho, wo) in enumerate(shapes):
                for i in range(j):
                    if ho and wo and shapes[i][0] and shapes[i][1] and canvases[j].untyped_storage().data_ptr() == canvases[i].untyped_storage().data_ptr():
                        raise ValueError(f"{who}: outs[{k}][{i}] and outs[{k}][{j}] must not share storage (every canvas of a window is written in the same launch)")
        result.append(canvases)
        if any(ho and wo for ho, wo in shapes):
            live.append((region, pitch, hr, wr, wx, wy, [(d.bit_length() - 1, c, wo) for d, c, (ho, wo) in zip(ds, canvases, shapes) if ho and wo]))
    if live:
        lib = _lib.load()
        host = (_lib.ToadHeatPyramidWindow * len(live))()
        for desc, (r, rp, hr, wr, wx, wy, levels) in zip(host, live):
            desc.region, desc.pitch, desc.Hr, desc.Wr, desc.wx, desc.wy = r.data_ptr(), rp, hr, wr, wx, wy
            for b, c, wo in levels:
                desc.outs[b], desc.out_pitches[b] = c.data_ptr(), _row_pitch(c, 3 * wo)
        bits = 0
        for d in ds:
            bits |= d
        _lib.check(lib.toad_region_heat_pyramid_windows_u8(host, len(live), _p(cells), cells.shape[0], cells.shape[1], cell, _p(lut), alpha, bits, int(smooth), _p(mask),
                                                           *plane, _stream()), "toad_region_heat_pyramid_windows_u8")
    return tuple(result)


def maxpool3x3s2_nhwc(x: torch.Tensor) -> torch.Tensor:
    _chk(x, "x")
    b, h, w, c = x.shape
    y = torch.empty((b, (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().toad_maxpool3x3s2_nhwc_f32(_p(x), _p(y), b, h, w, c, _stream()), "toad_maxpool3x3s2_nhwc_f32")
    return y


def avgpool_nhwc(x: torch.Tensor) -> torch.Tensor:
    """x [B,HW,C] -> [B,C] mean over HW."""
    _chk(x, "x")
    b, hw, c = x.shape
    y = torch.empty((b, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().toad_avgpool_nhwc_f32(_p(x), _p(y), b, hw, c, _stream()), "toad_avgpool_nhwc_f32")
    return y


# ---- e4m3 bags: 8-bit codes with one power-of-two exponent per bag (csrc/bag_e4m3.hip; the format: toad_amd/ingest.py) ----------------------
E4M3_EXP_MIN, E4M3_EXP_MAX = -7, 15        # the exponents at which every finite code is exactly an fp16 number
E4M3_MAX = 448.0                           # the largest finite e4m3fn value (code 0x7E)


def e4m3_exponent(amax) -> int:
    """The exponent of a bag whose largest magnitude is ``amax``: the largest e in -7 .. 15 with amax * 2^e <= 448, so the bag uses the top of the
    code range without saturating. 0 for amax == 0. -7 for amax > 57344: magnitudes up to fp16's 65504 then SATURATE at 448 * 2^7 = 57344.
    A NaN or infinite amax is a ValueError. Python numbers only: nothing here touches a device."""
    import math
    amax = float(amax)
    if math.isnan(amax) or math.isinf(amax):
        raise ValueError(f"e4m3_exponent: amax must be finite, got {amax!r} (a NaN or Inf in the bag?)")
    amax = abs(amax)
    if amax == 0.0:
        return 0
    for e in range(E4M3_EXP_MAX, E4M3_EXP_MIN, -1):
        if math.ldexp(amax, e) <= E4M3_MAX:
            return e
    return E4M3_EXP_MIN


def _e4m3_exp_arg(name: str, exp) -> int:
    if not isinstance(exp, int) or isinstance(exp, bool) or not E4M3_EXP_MIN <= exp <= E4M3_EXP_MAX:
        raise ValueError(f"{name}: exp must be an int in {E4M3_EXP_MIN} .. {E4M3_EXP_MAX}, got {exp!r}")
    return exp


def bag_dequantise_e4m3(codes: torch.Tensor, exp: int, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """The fp16 / fp32 bag of an e4m3 bag: out[i, j] = value(codes[i, j]) * 2^-exp, exact (toad_bag_dequant_e4m3). ``codes``: contiguous [N, K]
    torch.uint8 or the same bytes as torch.float8_e4m3fn. ``out``: a contiguous [N, K] fp16 or fp32 tensor on the same device - it may be a row view of
    a larger buffer, at any row - or None for a new one of ``out_dtype``. On a device tensor: one launch on the current stream, no synchronisation. A
    CPU tensor takes the same call through torch ops (view as float8_e4m3fn, up-cast, scale), with identical bits. Anything else is a ValueError."""
    name = "bag_dequantise_e4m3"
    exp = _e4m3_exp_arg(name, exp)
    if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.uint8, torch.float8_e4m3fn) or codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError(f"{name}: codes must be a contiguous [N, K] torch.uint8 or torch.float8_e4m3fn tensor")
    if out is None:
        if out_dtype not in (torch.float16, torch.float32):
            raise ValueError(f"{name}: out_dtype must be torch.float16 or torch.float32, got {out_dtype}")
        out = torch.empty(codes.shape, dtype=out_dtype, device=codes.device)
    elif not isinstance(out, torch.Tensor) or out.dtype not in (torch.float16, torch.float32) or out.shape != codes.shape or not out.is_contiguous() \
            or out.device != codes.device:
        raise ValueError(f"{name}: out must be a contiguous fp16 or fp32 tensor of the codes' shape {tuple(codes.shape)} on their device")
    if codes.numel() == 0:
        return out
    if not codes.is_cuda:
        out.copy_(codes.view(torch.float8_e4m3fn).to(torch.float32) * 2.0 ** -exp)       # exact in fp32, and exact again in the cast to fp16
        return out
    _lib.check(_lib.load().toad_bag_dequant_e4m3(_p(codes), _p(out), int(out.dtype == torch.float32), codes.numel(), exp, _stream()),
               "toad_bag_dequant_e4m3")
    return out


def bag_quantise_e4m3(x: torch.Tensor, exp: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """-> (codes uint8 [N, K], exp): the e4m3 bag of a contiguous fp32 or fp16 [N, K] bag (toad_bag_quant_e4m3). With y = |x| * 2^exp the code is the
    e4m3 value nearest to y, a tie going to the even code; y >= 448 (an infinite x included) saturates at 0x7E; the sign bit is kept; fp32 is rounded
    ONCE. ``exp=None``: e4m3_exponent of x.abs().amax() - one read-back, and a ValueError where x holds a NaN or an Inf; with ``exp`` given a NaN
    becomes a NaN code and there is no synchronisation. On a device tensor: one launch on the current stream. A CPU tensor takes the same call
    through torch ops (scale, clamp to +-448, convert), with identical bits."""
    name = "bag_quantise_e4m3"
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float16) or x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be a contiguous [N, K] fp32 or fp16 tensor")
    if exp is None:
        exp = e4m3_exponent(x.abs().amax().item() if x.numel() else 0.0)
    exp = _e4m3_exp_arg(name, exp)
    if not x.is_cuda:
        y = x.to(torch.float32) * 2.0 ** exp
        return torch.clamp(y, -E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8), exp     # (torch alone gives NaN above 448)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        _lib.check(_lib.load().toad_bag_quant_e4m3(_p(x), int(x.dtype == torch.float16), _p(codes), x.numel(), exp, _stream()), "toad_bag_quant_e4m3")
    return codes, exp


# ---- e4m3 shards: a list of e4m3 bags back to back, one exponent each, in one call (csrc/bag_e4m3.hip, "a LIST of bags") -------------------------------
E4M3_LIST_MAX = 64                         # TOAD_E4M3_LIST_MAX: bags per launch; a longer list is several launches inside the one call


def _e4m3_offsets_arg(name: str, offsets, rows: int):
    """-> the row offsets as a list of B + 1 ints: 0 first, non-decreasing, ``rows`` last."""
    try:
        offs = [int(o) for o in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: offsets must be B + 1 integers") from None
    if len(offs) < 1 or offs[0] != 0:
        raise ValueError(f"{name}: offsets must start with 0, got {offs[:1]}")
    for i in range(len(offs) - 1):
        if offs[i + 1] < offs[i]:
            raise ValueError(f"{name}: bag {i}: offsets decrease from {offs[i]} to {offs[i + 1]}")
    if offs[-1] != rows:
        raise ValueError(f"{name}: offsets end at {offs[-1]}, the concatenation has {rows} rows")
    return offs


def _e4m3_exps_arg(name: str, exps, nb: int):
    exps = exps.tolist() if isinstance(exps, torch.Tensor) else list(exps)
    if len(exps) != nb:
        raise ValueError(f"{name}: {len(exps)} exponents for {nb} bags")
    for i, e in enumerate(exps):
        if not isinstance(e, int) or isinstance(e, bool) or not E4M3_EXP_MIN <= e <= E4M3_EXP_MAX:
            raise ValueError(f"{name}: bag {i}: exp must be an int in {E4M3_EXP_MIN} .. {E4M3_EXP_MAX}, got {e!r}")
    return exps


def bags_dequantise_e4m3(codes: torch.Tensor, offsets, exps, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """The fp16 / fp32 concatenation of a list of e4m3 bags that lie back to back (toad_bags_dequant_e4m3): bag b is rows offsets[b] .. offsets[b + 1] of
    ``codes`` (contiguous [R, K] torch.uint8 or torch.float8_e4m3fn) and is decoded with exps[b], bit for bit what bag_dequantise_e4m3 gives on its slice.
    ``offsets``: B + 1 ints, 0 first, non-decreasing, R last (empty bags anywhere); ``exps``: B ints in -7 .. 15. ``out`` as for the single call. On a
    device tensor: ONE launch per E4M3_LIST_MAX non-empty bags on the current stream, no upload, no synchronisation. A CPU tensor goes bag by bag through
    the single call's CPU path. Anything else is a ValueError, with the bag named."""
    name = "bags_dequantise_e4m3"
    if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.uint8, torch.float8_e4m3fn) or codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError(f"{name}: codes must be a contiguous [R, K] torch.uint8 or torch.float8_e4m3fn tensor")
    offs = _e4m3_offsets_arg(name, offsets, codes.shape[0])
    nb = len(offs) - 1
    exps = _e4m3_exps_arg(name, exps, nb)
    if out is None:
        if out_dtype not in (torch.float16, torch.float32):
            raise ValueError(f"{name}: out_dtype must be torch.float16 or torch.float32, got {out_dtype}")
        out = torch.empty(codes.shape, dtype=out_dtype, device=codes.device)
    elif not isinstance(out, torch.Tensor) or out.dtype not in (torch.float16, torch.float32) or out.shape != codes.shape or not out.is_contiguous() \
            or out.device != codes.device:
        raise ValueError(f"{name}: out must be a contiguous fp16 or fp32 tensor of the codes' shape {tuple(codes.shape)} on their device")
    if codes.numel() == 0:
        return out
    if not codes.is_cuda:
        for b in range(nb):
            if offs[b + 1] > offs[b]:
                bag_dequantise_e4m3(codes[offs[b]:offs[b + 1]], exps[b], out=out[offs[b]:offs[b + 1]])
        return out
    _lib.check(_lib.load().toad_bags_dequant_e4m3(_p(codes), _p(out), int(out.dtype == torch.float32), codes.shape[1], (ctypes.c_int64 * (nb + 1))(*offs),
                                                  (ctypes.c_int * nb)(*exps), nb, _stream()), "toad_bags_dequant_e4m3")
    return out


def _e4m3_list_x(name: str, x, offsets):
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float16) or x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be a contiguous [R, K] fp32 or fp16 tensor")
    return _e4m3_offsets_arg(name, offsets, x.shape[0])


def bags_absmax(x: torch.Tensor, offsets) -> torch.Tensor:
    """-> uint32 [B] on x's device: the fp32 bit pattern of the largest |x| of each bag of the concatenation ``x`` (contiguous [R, K] fp32 or fp16; rows
    offsets[b] .. offsets[b + 1] are bag b), fp16 up-cast exactly (toad_bags_absmax_bits). The unsigned maximum of the sign-cleared patterns: an Inf gives
    0x7F800000, any NaN in the bag a pattern above it, an empty bag 0. One fill and one launch per E4M3_LIST_MAX non-empty bags on the current stream,
    NO read-back. A CPU tensor takes the same call through torch ops, with identical bits for bags without a NaN."""
    name = "bags_absmax"
    offs = _e4m3_list_x(name, x, offsets)
    nb = len(offs) - 1
    if not x.is_cuda:
        bits = torch.zeros(nb, dtype=torch.int64)
        for b in range(nb):
            if offs[b + 1] > offs[b] and x.shape[1]:
                bits[b] = (x[offs[b]:offs[b + 1]].to(torch.float32).view(torch.int32).to(torch.int64) & 0x7FFFFFFF).max()
        return bits.to(torch.int32).view(torch.uint32)         # (sign-cleared patterns fit int32; torch has few uint32 kernels)
    if not x.numel():                                          # (an empty tensor has no address to pass)
        return torch.zeros(nb, dtype=torch.int32, device=x.device).view(torch.uint32)
    amax = torch.empty(nb, dtype=torch.int32, device=x.device)
    if nb:
        _lib.check(_lib.load().toad_bags_absmax_bits(_p(x), int(x.dtype == torch.float16), _p(amax), x.shape[1], (ctypes.c_int64 * (nb + 1))(*offs), nb,
                                                     _stream()), "toad_bags_absmax_bits")
    return amax.view(torch.uint32)


def bags_quantise_e4m3(x: torch.Tensor, offsets, exps=None):
    """-> (codes uint8 [R, K], exps list of B ints): the e4m3 bags of a concatenation of fp32 or fp16 bags (toad_bags_quant_e4m3), bag b - rows
    offsets[b] .. offsets[b + 1] - with its own exponent, bit for bit what bag_quantise_e4m3 gives on its slice. ``exps=None``: e4m3_exponent of each bag's
    largest magnitude, from bags_absmax and ONE read-back of B words (not one per bag); a NaN or an Inf in a bag is a ValueError naming the bag. With
    ``exps`` given there is no synchronisation. On a device tensor: one launch per E4M3_LIST_MAX non-empty bags on the current stream. A CPU tensor goes
    bag by bag through the single call's CPU path."""
    import struct
    name = "bags_quantise_e4m3"
    offs = _e4m3_list_x(name, x, offsets)
    nb = len(offs) - 1
    if exps is None:
        exps = []
        for b, bits in enumerate(bags_absmax(x, offs).view(torch.int32).cpu().tolist()):
            bits &= 0xFFFFFFFF
            if bits >= 0x7F800000:
                raise ValueError(f"{name}: bag {b}: a NaN or Inf in the bag (abs-max bits {bits:#010x})")
            exps.append(e4m3_exponent(struct.unpack("<f", struct.pack("<I", bits))[0]))
    exps = _e4m3_exps_arg(name, exps, nb)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if not x.is_cuda:
        for b in range(nb):
            if offs[b + 1] > offs[b]:
                codes[offs[b]:offs[b + 1]] = bag_quantise_e4m3(x[offs[b]:offs[b + 1]], exps[b])[0]
        return codes, exps
    if x.numel():
        _lib.check(_lib.load().toad_bags_quant_e4m3(_p(x), int(x.dtype == torch.float16), _p(codes), x.shape[1], (ctypes.c_int64 * (nb + 1))(*offs),
                                                    (ctypes.c_int * nb)(*exps), nb, _stream()), "toad_bags_quant_e4m3")
    return codes, exps
