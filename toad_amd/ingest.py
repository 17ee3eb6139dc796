"""Bag ingest: slide records -> device-resident bags, overlapped with compute.

Reference behaviour being replaced: ``Generic_MIL_MTL_Dataset.__getitem__`` does ``torch.load(<slide_id>.pt)``
(datasets/dataset_mtl_concat.py:369-373), the loader collates one bag per batch (utils/utils.py:30-35,51-55) and
the train loop copies it to the device synchronously (utils/core_utils_mtl_concat.py:201-204). A 100k-patch bag is
410 MB: >= 6.5 ms over PCIe Gen5 x16, more than the 3.6 ms the kernels need for the whole step.

``BagPrefetcher`` keeps ``depth`` bags in flight: worker threads read and pin them, the host->device copy runs on a
dedicated HIP stream, and the consumer's stream only waits on the copy's event. Features stored as fp16/bf16 are copied
at half the bytes and upcast on the device. The wire format stays the reference's: one ``torch.save``d ``[N, 1024]``
tensor per slide.

e4m3 bags: a second wire format, 8 bits per feature (csrc/bag_e4m3.hip; DESIGN.md "e4m3 bags")
-----------------------------------------------------------------------------------------------
* Code: OCP ``e4m3fn``, the FP8 form gfx950 has (not MI300's ``fnuz``). Byte ``c`` has sign ``c >> 7``, ``e = (c >> 3) & 15``, ``m = c & 7``; its value
  is ``m * 2^-9`` for ``e == 0`` and ``(8 + m) * 2^(e - 10)`` otherwise. ``0x7F`` and ``0xFF`` are NaN, there is no infinity, the largest finite value
  is 448 (``0x7E``). This is ``torch.uint8 -> view(torch.float8_e4m3fn) -> float`` for all 256 codes.
* Bag: codes ``[N, K]`` (uint8, or the same bytes as ``torch.float8_e4m3fn``) and ONE integer ``exp`` per bag, ``-7 <= exp <= 15``. An element is
  ``value(code) * 2^-exp``. Inside that range every finite element is exactly an fp16 number, subnormal fp16 results included (at ``exp = 15`` code 1
  is ``2^-24``); at -8 and 16 that fails. A NaN code decodes to NaN. So the decode of an e4m3 bag IS an fp16 bag, and the x16 calls read it as stored.
* Quantiser, on real numbers, with ``y = |x| * 2^exp``: the code is the e4m3 value nearest to ``y``, a tie going to the even code; every ``y >= 448``
  (an infinite ``x`` included) gives ``0x7E``; the sign bit of ``x`` is kept, also on a zero result; NaN gives a code with ``c & 0x7F == 0x7F``. fp32
  input is rounded ONCE (not through fp16), fp16 input is up-cast exactly.
* ``exp`` is chosen by ``ops.e4m3_exponent(amax)``: the largest ``e`` in -7 .. 15 with ``amax * 2^e <= 448``; 0 for an all-zero bag; -7 for
  ``amax > 57344``, where magnitudes up to fp16's 65504 saturate.
* File: ``torch.save({"e4m3": codes as torch.float8_e4m3fn [N, K], "exp": int})`` - a plain dict, so it loads with ``weights_only=True``.
* Error: ``|decode(quantise(x)) - x| <= 2^-4 |x|`` where ``|x| * 2^exp >= 2^-6`` (half an ulp of a 4-bit significand) and ``<= 2^-10 * 2^-exp`` below
  (half the spacing of the e4m3 subnormals), for ``|x| * 2^exp <= 448``.
The codes cross the link; the decode runs on the copy stream right behind each bag's copy, into the landing buffer that is there for fp16 / fp32 files.

e4m3 shards (``E4M3Shard``, ``ShardPrefetcher``, ``BagBatch``, at the end of this file): the bags of one optimiser step as ONE record - one copy, one
decode launch for all of them, each bag with its own exponent - for steps of many small bags, where the work per record and not the link bounds the feed.
"""
from __future__ import annotations

import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterable, Iterator, Optional, Sequence, Tuple, Union

import torch

Record = Tuple[Union[str, Callable[[], torch.Tensor], torch.Tensor], int, int, float]   # (source, label, site, sex)


class E4M3Bag:
    """A bag as e4m3 codes ``[N, K]`` (kept as uint8; a ``torch.float8_e4m3fn`` tensor is taken as its bytes) and one exponent: see the module docstring."""
    __slots__ = ("codes", "exp")

    def __init__(self, codes: torch.Tensor, exp: int):
        if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.uint8, torch.float8_e4m3fn):
            raise ValueError("E4M3Bag: codes must be a torch.uint8 or torch.float8_e4m3fn tensor")
        if codes.dim() != 2:
            raise ValueError(f"bag must be [N, features], got {tuple(codes.shape)}")
        if not isinstance(exp, int) or isinstance(exp, bool) or not -7 <= exp <= 15:
            raise ValueError(f"E4M3Bag: exp must be an int in -7 .. 15, got {exp!r}")
        self.codes = codes.contiguous().view(torch.uint8)
        self.exp = exp

    @property
    def shape(self):
        return self.codes.shape


def _e4m3_from_dict(d: dict) -> E4M3Bag:
    if "e4m3" not in d or "exp" not in d:
        raise ValueError(f"an e4m3 bag is a dict with the keys 'e4m3' and 'exp', got {sorted(map(str, d))}")
    return E4M3Bag(d["e4m3"], d["exp"])


def quantise_bag(t: torch.Tensor, exp: Optional[int] = None) -> E4M3Bag:
    """The e4m3 form of an fp32 / fp16 ``[N, K]`` bag, on whatever device it lies (``ops.bag_quantise_e4m3``); ``exp=None`` picks the exponent from
    the bag's largest magnitude."""
    from . import ops
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("quantise_bag: bag must be a [N, features] tensor")
    if t.dtype not in (torch.float32, torch.float16):
        t = t.to(torch.float32)
    codes, exp = ops.bag_quantise_e4m3(t.contiguous(), exp)
    return E4M3Bag(codes, exp)


def save_bag_e4m3(path, bag, exp: Optional[int] = None) -> E4M3Bag:
    """Write ``bag`` - an ``E4M3Bag``, or a tensor that is quantised first (``exp`` as for ``quantise_bag``) - in the file form of the module docstring."""
    if not isinstance(bag, E4M3Bag):
        bag = quantise_bag(bag, exp)
    elif exp is not None and exp != bag.exp:
        raise ValueError(f"save_bag_e4m3: the bag has exp = {bag.exp}, not {exp}")
    torch.save({"e4m3": bag.codes.cpu().view(torch.float8_e4m3fn), "exp": int(bag.exp)}, path)
    return bag


def _load(source):
    """-> a contiguous [N, features] host tensor, or an ``E4M3Bag``."""
    if isinstance(source, (torch.Tensor, E4M3Bag, dict)):
        t = source
    elif callable(source):
        t = source()
    else:
        t = torch.load(source, map_location="cpu")            # the reference's .pt bag, or the e4m3 dict
    if isinstance(t, dict):
        t = _e4m3_from_dict(t)
    if isinstance(t, E4M3Bag):
        return t
    if t.dim() != 2:
        raise ValueError(f"bag must be [N, features], got {tuple(t.shape)}")
    return t.contiguous()


class BagPrefetcher:
    """Iterate ``(bag, label, site, sex)`` device tensors in record order with ``depth`` bags in flight. A record's source is a tensor, a path or a
    callable; an e4m3 bag (an ``E4M3Bag``, its dict form, or a path / callable that yields one) may stand in any place of the list: its codes cross the
    link and are decoded on the copy stream into the same fp16 / fp32 tensors and landing buffers, so the consumer cannot tell the kinds apart."""

    def __init__(self, records: Sequence[Record], device: Union[str, torch.device], depth: int = 2, workers: int = 2,
                 dtype: Optional[torch.dtype] = torch.float32, prepare: bool = False, arena_rows: int = 0,
                 arena_dtype: torch.dtype = torch.float32):
        """``arena_rows`` > 0: consecutive fp32 bags are landed BACK TO BACK in device buffers of that many rows (a new buffer when the next bag
        does not fit; a bag longer than the buffer gets an allocation of its own) and handed out as views. Bags that share a buffer are their own
        concatenation, so ``SlideShardedDP`` / ``ops.mil_multi_step`` batch them into one ragged multi-slide call without copying a row
        (``ops._adjacent_rows``); set it to the DP wrapper's ``batch_rows``. A buffer is released when the last view of it dies - so ONE retained
        bag keeps its whole landing buffer alive (``arena_rows`` x features x 4 bytes: 2 GB at 524,288 rows of 1,024 features); hold copies, not
        views, of bags that must outlive their step. One buffer serves one feature width: a bag of another width starts a fresh buffer.
        ``arena_dtype``: the element type of the landing buffers. ``torch.float32`` (default): fp16 / bf16 files are up-cast while they land.
        ``torch.float16`` (together with ``dtype=torch.float16``): fp16 files land AS THEY ARE - half the link bytes and half the buffer (1 GB at
        524,288 rows) - and are handed out as fp16 views, which ``ops._adjacent_rows`` joins like fp32 ones, so the batched trainer reads them
        through the x16 multi-slide calls (toad_mil_multi_step_x16_f32) with no up-cast and no copy. A file that is NOT fp16 is down-cast on
        landing: that loses bits (11-bit significands, |x| <= 65504), and it is the caller's choice - it asked for fp16.
        ``prepare``: hand the consumer ``ops.PreparedBag`` objects instead of fp32 tensors (toad_bag_prepare_f32, ABI 9): right behind
        its host-to-device copy, on the COPY stream, every bag is brought into the plane-tiled two-piece form the first Linear and its
        weight gradient take by LDS-DMA, and the fp32 copy is released. The training stream then never measures or splits the bag
        (-3 % of a 100k-patch step, more on boxes where the abs-max pass is slower); bags below 64 patches stay fp32 tensors.
        ``dtype``: what the consumer receives. ``torch.float32`` (default) up-casts fp16 / bf16 files on the device;
        ``torch.float16`` hands fp16 bags to the model as they are (its first Linear and weight gradient then run the two-term
        fp16 kernels, toad_mil_*_x16_f32: no up-cast pass, half the HBM reads of the bag); ``None`` keeps every file's own dtype."""
        self.records = list(records)
        self.device = torch.device(device)
        self.depth = max(1, int(depth))
        self.workers = max(1, int(workers))
        self.dtype = dtype
        self.prepare = bool(prepare)
        if self.prepare and dtype is not torch.float32:
            raise ValueError("BagPrefetcher(prepare=True) prepares fp32 bags: leave dtype at torch.float32")
        self.on_gpu = self.device.type == "cuda"
        if self.prepare and not self.on_gpu:
            raise ValueError("BagPrefetcher(prepare=True) needs a HIP device (toad_amd has no CPU path)")
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        self.arena_rows = max(0, int(arena_rows))
        if arena_dtype not in (torch.float32, torch.float16):
            raise ValueError("BagPrefetcher(arena_dtype=...) must be torch.float32 or torch.float16")
        self.arena_dtype = arena_dtype
        if self.arena_rows and (self.prepare or dtype is not arena_dtype):
            raise ValueError("BagPrefetcher(arena_rows=...) lands fp32 bags: leave dtype at torch.float32 and prepare off "
                             "(fp16 landing buffers: dtype=torch.float16 together with arena_dtype=torch.float16)")
        self._arena: Optional[torch.Tensor] = None              # current landing buffer [arena_rows, features] and the rows already taken
        self._arena_used = 0

    def _decode(self, t: E4M3Bag, dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fp16 / fp32 tensor of e4m3 bag ``t`` on the device: the CODES cross the link into a staging tensor and ops.bag_dequantise_e4m3 decodes them
        into ``out`` (or a new tensor of ``dtype``). Called with the copy stream current; the staging tensor is allocated and dropped here, under that
        stream, so the allocator's stream ordering covers its reuse."""
        from . import ops
        codes = t.codes.to(self.device, non_blocking=True) if self.on_gpu else t.codes
        return ops.bag_dequantise_e4m3(codes, t.exp, out=out, out_dtype=dtype)

    def _land(self, t) -> torch.Tensor:
        """Device copy (in ``arena_dtype``) of host bag ``t`` inside the current landing buffer (called on the copy stream, in record order)."""
        n, k = t.shape
        e4m3 = isinstance(t, E4M3Bag)
        if n > self.arena_rows or n == 0:
            if e4m3:
                return self._decode(t, self.arena_dtype)
            return t.to(self.device, non_blocking=True).to(self.arena_dtype)
        if self._arena is None or self._arena.shape[1] != k or self._arena_used + n > self.arena_rows:
            self._arena = torch.empty((self.arena_rows, k), dtype=self.arena_dtype, device=self.device)
            self._arena_used = 0
        view = self._arena[self._arena_used:self._arena_used + n]
        if e4m3:
            self._decode(t, out=view)                           # H2D of the codes, decoded straight into place
        else:
            view.copy_(t, non_blocking=True)                    # H2D (+ the cast of a file of another dtype) straight into place
        self._arena_used += n
        return view

    def __len__(self) -> int:
        return len(self.records)

    # -- stage 1 (worker thread): read + pin
    def _stage_host(self, rec: Record):
        src, label, site, sex = rec
        t = _load(src)
        meta = torch.tensor([int(label), int(site)], dtype=torch.int64)
        sx = torch.tensor([float(sex)], dtype=torch.float32)
        if self.on_gpu:                                         # page-locked so every copy is truly asynchronous
            if isinstance(t, E4M3Bag):
                if not t.codes.is_pinned():
                    t = E4M3Bag(t.codes.pin_memory(), t.exp)    # (the codes are uint8 here: pinning does not depend on float8 support)
            elif not t.is_pinned():
                t = t.pin_memory()
            meta, sx = meta.pin_memory(), sx.pin_memory()       # (a pageable source would be a synchronous copy queued
        return t, meta, sx                                      #  behind the bag transfer and stall the host)

    # -- stage 2 (consumer thread, copy stream): H2D + on-device upcast
    def _stage_device(self, host):
        t, meta, sx = host
        # an e4m3 bag outside a landing buffer decodes into `dtype` (fp16 where every file keeps its own: that is what the codes hold exactly)
        e4m3_dtype = self.dtype if self.dtype in (torch.float16, torch.float32) else torch.float16 if self.dtype is None else torch.float32
        if not self.on_gpu:
            if self.arena_rows:
                return (self._land(t), meta[0:1], meta[1:2], sx), None
            if isinstance(t, E4M3Bag):
                t = self._decode(t, e4m3_dtype)
            return (t if self.dtype is None else t.to(self.dtype), meta[0:1], meta[1:2], sx), None
        with torch.cuda.stream(self.copy_stream):
            if self.arena_rows:
                bag = self._land(t)
            elif isinstance(t, E4M3Bag):
                bag = self._decode(t, e4m3_dtype)
            else:
                bag = t.to(self.device, non_blocking=True)
            if self.dtype is not None and bag.dtype != self.dtype:
                bag = bag.to(self.dtype)                        # fp16/bf16 on disk: half the PCIe bytes, upcast here
            from . import ops
            # only bags the prepared-bag kernels take (32-bit row offsets: < 1,048,576 patches): a larger one stays an fp32 tensor and
            # runs on the fp32 path instead of raising in the model after its fp32 copy was dropped
            if self.prepare and bag.dtype == torch.float32 and bag.shape[0] >= 64 and bag.shape[1] == 1024 and ops.x16_ok(bag.shape[0]):
                bag = ops.prepare_bag(bag)                      # on the copy stream (ops use the current stream); the fp32 bag dies here
            meta_d = meta.to(self.device, non_blocking=True)
            sx_d = sx.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return (bag, meta_d[0:1], meta_d[1:2], sx_d), ev

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]:
        n = len(self.records)
        if n == 0:
            return
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            host_futs = {}                                       # index -> future of the pinned host bag
            dev_ready = {}                                       # index -> (tensors, event)
            next_host = 0

            def top_up(upto: int):
                nonlocal next_host
                while next_host < min(n, upto):
                    host_futs[next_host] = pool.submit(self._stage_host, self.records[next_host])
                    next_host += 1

            top_up(self.depth + 1)
            for i in range(n):
                # issue the device copies of everything whose host stage is done, up to `depth` ahead
                for jx in range(i, min(n, i + self.depth)):
                    if jx not in dev_ready and jx in host_futs and (jx == i or host_futs[jx].done()):
                        dev_ready[jx] = self._stage_device(host_futs.pop(jx).result())   # .result() re-raises loader errors
                    elif self.arena_rows and jx not in dev_ready:
                        break                                    # landing buffers are filled in record order: never overtake a bag that is not read yet
                top_up(i + self.depth + 2)
                tensors, ev = dev_ready.pop(i)
                if ev is not None:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(ev)                          # consumer stream waits for the copy, the host does not
                    for t in tensors:                           # allocator: do not recycle while the consumer uses it
                        for u in ((t.planes, t.amax) if getattr(t, "is_prepared_bag", False) else (t,)):
                            u.record_stream(cur)
                yield tensors


# ---- e4m3 shards: the bags of one optimiser step in ONE record, one copy and one decode (csrc/bag_e4m3.hip, "a LIST of bags"; DESIGN.md "e4m3 bags") ----
# File: torch.save({"e4m3_shard": codes as torch.float8_e4m3fn [R, K], "rows": int64 [B], "exp": int32 [B], "label": int64 [B], "site": int64 [B],
# "sex": float32 [B]}) - tensors in a plain dict, so it loads with weights_only=True. Bag b is rows sum(rows[:b]) .. sum(rows[:b + 1]) of the codes, a bag
# of the format above with exponent exp[b]. Per record BagPrefetcher pays a future, three pinned tensors, three copies, a staging allocation, a decode
# launch and an event; a shard pays them once for all its bags.
class E4M3Shard:
    """Many e4m3 bags back to back: ``codes`` uint8 [R, K] (a ``torch.float8_e4m3fn`` tensor is taken as its bytes), ``rows`` and ``exps`` (lists of B
    ints; bag i is the next rows[i] rows, with exponent exps[i]), ``label`` / ``site`` int64 [B], ``sex`` float32 [B]."""
    __slots__ = ("codes", "rows", "exps", "label", "site", "sex")

    def __init__(self, codes: torch.Tensor, rows, exps, label, site, sex):
        if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.uint8, torch.float8_e4m3fn):
            raise ValueError("E4M3Shard: codes must be a torch.uint8 or torch.float8_e4m3fn tensor")
        if codes.dim() != 2:
            raise ValueError(f"E4M3Shard: codes must be [rows, features], got {tuple(codes.shape)}")
        rows = rows.tolist() if isinstance(rows, torch.Tensor) else list(rows)
        exps = exps.tolist() if isinstance(exps, torch.Tensor) else list(exps)
        b = len(rows)
        if len(exps) != b:
            raise ValueError(f"E4M3Shard: {b} row counts and {len(exps)} exponents")
        for i, (r, e) in enumerate(zip(rows, exps)):
            if not isinstance(r, int) or isinstance(r, bool) or r < 0:
                raise ValueError(f"E4M3Shard: bag {i}: rows must be a non-negative int, got {r!r}")
            if not isinstance(e, int) or isinstance(e, bool) or not -7 <= e <= 15:
                raise ValueError(f"E4M3Shard: bag {i}: exp must be an int in -7 .. 15, got {e!r}")
        if sum(rows) != codes.shape[0]:
            raise ValueError(f"E4M3Shard: the bags have {sum(rows)} rows, the codes {codes.shape[0]}")
        meta = []
        for name, v, dt in (("label", label, torch.int64), ("site", site, torch.int64), ("sex", sex, torch.float32)):
            v = torch.as_tensor(v)
            if v.dim() != 1 or v.shape[0] != b:
                raise ValueError(f"E4M3Shard: {name} must have one entry per bag ({b}), got shape {tuple(v.shape)}")
            if (dt is torch.int64) == v.dtype.is_floating_point:
                raise ValueError(f"E4M3Shard: {name} must be {'integers' if dt is torch.int64 else 'floating point'}, got {v.dtype}")
            meta.append(v.to(dtype=dt).contiguous())
        self.codes = codes.contiguous().view(torch.uint8)
        self.rows, self.exps = rows, exps
        self.label, self.site, self.sex = meta

    def __len__(self) -> int:
        return len(self.rows)

    @property
    def offsets(self):
        """B + 1 row offsets: 0 first, the rows of the codes last."""
        offs = [0]
        for r in self.rows:
            offs.append(offs[-1] + r)
        return offs

    def bag(self, i: int) -> E4M3Bag:
        offs = self.offsets
        return E4M3Bag(self.codes[offs[i]:offs[i + 1]], self.exps[i])

    def records(self):
        """The per-bag ``Record`` tuples (E4M3Bag, label, site, sex) BagPrefetcher takes: the same shard fed down the per-record path."""
        return [(self.bag(i), int(self.label[i]), int(self.site[i]), float(self.sex[i])) for i in range(len(self))]


_SHARD_KEYS = ("e4m3_shard", "rows", "exp", "label", "site", "sex")


def _shard_from_dict(d: dict) -> E4M3Shard:
    if any(k not in d for k in _SHARD_KEYS):
        raise ValueError(f"an e4m3 shard is a dict with the keys {', '.join(_SHARD_KEYS)}, got {sorted(map(str, d))}")
    for k, dt in (("rows", torch.int64), ("exp", torch.int32)):
        if not isinstance(d[k], torch.Tensor) or d[k].dtype != dt or d[k].dim() != 1:
            raise ValueError(f"an e4m3 shard's '{k}' is a {dt} [B] tensor")
    for k in ("label", "site", "sex"):
        if not isinstance(d[k], torch.Tensor):
            raise ValueError(f"an e4m3 shard's '{k}' is a [B] tensor")
    return E4M3Shard(d["e4m3_shard"], d["rows"], d["exp"], d["label"], d["site"], d["sex"])


def save_shard_e4m3(path, shard: E4M3Shard) -> E4M3Shard:
    """Write ``shard`` in the file form above."""
    if not isinstance(shard, E4M3Shard):
        raise ValueError("save_shard_e4m3: shard must be an E4M3Shard (quantise_shard makes one)")
    torch.save({"e4m3_shard": shard.codes.cpu().view(torch.float8_e4m3fn), "rows": torch.tensor(shard.rows, dtype=torch.int64),
                "exp": torch.tensor(shard.exps, dtype=torch.int32), "label": shard.label.cpu(), "site": shard.site.cpu(), "sex": shard.sex.cpu()}, path)
    return shard


def quantise_shard(bags, offsets, label, site, sex, exps=None) -> E4M3Shard:
    """The shard of fp32 / fp16 bags, on whatever device they lie (``ops.bags_quantise_e4m3``). ``bags``: ONE [R, K] concatenation with ``offsets`` (B + 1
    row offsets), or a list of [N_b, K] bags (``offsets=None``; they are concatenated here). ``exps=None`` picks each bag's exponent from its largest
    magnitude, with one read-back for the whole shard. The codes stay on the device of the data; label / site / sex are kept on the host."""
    from . import ops
    if isinstance(bags, torch.Tensor):
        if offsets is None:
            raise ValueError("quantise_shard: a concatenation needs its row offsets")
        x = bags
    else:
        bags = list(bags)
        if offsets is not None:
            raise ValueError("quantise_shard: a list of bags brings its own offsets: pass offsets=None")
        if not bags or any(not isinstance(b, torch.Tensor) or b.dim() != 2 or b.shape[1] != bags[0].shape[1] for b in bags):
            raise ValueError("quantise_shard: bags must be a non-empty list of [N, features] tensors of one width")
        offsets = [0]
        for b in bags:
            offsets.append(offsets[-1] + b.shape[0])
        x = torch.cat(bags)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("quantise_shard: the concatenation must be a [R, features] tensor")
    if x.dtype not in (torch.float32, torch.float16):
        x = x.to(torch.float32)
    codes, exps = ops.bags_quantise_e4m3(x.contiguous(), offsets, exps)
    offs = [int(o) for o in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    cpu = lambda v: v.cpu() if isinstance(v, torch.Tensor) else v                         # noqa: E731
    return E4M3Shard(codes, [b - a for a, b in zip(offs, offs[1:])], exps, cpu(label), cpu(site), cpu(sex))


def _load_shard(source) -> E4M3Shard:
    if isinstance(source, (E4M3Shard, dict)):
        s = source
    elif callable(source):
        s = source()
    else:
        s = torch.load(source, map_location="cpu", weights_only=True)
    if isinstance(s, dict):
        s = _shard_from_dict(s)
    if not isinstance(s, E4M3Shard):
        raise ValueError(f"a shard source must give an E4M3Shard or its dict, got {type(s).__name__}")
    return s


class BagBatch:
    """What ShardPrefetcher yields: ``bags`` [R, K] (the decoded concatenation), ``offsets`` (Python list of B + 1 row offsets), ``sex`` float32 [B],
    ``label`` / ``site`` int64 [B], all but the offsets on the device. ``SlideShardedDP.step_batch`` takes it as it is."""
    __slots__ = ("bags", "offsets", "sex", "label", "site")

    def __init__(self, bags, offsets, sex, label, site):
        self.bags, self.offsets, self.sex, self.label, self.site = bags, offsets, sex, label, site

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def slides(self):
        """The ``dp.Slide`` tuples (bag view, sex [1], label [1], site [1]) - NOT BagPrefetcher's order, which is (bag, label, site, sex)."""
        o = self.offsets
        return [(self.bags[o[i]:o[i + 1]], self.sex[i:i + 1], self.label[i:i + 1], self.site[i:i + 1]) for i in range(len(self))]


class ShardPrefetcher:
    """Iterate one ``BagBatch`` per shard, in order, with ``depth`` shards in flight. A source is an ``E4M3Shard``, its dict, a path or a callable. Per
    shard, whatever the number of its bags: the host side (ONE future) pins the codes and two small metadata tensors (label and site as one int64 [2, B],
    sex); the device side, on the copy stream, makes one copy of the codes, two metadata copies, ONE ``ops.bags_dequantise_e4m3`` into a [R, K] tensor of
    ``dtype`` (fp16 or fp32) and one event. The consumer's stream waits on the event, the host does not. ``device="cpu"`` works through the CPU paths."""

    def __init__(self, shards, device: Union[str, torch.device], depth: int = 2, workers: int = 2, dtype: torch.dtype = torch.float16):
        self.shards = list(shards)
        self.device = torch.device(device)
        self.depth = max(1, int(depth))
        self.workers = max(1, int(workers))
        if dtype not in (torch.float16, torch.float32):
            raise ValueError("ShardPrefetcher(dtype=...) must be torch.float16 or torch.float32")
        self.dtype = dtype
        self.on_gpu = self.device.type == "cuda"
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None

    def __len__(self) -> int:
        return len(self.shards)

    # -- stage 1 (worker thread): read + pin
    def _stage_host(self, source):
        s = _load_shard(source)
        codes, meta, sx = s.codes, torch.stack([s.label, s.site]), s.sex
        if self.on_gpu:                                         # page-locked so every copy is truly asynchronous
            codes = codes if codes.is_pinned() else codes.pin_memory()
            meta, sx = meta.pin_memory(), sx if sx.is_pinned() else sx.pin_memory()
        return codes, s.offsets, s.exps, meta, sx

    # -- stage 2 (consumer thread, copy stream): one copy, one decode
    def _stage_device(self, host):
        from . import ops
        codes, offsets, exps, meta, sx = host
        if not self.on_gpu:
            return BagBatch(ops.bags_dequantise_e4m3(codes, offsets, exps, out_dtype=self.dtype), offsets, sx, meta[0], meta[1]), None
        with torch.cuda.stream(self.copy_stream):
            # (the staging tensor of the codes is allocated and dropped under the copy stream, so the allocator's stream ordering covers its reuse)
            bags = ops.bags_dequantise_e4m3(codes.to(self.device, non_blocking=True), offsets, exps, out_dtype=self.dtype)
            meta_d = meta.to(self.device, non_blocking=True)
            sx_d = sx.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return BagBatch(bags, offsets, sx_d, meta_d[0], meta_d[1]), ev

    def __iter__(self) -> Iterator[BagBatch]:
        n = len(self.shards)
        if n == 0:
            return
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            host_futs = {}                                       # index -> future of the pinned host shard
            dev_ready = {}                                       # index -> (batch, event)
            next_host = 0

            def top_up(upto: int):
                nonlocal next_host
                while next_host < min(n, upto):
                    host_futs[next_host] = pool.submit(self._stage_host, self.shards[next_host])
                    next_host += 1

            top_up(self.depth + 1)
            for i in range(n):
                # issue the device copies of everything whose host stage is done, up to `depth` ahead
                for jx in range(i, min(n, i + self.depth)):
                    if jx not in dev_ready and jx in host_futs and (jx == i or host_futs[jx].done()):
                        dev_ready[jx] = self._stage_device(host_futs.pop(jx).result())   # .result() re-raises loader errors
                top_up(i + self.depth + 2)
                batch, ev = dev_ready.pop(i)
                if ev is not None:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(ev)                          # consumer stream waits for the copy, the host does not
                    for t in (batch.bags, batch.sex, batch.label):   # (label and site are rows of one tensor) allocator: do not recycle while in use
                        t.record_stream(cur)
                yield batch
