"""bench_extract.py — BASELINE config 5: tiles -> ResNet-50-trunc extractor -> on-the-fly bag -> attention-MIL step.

    python bench_extract.py --gpus 1 --steps 5 --warmup 2 [--tiles 2048] [--chunk 512]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench_extract.py --gpus N ...

Same contract as bench.py (which stays the headline: the MIL step on resident 100k-patch bags). A "step" here = every
rank extracts one synthetic slide of `--tiles` 256x256 fp32 tiles (resident in HBM, NCHW like the reference feeds its
model) in chunks of `--chunk`, assembles the [tiles,1024] bag on the device, and runs the MIL training step on it
(forward + weighted CE + backward, one gradient all-reduce when N > 1, Adam). value = patches/s over the whole job.

  roofline      the extractor's GEMMs: 8.556 GFLOP per tile (43 convolutions as NHWC GEMMs) over
                the HIP-event time of the extractor calls inside the timed steps, against the fp32-equivalent MFMA
                ceiling of the fp16 two-piece arithmetic every one of them runs since round 3 (dense fp16 peak / 3 = 833.3 TFLOP/s);
  cpu_baseline  the CPU oracle of the extractor (oracle/resnet_oracle.py = the reference's op sequence on torch CPU,
                pinned to the reference) on a bounded sample of tiles on this box's host cores.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch
import torch.distributed as dist

from bench import C, MFMA_EQ_PEAK, SPLIT_TERMS, _physical_cores, claim_stdout, emit, write_outputs

FLOP_PER_TILE = 8_562_671_616          # sum of 2*M*K*N over the 43 convolutions at 256x256 (stem K = 147), SURVEY 8d config 5: 8.56 GFLOP


def cpu_extractor_baseline(n_tiles: int = 8, budget_s: float = 25.0):
    from oracle import resnet_oracle as ro          # reported baseline only
    logical = os.cpu_count() or 1
    phys = min(_physical_cores(), logical)
    sd = ro.make_params(1)
    x = ro.make_tiles(n_tiles, 256, 256, 5)

    def once():
        t0 = time.perf_counter()
        ro.forward(sd, x)
        return time.perf_counter() - t0

    cands = sorted({max(1, phys // 4), max(1, phys // 2), phys}) if phys > 8 else [phys]
    probe, t_start = {}, time.perf_counter()
    for th in cands:
        torch.set_num_threads(th)
        once()
        probe[th] = once()
        if time.perf_counter() - t_start > budget_s * 0.6:
            break
    best = min(probe, key=probe.get)
    torch.set_num_threads(best)
    times = [probe[best]]
    while len(times) < 3 or (time.perf_counter() - t_start < budget_s and len(times) < 7):
        times.append(once())
    times.sort()
    med = times[len(times) // 2]
    return {"value": round(n_tiles / med, 2), "unit": "patches/s", "cores": best, "kind": "port",
            "sample": f"median of {len(times)} x extractor forward of {n_tiles} tiles 3x256x256 (oracle/resnet_oracle.py, torch CPU fp32 "
                      f"conv2d + eval BN, the reference's op sequence; extractor only - it is >99.9 % of the per-patch work), "
                      f"{phys} physical / {logical} logical cores; threads probed {{"
                      + ", ".join(f"{k}: {v * 1e3:.0f} ms" for k, v in probe.items()) + "}"}


TRAFFIC_FILE = "r06_extractor_traffic.json"      # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over one extractor call (tools/gpu_run.sh xtraffic)
EXTRACTOR_KERNEL_SOURCES = ("toad_amd/csrc/conv.hip", "toad_amd/csrc/gemm_f32.hip", "toad_amd/csrc/gemm_h2.inc", "toad_amd/csrc/gemm_h2_epilogue.inc",
                            "toad_amd/csrc/gemm_narrow.inc", "toad_amd/csrc/gemm_stream.inc", "toad_amd/csrc/stem_halo.inc", "toad_amd/csrc/common.h")


def extractor_kernel_sha() -> str:
    """sha256 over the sources the extractor's kernels are compiled from: ties the committed traffic measurement to a kernel build (as bench.py does
    for the pool kernels); a later edit to any of them makes `roofline.traffic` null instead of silently stale."""
    import hashlib
    h = hashlib.sha256()
    for rel in EXTRACTOR_KERNEL_SOURCES:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def extractor_traffic(chunk, n, ext_ms):
    """HBM bytes of ONE extractor call (chunk tiles) from this round's PMC file, or None when the file was measured at another chunk size."""
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", TRAFFIC_FILE)) as f:
            t = json.load(f)
    except OSError:
        return None, "no PMC file for this round"
    if t.get("tiles_per_call") != chunk:
        return None, f"profiles/{TRAFFIC_FILE} was measured at {t.get('tiles_per_call')} tiles per call"
    if t.get("kernel_source_sha256") != extractor_kernel_sha():
        return None, f"profiles/{TRAFFIC_FILE} was measured on other kernel sources (sha mismatch): re-run tools/gpu_run.sh TAG xtraffic"
    per_call = t["hbm_bytes_per_call"]["total_with_fetch_x2"]
    tbs = per_call * (n / chunk) / (ext_ms * 1e-3) / 1e12
    return per_call, (f"HBM bytes per extractor call of {chunk} tiles (profiles/{TRAFFIC_FILE}: FETCH_SIZE x2 + WRITE_SIZE, separate passes); algorithmic "
                      f"{t['algorithmic_bytes_per_call']} B; at this run's extractor time that is {tbs:.2f} TB/s of 8 nominal (5.9 measured for a read/write mix)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", type=int, default=2048, help="tiles (= patches) per slide")
    ap.add_argument("--chunk", type=int, default=512, help="tiles per extractor call")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (bag, loss, params, grad) as DIR/<name>.npy (bench.py's header)")
    args = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    from toad_amd import launch
    launch.maybe_self_launch(__file__, sys.argv[1:], args.gpus)          # started plainly with --gpus N: spawn the N ranks
    claim_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start one process per GPU (or run this script plainly)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        launch.init_process_group("nccl", device=dev)

    from toad_amd import TOAD_fc_mtl_concat
    from toad_amd.dp import SlideShardedDP
    from toad_amd.resnet_custom import resnet50_baseline

    torch.manual_seed(1)
    ext = resnet50_baseline().relocate().eval()               # random init: pretrained weights need the network (also in the reference)
    mil = TOAD_fc_mtl_concat(dropout=False, n_classes=C)
    mil.relocate(); mil.train()
    dp = SlideShardedDP(mil, {"lr": 1e-4, "weight_decay": 1e-5})
    n, chunk = args.tiles, args.chunk
    g = torch.Generator(device=dev).manual_seed(4000 + rank)
    tiles = torch.randn(n, 3, 256, 256, device=dev, generator=g)      # normalised RGB tiles, resident in HBM
    meta = (torch.tensor([float(rank % 2)], device=dev), torch.tensor([rank % C], device=dev), torch.tensor([rank % 2], device=dev))
    bag = torch.empty(n, 1024, device=dev)
    ev = []

    def step(timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            for i in range(0, n, chunk):
                bag[i:i + chunk] = ext(tiles[i:i + chunk])
        e1.record()
        if timed:
            ev.append((e0, e1))
        return dp.step([(bag,) + meta], world)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(False)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses = step(True)
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, {"bag": bag, "loss": torch.stack([lv.reshape(-1) for lv in losses]), "params": dp.flat, "grad": dp.flat_grad})
    ext_ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        tf = FLOP_PER_TILE * n / (ext_ms * 1e-3)
        traffic, traffic_what = extractor_traffic(chunk, n, ext_ms)
        out = {"metric": "patches/sec end-to-end: 256x256 tiles -> ResNet50-trunc -> bag -> attention-MIL step", "value": round(n * world * args.steps / elapsed, 1),
               "unit": "patches/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 (storage + accumulation; GEMM operands as 2 x f16 pieces, 3 MFMA terms)", "data": "synthetic",
               "config": {"workload": f"{n} N(0,1) tiles 3x256x256 per GPU per step (resident in HBM) -> resnet50_baseline (random init, eval-BN folded) "
                                      f"in chunks of {chunk} -> bag [{n},1024] -> TOAD_fc_mtl_concat(big, 18 classes) fwd + CE + bwd + Adam",
                          "arithmetic": "fp32 storage/accumulation; conv-as-GEMM operands as two fp16 pieces (3 MFMA terms, one tensor-wide power-of-two "
                                        "scale per activation from producer-emitted abs-max scalars, per-row scales for the weights) = fp32-equivalent",
                          "parallelism": f"slide-sharded dp{world}"},
               "roofline": {"bound": "mfma", "kernel": "43 conv-as-GEMM launches per chunk: stem_halo_pool_kernel (stem + max-pool from the NCHW tiles, window in LDS) + conv3x3_h2_halo_kernel<2|4> (stride-1 3x3, activation halo in LDS) + gemm_nt_h2_stream_kernel<2,2|2,4> (Cout <= 128, short-K residual GEMMs, strided 3x3: A streamed through registers) + gemm_nt_h2_big_kernel (Cout >= 256); + strided gathers, average pool",
                            "achieved": round(tf / 1e12, 2), "peak": round(MFMA_EQ_PEAK / 1e12, 1), "unit": "TFLOP/s fp32-equivalent",
                            "frac": round(tf / MFMA_EQ_PEAK, 4), "traffic": traffic, "traffic_what": traffic_what,
                            "fp16_mfma_tflops_issued": round(tf * SPLIT_TERMS / 1e12, 1),
                            "algorithmic_flops": FLOP_PER_TILE * n, "extractor_ms_per_step": round(ext_ms, 3),
                            "extractor_share_of_step": round(ext_ms / ms, 4)},
               "last_loss": round(float(losses[-1][0].item()) * world, 5)}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_extractor_baseline()
            out["speedup_vs_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(out)


if __name__ == "__main__":
    main()
