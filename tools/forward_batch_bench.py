"""Throughput of TOAD_fc_mtl_concat.forward_batch (toad_mil_multi_fwd_f32 / toad_mil_multi_bwd_f32) against the routes it sits between.

  train: 52 x 10k-patch bags per optimiser step (bench.py --config 3's shape), three arms:
         batch   - forward_batch + torch cross_entropy (0.75 / 0.25, mean over the batch) + loss.backward() + torch.optim.Adam
         fused   - ops.mil_multi_step + FlatAdam (what --config 3 times: the loss is fixed inside the kernel)
         drop_in - the reference's loop body per slide: model(data, sex), two CrossEntropyLoss, backward, torch.optim.Adam, one step per slide
  eval:  128..4096-patch bags, forward only: forward_batch under no_grad vs forward_many (toad_amd.eval.forward_grouped), both grouped at
         131,072 rows.
  launches: one forward_batch + backward at B slides (for a rocprofv3 --kernel-trace --stats run: `--launches B`).

Each arm: warm-up, then device-synchronised wall time over at least --seconds (default 2) of whole iterations. Prints one JSON line per arm.
usage: forward_batch_bench.py [--train] [--eval] [--launches B] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

from toad_amd import TOAD_fc_mtl_concat, ops   # noqa: E402
from toad_amd.optim import FlatAdam            # noqa: E402

C = 18


def timed(fn, slides_per_iter, seconds, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    it, t0 = 0, time.perf_counter()
    while True:
        fn()
        it += 1
        torch.cuda.synchronize()                 # (an iteration is tens of ms: the check costs nothing measurable)
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    return dict(iters=it, seconds=round(dt, 3), slides_per_s=round(it * slides_per_iter / dt, 1), ms_per_iter=round(1e3 * dt / it, 3))


def make_model():
    torch.manual_seed(0)
    m = TOAD_fc_mtl_concat(n_classes=C)
    m.relocate()
    m.train()
    return m


def train_arms(seconds, B=52, n=10000):
    dev = torch.device("cuda:0")
    pool = torch.randn(B * n, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    bags = [pool[i * n:(i + 1) * n] for i in range(B)]            # landed back to back, as the ingest lands them (no concatenation copy)
    sex = (torch.arange(B, device=dev) % 2).float()
    label = torch.arange(B, device=dev) % C
    site = (torch.arange(B, device=dev) // 2) % 2
    res = {}

    model = make_model()
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5)

    def batch():
        outs = model.forward_batch(bags, sex)
        logits = torch.cat([o["logits"] for o in outs])
        slog = torch.cat([o["site_logits"] for o in outs])
        loss = 0.75 * F.cross_entropy(logits, label) + 0.25 * F.cross_entropy(slog, site)
        opt.zero_grad()
        loss.backward()
        opt.step()
    res["batch"] = timed(batch, B, seconds)

    model = make_model()
    w = model._weights()
    flat = model.flat_parameters()
    fgrad = torch.zeros_like(flat)
    offs, total = model.flat_offsets()
    g = {}
    for k, (o, num) in offs.items():
        g[k] = fgrad[o:o + num].view_as(w[k])
    d = w["wa"].shape[0]
    g["wab"] = fgrad[offs["wa"][0]:offs["wa"][0] + 2 * d * w["wa"].shape[1]].view(2 * d, -1)
    g["bab"] = fgrad[offs["ba"][0]:offs["ba"][0] + 2 * d]
    fopt = FlatAdam(flat, lr=2e-4, weight_decay=1e-5)
    wd = {k: v.detach() for k, v in w.items()}

    def fused():
        ops.mil_multi_step(wd, g, 0.0, bags, sex, label, site, 0.75 / B, 0.25 / B)
        fopt.step(fgrad)
    res["fused"] = timed(fused, B, seconds)

    model = make_model()
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5)
    ce = torch.nn.CrossEntropyLoss()
    sexes = [sex[i:i + 1] for i in range(B)]
    labels = [label[i:i + 1] for i in range(B)]
    sites = [site[i:i + 1] for i in range(B)]

    def drop_in():
        for i in range(B):
            out = model(bags[i], sexes[i])
            loss = ce(out["logits"], labels[i]) * 0.75 + ce(out["site_logits"], sites[i]) * 0.25
            loss.backward()
            opt.step()
            opt.zero_grad()
    res["drop_in"] = timed(drop_in, B, seconds, warmup=1)
    for k, v in res.items():
        v.update(arm=k, workload=f"train {B} x {n} patches per step")
    res["batch"]["vs_fused"] = round(res["batch"]["slides_per_s"] / res["fused"]["slides_per_s"], 3)
    res["batch"]["vs_drop_in"] = round(res["batch"]["slides_per_s"] / res["drop_in"]["slides_per_s"], 2)
    return res


def eval_arms(seconds, ns=512, lo=128, hi=4096, group_rows=131072):
    from toad_amd.eval import forward_grouped
    dev = torch.device("cuda:0")
    model = make_model()
    model.eval()
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(lo, hi + 1, (ns,), generator=g).tolist()
    slides = [(torch.randn(n, 1024, device=dev), torch.tensor([1], device=dev), torch.tensor([0], device=dev), torch.tensor([1.0], device=dev)) for n in lens]
    groups, cur, rows = [], [], 0
    for s in slides:
        if cur and rows + s[0].shape[0] > group_rows:
            groups.append(cur); cur, rows = [], 0
        cur.append(s); rows += s[0].shape[0]
    groups.append(cur)

    def batch():
        with torch.no_grad():
            for grp in groups:
                model.forward_batch([s[0] for s in grp], [s[3] for s in grp])

    def many():
        with torch.no_grad():
            for _ in forward_grouped(model, slides, group_rows):
                pass
    res = {"eval_forward_batch": timed(batch, ns, seconds), "eval_forward_many": timed(many, ns, seconds)}
    for k, v in res.items():
        v.update(arm=k, workload=f"eval {ns} slides of {lo}..{hi} patches, groups of <= {group_rows} rows")
    res["eval_forward_batch"]["vs_forward_many"] = round(res["eval_forward_batch"]["slides_per_s"] / res["eval_forward_many"]["slides_per_s"], 3)
    return res


def launches(B, n=1000):
    """One forward_batch + backward at B slides after a warm-up (run under rocprofv3 --kernel-trace --stats)."""
    dev = torch.device("cuda:0")
    model = make_model()
    bags = [torch.randn(n, 1024, device=dev) for _ in range(B)]
    sex = (torch.arange(B, device=dev) % 2).float()
    label = torch.arange(B, device=dev) % C
    for _ in range(2):
        outs = model.forward_batch(bags, sex)
        loss = sum(F.cross_entropy(o["logits"], label[i:i + 1]) for i, o in enumerate(outs))
        loss.backward()
    torch.cuda.synchronize()
    print(json.dumps(dict(arm="launches", B=B, patches=n, calls=2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.launches:
        launches(a.launches)
        return
    res = {}
    if a.train or not a.eval:
        res.update(train_arms(a.seconds))
    if a.eval or not a.train:
        res.update(eval_arms(a.seconds))
    lines = [json.dumps(v) for v in res.values()]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
