"""Convert a directory of the reference's feature bags (<slide_id>.pt, one torch.save'd [N, K] tensor each, as CLAM / TOAD extraction writes them and
datasets/dataset_mtl_concat.py:369-373 reads them) to e4m3 bags: {"e4m3": codes as torch.float8_e4m3fn [N, K], "exp": int} (toad_amd/ingest.py).
Runs on the CPU; the bits are those of the device quantiser. Files that already hold an e4m3 bag are copied through unchanged.

Per file it prints the exponent chosen (ops.e4m3_exponent of the bag's largest magnitude, or --exp), the share of elements that saturated (|x| 2^exp >
448: only with --exp, or for magnitudes above 57344) and the share of non-zero elements that became zero (|x| 2^exp <= 2^-10).

--shard B packs consecutive bags (in the order of their sorted file names) into e4m3 shards of B bags, shard_00000.pt, shard_00001.pt, ... (the last one
may hold fewer): one record for ingest.ShardPrefetcher, which lands and decodes it in one copy and one launch. A shard carries its slides' label, site
and sex, which --meta FILE.csv supplies: a header line and the columns slide_id,label,site,sex, one row per bag (slide_id is the file name without .pt).

usage: bags_to_e4m3.py SRC_DIR DST_DIR [--exp E] [--overwrite] [--shard B --meta FILE.csv]"""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402

from toad_amd import ingest, ops               # noqa: E402


def convert(src: str, dst: str, exp=None):
    """-> (E4M3Bag, saturated share, flushed-to-zero share) of the bag at `src`, written to `dst`."""
    bag = ingest._load(src)
    if isinstance(bag, ingest.E4M3Bag):
        ingest.save_bag_e4m3(dst, bag)
        return bag, 0.0, 0.0
    x = bag if bag.dtype in (torch.float32, torch.float16) else bag.to(torch.float32)
    out = ingest.save_bag_e4m3(dst, x, exp)
    n = max(1, x.numel())
    mag = x.to(torch.float32).abs() * 2.0 ** out.exp
    saturated = int((mag > ops.E4M3_MAX).sum()) / n
    zeroed = int((((out.codes & 0x7F) == 0) & (x != 0)).sum()) / n
    return out, saturated, zeroed


def read_meta(path: str) -> dict:
    """slide_id -> (label, site, sex) from a CSV with the columns slide_id,label,site,sex."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows or any(c not in rows[0] for c in ("slide_id", "label", "site", "sex")):
        sys.exit(f"{path}: expected the columns slide_id,label,site,sex")
    return {r["slide_id"]: (int(r["label"]), int(r["site"]), float(r["sex"])) for r in rows}


def pack_shards(src_dir: str, dst_dir: str, names, per_shard: int, meta: dict, exp=None, overwrite: bool = False):
    """Write the bags `names` of `src_dir` as shards of `per_shard` bags into `dst_dir`; -> the shard paths."""
    missing = [n[:-3] for n in names if n[:-3] not in meta]
    if missing:
        sys.exit(f"no label / site / sex row for {', '.join(missing)}")
    paths = []
    for s, lo in enumerate(range(0, len(names), per_shard)):
        group = names[lo:lo + per_shard]
        dst = os.path.join(dst_dir, f"shard_{s:05d}.pt")
        if os.path.exists(dst) and not overwrite:
            sys.exit(f"{dst} exists (pass --overwrite)")
        bags = []
        for name in group:
            bag = ingest._load(os.path.join(src_dir, name))
            if isinstance(bag, ingest.E4M3Bag):                 # already 8 bits: decoded exactly, so quantising it again at its exponent gives the same codes
                bag = ops.bag_dequantise_e4m3(bag.codes, bag.exp)
            bags.append(bag)
        if len({b.dtype for b in bags}) > 1:
            bags = [b.to(torch.float32) for b in bags]
        label, site, sex = zip(*(meta[n[:-3]] for n in group))
        shard = ingest.quantise_shard(bags, None, torch.tensor(label), torch.tensor(site), torch.tensor(sex, dtype=torch.float32),
                                      None if exp is None else [exp] * len(group))
        ingest.save_shard_e4m3(dst, shard)
        paths.append(dst)
        print(f"{os.path.basename(dst)}: {len(group)} bags, {shard.codes.shape[0]} rows, exps {shard.exps}", flush=True)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--exp", type=int, default=None, help="one exponent for every bag (-7 .. 15) instead of one chosen per bag")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--shard", type=int, default=None, metavar="B", help="pack consecutive bags into shards of B (needs --meta)")
    ap.add_argument("--meta", default=None, metavar="FILE.csv", help="slide_id,label,site,sex for every bag (with --shard)")
    a = ap.parse_args()
    if a.shard is not None and (a.shard < 1 or a.meta is None):
        sys.exit("--shard B needs B >= 1 and --meta FILE.csv")
    if a.shard is None and a.meta is not None:
        sys.exit("--meta goes with --shard")
    os.makedirs(a.dst, exist_ok=True)
    names = sorted(f for f in os.listdir(a.src) if f.endswith(".pt"))
    if not names:
        sys.exit(f"no .pt bags in {a.src}")
    if a.shard is not None:
        paths = pack_shards(a.src, a.dst, names, a.shard, read_meta(a.meta), a.exp, a.overwrite)
        before, after = sum(os.path.getsize(os.path.join(a.src, n)) for n in names), sum(os.path.getsize(p) for p in paths)
        print(f"{len(names)} bags in {len(paths)} shards: {before / 1e6:.1f} MB -> {after / 1e6:.1f} MB")
        return
    before = after = 0
    for name in names:
        src, dst = os.path.join(a.src, name), os.path.join(a.dst, name)
        if os.path.exists(dst) and not a.overwrite:
            sys.exit(f"{dst} exists (pass --overwrite)")
        bag, saturated, zeroed = convert(src, dst, a.exp)
        before += os.path.getsize(src)
        after += os.path.getsize(dst)
        print(f"{name}: {tuple(bag.shape)} exp {bag.exp} saturated {saturated:.3%} became zero {zeroed:.3%}", flush=True)
    print(f"{len(names)} bags: {before / 1e6:.1f} MB -> {after / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
