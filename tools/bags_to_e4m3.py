"""Convert a directory of the reference's feature bags (<slide_id>.pt, one torch.save'd [N, K] tensor each, as CLAM / TOAD extraction writes them and
datasets/dataset_mtl_concat.py:369-373 reads them) to e4m3 bags: {"e4m3": codes as torch.float8_e4m3fn [N, K], "exp": int} (toad_amd/ingest.py).
Runs on the CPU; the bits are those of the device quantiser. Files that already hold an e4m3 bag are copied through unchanged.

Per file it prints the exponent chosen (ops.e4m3_exponent of the bag's largest magnitude, or --exp), the share of elements that saturated (|x| 2^exp >
448: only with --exp, or for magnitudes above 57344) and the share of non-zero elements that became zero (|x| 2^exp <= 2^-10).

usage: bags_to_e4m3.py SRC_DIR DST_DIR [--exp E] [--overwrite]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--exp", type=int, default=None, help="one exponent for every bag (-7 .. 15) instead of one chosen per bag")
    ap.add_argument("--overwrite", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dst, exist_ok=True)
    names = sorted(f for f in os.listdir(a.src) if f.endswith(".pt"))
    if not names:
        sys.exit(f"no .pt bags in {a.src}")
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
