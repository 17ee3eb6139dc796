"""What the e4m3 wire format does to the model's outputs on the golden cases, computed on the CPU with the oracle: for every case of
tests/golden/toad_golden.npz the bag is rebuilt (tests/helpers.case_inputs), quantised (ops.bag_quantise_e4m3, exponent chosen from the bag) and decoded,
and the oracle's forward runs on both. Reported: the largest change of the logits, of the softmax attention and of the per-patch raw scores.
MEASURED, not bounded, and the golden bags are synthetic (a closed-form wave, constant rows, Gaussian noise): it says nothing about a trained model's AUC.

usage: e4m3_accuracy.py [--out profiles/bag_e4m3_accuracy.md]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                             # noqa: E402
import torch                                   # noqa: E402

from oracle import toad_oracle as orc          # noqa: E402
from tests.helpers import case_inputs          # noqa: E402
from toad_amd import ops                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    golden = np.load(os.path.join(REPO, "tests", "golden", "toad_golden.npz"), allow_pickle=False)
    names = sorted({k.split("/")[0] for k in golden.files if "/" in k and not k.startswith("api/")}, key=lambda s: (len(s), s))
    rows = ["| case | patches | bag abs-max | exp | max rel. element error | logits: max abs change (scale) | softmax attention: max abs change (max) | raw scores: max abs change (spread) |",
            "|---|---|---|---|---|---|---|---|"]
    for name in names:
        ci = case_inputs(golden, name)
        x = ci["x"]
        if x.shape[0] == 0:
            continue
        codes, exp = ops.bag_quantise_e4m3(x.contiguous())
        xq = ops.bag_dequantise_e4m3(codes, exp, out_dtype=torch.float32)
        with torch.no_grad():
            o0, _ = orc.forward(ci["params"], x, ci["sex"])
            o1, _ = orc.forward(ci["params"], xq, ci["sex"])
        nz = x != 0
        rel = ((xq - x).abs()[nz] / x.abs()[nz]).max().item() if nz.any() else 0.0
        a0, a1 = o0["A"][0], o1["A"][0]
        s0, s1 = torch.softmax(a0, 0), torch.softmax(a1, 0)
        rows.append(f"| {name} | {x.shape[0]} | {x.abs().max().item():.4g} | {exp} | {rel:.3e} | {(o1['logits'] - o0['logits']).abs().max().item():.3e} "
                    f"({o0['logits'].abs().max().item():.3g}) | {(s1 - s0).abs().max().item():.3e} ({s0.max().item():.3g}) | "
                    f"{(a1 - a0).abs().max().item():.3e} ({(a0.max() - a0.min()).item():.3g}) |")
        print(rows[-1], flush=True)
    text = "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
