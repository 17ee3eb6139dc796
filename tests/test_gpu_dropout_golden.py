"""GPU: the drop-in module built with dropout=True (state dict in the reference's attention_net.{0,3,6.*} names) and with size_arg="small"
against tests/golden/toad_dropout_golden.npz, the REFERENCE's outputs and gradients for those configurations
(oracle/pin_against_reference.py DROPOUT_CASES). tests/test_gpu_model.py compares the same configurations with the oracle only; the
train-mode dropout cases of the fixture reach the kernels through the oracle (tests/test_dropout_golden.py pins its ``masks=`` branches to
the reference, test_gpu_model.py holds the kernels to those branches with the device's own masks)."""
import os

import numpy as np
import pytest
import torch

from oracle import toad_oracle as orc
from tests.helpers import (LAYER2_KEYS, MASK_FREE_KEYS, SLOT2KEY, assert_grad_close, case_inputs, check_activations_vs_golden, check_outputs_vs_golden,
                           check_trunk_grads_vs_golden_blocks, grad_scale, relu_flip_positions)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every case of the fixture whose forward is deterministic: dropout=True under eval(), size_arg="small" under train() without dropout
CASES = ["de256", "de10000", "s65", "s777", "sde300"]


@pytest.fixture(scope="module")
def dg():
    return np.load(os.path.join(REPO, "tests", "golden", "toad_dropout_golden.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", CASES)
def test_module_matches_reference_golden_with_dropout_and_small(cuda, dg, name):
    """The call sequence of test_gpu_model.py::test_module_matches_reference_golden, its bounds (1e-4 on outputs, max(2e-5 scale, 10 dev) on
    gradients) and its handling of legitimate ReLU-mask flips, for the configurations the first fixture lacks."""
    from toad_amd import TOAD_fc_mtl_concat, functional as F_
    ci = case_inputs(dg, name)
    assert ci["masks"] is None and ci["train"] == (not ci["dropout"])
    model = TOAD_fc_mtl_concat(size_arg=ci["size_arg"], dropout=ci["dropout"], n_classes=ci["c"])
    state = {orc.dropout_key(k): v for k, v in ci["params"].items()} if ci["dropout"] else ci["params"]
    if ci["dropout"]:
        assert "attention_net.3.weight" in state and "attention_net.6.attention_c.bias" in state and "attention_net.2.weight" not in state
    model.load_state_dict(state, strict=True)
    model.relocate()
    model.train(ci["train"])
    data, sex = ci["x"].to(cuda), ci["sex"].to(cuda)
    label, site = ci["label"].to(cuda), ci["site"].to(cuda)
    res = model(data, sex, return_features=True)
    loss_fn = torch.nn.CrossEntropyLoss()
    loss = loss_fn(res["logits"], label) * 0.75 + loss_fn(res["site_logits"], site) * 0.25
    loss.backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    assert set(dict(model.named_parameters())) == set(state)
    grads = {orc.plain_key(k): p.grad for k, p in model.named_parameters()}
    assert set(grads) == set(orc.PARAM_KEYS)
    d = orc.SIZE_DICT[ci["size_arg"]][2]
    assert grads["attention_net.4.attention_a.0.weight"].shape == (d, 512)
    # as in test_module_matches_reference_golden: where the device's ReLU mask differs legitimately from the exact forward's, the gradients
    # behind that mask are compared with the fp64 backward on the device's own activations instead (same bound)
    w = {s_: ci["params"][k].to(cuda) for s_, k in SLOT2KEY.items()}
    outs, sv = F_.mil_forward(w, data, sex)
    assert torch.equal(outs["logits"], res["logits"].detach())
    pos1, pos2 = relu_flip_positions(ci["params"], ci["x"], sv.h1, sv.h)
    f1, f2 = int(pos1.shape[0]), int(pos2.shape[0])
    assert check_activations_vs_golden(dg, name, sv.h1, sv.h) == (name == "de10000")
    rows = check_trunk_grads_vs_golden_blocks(dg, name, grads, ci["x"], pos1, pos2)
    assert (rows > 0) == (name in ("de10000", "s777", "sde300")), (name, rows)
    n_flips = f1 + f2
    assert n_flips <= 4, (name, f1, f2)              # N(0,1) bags: expected 0.7 flipped mask elements per 10^7 (test_gpu_model.py RANDN_CASES)
    golden_keys = None if n_flips == 0 else (MASK_FREE_KEYS + (LAYER2_KEYS if f2 == 0 else ()))
    check_outputs_vs_golden(dg, name, out, loss.item(), grads, atol=1e-4, grad_keys=golden_keys)
    if n_flips:
        dl, ds = orc.loss_grad(outs["logits"].cpu(), ci["label"], outs["site_logits"].cpu(), ci["site"])
        sv_cpu = orc.Saved(x=ci["x"], h1=sv.h1.cpu(), h=sv.h.cpu(), p=sv.p.cpu(), a_raw=sv.a_raw.cpu(), m=sv.m.cpu(), mcat=sv.mcat.cpu(), sex=ci["sex"])
        s64 = orc.Saved(**{k: (v.double() if (v is not None and v.is_floating_point()) else v) for k, v in sv_cpu.__dict__.items()})
        og = orc.backward({k: v.double() for k, v in ci["params"].items()}, s64, dl.double(), ds.double())
        o32 = orc.backward(ci["params"], sv_cpu, dl, ds)
        for k in orc.PARAM_KEYS:
            if k in golden_keys:
                continue
            noise = (o32[k].double() - og[k]).abs().max().item()
            assert_grad_close(grads[k], og[k], 2e-5, grad_scale(og, k), what=f"{name}:{k} ({f1}+{f2} legit ReLU flips)", floor=10.0 * noise)
    a_only = model(data, sex, attention_only=True)
    assert a_only.shape == (ci["n"],)
    assert torch.equal(a_only, res["A"][0].detach())
