"""CPU: the oracle's dropout and size_arg="small" branches against tests/golden/toad_dropout_golden.npz - the REFERENCE's outputs for
RefModel(dropout=True) in eval and in train mode (with its own nn.Dropout draws, captured by forward hooks) and for size_arg="small",
written by oracle/pin_against_reference.py (DROPOUT_CASES) where the reference is present. No reference is needed here."""
import os

import numpy as np
import pytest
import torch

from oracle import toad_oracle as orc
from tests.helpers import MASK_WIDTHS, case_inputs, check_outputs_vs_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["de256", "de10000", "s65", "s777", "sde300", "dt256", "dt777_c2", "sdt300", "dt1"]
TRAIN_DROPOUT = ("dt256", "dt777_c2", "sdt300", "dt1")


@pytest.fixture(scope="module")
def dg():
    return np.load(os.path.join(REPO, "tests", "golden", "toad_dropout_golden.npz"), allow_pickle=False)


def test_fixture_holds_the_cases_the_pin_script_lists(dg):
    assert sorted({k.split("/")[0] for k in dg.files}) == sorted(CASES)
    flags = {name: tuple(int(v) for v in dg[name + "/meta"][7:10]) for name in CASES}           # (small, dropout, train)
    assert flags == {"de256": (0, 1, 0), "de10000": (0, 1, 0), "s65": (1, 0, 1), "s777": (1, 0, 1), "sde300": (1, 1, 0),
                     "dt256": (0, 1, 1), "dt777_c2": (0, 1, 1), "sdt300": (1, 1, 1), "dt1": (0, 1, 1)}
    for name in CASES:
        assert (name + "/mask_kept/h1" in dg.files) == (name in TRAIN_DROPOUT), name


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_with_dropout_and_small(dg, name):
    """Forward within 2e-5, gradients within check_outputs_vs_golden's bounds: the comparison tests/test_oracle_golden.py makes for the
    first fixture. In the train-mode dropout cases the oracle receives the reference's own masks (``masks=``), so its mask placement, its
    1/0.75 factors in the two ReLU backward steps and the tanh / sigmoid branch terms are held to the reference's autograd."""
    ci = case_inputs(dg, name)
    assert (ci["masks"] is not None) == (ci["dropout"] and ci["train"])
    out, loss, grads = orc.fwd_bwd(ci["params"], ci["x"], ci["sex"], ci["label"], ci["site"], masks=ci["masks"])
    feat, _ = orc.forward(ci["params"], ci["x"], ci["sex"], return_features=True, masks=ci["masks"])
    out = {k: v.detach() for k, v in out.items()}
    out["features"] = feat["features"]
    check_outputs_vs_golden(dg, name, out, loss, grads, atol=2e-5)
    a = orc.forward(ci["params"], ci["x"], ci["sex"], attention_only=True, masks=ci["masks"])
    from tests.helpers import strided_sample
    assert np.abs(strided_sample(a) - dg[name + "/A_only_sample"]).max() <= 2e-5


@pytest.mark.parametrize("name", ["dt256", "dt777_c2", "sdt300"])
def test_captured_masks_look_like_dropout_and_matter(dg, name):
    """The stored masks are nn.Dropout(0.25) draws (a quarter dropped, within 5 sigma of the binomial; the unobservable elements behind a ReLU
    zero are stored as kept, which only lowers the fraction) - and the comparison above depends on them: without the masks, or with the masks
    of the two trunk sites swapped, the oracle misses the reference's logits by far more than the bound."""
    ci = case_inputs(dg, name)
    for k, w in MASK_WIDTHS[ci["size_arg"]]:
        m = ci["masks"][k]
        assert m.shape == (ci["n"], w) and set(m.unique().tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.75))}
        frac, sigma = float((m == 0).float().mean()), (0.25 * 0.75 / m.numel()) ** 0.5
        if k in ("a", "b"):
            assert abs(frac - 0.25) <= 5 * sigma, (k, frac)
        else:
            assert 0.25 * 0.3 <= frac <= 0.25 + 5 * sigma, (k, frac)       # about half of the ReLU outputs are zero and count as kept
    ref = torch.from_numpy(dg[name + "/logits"])
    for wrong in (None, dict(ci["masks"], h1=ci["masks"]["h"], h=ci["masks"]["h1"])):
        out, _ = orc.forward(ci["params"], ci["x"], ci["sex"], masks=wrong)
        assert (out["logits"] - ref).abs().max().item() > 1e-3


def test_dropout_key_names_are_the_reference_state_dict(golden):
    """oracle.dropout_key / plain_key (attention_net.{2,4} <-> attention_net.{3,6}) against the reference's own state-dict listing for
    dropout=True, recorded in toad_golden.npz (api/state_dict rows "classes|dropout|key|shape")."""
    rows = [r.split("|") for r in str(golden["api/state_dict"]).split("\n")]
    for dr, c in ((1, 2), (0, 18)):
        listed = {k: tuple(int(v) for v in shp.split(",")) for cc, d, k, shp in rows if int(d) == dr}
        assert all(int(cc) == c for cc, d, _, _ in rows if int(d) == dr) and len(listed) == 14
        shapes = orc.param_shapes(c)
        mine = {(orc.dropout_key(k) if dr else k): shapes[k] for k in orc.PARAM_KEYS}
        assert mine == listed
        assert [orc.plain_key(k) if dr else k for k in listed] == list(orc.PARAM_KEYS)          # same order, and the way back
    assert [k for k in orc.PARAM_KEYS if orc.dropout_key(k) != k] == [k for k in orc.PARAM_KEYS if k.startswith(("attention_net.2.", "attention_net.4."))]
