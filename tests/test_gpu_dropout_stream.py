"""GPU: the dropout masks of the device against their host statement (tests/drop_ref.py): the exported stream bit for bit, and the
placement of that stream in the fused forward. Every other dropout test takes its masks from toad_dropout_mask_f32, the hash the fused
kernels use; a change to the hash, the threshold or the seed handling moves both and passes there. tests/test_dropout_stream_host.py
holds the host statement to the statistics dropout needs."""
import numpy as np
import pytest
import torch

from oracle import toad_oracle as orc
from tests import drop_ref
from tests.helpers import SLOT2KEY

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4097, 300 * 512, 5000 * 384)
_DRAWN = 0x2F3C59A1B6D7E845 & (2 ** 62 - 1)                        # "one drawn seed" of the module (it draws from [0, 2^62))
_SA = drop_ref.drop_seeds(_DRAWN)[2]
SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 64 - 1) + drop_ref.drop_seeds(_DRAWN) \
    + tuple((_SA + 2 * b * drop_ref.GOLDEN) & drop_ref.M64 for b in (1, 2))      # slides 1, 2 of a batch


@pytest.mark.parametrize("p", [0.25, 0.5, 0.1])
def test_exported_stream_equals_the_host_statement(cuda, p):
    """ops.dropout_mask(n, p, seed) == drop_ref.keep(n, p, seed), exactly: lengths around the wave and block sizes and the two bag shapes
    of the model tests; p = 0.1 has no exact fp32 value (the threshold is taken from the rounded float); seeds with an empty or full high
    word, the four site seeds of a forward and the branch seeds of the next two slides of a batch (which wrap modulo 2^64)."""
    from toad_amd import functional as F_, ops
    assert F_.drop_seeds(_DRAWN) == drop_ref.drop_seeds(_DRAWN) and F_._GOLDEN == drop_ref.GOLDEN and F_.DROP_P == 0.25
    for seed in SEEDS:
        dev = ops.dropout_mask(SIZES[-1], p, seed, cuda).cpu().numpy()
        ref = drop_ref.keep(SIZES[-1], p, seed)
        for n in SIZES:                                             # element e of the stream does not depend on the length asked for ...
            got = dev[:n] if n == SIZES[-1] else ops.dropout_mask(n, p, seed, cuda).cpu().numpy()      # ... which every shorter call shows
            assert got.dtype == np.float32 and got.shape == (n,)
            bad = np.flatnonzero(got != ref[:n])
            assert bad.size == 0, (p, hex(seed), n, bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())


_PARAMS = {}


def _weights(cuda):
    if not _PARAMS:
        _PARAMS["cpu"] = orc.random_params(18, 2000)
        _PARAMS["dev"] = {s: _PARAMS["cpu"][k].to(cuda) for s, k in SLOT2KEY.items()}
    return _PARAMS["cpu"], _PARAMS["dev"]


@pytest.mark.parametrize("n", [1, 257, 777, 3000, 9000])
def test_fused_forward_places_the_stream_where_the_host_statement_says(cuda, n):
    """F_.mil_forward with dropout: whole tiles, K-split remainder tiles with their fix-up, and the half-height plan of 2.6k ... 16k rows.
    Element (row, column) of a site draws index row * width + column of its stream (drop_ref.drop_seeds): what the twin drops is exactly 0
    in H1 / H; what it keeps is 4/3 x the same layer without dropout on the same input, within the per-op GEMM bound of
    test_gpu_kernels.py (1e-5 of the output's scale); the raw scores equal ((tanh(Pa) ma) (sigmoid(Pb) mb)) Wc^T + bc in fp64 from the
    saved pre-activations with the twin's branch masks, within 1e-4 absolute as in test_train_mode_dropout_matches_oracle_with_the_same_masks."""
    from toad_amd import functional as F_, ops
    params, w = _weights(cuda)
    x = orc.random_bag(n, 1000 + n).to(cuda)
    sex = torch.ones(1, device=cuda)
    seed = (_DRAWN + n) & (2 ** 62 - 1)
    s1, s2, sa, sb = drop_ref.drop_seeds(seed)
    _, sv = F_.mil_forward(w, x, sex, F_.DROP_P, seed)
    for name, got, inp, wk, bk, sd in (("h1", sv.h1, x, "w1", "b1", s1), ("h", sv.h, sv.h1, "w2", "b2", s2)):
        k = torch.from_numpy(drop_ref.keep(n * 512, 0.25, sd).reshape(n, 512))
        plain = ops.linear_act_fwd(inp, w[wk], w[bk], ops.ACT_RELU).cpu()
        got = got.cpu()
        assert got.shape == (n, 512)
        assert 0.15 < float((k == 0).float().mean()) < 0.35                   # the twin drops a quarter (n = 1: 512 draws)
        assert int((got[k == 0] != 0).sum()) == 0, (name, n)
        want = plain * k                                                      # k: 0 or float32(4/3)
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 1e-5 * scale, (name, n, err, scale)
        # and the comparison is not vacuous: the kept elements are not all ReLU zeros
        assert int((got[k != 0] != 0).sum()) > 0.2 * int((k != 0).sum()), (name, n)
    d = 384
    ma = torch.from_numpy(drop_ref.keep(n * d, 0.25, sa).reshape(n, d)).double()
    mb = torch.from_numpy(drop_ref.keep(n * d, 0.25, sb).reshape(n, d)).double()
    p = sv.p.cpu().double()
    a_ref = (torch.tanh(p[:, :d]) * ma * (torch.sigmoid(p[:, d:]) * mb)) @ params["attention_net.4.attention_c.weight"].double().t() \
        + params["attention_net.4.attention_c.bias"].double()
    assert sv.a_raw.shape == (n, 2)
    err = float((sv.a_raw.cpu().double() - a_ref).abs().max())
    assert err <= 1e-4, (n, err)
    # the scores depend on the masks by far more than the bound: the branch streams of the NEXT slide of a batch (seeds + 2 GOLDEN) give other
    # scores. (Exchanging ma and mb would show nothing: the gate is the product of all four factors.)
    step = 2 * drop_ref.GOLDEN
    ma2 = torch.from_numpy(drop_ref.keep(n * d, 0.25, (sa + step) & drop_ref.M64).reshape(n, d)).double()
    mb2 = torch.from_numpy(drop_ref.keep(n * d, 0.25, (sb + step) & drop_ref.M64).reshape(n, d)).double()
    a_other = (torch.tanh(p[:, :d]) * ma2 * (torch.sigmoid(p[:, d:]) * mb2)) @ params["attention_net.4.attention_c.weight"].double().t() \
        + params["attention_net.4.attention_c.bias"].double()
    assert float((a_other - a_ref).abs().max()) > 1e-2
