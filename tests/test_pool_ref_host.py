"""CPU: the float64 statement behind tests/test_gpu_pool_bwd.py (tests/pool_ref.py) - the oracle's pool backward against autograd of the plainly
written forward, the analytic |dP| bound against the reference's own maxima on every family the GPU test holds to the cap, the dropout masks."""
import pytest
import torch

from tests import drop_ref
from tests import pool_ref as R


@pytest.mark.parametrize("d,l,t", [(384, 512, 2), (100, 200, 1)])
@pytest.mark.parametrize("drop", [False, True])
def test_oracle_pool_backward_equals_fp64_autograd(d, l, t, drop):
    """orc.gated_pool_bwd on float64 inputs == torch.autograd of forward_plain, with an external dA and (drop) the two branch masks: 1e-12 of
    each gradient's scale. (tests/test_oracle_golden.py holds the whole-model backward to autograd in fp32 at 2e-5, at the TOAD shape only.)"""
    n = 77
    p, h, wc, bc = R.pool_inputs(n, d, l, t, 5 + d)
    dm, da = R.grad_inputs(n, l, t, 6 + d)
    ma, mb = R.drop_masks(n, d, R.DROP_P, *R.seeds(n, d)) if drop else (None, None)
    dbl = lambda x: None if x is None else x.double()
    leaves = [x.double().requires_grad_(True) for x in (p[:, :d], p[:, d:], h, wc, bc)]
    a_raw, m = R.forward_plain(*leaves, dbl(ma), dbl(mb))
    ((m * dm.double()).sum() + (a_raw * da.double()).sum()).backward()
    ref = R.reference(p, h, wc, bc, dm, da, ma, mb)
    assert ref["dp"].dtype == torch.float64
    assert (ref["a_raw"] - a_raw.detach()).abs().max().item() <= 1e-12 and (ref["m"] - m.detach()).abs().max().item() <= 1e-12
    # (H's gradient: the oracle returns the pooling part softmax(A) dM, which is all of it here - H enters through M only)
    for name, got, leaf in (("dpa", ref["dpa"], leaves[0]), ("dpb", ref["dpb"], leaves[1]), ("dh", ref["dh"], leaves[2]), ("dwc", ref["dwc"], leaves[3]),
                            ("dbc", ref["dbc"], leaves[4])):
        sc = leaf.grad.abs().max().item()
        assert sc > 0 and (got - leaf.grad).abs().max().item() <= 1e-12 * sc, name


def _family_ratios(d, l, t, n, scale=1.0):
    """[(label, bound per block, max |dP| per block)] of the four members (da_ext, dropout) of a family at one size."""
    p, h, wc, bc = R.pool_inputs(n, d, l, t, 1000 + n + d, scale)
    dm, da = R.grad_inputs(n, l, t, n)
    out = []
    for drop in (0.0, R.DROP_P):
        ma, mb = R.drop_masks(n, d, drop, *R.seeds(n, d)) if drop else (None, None)
        for ext in (None, da):
            ref = R.reference(p, h, wc, bc, dm, ext, ma, mb)
            out.append(((n, drop, ext is not None), *R.bound_ratios(ref, wc, drop)))
    return out


@pytest.mark.parametrize("d,l,t", R.EXACT_SHAPES + R.COVER_SHAPES)
def test_bound_holds_and_stays_within_the_cap_in_fp64(d, l, t):
    """The statement's bound is >= the reference's block maximum of |dP| on every input, and on the ordinary families it is within CAP of it in
    every block: the cap tests/test_gpu_pool_bwd.py asserts on the kernel is one the exact arithmetic keeps with room."""
    lo, hi = float("inf"), 0.0
    cases = [(n, 1.0) for n in R.AMAX_NS] + [(513, 4.0)]
    for n, scale in cases:
        for label, bound, mx in _family_ratios(d, l, t, n, scale):
            assert bound.shape == mx.shape == ((n + 255) // 256,)
            assert (bound >= mx).all(), (label, scale)
            nz = mx > 0
            if not nz.any():                    # n == 1 without da_ext: dS is exactly zero (softmax of one score), or round-off of it
                assert n == 1 and not label[2], (label, scale)
                continue
            r = bound[nz] / mx[nz]
            lo, hi = min(lo, r.min().item()), max(hi, r.max().item())
            if (d, l, t) in R.ORDINARY_SHAPES:
                assert r.max().item() <= R.CAP, f"{(d, l, t)} {label} scale {scale}: bound / max |dP| = {r.max().item():.2f} in block {int(r.argmax())}"
    print(f"POOLBWD fp64 ratio {(d, l, t)}: {lo:.2f} .. {hi:.2f}")
    assert lo >= 1.0


def test_fold_and_bound_on_a_hand_made_case():
    """fold256 takes the maximum of |.| per 256 rows (the last block short); row_bound is sum_t |dS| max_e |Wc| times the squared keep scale."""
    v = torch.zeros(600); v[255] = -3.0; v[256] = 2.0; v[599] = 0.5
    assert R.fold256(v).tolist() == [3.0, 2.0, 0.5]
    m = torch.zeros(257, 3); m[0, 2] = -7.0; m[256, 1] = 1.5
    assert R.fold256(m).tolist() == [7.0, 1.5]
    ds = torch.tensor([[1.0, -2.0], [0.0, 0.5]]); wc = torch.tensor([[0.1, -0.4, 0.2], [0.3, 0.0, -0.1]])
    assert torch.allclose(R.row_bound(ds, wc), torch.tensor([0.4 + 0.6, 0.15], dtype=torch.float64), rtol=1e-7)
    assert torch.allclose(R.row_bound(ds, wc, 0.25), torch.tensor([1.0, 0.15], dtype=torch.float64) * 16 / 9, rtol=1e-7)


def test_drop_masks_index_row_times_d_plus_column():
    """The masks come from drop_ref.keep over n * D flat elements, element (row, column) at row * D + column - never from the device."""
    n, d = 9, 100
    sa, sb = R.seeds(n, d)
    assert sa != sb and sa >> 32 and sb >> 32
    ma, mb = R.drop_masks(n, d, R.DROP_P, sa, sb)
    flat = torch.from_numpy(drop_ref.keep(n * d, R.DROP_P, sa).copy())
    assert ma.shape == (n, d) and ma[3, 7].item() == flat[3 * d + 7].item() and torch.equal(ma.reshape(-1), flat)
    assert set(ma.unique().tolist()) == {0.0, float(torch.tensor(1.0) / 0.75)} and not torch.equal(ma, mb)
    either = ((ma == 0) | (mb == 0)).float().mean().item()
    assert 0.3 <= either <= 0.55                                   # 1 - (3/4)^2 = 7/16 expected
    ones = R.drop_masks(n, d, 0.0, sa, sb)
    assert all(torch.equal(k, torch.ones(n, d)) for k in ones)
