"""GPU: the weight-gradient (TN) GEMMs under every row-split plan and launch. tests/wgrad_ref.py holds the shapes (by the regime of the host plan
each one reaches), the operand families and the arithmetic; tests/test_wgrad_plans_host.py shows on the CPU that every listed shape is in its
regime, that the families meet their preconditions and that the emulated arithmetic is exact on the integer families. Here the kernels run:

  * integer families (small_int, two_piece_int): dW and db must EQUAL the int64 reference, through ops.linear_wgrad (fp32 X and prepared bag:
    gemm_tn_h2_big_kernel<false>, gemm_tn_pt_kernel) and through ops.linear_wgrad_batch (gemm_tn_h2_batch_kernel<false> and <true>);
  * real-valued families (randn, decades, late_giant): every element inside the derived bound of wgrad_ref (the ratios are printed);
  * the whole-slide route (ops.mil_bwd) against the per-op one (functional.mil_backward) at the batched launch's row limits.
Every call runs twice and must repeat bitwise, on a workspace filled with NaN bit patterns, and the library's fallback-launch count must not move."""
import numpy as np
import pytest
import torch

from tests import wgrad_ref as R
from tests.helpers import assert_step_grad_matches_per_op

pytestmark = pytest.mark.gpu

VARIANTS = [(want_db, given, beta) for want_db in (True, False) for given in (True, False) for beta in (0.0, 1.0)]


@pytest.fixture(autouse=True)
def no_fallback_launch(cuda):
    from toad_amd import _lib
    lib = _lib.load()
    before = lib.toad_fallback_launches()
    yield
    torch.cuda.synchronize()
    assert lib.toad_fallback_launches() == before, "a weight gradient fell back to the exact-fp32 kernels"


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def _poisoned_ws(nbytes, cuda):
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=cuda)


def _per_op_twice(ops, lib, cuda, dy, x, dy_amax, x_amax, want_db, beta, base):
    """ops.linear_wgrad twice, each on a NaN-filled workspace and a fresh destination (NaN for beta = 0: it must not be read) -> (dW, db)."""
    m, n = dy.shape
    k = x.shape[1]
    outs = []
    for _ in range(2):
        ops._ws(lib.toad_linear_wgrad_ws_bytes(m, n, k), cuda, "wgrad").fill_(0xFF)
        dw = base[0].clone() if beta else _nan((n, k), cuda)
        db = None if not want_db else (base[1].clone() if beta else _nan((n,), cuda))
        outs.append(ops.linear_wgrad(dy, x, dw, db, beta, want_db, dy_amax, x_amax))
    assert torch.equal(outs[0][0], outs[1][0]) and (not want_db or torch.equal(outs[0][1], outs[1][1])), "not reproducible run to run"
    assert want_db or outs[0][1] is None
    return outs[0]


@pytest.mark.parametrize("regime,m,n,k", R.PER_OP_CASES)
def test_per_op_integer_products_equal_int64(cuda, regime, m, n, k):
    from toad_amd import _lib, ops
    lib = _lib.load()
    base_np = R.int_base(n, k, 5)
    base = (_dev(base_np[0], cuda), _dev(base_np[1], cuda))
    for family in R.INT_FAMILIES:
        dy_np, x_np = R.int_operands(family, m, n, k, R.PER_OP_SEED + m)
        dw_ref, db_ref = R.ref_int64(dy_np, x_np)
        ref = {0.0: (_dev(dw_ref.astype(np.float32), cuda), _dev(db_ref.astype(np.float32), cuda)),
               1.0: (_dev((dw_ref + base_np[0].astype(np.int64)).astype(np.float32), cuda), _dev((db_ref + base_np[1].astype(np.int64)).astype(np.float32), cuda))}
        dy, x = _dev(dy_np, cuda), _dev(x_np, cuda)
        amax = (_dev(R.amax_rows256(dy_np), cuda), _dev(R.amax_rows256(x_np), cuda))
        kinds = [("fp32", x)] + ([("prepared", ops.prepare_bag(x))] if k % 8 == 0 else [])      # (a prepared bag has K % 8 == 0)
        for kind, xk in kinds:
            if kind == "prepared":
                assert torch.equal(xk.amax, amax[1])
            for want_db, given, beta in VARIANTS:
                dw, db = _per_op_twice(ops, lib, cuda, dy, xk, amax[0] if given else None, amax[1] if given and kind == "fp32" else None, want_db, beta, base)
                what = (regime, m, n, k, family, kind, want_db, given, beta)
                assert torch.equal(dw, ref[beta][0]), what + ("dW", int((dw != ref[beta][0]).sum()))
                assert not want_db or torch.equal(db, ref[beta][1]), what + ("db",)


def _batch_operands(cuda, family, m, jobs, x16=False):
    """[(dy, x, dy_amax, x_amax)] on the device (the last x as halves with x16), their numpy operands and int64 references."""
    dev, host, refs = [], [], []
    for i, (n, k) in enumerate(jobs):
        half = x16 and i == len(jobs) - 1
        dy_np, x_np = R.int_operands(family, m, n, k, R.BATCH_SEED + m + i, 11 if half else 20)
        host.append((dy_np, x_np))
        refs.append(R.ref_int64(dy_np, x_np))
        x = _dev(x_np, cuda)
        dev.append((_dev(dy_np, cuda), x.half() if half else x, _dev(R.amax_rows256(dy_np), cuda), None if half else _dev(R.amax_rows256(x_np), cuda)))
    return dev, host, refs


def _batch_twice(ops, cuda, dev_jobs, want_db, beta, bases, ws_bytes=None):
    m = dev_jobs[0][0].shape[0]
    shapes = [(j[0].shape[1], j[1].shape[1]) for j in dev_jobs]
    nbytes = ops.linear_wgrad_batch_ws_bytes(m, shapes) if ws_bytes is None else ws_bytes
    runs = []
    for _ in range(2):
        outs = [(bases[i][0].clone() if beta else _nan(s, cuda), None if not want_db else (bases[i][1].clone() if beta else _nan((s[0],), cuda)))
                for i, s in enumerate(shapes)]
        runs.append(ops.linear_wgrad_batch(dev_jobs, outs, beta, want_db, ws=[_poisoned_ws(nbytes, cuda) for _ in shapes]))
    for (dw0, db0), (dw1, db1) in zip(*runs):
        assert torch.equal(dw0, dw1) and (not want_db or torch.equal(db0, db1)), "not reproducible run to run"
    return runs[0]


def _check_batch(cuda, outs, refs, bases_np, beta, want_db, what):
    for i, ((dw, db), (dw_ref, db_ref)) in enumerate(zip(outs, refs)):
        if beta:
            dw_ref, db_ref = dw_ref + bases_np[i][0].astype(np.int64), db_ref + bases_np[i][1].astype(np.int64)
        assert torch.equal(dw, _dev(dw_ref.astype(np.float32), cuda)), what + (i, "dW")
        assert not want_db or torch.equal(db, _dev(db_ref.astype(np.float32), cuda)), what + (i, "db")


@pytest.mark.parametrize("regime,m,jobs", R.BATCH_CASES)
def test_batched_integer_products_equal_int64(cuda, regime, m, jobs):
    from toad_amd import ops
    bases_np = [R.int_base(n, k, 7 + i) for i, (n, k) in enumerate(jobs)]
    bases = [(_dev(b[0], cuda), _dev(b[1], cuda)) for b in bases_np]
    for family in R.INT_FAMILIES:
        dev_jobs, _, refs = _batch_operands(cuda, family, m, jobs)
        for want_db in (True, False):
            for beta in (0.0, 1.0):
                outs = _batch_twice(ops, cuda, dev_jobs, want_db, beta, bases)
                _check_batch(cuda, outs, refs, bases_np, beta, want_db, (regime, m, family, want_db, beta))


@pytest.mark.parametrize("regime,m,jobs", R.BATCH_X16_CASES)
def test_batched_fp16_bag_products_equal_int64_and_the_fp32_launch(cuda, regime, m, jobs):
    """The third job on an fp16 X: all three products equal int64, and products 0 and 1 are bitwise those of the fp32 launch of the same jobs."""
    from toad_amd import ops
    bases_np = [R.int_base(n, k, 7 + i) for i, (n, k) in enumerate(jobs)]
    bases = [(_dev(b[0], cuda), _dev(b[1], cuda)) for b in bases_np]
    for family in R.INT_FAMILIES:
        dev16, host, refs = _batch_operands(cuda, family, m, jobs, x16=True)
        assert dev16[2][1].dtype == torch.float16 and np.array_equal(dev16[2][1].float().cpu().numpy(), host[2][1])
        dev32 = dev16[:2] + [(dev16[2][0], dev16[2][1].float(), dev16[2][2], _dev(R.amax_rows256(host[2][1]), cuda))]
        for beta in (0.0, 1.0):
            o16 = _batch_twice(ops, cuda, dev16, True, beta, bases)
            o32 = _batch_twice(ops, cuda, dev32, True, beta, bases)
            _check_batch(cuda, o16, refs, bases_np, beta, True, (regime, m, family, "x16", beta))
            _check_batch(cuda, o32, refs, bases_np, beta, True, (regime, m, family, "fp32", beta))
            for i in (0, 1):
                assert torch.equal(o16[i][0], o32[i][0]) and torch.equal(o16[i][1], o32[i][1]), (family, i)


def test_batched_entry_takes_exactly_the_restated_need(cuda):
    """wgrad_batch_ok's `need`, restated in wgrad_ref: that many bytes per job are accepted (and the result is exact), one float less is refused."""
    from toad_amd import ops
    _, m, jobs = R.BATCH_CASES[-1]
    need = max(R.batch_need_bytes(m, jobs, i) for i in range(len(jobs)))
    dev_jobs, _, refs = _batch_operands(cuda, "small_int", m, jobs)
    outs = _batch_twice(ops, cuda, dev_jobs, True, 0.0, None, ws_bytes=need)
    _check_batch(cuda, outs, refs, None, 0.0, True, ("need", m))
    with pytest.raises(RuntimeError, match=r"rc=-2"):
        _batch_twice(ops, cuda, dev_jobs, True, 0.0, None, ws_bytes=need - 4)


@pytest.mark.parametrize("regime,m,jobs", R.BATCH_REFUSED)
def test_batched_entry_refuses_and_writes_nothing(cuda, regime, m, jobs):
    from toad_amd import ops
    g = torch.Generator(device=cuda).manual_seed(m)
    dev_jobs, outs, wss = [], [], []
    for n, k in jobs:
        dy = torch.randn(m, n, device=cuda, generator=g); x = torch.randn(m, k, device=cuda, generator=g)
        dev_jobs.append((dy, x, ops.absmax_rows256(dy), ops.absmax_rows256(x)))
        outs.append((torch.full((n, k), 7.0, device=cuda), torch.full((n,), 7.0, device=cuda)))
        wss.append(_poisoned_ws(1 << 20, cuda))
    with pytest.raises(RuntimeError, match=r"rc=-2"):
        ops.linear_wgrad_batch(dev_jobs, outs, 0.0, True, ws=wss)
    torch.cuda.synchronize()
    for (dw, db), ws in zip(outs, wss):
        assert bool((dw == 7.0).all()) and bool((db == 7.0).all()) and bool((ws == 0xFF).all()), regime


def _ratio(got, ref, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("m", R.REAL_MS)
@pytest.mark.parametrize("family", R.REAL_FAMILIES)
def test_real_valued_products_stay_inside_the_derived_bound(cuda, family, m):
    """Every element of dW within c1 sum_r |dy x| + c2 M amax amax and of db within its summation bound (wgrad_ref's docstring derives both), per-op
    on fp32 X and on the prepared bag, and batched. The largest err / bound per route is printed (profiles/wgrad_plan_bound.md keeps them)."""
    from toad_amd import _lib, ops
    lib = _lib.load()
    host = [R.real_family(family, m, n, k, R.REAL_SEED + m + i) for i, (n, k) in enumerate(R.REAL_JOBS)]
    dev_jobs = [(_dev(dy, cuda), _dev(x, cuda), _dev(R.amax_rows256(dy), cuda), _dev(R.amax_rows256(x), cuda)) for dy, x in host]
    refs = [R.ref_f64(dy, x) for dy, x in host]
    ratios = {}
    # per-op, on the operands of job 0: abs-max arrays measured inside (fp32 X) / made by prepare_bag
    (dy_np, x_np), (dy, x, _, _), (rw, rb) = host[0], dev_jobs[0], refs[0]
    p = R.tn_plan(m, *R.REAL_PER_OP)
    bw, bb = R.tn_bound(dy_np, x_np, p.rows_per_split, p.nsplit), R.db_bound(dy_np, p.rows_per_split, p.nsplit)
    for route, xk in (("per-op fp32", x), ("per-op prepared", ops.prepare_bag(x))):
        dw, db = _per_op_twice(ops, lib, cuda, dy, xk, None, None, True, 0.0, None)
        ratios[route] = (_ratio(dw, rw, bw), _ratio(db, rb, bb))
    bp = R.tn_batch_plan(m, R.REAL_JOBS)
    outs = _batch_twice(ops, cuda, dev_jobs, True, 0.0, None)
    for i, ((dw, db), (dy_np, x_np), (rw, rb)) in enumerate(zip(outs, host, refs)):
        ratios[f"batched job {i}"] = (_ratio(dw, rw, R.tn_bound(dy_np, x_np, bp.rows_per_split, bp.nsplit)),
                                      _ratio(db, rb, R.db_bound(dy_np, bp.rows_per_split, bp.nsplit)))
    for route, (a, b) in ratios.items():
        print(f"wgrad bound (MI355X) {family} M={m} {route}: dW err/bound {a:.3e}, db err/bound {b:.3e}")
    for route, (a, b) in ratios.items():
        assert a <= 1.0 and b <= 1.0, (family, m, route, a, b)


@pytest.mark.parametrize("n", R.SLIDE_NS_BATCHED + R.SLIDE_NS_BITWISE)
def test_whole_slide_backward_against_the_per_op_route(cuda, n):
    """ops.mil_bwd against functional.mil_backward at the row limits of the batched launch (helpers.assert_step_grad_matches_per_op: 2e-6 of the
    tensor's maximum for the six batched gradients inside 64 ... 262,144 rows, bitwise for everything else and outside). The bags of 262,144 rows
    and more run once; the others twice, bitwise the same."""
    from toad_amd import TOAD_fc_mtl_concat, functional as F_, ops
    torch.manual_seed(n)
    model = TOAD_fc_mtl_concat(n_classes=18); model.relocate()
    w = {k: v.detach() for k, v in model._weights().items()}
    g = torch.Generator(device=cuda).manual_seed(n + 1)
    x = torch.randn(n, 1024, device=cuda, generator=g); sex = torch.ones(1, device=cuda)
    dl = torch.randn(1, 18, device=cuda, generator=g); dsite = torch.randn(1, 2, device=cuda, generator=g)
    _, sv = F_.mil_forward(w, x, sex)
    g_ref, _ = F_.mil_backward(w, sv, dl, dsite)
    ref = dict(g_ref); ref["wab"] = torch.cat([g_ref["wa"], g_ref["wb"]], 0); ref["bab"] = torch.cat([g_ref["ba"], g_ref["bb"]], 0)
    del sv
    ops._ws(ops._scratch_bytes(n, 18, w["wc"].shape[1]), cuda, "mil").fill_(0xFF)
    arena = ops.mil_fwd(w, x, sex)
    runs = []
    for _ in range(1 if n >= 262144 else 2):
        grads = {k: _nan(tuple(w[k].shape), cuda) for k in ops.STEP_SLOTS}
        ops.mil_bwd(w, grads, 0.0, x, arena, dl, dsite)
        runs.append(grads)
    for k in ops.STEP_SLOTS:
        assert_step_grad_matches_per_op(runs[0][k], ref[k], k, n)
        assert torch.equal(runs[0][k], runs[-1][k]), k
