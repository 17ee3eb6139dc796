"""GPU: the NT GEMMs (forward and data-gradient Linears, launch_nt_h2) under every tile plan, K-split and fix-up launch. tests/nt_ref.py holds the
shapes (by the regime of the host plan each one reaches), the operand families and the arithmetic; tests/test_nt_plans_host.py shows on the CPU that
the restated plan is the library's, that every listed shape is in its regime, that the families meet their preconditions and that the emulated
arithmetic is exact on the integer families. Here the kernels run, through ops.linear_act_fwd and ops.linear_dgrad only:

  * integer families: Y must EQUAL the exact reference and the returned abs-max array the exact per-256-row-block maximum of |Y|.
    Every row of nt_ref.CASES runs the two plain forwards (x_amax given / self-measured) on small_int, pow2_blocks and late_outlier_int; the rows
    marked `full` (one per regime) run all seven modes - + bias and ReLU with the one-bit image written over a poisoned buffer, + train-mode
    dropout (p = 0.5, masks from tests/drop_ref.py), the plain dgrad, the dgrad with an addend buffer and the fp32 mask (256-row tiles even inside
    the half-height range), the dgrad that reads the image - and, up to 2,561 rows, the two 20-bit two-piece families as well;
  * real-valued families on three shapes: every element inside the derived bound of nt_ref (the ratios are printed; profiles/nt_plan_bound.md
    keeps them), the recomputed pooling addend among the modes;
  * the whole-slide route (ops.mil_fwd) on an fp32 bag, its fp16 copy and its prepared form: the only way to the fp16 and plane-tiled operand modes.
Every call runs twice and must repeat bitwise, on a workspace filled with 0xFF and a NaN destination, and the library's fallback-launch count
must not move."""
import numpy as np
import pytest
import torch

from tests import nt_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_fallback_launch(cuda):
    from toad_amd import _lib
    lib = _lib.load()
    before = lib.toad_fallback_launches()
    yield
    torch.cuda.synchronize()
    assert lib.toad_fallback_launches() == before, "an NT product fell back to the exact-fp32 kernels"


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def _poisoned_bits(nbytes, cuda):
    """Random bytes, the same on every call: a word the forward did not write keeps, and zeroes, half of what a dgrad that read it would mask."""
    return torch.randint(0, 256, (int(nbytes),), dtype=torch.uint8, device=cuda, generator=torch.Generator(device=cuda).manual_seed(99))


def _twice(call, cuda, m, n, k):
    """call(out) twice, each on a workspace filled with 0xFF and a NaN destination; the results (tuples of tensors / None) must repeat bitwise."""
    from toad_amd import _lib, ops
    lib = _lib.load()
    runs = []
    for _ in range(2):
        ops._ws(lib.toad_linear_ws_bytes(m, n, k), cuda).fill_(0xFF)
        runs.append(call(_nan((m, n), cuda)))
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b), "not reproducible run to run"
    return runs[0]


def _run_mode(cuda, mode, a, w, a_amax, bias, addend, src, bits):
    """One mode of nt_ref.MODES on device operands -> (Y, y_amax, bits or None). A dgrad's dY is `a`, its W^T [K_out, N_red] is `w`."""
    from toad_amd import ops
    m, k = a.shape
    n = w.shape[0]
    if mode == "fwd_given":
        return _twice(lambda out: ops.linear_act_fwd(a, w, None, ops.ACT_NONE, out=out, x_amax=a_amax, want_amax=True) + (None,), cuda, m, n, k)
    if mode == "fwd_self":
        return _twice(lambda out: ops.linear_act_fwd(a, w, None, ops.ACT_NONE, out=out, want_amax=True) + (None,), cuda, m, n, k)
    if mode == "fwd_bias_relu":
        return _twice(lambda out: ops.linear_act_fwd(a, w, bias, ops.ACT_RELU, out=out, want_amax=True,
                                                     bits_out=_poisoned_bits(ops.relu_bits_bytes(m, n), cuda)), cuda, m, n, k)
    if mode == "fwd_drop":
        return _twice(lambda out: ops.linear_act_fwd(a, w, bias, ops.ACT_RELU, out=out, drop_p=R.DROP_P, drop_seed=R.DROP_SEED, x_amax=a_amax,
                                                     want_amax=True) + (None,), cuda, m, n, k)
    if mode == "dgrad_plain":
        return _twice(lambda out: ops.linear_dgrad(a, w, out=out, dy_amax=a_amax, want_amax=True) + (None,), cuda, m, n, k)
    if mode == "dgrad_addend_mask":
        return _twice(lambda out: ops.linear_dgrad(a, w, addend=addend, relu_src=src, out=out, mask_scale=2.0, want_amax=True) + (None,), cuda, m, n, k)
    if mode == "dgrad_bits":
        return _twice(lambda out: ops.linear_dgrad(a, w, relu_src=src, out=out, mask_scale=2.0, want_amax=True, relu_bits=bits) + (None,), cuda, m, n, k)
    raise ValueError(mode)


@pytest.mark.parametrize("case", R.CASES + [R.ADDEND_CASE], ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_integer_products_equal_the_exact_reference(cuda, case):
    from toad_amd import ops
    m, n, k = case.M, case.N, case.K
    seed = R.CASE_SEED + m
    modes = R.MODES if case.full else R.LIGHT_MODES
    for family in R.case_families(case):
        a_np, w_np = R.int_operands(family, m, n, k, seed)
        bias_np, addend_np = R.mode_sides(family, m, n, seed)
        a, w, bias, addend = _dev(a_np, cuda), _dev(w_np, cuda), _dev(bias_np, cuda), _dev(addend_np, cuda)
        a_amax = _dev(R.amax_rows256(a_np), cuda)
        plain = R.ref_exact(family, a_np, w_np)                                # one product per family, shared by the modes
        src_np = src = bits = None
        for mode in modes:
            epi = R.mode_epilogue(mode, bias_np, addend_np, src_np)
            ref = plain.astype(np.float64)
            if "bias" in epi:
                ref = np.maximum(ref + bias_np.astype(np.float64), 0.0)
            if "keep" in epi:
                ref = ref * epi["keep"].astype(np.float64)
            if "addend" in epi:
                ref = ref + addend_np.astype(np.float64)
            if "mask_src" in epi:
                ref = np.where(src_np > 0, ref * 2.0, 0.0)
            ref32 = ref.astype(np.float32)
            assert np.array_equal(ref32.astype(np.float64), ref)
            y, y_amax, out_bits = _run_mode(cuda, mode, a, w, a_amax, bias, addend, src, bits)
            what = (m, n, k, family, mode)
            ref_d = _dev(ref32, cuda)
            assert torch.equal(y, ref_d), what + (int((y != ref_d).sum()),)
            assert torch.equal(y_amax, _dev(R.exact_amax(ref32), cuda)), what + ("y_amax",)
            if mode == "fwd_bias_relu":
                src_np, src, bits = ref32, ref_d, out_bits
                assert bits is not None
            if mode == "dgrad_bits":
                # ... and the same call without the image (fp32 mask only): the same tiles, the same sums. Where a one-stage reduction makes the
                # launch mask with the fp32 activations anyway (nt_route: read_bits false, the (1, 512, 32) row) this is the comparison the row is for.
                y2, a2 = ops.linear_dgrad(a, w, relu_src=src, mask_scale=2.0, want_amax=True)
                assert torch.equal(y, y2) and torch.equal(y_amax, a2), what + ("fp32 mask",)


def _pool_operands(m, n, seed):
    """(A_raw [M,2], stats [2,2], dM [2,N]) of the recomputed pooling addend and its float64 value [M,N] with the derived bound of its error:
    p_t = exp(a_t - mx_t) / s_t; the kernel forms exp2((a - mx) log2 e) (argument error <= 3 * 2^-24 |z| log2 e, i.e. relative 3 * 2^-24 |z| in
    the result; the exponential itself to 2^-22), the reciprocal of s_t (2^-23), three products and one sum (2^-24 each):
    |err| <= sum_t (|z_t| + 4) 2^-22 p_t |dM_t|."""
    g = np.random.default_rng(seed + 9)
    a_raw = (g.standard_normal((m, 2)) * 2.0).astype(np.float32)
    dm = (g.standard_normal((2, n)) * 0.5).astype(np.float32)
    mx = a_raw.max(0)
    s = np.exp(a_raw - mx).sum(0, dtype=np.float32)
    stats = np.stack([mx, s], 1).astype(np.float32)
    z = a_raw.astype(np.float64) - mx.astype(np.float64)
    p = np.exp(z) / s.astype(np.float64)
    return a_raw, stats, dm, p @ dm.astype(np.float64), ((np.abs(z) + 4.0) * 2.0 ** -22 * p) @ np.abs(dm).astype(np.float64)


REAL_MODES = ("fwd_given", "fwd_self", "fwd_bias_relu", "dgrad_plain", "dgrad_addend_mask", "dgrad_bits", "dgrad_pool_mask")


@pytest.mark.parametrize("shape", R.REAL_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", R.REAL_FAMILIES)
def test_real_valued_products_stay_inside_the_derived_bound(cuda, family, shape):
    """Every element within c1 (sum_k |a w| + |bias| + |addend|) + c2 K A_b B_n (nt_ref's docstring derives it; the pooled addend adds the error
    of its own formation, _pool_operands). The largest err / bound per mode is printed before anything is asserted."""
    from toad_amd import ops
    m, n, k = shape
    a_np, w_np = R.real_family(family, m, n, k, R.REAL_SEED + m)
    bias_np, addend_np = R.real_sides(m, n, R.REAL_SEED + m)
    a, w, bias, addend = _dev(a_np, cuda), _dev(w_np, cuda), _dev(bias_np, cuda), _dev(addend_np, cuda)
    a_amax = _dev(R.amax_rows256(a_np), cuda)
    plain = R.ref_f64(a_np, w_np)
    s_abs = np.abs(a_np).astype(np.float64) @ np.abs(w_np).astype(np.float64).T
    scale = (np.repeat(R.amax_rows256(a_np).astype(np.float64), R.PB)[:m].reshape(-1, 1) * np.abs(w_np).astype(np.float64).max(1).reshape(1, -1)) * k
    src_np = np.maximum(plain + bias_np, 0.0).astype(np.float32)
    src = _dev(src_np, cuda)
    a_raw, stats, dm, pool, pool_err = _pool_operands(m, n, R.REAL_SEED + m)
    ratios = {}
    bits = None
    for mode in REAL_MODES:
        route = "pool_mask" if mode == "dgrad_pool_mask" else R.MODE_ROUTE[mode]
        lp = R.launch_plan(m, n, k, R.nt_route(m, n, k, route)[0])
        c1, c2 = R.bound_coeffs(k, R.max_g(lp), R.MODE_OPERAND.get(mode, "given"))
        ref, side, extra = plain, 0.0, 0.0
        if mode == "fwd_bias_relu":
            ref, side = np.maximum(plain + bias_np, 0.0), np.abs(bias_np).astype(np.float64)
        elif mode == "dgrad_addend_mask":
            ref, side = np.where(src_np > 0, (plain + addend_np) * 2.0, 0.0), np.abs(addend_np).astype(np.float64)
        elif mode == "dgrad_bits":
            ref = np.where(src_np > 0, plain * 2.0, 0.0)
        elif mode == "dgrad_pool_mask":
            ref, side, extra = np.where(src_np > 0, (plain + pool) * 2.0, 0.0), np.abs(pool), pool_err
        bound = (c1 * (s_abs + side) + c2 * scale + extra) * (2.0 if "mask" in mode or mode == "dgrad_bits" else 1.0)
        if mode == "dgrad_pool_mask":
            pl = (_dev(a_raw, cuda), _dev(stats, cuda), _dev(dm, cuda))
            y, y_amax, _ = _twice(lambda out: ops.linear_dgrad(a, w, relu_src=src, out=out, mask_scale=2.0, pool=pl, want_amax=True) + (None,), cuda, m, n, k)
        else:
            y, y_amax, out_bits = _run_mode(cuda, mode, a, w, a_amax, bias, addend, src, bits)
            if mode == "fwd_bias_relu":
                bits = out_bits
                src = y                                    # the masked dgrads mask with what THIS forward wrote (its image describes it) ...
                src_np = y.cpu().numpy()                   # ... and so do their references
        got = y.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (family, shape, mode)
        ratios[mode] = float((np.abs(got - ref) / bound).max())
        assert torch.equal(y_amax.cpu(), torch.from_numpy(R.exact_amax(y.cpu().numpy()))), (family, shape, mode, "y_amax")
    for mode, r in ratios.items():
        print(f"nt bound (MI355X) {family} {m}x{n}x{k} {mode}: err/bound {r:.3e}")
    for mode, r in ratios.items():
        assert r <= 1.0, (family, shape, mode, r)


@pytest.mark.parametrize("n", R.SLIDE_NS)
def test_whole_slide_forward_on_fp32_fp16_and_prepared_bags(cuda, n):
    """ops.mil_fwd on a small_int bag (fp16-exact) as fp32, as its fp16 copy and in its prepared form: the fp16 (AMODE 1) and plane-tiled (AMODE 2)
    operand modes of the NT kernel are reached this way only. W1 and b1 are small integers over 128, so the first Linear is EXACT under every plan
    (the fp16 and prepared bags run 256-row tiles where the fp32 bag takes half-height ones): H1 must equal the int64 reference on all three,
    and with one H1 the rest of the forward is the same launches on the same values - bitwise equal. The fp32 call also equals the per-op chain
    where tests/test_gpu_h2.py::test_whole_slide_calls_are_bitwise_the_per_op_path claims it."""
    from toad_amd import TOAD_fc_mtl_concat, functional as F_, ops
    torch.manual_seed(n)
    model = TOAD_fc_mtl_concat(n_classes=18); model.relocate()
    w = {k: v.detach().clone() for k, v in model._weights().items()}
    x_np, w1_np = R.int_operands("small_int", n, 512, 1024, R.CASE_SEED + n)
    b1_np = R.int_sides(n, 512, R.CASE_SEED + n)[0]
    assert R.int_ok("small_int", x_np, w1_np) and np.array_equal(x_np.astype(np.float16).astype(np.float32), x_np)
    w["w1"].copy_(_dev(w1_np / 128.0, cuda)); w["b1"].copy_(_dev(b1_np / 128.0, cuda))
    h1_ref = _dev(R.ref_exact("small_int", x_np, w1_np, bias=b1_np, relu=True) / np.float32(128.0), cuda)
    x = _dev(x_np, cuda); sex = torch.ones(1, device=cuda)
    c, d = 18, w["wc"].shape[1]
    views = [("h1", (n, 512)), ("h", (n, 512)), ("p", (n, 2 * d)), ("a_raw", (n, 2)), ("mcat", (2, 513)), ("logits", (1, c)), ("site_logits", (1, 2)),
             ("y_prob", (1, c)), ("h1_amax", (ops.amax_floats(n),)), ("h_amax", (ops.amax_floats(n),))]
    got = {}
    for kind, bag in (("fp32", x), ("fp16", x.half()), ("prepared", ops.prepare_bag(x))):
        runs = []
        for _ in range(2):
            ops._ws(ops._scratch_bytes(n, c, d), cuda, "mil").fill_(0xFF)
            arena = ops.mil_fwd(w, bag, sex)
            runs.append({name: arena.view(name, shp).clone() for name, shp in views})
        for name, _ in views:
            assert torch.equal(runs[0][name], runs[1][name]), (n, kind, name, "not reproducible run to run")
        assert torch.equal(runs[0]["h1"], h1_ref), (n, kind, int((runs[0]["h1"] != h1_ref).sum()))
        got[kind] = runs[0]
    for kind in ("fp16", "prepared"):
        for name, _ in views:
            assert torch.equal(got[kind][name], got["fp32"][name]), (n, kind, name)
    outs, sv = F_.mil_forward(w, x, sex)
    g = got["fp32"]
    assert torch.equal(g["logits"], outs["logits"]) and torch.equal(g["site_logits"], outs["site_logits"]) and torch.equal(g["a_raw"], outs["A_nt"])
    assert torch.equal(g["mcat"], outs["features"]) and torch.equal(g["y_prob"], outs["Y_prob"])
    assert torch.equal(g["h"], sv.h) and torch.equal(g["p"], sv.p) and torch.equal(g["h_amax"], sv.h_amax)
