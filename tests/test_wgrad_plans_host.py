"""CPU: the restated weight-gradient plans of tests/wgrad_ref.py against the library's own workspace sizes, the regime table behind
tests/test_gpu_wgrad_plans.py, the operand families' preconditions, and the numpy emulation of the two-piece arithmetic: bitwise on the integer
families under every listed plan, inside the derived bound on the real-valued ones."""
import numpy as np
import pytest

from tests import wgrad_ref as R

PER_OP_SHAPES = sorted({(m, n, k) for _, m, n, k in R.PER_OP_CASES} | {(m,) + R.REAL_PER_OP for m in R.REAL_MS} |
                       {(m, n, k) for _, m, jobs in R.BATCH_CASES + R.BATCH_X16_CASES for n, k in jobs} |
                       {(m, n, k) for m in R.REAL_MS for n, k in R.REAL_JOBS} |
                       {(m, n, k) for m in R.SLIDE_NS_BATCHED + R.SLIDE_NS_BITWISE for n, k in R.MODEL_JOBS})


def _lib():
    from toad_amd import _lib
    return _lib.load(), _lib


def test_restated_plans_reproduce_the_workspace_size():
    lib, _ = _lib()
    for m, n, k in PER_OP_SHAPES:
        assert lib.toad_linear_wgrad_ws_bytes(m, n, k) == R.wgrad_ws_bytes(m, n, k), (m, n, k)
    # ... and on a sweep across the thresholds of both plans (256-row units of wgrad_plan, 32 / 128-row units and the 8192 switch of tn_plan)
    for n, k in [(256, 256), (512, 1024), (768, 512), (132, 36), (2816, 768), (1536, 1536), (4, 4)]:
        for m in [1, 2, 255, 256, 257, 2047, 2048, 2049, 4100, 8191, 8192, 8193, 10000, 16385, 50000, 100000, 262144, 262145, 1000003]:
            assert lib.toad_linear_wgrad_ws_bytes(m, n, k) == R.wgrad_ws_bytes(m, n, k), (m, n, k)
    assert lib.toad_linear_wgrad_ws_bytes(0, 4, 4) == 0 == R.wgrad_ws_bytes(0, 4, 4)


def _fake_jobs(_l, jobs, ptr=1 << 21):
    arr = (_l.ToadWgradJob * len(jobs))()
    for i, (n, k) in enumerate(jobs):
        arr[i] = _l.ToadWgradJob(ptr, ptr, ptr, ptr, ptr, ptr, n, k, ptr)
    return arr


def test_restated_batch_plan_reproduces_the_need_of_wgrad_batch_ok():
    """wgrad_batch_ok refuses a workspace one float short of the restated `need` of the LARGEST job before anything touches the device (the GPU
    file shows that exactly `need` bytes are accepted); and what ops.linear_wgrad_batch allocates covers every listed case."""
    from toad_amd import ops
    lib, _l = _lib()
    for _, m, jobs in R.BATCH_CASES + R.BATCH_X16_CASES + [("real", mm, R.REAL_JOBS) for mm in R.REAL_MS]:
        need = max(R.batch_need_bytes(m, jobs, i) for i in range(len(jobs)))
        assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, jobs), len(jobs), m, 0.0, 0, need - 4, None) == -2, (m, jobs)
        assert b"toad_linear_wgrad_batch_f32" in lib.toad_last_error()
        assert R.batch_ok(m, jobs, need) and not R.batch_ok(m, jobs, need - 4) and ops.linear_wgrad_batch_ws_bytes(m, jobs) >= need, (m, jobs)
        p = R.tn_batch_plan(m, jobs)
        assert 1 <= p.nsplit * p.tiles_all <= R.PB_GRID
    # the whole-slide calls size the three workspaces by the per-op plans (csrc/step.hip): that admits the batched launch at every bag length
    # the whole-slide cases of tests/test_gpu_wgrad_plans.py list as batched, so those cases do compare the batched launch with the per-op one
    # (a bag of 257 ... 448 rows is NOT admitted - 10 splits needed at 300 rows, room for 5 - and takes the three per-op launches)
    for m in R.SLIDE_NS_BATCHED:
        assert R.batch_ok(m, R.MODEL_JOBS, R.slide_ws_bytes_each(m, R.MODEL_JOBS)), m
    for m in R.SLIDE_NS_BITWISE:
        assert not R.batch_ok(m, R.MODEL_JOBS, 1 << 50), m


def test_batched_entry_refuses_without_a_gpu():
    lib, _l = _lib()
    big = 1 << 40
    for _, m, jobs in R.BATCH_REFUSED:
        assert not R.batch_ok(m, jobs, big)
        assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, jobs), len(jobs), m, 0.0, 0, big, None) == -2, (m, len(jobs))
        assert b"2 or 3 jobs" in lib.toad_last_error()
    two = [(256, 256), (256, 256)]
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, two), 1, 300, 0.0, 0, big, None) == -2            # one job
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, two), 2, 300, 0.0, 1, big, None) == -2            # an fp16 X only as the last of THREE
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, [(256, 256)] * 2 + [(256, 36)]), 3, 300, 0.0, 1, big, None) == -2   # fp16 X: K % 8
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, [(4096, 4096), (256, 256)]), 2, 300, 0.0, 0, big, None) == -2      # 257 tiles
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, [(256, 6), (256, 256)]), 2, 300, 0.0, 0, big, None) == -2 and b"multiples of 4" in lib.toad_last_error()
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, two, ptr=(1 << 21) + 4), 2, 300, 0.0, 0, big, None) == -4
    assert lib.toad_linear_wgrad_batch_f32(None, 2, 300, 0.0, 0, big, None) == -1
    assert lib.toad_linear_wgrad_batch_f32(_fake_jobs(_l, two), 2, 300, 0.0, 7, big, None) == -1


def test_plans_partition_rows_and_items():
    """Every plan of a listed shape cuts [0, M) into non-empty splits of whole stages (but the last), and hands every (split, tile) to exactly one
    workgroup."""
    for m, n, k in PER_OP_SHAPES:
        p = R.tn_plan(m, n, k)
        rows = R.split_rows(m, p.rows_per_split, p.nsplit)
        assert p.rows_per_split % R.BK == 0 and rows[0][0] == 0 and rows[-1][1] == m and all(b < e for b, e in rows), (m, n, k)
        assert all(rows[i][1] == rows[i + 1][0] for i in range(len(rows) - 1))
        items = [it for v in R.tn_walk(p.nsplit, p.tiles).values() for it in v]
        assert sorted(items) == [(s, t) for s in range(p.nsplit) for t in range(p.tiles)], (m, n, k)
    for _, m, jobs in R.BATCH_CASES + R.BATCH_X16_CASES + [("real", mm, R.REAL_JOBS) for mm in R.REAL_MS] + \
            [("slide", mm, R.MODEL_JOBS) for mm in R.SLIDE_NS_BATCHED]:
        p = R.tn_batch_plan(m, jobs)
        rows = R.split_rows(m, p.rows_per_split, p.nsplit)
        assert p.rows_per_split % R.BK == 0 and rows[-1][1] == m and all(b < e for b, e in rows), (m, jobs)
        items = [it for it in R.tn_batch_items(p.nsplit, p.tiles_all).values() if it is not None]
        assert sorted(items) == [(s, t) for s in range(p.nsplit) for t in range(p.tiles_all)], (m, jobs)


def test_every_regime_is_reached_by_its_listed_shapes():
    """A plan change that moves a listed shape out of the regime it is listed for fails here, not on the GPU."""
    for regime, m, n, k in R.PER_OP_CASES:
        if regime != "switch_8192":
            assert regime in R.per_op_regimes(m, n, k), (regime, m, n, k, R.tn_plan(m, n, k))
    assert "mult4_not_8" in R.per_op_regimes(300, 132, 36)
    # the M >= 8192 switch of max_splits: 32-row units below it, 128-row units from it on
    a, b, c = (R.tn_plan(m, 256, 256) for m in (8191, 8192, 8193))
    assert (a.nsplit, a.rows_per_split) == (256, 32) and (b.nsplit, b.rows_per_split) == (64, 128) and (c.nsplit, c.rows_per_split) == (52, 160)
    assert R.split_stages(8193, c.rows_per_split, c.nsplit)[-1] == 2 and 8193 - 51 * 160 == 33          # ... whose last stage holds ONE row
    # with the model's shapes every workgroup has one item: the multi-item walk needs the listed shapes
    for n, k in R.MODEL_JOBS:
        assert all(R.tn_plan(m, n, k).items_max == 1 for m in (64, 300, 8192, 100000))
    assert R.tn_plan(300, 1536, 1536).items_max == 2 and R.tn_plan(300, 1536, 1536).any_idle
    assert R.tn_plan(300, 2816, 768).tiles == 33
    # batched launch
    by = {(r, m): R.tn_batch_plan(m, j) for r, m, j in R.BATCH_CASES}
    assert by["model", 64] == (2, 32, 18) and by["model", 8192].nsplit == 14 and by["model", 300].nsplit == 10
    for m in (65, 97):                                               # a last split of one row
        p = by["model", m]
        assert m - (p.nsplit - 1) * p.rows_per_split == 1
    assert by["two_jobs_switch", 8191][:2] == (128, 64) and by["two_jobs_switch", 8192][:2] == (64, 128)
    assert R.tn_batch_plan(8191, R.MODEL_JOBS) == R.tn_batch_plan(8192, R.MODEL_JOBS)       # the model's 18 tiles never reach the switch
    assert by["partial_middle", 300].tiles_all == 8
    assert R.tn_batch_plan(262144, R.MODEL_JOBS).nsplit == 14
    for _, m, jobs in R.BATCH_REFUSED:
        assert not R.batch_ok(m, jobs, 1 << 40)


def _int_families(m, n, k, seed, x_bits=20):
    for family in R.INT_FAMILIES:
        dy, x = R.int_operands(family, m, n, k, seed, x_bits)
        assert R.int_ok(family, dy, x, x_bits), (family, m, n, k)
        yield family, dy, x


def _check_int(dy, x, rps, nsplit, modes, what):
    dw_ref, db_ref = R.ref_int64(dy, x)
    base = R.int_base(dy.shape[1], x.shape[1], 5)
    for mode in modes:
        dw, db = R.emulate_tn(dy, x, rps, nsplit, mode)
        assert np.array_equal(dw.astype(np.int64), dw_ref) and np.array_equal(dw, np.rint(dw)), (what, mode)
        assert np.array_equal(db.astype(np.int64), db_ref), (what, mode)
    dw, db = R.emulate_tn(dy, x, rps, nsplit, modes[0], 1.0, base)
    assert np.array_equal(dw.astype(np.int64), dw_ref + base[0].astype(np.int64)) and np.array_equal(db.astype(np.int64), db_ref + base[1].astype(np.int64)), what


@pytest.mark.parametrize("regime,m,n,k", R.PER_OP_CASES)
def test_integer_families_are_exact_under_the_per_op_plan(regime, m, n, k):
    """Preconditions, the exact split (global scale and the prepared bag's per-tile scales) and the emulated product == int64."""
    p = R.tn_plan(m, n, k)
    for name, dy, x in _int_families(m, n, k, R.PER_OP_SEED + m):
        assert R.two_piece_exact(dy, R.h2_exp_from_amax(np.abs(dy).max())) and R.two_piece_exact(x, R.h2_exp_from_amax(np.abs(x).max())), name
        assert R.two_piece_exact(x, R.tile_exps(x)), name
        if name == "two_piece_int":
            _, mpiece, _ = R.h2_split(x, R.h2_exp_from_amax(np.abs(x).max()))
            assert (mpiece != 0).mean() > 0.5                                   # the second piece carries real bits
        _check_int(dy, x, p.rows_per_split, p.nsplit, ["f32", "pt"] + (["f16"] if name == "small_int" else []), (name, m, n, k))


@pytest.mark.parametrize("regime,m,jobs", [c for c in R.BATCH_CASES + R.BATCH_X16_CASES if c[1] <= 300 or c[0] == "two_jobs_switch"] +
                         [("model_job1", 8192, [R.MODEL_JOBS[1]] * 2)])
def test_integer_families_are_exact_under_the_batch_plan(regime, m, jobs):
    p = R.tn_batch_plan(m, R.MODEL_JOBS if regime == "model_job1" else jobs)
    for i, (n, k) in enumerate(jobs[:1] if regime == "model_job1" else jobs):
        last16 = regime == "x16" and i == 2
        for name, dy, x in _int_families(m, n, k, R.BATCH_SEED + m + i, 11 if last16 else 20):
            _check_int(dy, x, p.rows_per_split, p.nsplit, ["f16"] if last16 else ["f32"], (name, m, i))


def test_family_preconditions_hold_for_every_batched_case():
    """... also for the operands of the large batched cases, whose emulation the test above leaves out."""
    for regime, m, jobs in R.BATCH_CASES + R.BATCH_X16_CASES:
        for i, (n, k) in enumerate(jobs):
            for _ in _int_families(m, n, k, R.BATCH_SEED + m + i, 11 if regime == "x16" and i == 2 else 20):
                pass


def test_a_two_piece_operand_needs_both_pieces():
    """The exactness argument is not vacuous: 20-bit integers are NOT fp16 numbers, and more than 22 bits no longer split exactly."""
    _, x = R.two_piece_int(97, 8, 64, 3)
    h, _, u = R.h2_split(x, R.h2_exp_from_amax(np.abs(x).max()))
    assert not np.array_equal(h.astype(np.float64), u)
    wide = x * 16.0 + 1.0
    assert not R.two_piece_exact(wide, R.h2_exp_from_amax(np.abs(wide).max()))


def real_ratios(family, m, verbose=True):
    """Largest err / bound of the emulation against fp64: {route: (dW ratio, db ratio)} - also what profiles/wgrad_plan_bound.md tabulates."""
    out = {}
    n, k = R.REAL_PER_OP
    assert (n, k) == R.REAL_JOBS[0]                     # the per-op routes run on the operands of the batch's first job
    cases = [("per-op fp32", n, k, R.tn_plan(m, n, k), "f32", 0), ("per-op prepared", n, k, R.tn_plan(m, n, k), "pt", 0)]
    bp = R.tn_batch_plan(m, R.REAL_JOBS)
    cases += [(f"batched job {i}", jn, jk, bp, "f32", i) for i, (jn, jk) in enumerate(R.REAL_JOBS)]
    for route, n_, k_, p, mode, s in cases:
        dy, x = R.real_family(family, m, n_, k_, R.REAL_SEED + m + s)
        dw, db = R.emulate_tn(dy, x, p.rows_per_split, p.nsplit, mode)
        rw, rb = R.ref_f64(dy, x)
        assert np.isfinite(dw).all() and np.isfinite(db).all(), (family, m, route)
        out[route] = (float((np.abs(dw - rw) / R.tn_bound(dy, x, p.rows_per_split, p.nsplit)).max()),
                      float((np.abs(db - rb) / R.db_bound(dy, p.rows_per_split, p.nsplit)).max()))
        if verbose:
            print(f"wgrad bound (emulation) {family} M={m} {route}: dW err/bound {out[route][0]:.3e}, db err/bound {out[route][1]:.3e}")
    return out


@pytest.mark.parametrize("m", R.REAL_MS)
@pytest.mark.parametrize("family", R.REAL_FAMILIES)
def test_emulated_product_stays_inside_the_derived_bound(family, m):
    for route, (rw, rb) in real_ratios(family, m).items():
        assert rw <= 1.0 and rb <= 1.0, (family, m, route, rw, rb)


def test_bound_notices_a_dropped_tail_stage():
    """What the bound is for: the rows of one 32-row stage dropped from one split of 20,000 rows move most elements out of it."""
    m, (n, k) = 20000, R.REAL_PER_OP
    p = R.tn_plan(m, n, k)
    dy, x = R.real_family("randn", m, n, k, 77)
    b, e = R.split_rows(m, p.rows_per_split, p.nsplit)[3]
    keep = np.ones(m, dtype=bool); keep[e - 32:e] = False
    dw, _ = R.emulate_tn(dy[keep], x[keep], p.rows_per_split, p.nsplit)
    rw, _ = R.ref_f64(dy, x)
    assert (np.abs(dw - rw) > R.tn_bound(dy, x, p.rows_per_split, p.nsplit)).mean() > 0.5
