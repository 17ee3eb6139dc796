"""TEST INFRASTRUCTURE ONLY - numpy statement of the weight-gradient (TN) GEMMs of toad_amd/csrc: dW = dY^T X, db = column sums of dY.
It does not import the product package.

  * the three host plans, restated from the C sources: tn_plan (gemm_tn.inc), tn_batch_plan and wgrad_plan (gemm_f32.hip), the workgroup walk of
    gemm_tn_h2_body (gemm_h2.inc) and the workspace sizes built on them;
  * seeded operand families, each with its precondition as a function checked on the CPU;
  * a numpy emulation of the two-piece arithmetic under any plan;
  * the per-element error bound of a TN product under ONE power-of-two scale per operand.

The h2 arithmetic (csrc/h2_arith.h, gemm_h2.inc gemm_tn_h2_body)
    k(a)   = 14 - e with amax = f 2^e, f in [0.5, 1)       so that amax 2^k lies in [2^13, 2^14); amax over the WHOLE operand
    u      = a 2^k ;  h = rn16(u) ;  m = rn16(u - h)       one rounding each (v_fma_mix*_f16 rounds the exact residual once)
    slab_s = sum over the rows of split s of  m_a h_b + h_a m_b + h_a h_b      fp16 x fp16 products are exact in fp32; fp32 accumulation
    dW     = beta dW + (sum_s slab_s) 2^-(ka + kb)         slabs in fixed order, two exact power-of-two factors
    db     = beta db + sum_s (column sums of the unscaled fp32 dY rows of split s)
An fp16 X (B16) is its own first piece under scale 1 (m_b = 0). A prepared (plane-tiled) X carries one scale per 256-row tile; the kernel moves
the accumulators between tile scales by exact powers of two (gemm_pt.inc).

Why integer operands make every plan bitwise checkable. Let a, b be integers and |a| 2^ka, |b| 2^kb < 2^14.
  small_int      |a|, |b| <= 8: four significant bits, so h = u and m = 0 under ANY power-of-two scale that keeps u in fp16 range; every product is an
                 integer multiple of 2^(ka+kb) and every partial sum of them is too, of magnitude <= 2^(ka+kb) sum_r |a_r b_r|. While that sum of
                 absolute products stays below 2^24 every partial sum is an fp32 number, in any order, inside an MFMA or across slabs.
                 Shape-level sufficient condition: 64 M < 2^24 (the products reach 8 * 8; a draft of this family stated 16 M, which only covers |a|, |b|
                 <= 4); the function below checks the operands' actual column sums.
  two_piece_int  |b| < 2^20 (20 significant bits), a in {-1, 0, 1}. u_b = b 2^kb with kb >= -6, u_b < 2^14: h keeps the leading 11 bits, the residual
                 u - h has at most 20 - 11 + 1 = 10 significant bits (one more when the rounding of h carries) and is an fp16 number, so h + m = u
                 EXACTLY: two_piece_exact() settles this element by element with numpy's float16. u_a = +-2^13 or 0: m_a = 0, so the dropped m m
                 term is zero and the h_a m_b products carry real bits. Every term is a multiple of 2^(ka+kb) again; with at most 8 non-zero a per
                 column the absolute sum is <= 8 (2^20 - 1) < 2^24 units.
  In both families the descale multiplies by powers of two, beta = 1 adds an integer base (kept below 2^24 in sum), and db sums small integers: dW and
  db must EQUAL the int64 reference, whatever the plan. A dropped, doubled or misplaced row, stage, tile, split or slab changes an integer.
  What the integer families do NOT see: a wrong operand scale (exact integers stay exact under any power of two that does not overflow). The
  `late_giant` family does: a scale taken without the last row overflows fp16 there.

The bound for real operands (bound_coeffs, tn_bound). A = amax |dY|, B = amax |X| over the whole operands, scaled values |u| < 2^14.
  1 representation. Normal fp16 results carry 11 bits: |u - h| <= 2^-11 |u|, |r - m| <= 2^-11 |r| with r = u - h, so e = u - (h + m) has
    |e| <= 2^-22 |u|; where r falls into the fp16 subnormal range (|r| < 2^-14, spacing 2^-24) the error is absolute, |e| <= 2^-25. Together
    |e| <= 2^-22 |u| + 2^-25, and |m| <= (1 + 2^-11) 2^-11 |u|.
  2 the three-term product. P = h_a h_b + h_a m_b + m_a h_b = u_a u_b - e_a u_b - e_b (u_a - e_a) - m_a m_b, so
    |P - u_a u_b| <= (2 * 2^-22 + (1 + 2^-11)^2 2^-22) |u_a u_b| + 2^-25 (|u_a| + |u_b|) + |e_a e_b|
                  <= 3.01 * 2^-22 |u_a u_b| + 2^-10 + 2^-44        per row (|u| < 2^14).
  3 fp32 accumulation. A term reaches the output through at most d = 3 rows_per_split + nsplit + 1 additions: three MFMA terms per row of its
    split, the slabs, the beta add. For any order of d roundings of unit u32 the error is at most gamma_d = d u32 / (1 - d u32) times the sum of the
    absolute terms, which is <= 1.002 sum |u_a u_b| (the m-piece terms add 2 * 2^-11 (1 + 2^-11)). u32 = 2^-23: twice the round-to-nearest unit,
    so the bound also holds for a matrix unit that truncates aligned addends.
  Back in the operands' units one scaled unit of a product is 2^-(ka+kb) <= A B 2^-26, and sum |u_a u_b| = 2^(ka+kb) sum |a b|:
    |err_ij| <= c1 sum_r |dy_ri x_rj| + c2 M A B,   c1 = 3.01 * 2^-22 + 1.01 gamma_d,   c2 = 2^-35
    (c2: (2^-10 + 2^-44) (1 + gamma_d) <= 2^-9 scaled units per row, times 2^-26 A B).
  Nothing in it is fitted to a measurement; c1 depends on the plan only through d. An fp16 X has e_b = m_b = 0 and a prepared X is scaled per
  256-row tile by at least the global scale: both lie inside the same bound. db: plain fp32 adds (unit 2^-24) of the rows of a split in four
  interleaved chains, their combination, the slabs and beta: |err_i| <= gamma'_(rows_per_split / 4 + nsplit + 3) sum_r |dy_ri|.
"""
from collections import namedtuple

import numpy as np

BK, PB, BM, BN = 32, 256, 128, 128            # h2_arith.h BK, PB; gemm_f32.hip BM, BN
NUM_XCD, BLOCKS_PER_XCD = 8, 32               # common.h kNumXCD; h2_arith.h PB_BLOCKS_PER_XCD
PB_GRID = NUM_XCD * BLOCKS_PER_XCD
ROWBLK = 256                                  # common.h H2_ROWBLK
BATCH_MIN_ROWS, BATCH_MAX_ROWS = 64, 262144   # gemm_f32.hip wgrad_batch_ok; common.h kTnBatchMaxRows


def _cdiv(a, b):
    return (a + b - 1) // b


def nblk(rows):
    return _cdiv(rows, ROWBLK)


# ---- the plans --------------------------------------------------------------------------------------------------------------------------------
TnPlan = namedtuple("TnPlan", "ti tj tiles spx nsplit rows_per_split items_max any_idle")
TnBatchPlan = namedtuple("TnBatchPlan", "nsplit rows_per_split tiles_all")
WgradPlan = namedtuple("WgradPlan", "nsplit rows_per_split tiles_i tiles_j")


def _tn_max_splits(M):
    return _cdiv(M, 128) if M >= 8192 else _cdiv(M, 32)


def _round_rows(M, ns):
    """rows per split: ceil(M / ns) rounded UP to whole 32-row stages."""
    return _cdiv(_cdiv(M, ns), BK) * BK


def tn_walk(nsplit, tiles):
    """gemm_tn_h2_body / gemm_tn_pt_kernel without ONE_ITEM: {workgroup b: [(split, tile), ...] in the order it walks them}."""
    walk = {}
    for b in range(PB_GRID):
        xcd, jb = b % NUM_XCD, b // NUM_XCD
        splits_x = (nsplit - xcd + NUM_XCD - 1) // NUM_XCD
        items_x = splits_x * tiles
        n_items = _cdiv(items_x - jb, BLOCKS_PER_XCD) if jb < items_x else 0
        walk[b] = [(((jb + i * BLOCKS_PER_XCD) // tiles) * NUM_XCD + xcd, (jb + i * BLOCKS_PER_XCD) % tiles) for i in range(n_items)]
    return walk


def tn_plan(M, I, J):
    """gemm_tn.inc tn_plan, plus what the workgroup walk makes of it: the largest number of items on one workgroup and whether any has none."""
    ti, tj = _cdiv(I, PB), _cdiv(J, PB)
    tiles = ti * tj
    spx = max(BLOCKS_PER_XCD // tiles, 1)
    max_splits = _tn_max_splits(M)
    while spx > 1 and spx * NUM_XCD > max_splits:
        spx -= 1
    ns = spx * NUM_XCD
    if ns > max_splits:
        ns = max(max_splits, 1)
    rps = _round_rows(M, ns)
    nsplit = _cdiv(M, rps)
    counts = [len(v) for v in tn_walk(nsplit, tiles).values()]
    return TnPlan(ti, tj, tiles, _cdiv(nsplit, NUM_XCD), nsplit, rps, max(counts), min(counts) == 0)


def tn_batch_plan(M, jobs):
    """gemm_f32.hip tn_batch_plan; jobs = [(N, K), ...]. nsplit = 0: refused (no tiles, or more than one item per workgroup)."""
    tiles_all = sum(_cdiv(n, PB) * _cdiv(k, PB) for n, k in jobs)
    if tiles_all <= 0 or tiles_all > PB_GRID:
        return TnBatchPlan(0, 0, tiles_all)
    s = max(min(PB_GRID // tiles_all, _tn_max_splits(M)), 1)
    rps = _round_rows(M, s)
    return TnBatchPlan(_cdiv(M, rps), rps, tiles_all)


def tn_batch_items(nsplit, tiles_all):
    """gemm_tn_h2_batch_kernel: {workgroup b: (split, tile of all products) or None}."""
    out = {}
    for b in range(PB_GRID):
        k = (b % NUM_XCD) * BLOCKS_PER_XCD + b // NUM_XCD
        out[b] = (k // tiles_all, k % tiles_all) if k < nsplit * tiles_all else None
    return out


def wgrad_plan(M, N, K):
    """gemm_f32.hip wgrad_plan: the plan of the exact-fp32 TN kernel. No entry point reaches that kernel any more (tn_big_ok accepts every shape
    they admit), but the plan still sizes the workspace."""
    tiles_i, tiles_j = _cdiv(N, BM), _cdiv(K, BN)
    tiles = tiles_i * tiles_j
    max_splits = _cdiv(M, 256)
    if max_splits >= NUM_XCD:
        spx = 1
        while (tiles * spx) % 32 != 0 and spx < 32:
            spx += 1
        unit = spx
        while tiles * spx < 64 and (spx + unit) * NUM_XCD <= max_splits:
            spx += unit
        if spx * NUM_XCD > max_splits:
            spx = max_splits // NUM_XCD
        best = max(spx, 1) * NUM_XCD
    else:
        best = max_splits
    rps = _round_rows(M, best)
    return WgradPlan(_cdiv(M, rps), rps, tiles_i, tiles_j)


def _amax_area_bytes(M):
    return (2 * nblk(M) + 64) * 4


def wgrad_ws_bytes(M, N, K):
    """toad_linear_wgrad_ws_bytes."""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    ns = max(wgrad_plan(M, N, K).nsplit, tn_plan(M, N, K).nsplit)
    return ns * (N * K + N) * 4 + _amax_area_bytes(M)


def batch_need_bytes(M, jobs, i):
    """the `need` expression of wgrad_batch_ok for job i."""
    n, k = jobs[i]
    return tn_batch_plan(M, jobs).nsplit * (n * k + n) * 4 + _amax_area_bytes(M)


def slide_ws_bytes_each(M, jobs):
    """What the whole-slide calls give each of the three weight gradients (csrc/step.hip): the largest of the per-op sizes."""
    return max(wgrad_ws_bytes(M, n, k) for n, k in jobs)


def batch_ok(M, jobs, ws_bytes_each):
    """The shape part of wgrad_batch_ok (pointers and the fp16 rules aside)."""
    if not 2 <= len(jobs) <= 3 or not BATCH_MIN_ROWS <= M <= BATCH_MAX_ROWS:
        return False
    if tn_batch_plan(M, jobs).nsplit < 1 or any(n < 4 or k < 4 for n, k in jobs):
        return False
    return all(batch_need_bytes(M, jobs, i) <= ws_bytes_each for i in range(len(jobs)))


def split_rows(M, rows_per_split, nsplit):
    """[(first row, end row)] of every split."""
    return [(s * rows_per_split, min(M, (s + 1) * rows_per_split)) for s in range(nsplit)]


def split_stages(M, rows_per_split, nsplit):
    return [_cdiv(e - b, BK) for b, e in split_rows(M, rows_per_split, nsplit)]


# ---- the shapes of tests/test_gpu_wgrad_plans.py, by the regime each is there for ----------------------------------------------------------------
MODEL_JOBS = [(768, 512), (512, 512), (512, 1024)]            # dWab = dP^T H, dW2 = dZ2^T H1, dW1 = dZ1^T X
PER_OP_CASES = [                                              # (regime, M, N, K)
    ("one_stage", 1, 256, 256), ("one_stage", 31, 256, 256), ("one_stage", 32, 256, 256), ("one_stage", 33, 256, 256),
    ("last_split_one_row", 65, 256, 256), ("last_split_one_row", 97, 256, 256),
    ("idle_xcds", 300, 512, 512),
    ("switch_8192", 8191, 256, 256), ("switch_8192", 8192, 256, 256), ("switch_8192", 8193, 256, 256),
    ("walk_two_items", 300, 1536, 1536),
    ("uneven_walk", 300, 2816, 768),
    ("partial_tiles", 97, 132, 36), ("partial_tiles", 300, 132, 36), ("partial_tiles", 97, 260, 516), ("partial_tiles", 300, 260, 516),
    ("partial_tiles", 300, 260, 520),                         # ... and one with K % 8 == 0, which a prepared bag needs
]
BATCH_CASES = [                                               # (regime, M, jobs)
    ("model", 64, MODEL_JOBS), ("model", 65, MODEL_JOBS), ("model", 97, MODEL_JOBS), ("model", 300, MODEL_JOBS), ("model", 8192, MODEL_JOBS),
    ("two_jobs_switch", 8191, [(256, 256), (256, 256)]), ("two_jobs_switch", 8192, [(256, 256), (256, 256)]),
    ("partial_middle", 300, [(256, 256), (260, 516), (256, 256)]),
]
BATCH_X16_CASES = [("x16", 97, MODEL_JOBS), ("x16", 300, MODEL_JOBS)]
BATCH_REFUSED = [("rows_below", 63, [(8, 8), (8, 8)]), ("rows_above", 262145, [(8, 8), (8, 8)]), ("four_jobs", 300, [(8, 8)] * 4)]
REAL_MS = [300, 8193, 20000]
REAL_PER_OP = (256, 512)                                      # (N, K) of the per-op real-valued cases
REAL_JOBS = [(256, 512), (512, 256), (256, 256)]
REAL_FAMILIES = ("randn", "decades", "late_giant")
SLIDE_NS_BATCHED = [64, 65, 97, 8192, 262144]                 # whole-slide route: inside the batched launch's row range
SLIDE_NS_BITWISE = [63, 262145]                               # ... and just outside it


def per_op_regimes(M, N, K):
    """The set of regime names the restated tn_plan puts (M, N, K) in."""
    p = tn_plan(M, N, K)
    stages = split_stages(M, p.rows_per_split, p.nsplit)
    rows = split_rows(M, p.rows_per_split, p.nsplit)
    out = set()
    if all(s == 1 for s in stages):
        out.add("one_stage")
    if p.nsplit > 1 and rows[-1][1] - rows[-1][0] == 1:
        out.add("last_split_one_row")
    if p.nsplit < NUM_XCD:
        out.add("idle_xcds")
    if p.tiles > BLOCKS_PER_XCD and p.items_max >= 2:
        out.add("walk_two_items")
    if p.items_max >= 2 and len({len(v) for v in tn_walk(p.nsplit, p.tiles).values() if v}) > 1:
        out.add("uneven_walk")
    if N % PB or K % PB:
        out.add("partial_tiles")
    if (N % 4 == 0 and N % 8) or (K % 4 == 0 and K % 8):
        out.add("mult4_not_8")
    return out


# ---- operand families ------------------------------------------------------------------------------------------------------------------------
def amax_rows256(x):
    """toad_absmax_rows256_f32: one abs-max per 256 rows."""
    m = x.shape[0]
    return np.array([np.abs(x[b * ROWBLK:min(m, (b + 1) * ROWBLK)]).max() for b in range(nblk(m))], dtype=np.float32)


def small_int(M, N, K, seed):
    """(dY [M,N], X [M,K]) fp32 integers in [-8, 8]: +-8 in row 0 and in the LAST row of each operand and nowhere else (so nowhere else in the last
    256-row block): the last row alone decides that block's abs-max. X is an fp16 matrix as well."""
    g = np.random.default_rng(seed)
    dy = g.integers(-7, 8, size=(M, N)).astype(np.float32)
    x = g.integers(-7, 8, size=(M, K)).astype(np.float32)
    for t, w in ((dy, N), (x, K)):
        t[0, g.integers(0, w)] = 8.0
        t[M - 1, g.integers(0, w)] = -8.0 if M > 1 else 8.0
        t[M - 1, w - 1] = 8.0                      # the last element of the operand
    return dy, x


def two_piece_int(M, N, K, seed, x_bits=20):
    """dY [M,N] in {-1, 0, 1} with at most 8 non-zeros per column (half of them at rows next to a multiple of 32, rows 0 and M - 1 among them);
    X [M,K] integers of up to x_bits bits with |x| = 2^x_bits - 1 planted in the first and the last row. x_bits = 11: an fp16 matrix as well."""
    g = np.random.default_rng(seed)
    top = (1 << x_bits) - 1
    x = (g.integers(0, top + 1, size=(M, K)) * g.choice([-1, 1], size=(M, K))).astype(np.float32)
    x[0, 0] = top
    x[M - 1, K - 1] = -top
    dy = np.zeros((M, N), dtype=np.float32)
    for i in range(N):
        forced = [0, M - 1] if i == 0 else ([M - 1] if i == N - 1 else [])          # the first and the last row reach the first and the last column
        edge = 32 * g.integers(0, _cdiv(M, 32) + 1, size=4) + g.integers(-1, 2, size=4)
        free = np.unique(np.clip(np.concatenate([g.integers(0, M, size=4), edge]), 0, M - 1))[:8 - len(forced)]
        rows = np.unique(np.concatenate([free, forced]).astype(np.int64))
        dy[rows, i] = g.choice([-1.0, 1.0], size=rows.size)
    return dy, x


def abs_sum_max(dy, x):
    """max over (i, j) of sum_r |dy_ri x_rj| (float64: exact for the integer families)."""
    return float((np.abs(dy).astype(np.float64).T @ np.abs(x).astype(np.float64)).max())


def small_int_ok(dy, x, base_max=0):
    """Precondition of small_int: integers of at most 4 bits, +-8 only in the first and last row, every sum of absolute products (plus the integer
    base of a beta = 1 call) below 2^24."""
    ints = all(np.array_equal(t, np.rint(t)) and np.abs(t).max() == 8 for t in (dy, x))
    planted = all(np.abs(t[1:-1]).max(initial=0) <= 7 for t in (dy, x))
    return ints and planted and abs_sum_max(dy, x) + base_max < 2 ** 24 and np.abs(dy).sum(0).max() + base_max < 2 ** 24


def two_piece_int_ok(dy, x, base_max=0, x_bits=20):
    """Precondition of two_piece_int: dY in {-1, 0, 1} with at most 8 non-zeros per column, X integers with amax exactly 2^x_bits - 1, every sum of
    absolute products (plus the base) below 2^24."""
    ints = np.array_equal(x, np.rint(x)) and np.abs(x).max() == (1 << x_bits) - 1 and set(np.unique(dy)) <= {-1.0, 0.0, 1.0}
    return ints and (dy != 0).sum(0).max() <= 8 and abs_sum_max(dy, x) + base_max < 2 ** 24


INT_BASE_MAX = 1000
INT_FAMILIES = ("small_int", "two_piece_int")
PER_OP_SEED, BATCH_SEED, REAL_SEED = 100, 200, 1000           # + M (+ the job's index): the CPU file checks the very operands the GPU file runs


def int_operands(family, M, N, K, seed, x_bits=20):
    return small_int(M, N, K, seed) if family == "small_int" else two_piece_int(M, N, K, seed + 1, x_bits)


def int_ok(family, dy, x, x_bits=20):
    return small_int_ok(dy, x, INT_BASE_MAX) if family == "small_int" else two_piece_int_ok(dy, x, INT_BASE_MAX, x_bits)


def real_family(name, M, N, K, seed):
    """randn; decades: every row of each operand times 10^uniform(-4, 4); late_giant: row M - 1 of both operands 1e4 times the rest."""
    g = np.random.default_rng(seed)
    dy = g.standard_normal((M, N)).astype(np.float32)
    x = g.standard_normal((M, K)).astype(np.float32)
    if name == "decades":
        dy *= (10.0 ** g.uniform(-4, 4, size=(M, 1))).astype(np.float32)
        x *= (10.0 ** g.uniform(-4, 4, size=(M, 1))).astype(np.float32)
    elif name == "late_giant":
        dy[M - 1] *= 1e4
        x[M - 1] *= 1e4
    elif name != "randn":
        raise ValueError(name)
    return dy, x


def int_base(N, K, seed):
    """The integer destination of a beta = 1 call: (dW0 [N,K], db0 [N]) in [-1000, 1000]."""
    g = np.random.default_rng(seed)
    return g.integers(-1000, 1001, size=(N, K)).astype(np.float32), g.integers(-1000, 1001, size=(N,)).astype(np.float32)


def ref_int64(dy, x):
    """(dW, db) as int64; the float64 products and sums are exact for the integer families (asserted)."""
    assert abs_sum_max(dy, x) < 2 ** 52
    dw = dy.astype(np.float64).T @ x.astype(np.float64)
    db = dy.astype(np.float64).sum(0)
    assert np.array_equal(dw, np.rint(dw)) and np.array_equal(db, np.rint(db))
    return dw.astype(np.int64), db.astype(np.int64)


def ref_f64(dy, x):
    return dy.astype(np.float64).T @ x.astype(np.float64), dy.astype(np.float64).sum(0)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------
def h2_exp_from_amax(amax):
    """h2_arith.h: k with amax 2^k in [2^13, 2^14), clamped to +-120; amax = 0 -> 14."""
    _, e = np.frexp(np.float32(amax))
    return int(np.clip(14 - int(e), -120, 120))


def h2_split(v, k):
    """(h, m) float16 planes of v 2^k, k a scalar or one exponent per row. The residual is formed exactly (float64) and rounded once."""
    u = v.astype(np.float64) * np.exp2(np.asarray(k, dtype=np.float64))
    h = u.astype(np.float16)
    m = (u - h.astype(np.float64)).astype(np.float16)
    return h, m, u


def two_piece_exact(v, k):
    """True when h + m reproduces every element of v 2^k."""
    h, m, u = h2_split(v, k)
    return bool(np.array_equal(h.astype(np.float64) + m.astype(np.float64), u) and np.isfinite(h.astype(np.float32)).all())


def tile_exps(x):
    """One exponent per ROW of a prepared X: that of its 256-row tile (gemm_pt.inc pt_split_kernel)."""
    return np.repeat([h2_exp_from_amax(a) for a in amax_rows256(x)], ROWBLK)[:x.shape[0]].reshape(-1, 1)


def emulate_tn(dy, x, rows_per_split, nsplit, x_mode="f32", beta=0.0, base=None):
    """(dW, db) fp32 as the two-piece kernels form them under the given plan. x_mode: "f32" (one scale), "f16" (X used as halves, scale 1) or
    "pt" (one scale per 256-row tile, accumulated at the scale of the operand's maximum). Each split's three terms are fp32 matrix products,
    summed m.h + h.m + h.h; slabs are summed in order: AN fp32 order, not the MFMA's - integers must not care and the bound covers any."""
    M = dy.shape[0]
    ka = h2_exp_from_amax(np.abs(dy).max())
    ha, ma, _ = h2_split(dy, ka)
    if x_mode == "f16":
        kb = 0
        hb, mb = x.astype(np.float16), None
        assert np.array_equal(hb.astype(np.float32), x), "an fp16 X must hold fp16 values"
    elif x_mode == "pt":
        kb = h2_exp_from_amax(np.abs(x).max())
        kt = tile_exps(x)
        hb, mb, _ = h2_split(x, kt)
        # the kernel rescales the ACCUMULATOR between tiles; scaling the pieces to the reference exponent instead is the same exact power of two
        hb = hb.astype(np.float32) * np.exp2(kb - kt).astype(np.float32)
        mb = mb.astype(np.float32) * np.exp2(kb - kt).astype(np.float32)
    else:
        kb = h2_exp_from_amax(np.abs(x).max())
        hb, mb, _ = h2_split(x, kb)
    ha, ma, hb = ha.astype(np.float32), ma.astype(np.float32), hb.astype(np.float32)
    mb = None if mb is None else mb.astype(np.float32)
    acc = None
    cs = None
    for b, e in split_rows(M, rows_per_split, nsplit):
        slab = ma[b:e].T @ hb[b:e]
        if mb is not None:
            slab = slab + ha[b:e].T @ mb[b:e]
        slab = slab + ha[b:e].T @ hb[b:e]
        col = dy[b:e].sum(0, dtype=np.float32)
        acc = slab if acc is None else acc + slab
        cs = col if cs is None else cs + col
    e = -(ka + kb)
    e1 = e >> 1
    dw = (acc * np.float32(2.0 ** e1)) * np.float32(2.0 ** (e - e1))
    if beta != 0.0:
        dw = dw + np.float32(beta) * base[0]
        cs = cs + np.float32(beta) * base[1]
    return dw.astype(np.float32), cs.astype(np.float32)


U32_MFMA = 2.0 ** -23          # see the docstring: covers a truncating matrix unit
U32 = 2.0 ** -24


def _gamma(d, u):
    assert d * u < 0.5
    return d * u / (1.0 - d * u)


def bound_coeffs(rows_per_split, nsplit):
    """(c1, c2) of |err_ij| <= c1 sum_r |dy_ri x_rj| + c2 M amax|dY| amax|X| - the docstring derives them."""
    d = 3 * rows_per_split + nsplit + 1
    return 3.01 * 2.0 ** -22 + 1.01 * _gamma(d, U32_MFMA), 2.0 ** -35


def tn_bound(dy, x, rows_per_split, nsplit):
    """[N,K] float64 bound of |dW - dY^T X| per element."""
    c1, c2 = bound_coeffs(rows_per_split, nsplit)
    s = np.abs(dy).astype(np.float64).T @ np.abs(x).astype(np.float64)
    return c1 * s + c2 * dy.shape[0] * float(np.abs(dy).max()) * float(np.abs(x).max())


def db_bound(dy, rows_per_split, nsplit):
    """[N] float64 bound of |db - column sums of dY|."""
    return _gamma(rows_per_split // 4 + nsplit + 3, U32) * np.abs(dy).astype(np.float64).sum(0)
