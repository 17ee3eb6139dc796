"""TEST INFRASTRUCTURE ONLY - numpy statement of the NT GEMMs of toad_amd/csrc behind launch_nt_h2: Y = epi(A W^T), A [M,K] fp32, W [N,K].
It does not import the product package.

  * the host plan, restated from the C sources: nt_natural_g / nt_plan / nt_row_tile (gemm_nt_f32.inc), nt_half_tiles and the tile-height /
    read_bits part of nt_route (gemm_f32.hip), the workgroup-to-item walk of gemm_nt_h2_big_kernel (gemm_h2.inc), the launcher's fix-up choice and
    stagger threshold (launch_nt_h2). toad_nt_plan reports the library's own plan; tests/test_nt_plans_host.py holds the two together;
  * regimes(M, N, K, epilogue): what a shape reaches, and CASES: the smallest shapes per regime that tests/test_gpu_nt_plans.py runs;
  * seeded operand families, each with its precondition as a function checked on the CPU;
  * emulate_nt: the two-piece arithmetic under any plan, in both operand modes;
  * nt_bound: the per-element error bound for real operands.

The arithmetic (csrc/h2_arith.h, gemm_h2.inc, gemm_h2_epilogue.inc, nt_fixup_h2_kernel)
    kb[n]  = 14 - e of row n of W (split_planes_h2_kernel: one scale per weight row); ka of an ITEM (a tile, or one K-slice of a remainder tile):
             "given" (x_amax passed, AMODE 0): 14 - e of the abs-max slot of the tile's 256-row block (two half-height tiles share a slot);
             "self"  (x_amax = None, AMODE 3): 14 - e - RUN_MARGIN of the item's FIRST 32-deep stage; an item whose own maximum outgrows that room
             (exponent of the maximum < ka - 1) is poisoned, its epilogue skipped, and a second pass repeats it with 14 - e of its true maximum.
    slab   = sum over the item's stages of  m_a h_w + h_a m_w + h_a h_w       fp16 x fp16 products exact in fp32, fp32 accumulation
    whole tile:     y = epi((slab f1) f2[n]),   f1 f2[n] = 2^-(ka + kb[n])
    K-split tile:   v = slab_0 c_0 + slab_1 c_1 + ... in slice order, c_p = 1 (given) or 2^(kt - ka_p) (self; kt from the completed block maximum),
                    y = epi((v f1) f2[n]) with kt
    epi(x) = mask(drop(relu(x + bias + addend))): bias, addend, ReLU, dropout keep factor, (mask_src > 0) ? . mask_scale : 0
    y_amax[b] = max |y| over the stored rows of 256-row block b.

Why integer operands make every plan bitwise checkable. Every family below keeps h + m = u EXACTLY at every exponent an item can take (emulate_nt
checks it element by element and reports it), so each product term is an integer multiple of 2^(ka + kb) and so is every partial sum; while the sum of
absolute products (plus |bias| + |addend|) stays below 2^24 every partial sum is an fp32 number in any order - inside an MFMA, across stages,
across slabs (c_p is a power of two that brings slice p's unit to the tile's). The descale and a mask_scale / keep factor of 2 are exact: Y must EQUAL
the int64 reference and y_amax the exact block maximum, under every plan. A dropped, doubled or misplaced row, stage, tile, slice or slab changes
an integer.
  small_int         |a|, |w| <= 8 (+-8 in the first and last row and the last element): four bits, h = u and m = 0 at any exponent in fp16 range.
  two_piece_int_a   |a| < 2^20, w in {-1, 0, 1} with at most 8 non-zeros per W row: at most 8 terms per output, < 2^23. Given mode: u = a 2^-6, h keeps
                    11 bits, the residual 10. Self mode: ka lies between 3 bits below and 1 bit above that exponent (first-stage maximum and
                    RUN_MARGIN); u < 2^15 still leaves a residual of at most 10 bits above 2^-9 >> fp16's 2^-24 spacing: exact in both modes
                    (checked, not assumed: emulate_nt's `exact_split`).
  two_piece_int_w   the mirror: 20-bit W through the per-row scales of split_planes_h2_kernel, a in {-1, 0, 1} with at most 8 non-zeros per A row.
  late_outlier_int  small_int with the last 32 columns of A times 2^12 (|a| <= 2^15; K <= 1024 keeps the absolute sums below 2^24). Given mode: one
                    scale for the block, u = a 2^-2. Self mode: every item that holds the last stage behind a small first stage is POISONED and
                    re-run, and the K-slices of one tile carry different exponents (c_p != 1 in the fix-up).
  pow2_blocks       small_int with block b of A times 2^e_b and row n of W times 2^f_n, exponents in [-30, 30], neighbours at least 2^20 apart and
                    alternating in direction. Exact under every CORRECT scale; no bias / addend (they would round). What the plain integer families
                    do NOT see is a wrong scale: exact integers stay exact under any power of two that does not overflow. This family does: a tile that
                    scales with a neighbouring block's abs-max slot (the other half of a shared slot's neighbour, on half-height tiles) overflows fp16
                    where the neighbour is the smaller one, a descale with another slot or another row's binv is off by >= 2^20.

The bound for real operands (nt_bound). A_b = abs-max of the row's 256-row block, B_n = abs-max of W's row n, scaled values |u| < 2^14 (self: 2^15).
  1 representation and 2 the three-term product: as in tests/wgrad_ref.py: |P - u_a u_w| <= 3.01 * 2^-22 |u_a u_w| + 2^-25 (|u_a| + |u_w|) + 2^-44
    per k, the absolute part <= 2^-10 (given) or 1.5 * 2^-10 (self) scaled units.
  3 fp32 accumulation: a term reaches the output through at most d = 3 K + g + 3 additions / roundings (three MFMA terms per k, g slabs, bias, addend,
    mask scale); gamma_d with u32 = 2^-23 as in wgrad_ref (covers a truncating matrix unit), on sum |a w| + |bias| + |addend|.
  One scaled unit is 2^-(ka+kb) <= A_b B_n 2^-26 (given); in self mode 2^-ka <= 2^-10 times the item's maximum (first-stage rule + the poison
  test), so <= A_b B_n 2^-23:
    |err_mn| <= c1 (sum_k |a_mk w_nk| + |bias_n| + |addend_mn|) + c2 K A_b B_n,   c1 = 3.01 * 2^-22 + 1.01 gamma_d,   c2 = 2^-35 (given), 2^-32 (self).
  ReLU is 1-Lipschitz and the mask keeps or zeroes: neither widens it. Nothing in it is fitted to a measurement.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import drop_ref
from tests.wgrad_ref import U32_MFMA, _gamma, amax_rows256, h2_exp_from_amax, h2_split, nblk

BK, PB = 32, 256
NUM_XCD, BLOCKS_PER_XCD = 8, 32
PB_GRID = NUM_XCD * BLOCKS_PER_XCD
PB_GMAX = 16
RUN_MARGIN = 3
STAGGER_TILES = 2 * PB_GRID


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------
NtPlan = namedtuple("NtPlan", "mt_x tiles rounds rem g")
Item = namedtuple("Item", "wg xcd row_tile col_tile k0 k1 part")           # part: index of the K-slice, None for a whole-K item


def nt_natural_g(rem, rem_all, nk):
    g = BLOCKS_PER_XCD // rem if rem > 0 else 0
    g = min(g, nk, PB_GMAX)
    if g > 2:
        cap = 64 // rem_all if rem_all > 0 else g
        g = min(g, max(cap, 2))
    return g


def _xcd_tiles(x, tiles_m, tiles_n):
    return ((tiles_m - x + NUM_XCD - 1) // NUM_XCD) * tiles_n


@functools.lru_cache(maxsize=None)
def _nt_plans(tiles_m, tiles_n, nk):
    """nt_plan for the 8 XCDs at once (rem_all and the slowest XCD's time are the same for all of them)."""
    rr = [divmod(_xcd_tiles(x, tiles_m, tiles_n), BLOCKS_PER_XCD) for x in range(NUM_XCD)]
    rem_all = sum(m for _, m in rr)
    lcm = 720720                                     # tile times in units of 1 / lcm(1..16)
    nat = [nt_natural_g(m, rem_all, nk) for _, m in rr]
    t_max = max(r * lcm + (lcm // gx if m > 0 else 0) for (r, m), gx in zip(rr, nat))
    out = []
    for x, ((rounds, rem), g) in enumerate(zip(rr, nat)):
        if g > 1:                                    # no XCD slices finer than the slowest XCD makes useful
            gg = 1
            while gg < g and rounds * lcm + lcm // gg > t_max:
                gg += 1
            g = gg
        out.append(NtPlan((tiles_m - x + NUM_XCD - 1) // NUM_XCD, rounds * BLOCKS_PER_XCD + rem, rounds, rem, g))
    return tuple(out)


def nt_plan(xcd, tiles_m, tiles_n, nk):
    return _nt_plans(tiles_m, tiles_n, nk)[xcd]


def nt_row_tile(q, tiles_n, xcd):
    return (q // tiles_n) * NUM_XCD + xcd


def nt_half_tiles(M, N):
    tiles_n = _cdiv(N, PB)
    tm128, tm256 = _cdiv(M, 128), _cdiv(M, PB)
    if _cdiv(tm128, NUM_XCD) * tiles_n > BLOCKS_PER_XCD:
        return False
    g = min(BLOCKS_PER_XCD // (_cdiv(tm256, NUM_XCD) * tiles_n), max(64 // (tm256 * tiles_n), 2))
    return g <= 2


EPILOGUES = ("plain", "addend", "mask", "addend_mask", "bits", "pool_mask", "pool_bits", "pool")


def nt_route(M, N, K, epilogue="plain"):
    """(half, read_bits) of an fp32-A launch: the part of nt_route that picks the tile height and whether a dgrad reads the one-bit image."""
    assert epilogue in EPILOGUES
    addend = epilogue.startswith("addend")
    pool = epilogue.startswith("pool")
    mask_src = epilogue.endswith("mask") or epilogue.endswith("bits")
    mask_bits = epilogue.endswith("bits")
    half = (not addend) and (not pool or mask_src) and nt_half_tiles(M, N)
    read_bits = mask_bits
    if mask_bits and not half and K // BK < 2:
        tiles_m, tiles_n = _cdiv(M, PB), _cdiv(N, PB)
        if any(nt_plan(x, tiles_m, tiles_n, 2).g > 1 for x in range(NUM_XCD)):
            read_bits = False
    return half, read_bits


LaunchPlan = namedtuple("LaunchPlan", "half fixup xcd tiles_m tiles_n nk stagger")     # xcd: [NtPlan] as the kernel uses them


def launch_plan(M, N, K, half):
    """What launch_nt_h2 launches: the per-XCD plans its workgroups walk (half-height launches never split), the fix-up instantiation (0 = none)
    and whether the workgroups start staggered."""
    tiles_n, nk = _cdiv(N, PB), K // BK
    tiles_m = _cdiv(M, 128) if half else _cdiv(M, PB)
    plans = []
    for x in range(NUM_XCD):
        p = nt_plan(x, tiles_m, tiles_n, nk)
        plans.append(p._replace(g=(1 if p.rem > 0 else 0)) if half else p)
    max_rem = max([p.rem for p in plans if p.g > 1], default=0)
    rem_all = sum(p.rem for p in plans if p.g > 1)
    fixup = 0 if max_rem == 0 else (4 if rem_all > 8 else 1)
    return LaunchPlan(half, fixup, plans, tiles_m, tiles_n, nk, _cdiv(M, PB) * tiles_n >= STAGGER_TILES)


def walk(lp):
    """gemm_nt_h2_big_kernel's work list: every item of every workgroup, in the order the workgroup runs them."""
    items = []
    for b in range(PB_GRID):
        xcd, j = b % NUM_XCD, b // NUM_XCD
        p = lp.xcd[xcd]
        for i in range(p.rounds):
            q = j + i * BLOCKS_PER_XCD
            items.append(Item(b, xcd, nt_row_tile(q, lp.tiles_n, xcd), q % lp.tiles_n, 0, lp.nk, None))
        if j < p.rem * p.g:
            q = p.rounds * BLOCKS_PER_XCD + j // p.g
            part = j % p.g
            items.append(Item(b, xcd, nt_row_tile(q, lp.tiles_n, xcd), q % lp.tiles_n, (part * lp.nk) // p.g, ((part + 1) * lp.nk) // p.g,
                              part if p.g > 1 else None))
    return items


def tile_slices(lp):
    """{(row tile, column tile): [(k0, k1), ...] in slice order}. A slice's slab is the one of its workgroup; the fix-up reads slab
    xcd + 8 (tr g + p) for slice p of the XCD's tr-th remainder tile - the workgroup the walk gave it to (asserted)."""
    out = {}
    for it in walk(lp):
        out.setdefault((it.row_tile, it.col_tile), []).append(it)
    res = {}
    for key, its in out.items():
        its.sort(key=lambda t: -1 if t.part is None else t.part)
        for it in its:
            if it.part is not None:
                p = lp.xcd[it.xcd]
                tr = (it.wg // NUM_XCD) // p.g
                assert it.wg == it.xcd + NUM_XCD * (tr * p.g + it.part)
        res[key] = [(it.k0, it.k1) for it in its]
    return res


def plan_facts(M, N, K, epilogue="plain"):
    half, read_bits = nt_route(M, N, K, epilogue)
    lp = launch_plan(M, N, K, half)
    split = [p for p in lp.xcd if p.g > 1]
    tiles_m256, tiles_n, nk = _cdiv(M, PB), lp.tiles_n, lp.nk
    rem_all_nat = sum(_xcd_tiles(x, tiles_m256, tiles_n) % BLOCKS_PER_XCD for x in range(NUM_XCD))
    natural = [nt_natural_g(_xcd_tiles(x, tiles_m256, tiles_n) % BLOCKS_PER_XCD, rem_all_nat, nk) for x in range(NUM_XCD)]
    nk_capped = any(nt_natural_g(_xcd_tiles(x, tiles_m256, tiles_n) % BLOCKS_PER_XCD, rem_all_nat, 1 << 20) > nk for x in range(NUM_XCD))
    wg_busy = {it.wg for it in walk(lp)}
    return dict(half=half, read_bits=read_bits, fixup=lp.fixup, stagger=lp.stagger, plans=lp.xcd,
                gs=sorted({p.g for p in split}), xcds_split=len(split), rem_all=sum(p.rem for p in split),
                rounds=sorted({p.rounds for p in lp.xcd}), uneven=any(nk % p.g for p in split), one_stage=bool(split) and all(nk == p.g for p in split),
                whole_rem=[p.rem for p in lp.xcd if p.g == 1], natural=natural, nk_capped=nk_capped, all_busy=len(wg_busy) == PB_GRID,
                last_rows=M - (lp.tiles_m - 1) * (128 if half else PB))


def regimes(M, N, K, epilogue="plain"):
    """The set of regime names the restated plan puts a launch of (M, N, K) with this epilogue in."""
    f = plan_facts(M, N, K, epilogue)
    out = set()
    out.add("half" if f["half"] else "full")
    out.add("fixup%d" % f["fixup"])
    for g in f["gs"]:
        out.add("g%d" % g)
    if len(f["gs"]) == 1 and 0 < f["xcds_split"]:
        out.add("g%d_on_%d" % (f["gs"][0], f["xcds_split"]))
    if f["uneven"]:
        out.add("uneven")
    if f["one_stage"]:
        out.add("one_stage")
    if f["gs"] and f["nk_capped"]:
        out.add("nk_limits_g")
    if not f["half"] and not f["gs"] and K // BK == 1 and any(p.rem for p in f["plans"]):
        out.add("one_stage_whole")
    if not f["half"] and not f["gs"] and K // BK >= 2 and any(n > 1 for n in f["natural"]):
        out.add("slowest_off")
    if any(p.rounds for p in f["plans"]) and f["gs"]:
        out.add("round_plus_rem")
    if not f["half"] and f["rounds"] != [0] and all(p.rem == 0 for p in f["plans"]):
        out.add("exact_rounds")
    if f["gs"] and len({p.g for p in f["plans"] if p.tiles}) > 1:            # XCDs of one launch run different plans
        out.add("mixed")
    if f["stagger"]:
        out.add("stagger")
    if f["all_busy"]:
        out.add("all_busy")
    if N % PB:
        out.add("partial_cols")
    if f["last_rows"] == 1:
        out.add("last_tile_one_row")
    if epilogue.endswith("bits") and not f["read_bits"]:
        out.add("bits_not_read")
    return out


# ---- the shapes of tests/test_gpu_nt_plans.py: (regimes the row is there for, (M, N, K), extra facts) -------------------------------------------------
# "full": the whole set of modes and integer families runs on this row (one per regime); the other rows run the two plain forwards on small_int,
# pow2_blocks and late_outlier_int.
Case = namedtuple("Case", "want M N K full facts")
CASES = [
    Case({"g16", "one_stage", "fixup1"}, 1, 512, 512, True, dict(rem_all=2)),
    Case({"g16", "one_stage", "fixup1"}, 255, 512, 512, False, {}),
    Case({"g16", "one_stage", "fixup1"}, 256, 512, 512, False, {}),
    Case({"g16", "one_stage", "fixup1"}, 257, 512, 512, False, dict(rem_all=4)),
    Case({"g16", "uneven"}, 1, 512, 768, True, {}),
    Case({"g10", "uneven"}, 513, 512, 768, True, dict(rem_all=6)),
    Case({"g8"}, 769, 512, 768, False, {}),
    Case({"g6", "fixup4"}, 1025, 512, 768, True, dict(rem_all=10)),
    Case({"g5", "uneven"}, 1281, 512, 768, False, {}),
    Case({"g4_on_7"}, 1537, 512, 768, False, {}),
    Case({"g4_on_8"}, 1793, 512, 768, False, {}),
    Case({"g3"}, 2049, 512, 768, True, dict(xcd0_tiles=4)),
    Case({"g2", "nk_limits_g"}, 1, 512, 64, False, {}),
    Case({"one_stage_whole", "fixup0"}, 1, 512, 32, True, {}),
    Case({"full", "g3"}, 2560, 512, 512, False, {}),
    Case({"half", "last_tile_one_row"}, 2561, 512, 512, True, {}),
    Case({"half"}, 2688, 512, 512, False, dict(last_rows=128)),
    Case({"half", "last_tile_one_row"}, 2689, 512, 512, False, {}),
    Case({"half", "fixup0"}, 16384, 512, 64, False, {}),
    Case({"slowest_off", "fixup0", "full"}, 16385, 512, 64, True, dict(xcd0_tiles=18)),
    Case({"exact_rounds", "fixup0"}, 32513, 512, 64, False, {}),
    Case({"round_plus_rem", "g16_on_1", "mixed"}, 32769, 512, 768, True, {}),
    Case({"round_plus_rem", "g10"}, 33281, 512, 768, False, {}),
    Case({"round_plus_rem", "g2"}, 34817, 512, 64, False, {}),
    Case({"round_plus_rem", "g3"}, 34817, 512, 96, False, {}),
    Case({"mixed", "g2_on_1", "round_plus_rem"}, 20481, 768, 64, True, {}),
    Case({"stagger", "exact_rounds"}, 65281, 512, 64, False, {}),
    Case({"stagger", "round_plus_rem"}, 65537, 512, 64, True, {}),
    Case({"stagger", "round_plus_rem"}, 67329, 512, 64, False, {}),
    Case({"partial_cols"}, 300, 4, 64, False, {}),
    Case({"partial_cols", "g16"}, 300, 260, 512, True, {}),
    Case({"g8"}, 1, 1024, 512, False, {}),
    Case({"half"}, 6145, 1024, 64, False, {}),                   # 49 half-height row tiles: 28 workgroups busy on XCD 0, 24 on the others
    Case({"all_busy", "half"}, 8065, 1024, 64, False, {}),       # (the smallest M at N = 1024 whose 128-row tiles fill all 32 workgroups of every XCD)
    Case({"half"}, 1793, 768, 512, False, {}),
]
ADDEND_CASE = Case({"full", "g2"}, 10000, 512, 768, True, {})       # dgrad with an addend buffer INSIDE the half-tile range: stays on 256-row tiles
HALF_RANGE = {256: (5377, 32768), 512: (2561, 16384), 768: (1793, 10240), 1024: (1281, 8192)}       # N: first, last M on half-height tiles
REAL_CASES = [(257, 512, 512), (2561, 512, 512), (32769, 512, 768)]                                # g = 16, half-height, round + remainder
REAL_FAMILIES = ("randn", "decades", "late_giant")
SLIDE_NS = [257, 2561, 16385, 33025]
EMU_MAX_ROWS = 2561
CASE_SEED, REAL_SEED = 300, 1300


# ---- operand families ------------------------------------------------------------------------------------------------------------------------
INT_FAMILIES = ("small_int", "two_piece_int_a", "two_piece_int_w", "pow2_blocks", "late_outlier_int")
LIGHT_FAMILIES = ("small_int", "pow2_blocks", "late_outlier_int")        # the rows that are not `full`
INT_SIDE_MAX = 1000
# the modes of tests/test_gpu_nt_plans.py: the epilogue that decides the route (nt_route), and how the A operand gets its scales
MODES = ("fwd_given", "fwd_self", "fwd_bias_relu", "fwd_drop", "dgrad_plain", "dgrad_addend_mask", "dgrad_bits")
DROP_P, DROP_SEED = 0.5, 0x5EED0F7E57            # keep factor 2: exact
LIGHT_MODES = ("fwd_given", "fwd_self")
MODE_ROUTE = {"fwd_given": "plain", "fwd_self": "plain", "fwd_bias_relu": "plain", "fwd_drop": "plain", "dgrad_plain": "plain", "dgrad_addend_mask": "addend_mask",
              "dgrad_bits": "bits"}
MODE_OPERAND = {"fwd_given": "given", "fwd_self": "self", "fwd_bias_relu": "self", "fwd_drop": "given", "dgrad_plain": "given", "dgrad_addend_mask": "given",
                "dgrad_bits": "given"}                    # (the plain dgrad is handed dy_amax - without it the entry point measures dY inside the GEMM like a
                                                          #  forward; a masked dgrad without it measures dY with a pass of its own: the same array)


def mode_epilogue(mode, bias, addend, src):
    """Keyword arguments of ref_f64 / emulate_nt for a mode; src: the ReLU output the two masked dgrads mask with (mask_scale 2: exact).
    fwd_drop: bias, ReLU and train-mode dropout with p = 0.5 from the host statement of the stream (tests/drop_ref.py), x_amax given."""
    if mode == "fwd_bias_relu":
        return dict(bias=bias, relu=True)
    if mode == "fwd_drop":
        m, n = addend.shape
        return dict(bias=bias, relu=True, keep=drop_ref.keep(m * n, DROP_P, DROP_SEED).reshape(m, n))
    if mode == "dgrad_addend_mask":
        return dict(addend=addend, mask_src=src, mask_scale=2.0)
    if mode == "dgrad_bits":
        return dict(mask_src=src, mask_scale=2.0)
    return {}


def case_families(case):
    """The integer families a row of the table runs: all of them (and all modes) on the `full` rows of at most EMU_MAX_ROWS rows, the three cheap
    ones on the others (the two-piece families need a float64 product per reference and add nothing a longer operand could show)."""
    return INT_FAMILIES if case.full and case.M <= EMU_MAX_ROWS else LIGHT_FAMILIES


def mode_sides(family, M, N, seed):
    """(bias, addend) of a family: integers, or zeros for pow2_blocks (anything else would round against its scaled values)."""
    if family == "pow2_blocks":
        return np.zeros((N,), dtype=np.float32), np.zeros((M, N), dtype=np.float32)
    return int_sides(M, N, seed)


def _small(g, rows, cols):
    t = g.integers(-7, 8, size=(rows, cols)).astype(np.float32)
    t[0, g.integers(0, cols)] = 8.0
    t[rows - 1, g.integers(0, cols)] = -8.0 if rows > 1 else 8.0
    t[rows - 1, cols - 1] = 8.0
    return t


def _sparse_pm1(g, rows, cols):
    """{-1, 0, 1} with at most 8 non-zeros per row, half of them next to a multiple of 32 (stage edges); the first and last column are reached."""
    t = np.zeros((rows, cols), dtype=np.float32)
    n = min(6, cols)                                  # + the two forced corners below (both in the only row of a one-row operand): at most 8
    free = g.integers(0, cols, size=(rows, 4))
    edge = np.clip(32 * g.integers(0, _cdiv(cols, 32) + 1, size=(rows, 4)) + g.integers(-1, 2, size=(rows, 4)), 0, cols - 1)
    idx = np.concatenate([free, edge], axis=1)[:, :n]
    np.put_along_axis(t, idx, g.choice([-1.0, 1.0], size=idx.shape).astype(np.float32), axis=1)
    t[0, 0] = 1.0
    t[rows - 1, cols - 1] = -1.0
    return t


def _bits20(g, rows, cols):
    top = (1 << 20) - 1
    t = (g.integers(0, top + 1, size=(rows, cols)) * g.choice([-1, 1], size=(rows, cols))).astype(np.float32)
    t[0, 0] = top
    t[rows - 1, cols - 1] = -top
    return t


def _alternating_exps(g, n):
    """n exponents in [-30, 30], neighbours at least 20 apart, alternating low / high (so every interior entry has a smaller AND a larger neighbour
    ... of its pair: low in [-30, -10], high in [10, 30])."""
    lo, hi = g.integers(-30, -9, size=n), g.integers(10, 31, size=n)
    par = (np.arange(n) + int(g.integers(0, 2))) % 2
    return np.where(par == 0, lo, hi).astype(np.int64)


def pow2_exps(M, N, seed):
    g = np.random.default_rng(seed + 77)
    return _alternating_exps(g, nblk(M)), _alternating_exps(g, N)


def int_operands(family, M, N, K, seed):
    """(A [M,K], W [N,K]) fp32."""
    g = np.random.default_rng(seed + INT_FAMILIES.index(family))
    if family == "two_piece_int_a":
        return _bits20(g, M, K), _sparse_pm1(g, N, K)
    if family == "two_piece_int_w":
        return _sparse_pm1(g, M, K), _bits20(g, N, K)
    a, w = _small(g, M, K), _small(g, N, K)
    if family == "late_outlier_int":
        a[:, K - 32:] *= np.float32(4096.0)
    elif family == "pow2_blocks":
        eb, fn = pow2_exps(M, N, seed)
        a *= np.exp2(np.repeat(eb, PB)[:M]).astype(np.float32).reshape(-1, 1)
        w *= np.exp2(fn).astype(np.float32).reshape(-1, 1)
    elif family != "small_int":
        raise ValueError(family)
    return a, w


def int_sides(M, N, seed):
    """Integer bias [N] and addend [M,N] in [-1000, 1000] (zeros for pow2_blocks: the caller leaves them out there)."""
    g = np.random.default_rng(seed + 55)
    return g.integers(-INT_SIDE_MAX, INT_SIDE_MAX + 1, size=(N,)).astype(np.float32), g.integers(-INT_SIDE_MAX, INT_SIDE_MAX + 1, size=(M, N)).astype(np.float32)


def _abs_sum_bound(a, w):
    """>= max_mn sum_k |a_mk w_nk| without the product: (largest absolute row sum of A) x max |W|, or the mirror, whichever is smaller."""
    ra, rw = np.abs(a).astype(np.float64).sum(1).max(), np.abs(w).astype(np.float64).sum(1).max()
    return min(ra * float(np.abs(w).max()), rw * float(np.abs(a).max()))


def _ints(t):
    return bool(np.array_equal(t, np.rint(t)))


def int_ok(family, a, w, M=None, N=None, seed=None):
    """The family's precondition on the very operands."""
    side = 2 * INT_SIDE_MAX
    if family == "small_int":
        return _ints(a) and _ints(w) and np.abs(a).max() == 8 and np.abs(w).max() == 8 and _abs_sum_bound(a, w) + side < 2 ** 24
    if family in ("two_piece_int_a", "two_piece_int_w"):
        big, sp = (a, w) if family == "two_piece_int_a" else (w, a)
        return (_ints(big) and np.abs(big).max() == (1 << 20) - 1 and set(np.unique(sp)) <= {-1.0, 0.0, 1.0} and (sp != 0).sum(1).max() <= 8
                and 8 * ((1 << 20) - 1) + side < 2 ** 24)
    if family == "late_outlier_int":
        K = a.shape[1]
        head, tail = a[:, :K - 32], a[:, K - 32:] / np.float32(4096.0)
        return (K <= 1024 and _ints(a) and _ints(w) and np.abs(head).max(initial=0) <= 8 and np.abs(tail).max() == 8 and _ints(tail)
                and np.abs(w).max() == 8 and _abs_sum_bound(a, w) + side < 2 ** 24)
    if family == "pow2_blocks":
        eb, fn = pow2_exps(M, N, seed)
        a0 = a.astype(np.float64) * np.exp2(-np.repeat(eb, PB)[:a.shape[0]]).reshape(-1, 1)
        w0 = w.astype(np.float64) * np.exp2(-fn).reshape(-1, 1)
        apart = (np.abs(np.diff(eb)) >= 20).all() and (np.abs(np.diff(fn)) >= 20).all() and np.abs(eb).max() <= 30 and np.abs(fn).max() <= 30
        return bool(apart and _ints(a0) and _ints(w0) and np.abs(a0).max() == 8 and np.abs(w0).max() == 8 and _abs_sum_bound(a0, w0) < 2 ** 24)
    raise ValueError(family)


def ref_f64(a, w, bias=None, addend=None, relu=False, keep=None, mask_src=None, mask_scale=1.0):
    y = a.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        y = y + bias.astype(np.float64)
    if addend is not None:
        y = y + addend.astype(np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    if keep is not None:
        y = y * keep.astype(np.float64)
    if mask_src is not None:
        y = np.where(mask_src > 0, y * mask_scale, 0.0)
    return y


def ref_exact(family, a, w, **epi):
    """The exact result as fp32 (asserted representable): int64 for the plain integer families, an integer times a power of two for pow2_blocks."""
    y = ref_f64(a, w, **epi)                     # float64 products and sums of these operands are exact: < 2^53 in units of the smallest term
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    if family != "pow2_blocks":
        assert np.array_equal(y, np.rint(y))
    return y32


def real_family(name, M, N, K, seed):
    """randn; decades: every row of each operand times 10^uniform(-4, 4); late_giant: row M - 1 and column K - 1 of A and row N - 1 of W times 1e4
    (a block scale taken without the last row, or an item scale that never meets the last column, overflows there)."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((M, K)).astype(np.float32)
    w = g.standard_normal((N, K)).astype(np.float32)
    if name == "decades":
        a *= (10.0 ** g.uniform(-4, 4, size=(M, 1))).astype(np.float32)
        w *= (10.0 ** g.uniform(-4, 4, size=(N, 1))).astype(np.float32)
    elif name == "late_giant":
        a[M - 1] *= np.float32(1e4)
        a[:, K - 1] *= np.float32(1e4)
        w[N - 1] *= np.float32(1e4)
    elif name != "randn":
        raise ValueError(name)
    return a, w


def real_sides(M, N, seed):
    g = np.random.default_rng(seed + 55)
    return g.standard_normal((N,)).astype(np.float32), g.standard_normal((M, N)).astype(np.float32)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------
def _pow2(e):
    return np.exp2(np.asarray(e, dtype=np.float64)).astype(np.float32)


def row_exps(w):
    return np.array([h2_exp_from_amax(v) for v in np.abs(w).max(1)], dtype=np.int64)


def emulate_nt(a, w, lp, mode="given", bias=None, addend=None, relu=False, keep=None, mask_src=None, mask_scale=1.0):
    """(Y, y_amax, info) fp32 as the kernels form them under launch plan `lp`. mode: "given" (abs-max array of A) or "self" (AMODE 3).
    Each slice's three terms are fp32 matrix products summed m.h + h.m + h.h: AN fp32 order, not the MFMA's - integers must not care and the
    bound covers any. Rows no item stores stay NaN. info: items, poisoned items, exact_split (h + m == u everywhere, finite)."""
    M, K = a.shape
    N = w.shape[0]
    TM = 128 if lp.half else PB
    kb = row_exps(w)
    with np.errstate(over="ignore", invalid="ignore"):
        hw, mw, uw = h2_split(w, kb.reshape(-1, 1))
        exact = bool(np.array_equal(hw.astype(np.float64) + mw.astype(np.float64), uw))
        hw, mw = hw.astype(np.float32), mw.astype(np.float32)
        amax = amax_rows256(a)
        y = np.full((M, N), np.nan, dtype=np.float32)
        n_items = n_poisoned = 0
        for (tm, tn), sl in sorted(tile_slices(lp).items()):
            r0, r1, c0, c1 = tm * TM, min(M, (tm + 1) * TM), tn * PB, min(N, (tn + 1) * PB)
            if r0 >= M:
                continue
            blk = r0 // PB
            slabs, kes = [], []
            for k0, k1 in sl:
                ar = a[r0:r1, k0 * BK:k1 * BK]
                n_items += 1
                if mode == "given":
                    ke = h2_exp_from_amax(amax[blk])
                else:
                    ke = h2_exp_from_amax(np.abs(ar[:, :BK]).max()) - RUN_MARGIN
                    fin = np.abs(ar).max()
                    if h2_exp_from_amax(fin) < ke - 1:
                        n_poisoned += 1                           # ... and re-run with the exponent of its true maximum
                        ke = h2_exp_from_amax(fin)
                ha, ma, ua = h2_split(ar, ke)
                exact = exact and bool(np.array_equal(ha.astype(np.float64) + ma.astype(np.float64), ua)) and bool(np.isfinite(ha.astype(np.float32)).all())
                ha, ma = ha.astype(np.float32), ma.astype(np.float32)
                hb, mb = hw[c0:c1, k0 * BK:k1 * BK], mw[c0:c1, k0 * BK:k1 * BK]
                slabs.append((ma @ hb.T + ha @ mb.T) + ha @ hb.T)
                kes.append(ke)
            if len(sl) == 1:
                v, kt = slabs[0], kes[0]
            else:
                kt = h2_exp_from_amax(amax[blk])
                f = [_pow2(max(kt - ke, -126)) if mode == "self" else np.float32(1.0) for ke in kes]
                v = slabs[0] * f[0] if mode == "self" else slabs[0]
                for s_, f_ in zip(slabs[1:], f[1:]):
                    v = v + (s_ * f_ if mode == "self" else s_)
            e1 = (-kt) >> 1
            f2 = _pow2(np.clip(-kt - e1 - kb[c0:c1], -126, 127)).reshape(1, -1)
            x = (v * _pow2(e1)) * f2
            if bias is not None:
                x = x + bias[c0:c1].reshape(1, -1)
            if addend is not None:
                x = x + addend[r0:r1, c0:c1]
            if relu:
                x = np.where(x > 0, x, np.float32(0.0))
            if keep is not None:
                x = x * keep[r0:r1, c0:c1]
            if mask_src is not None:
                x = np.where(mask_src[r0:r1, c0:c1] > 0, x * np.float32(mask_scale), np.float32(0.0))
            y[r0:r1, c0:c1] = x.astype(np.float32)
        y_amax = np.array([np.nanmax(np.abs(y[b * PB:(b + 1) * PB])) if np.isfinite(y[b * PB:(b + 1) * PB]).any() else 0.0 for b in range(nblk(M))],
                          dtype=np.float32)
    return y, y_amax, dict(items=n_items, poisoned=n_poisoned, exact_split=exact)


def exact_amax(y):
    return amax_rows256(y)


def bound_coeffs(K, g, mode):
    """(c1, c2) of |err_mn| <= c1 (sum_k |a w| + |bias| + |addend|) + c2 K A_b B_n - the docstring derives them."""
    d = 3 * K + g + 3
    return 3.01 * 2.0 ** -22 + 1.01 * _gamma(d, U32_MFMA), (2.0 ** -35 if mode == "given" else 2.0 ** -32)


def nt_bound(a, w, g, mode, bias=None, addend=None):
    """[M,N] float64 bound of |Y - epi(A W^T)| per element; g: the largest number of K-slices of any tile of the launch."""
    M, K = a.shape
    c1, c2 = bound_coeffs(K, max(g, 1), mode)
    s = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    if bias is not None:
        s = s + np.abs(bias).astype(np.float64)
    if addend is not None:
        s = s + np.abs(addend).astype(np.float64)
    ab = np.repeat(amax_rows256(a).astype(np.float64), PB)[:M].reshape(-1, 1)
    bn = np.abs(w).astype(np.float64).max(1).reshape(1, -1)
    return c1 * s + c2 * K * ab * bn


def deep_last_slice(lp):
    """True when some item holds the LAST stage of the reduction behind at least one other stage (what late_outlier_int needs to poison it)."""
    return any(sl[-1][1] - sl[-1][0] >= 2 for sl in tile_slices(lp).values())


def max_g(lp):
    return max([p.g for p in lp.xcd], default=1)
