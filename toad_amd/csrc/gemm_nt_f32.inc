// gemm_nt_f32.inc — part of the single translation unit gemm_f32.hip (included inside namespace toad; without -fgpu-rdc a kernel
// and its launcher must share a TU): generic 128x128 NT kernel, the exact-fp32 persistent 256x256 NT kernel, the shared tile plan / epilogue helpers, the K-split fix-up.
// ------------------------------------------------------------------------------------------
// NT: C[M,N] = epi(A[M,K] B[N,K]^T);   epi: +bias[col], +addend[row,col], relu, mask(mask_src>0)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void gemm_nt_f32_kernel(
    const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb,
    float *C, int64_t ldc, int M, int N, int K,
    const float *__restrict__ bias, EpiScalars es, const float *addend, const float *__restrict__ mask_src,
    int tiles_m, int tiles_n) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int relu = es.relu;
    int tm, tn;
    if (!map_tile(tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x;
    const int c4 = tid & 7, r0 = tid >> 3;     // staging: float4 column, first row
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, hi = lane >> 5;

    const float *ap[4], *bp[4];
    bool aok[4], bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ra = m0 + r0 + 32 * j, rb = n0 + r0 + 32 * j;
        aok[j] = ra < M;
        bok[j] = rb < N;
        ap[j] = A + (int64_t)(aok[j] ? ra : 0) * lda + c4 * 4;
        bp[j] = B + (int64_t)(bok[j] ? rb : 0) * ldb + c4 * 4;
    }
    f32x4 ra[4], rb[4];
    auto gload = [&](int k0) {
        const bool kok = (k0 + c4 * 4) < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ra[j] = (aok[j] && kok) ? ld4(ap[j] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[j] = (bok[j] && kok) ? ld4(bp[j] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lstore = [&](int buf) {
        float *As = smem + buf * 2 * NT_TILE, *Bs = As + NT_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st4(As + (r0 + 32 * j) * NT_LD + c4 * 4, ra[j]);
            st4(Bs + (r0 + 32 * j) * NT_LD + c4 * 4, rb[j]);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // Fragment pipeline: the four 8-deep k-groups of a tile are read one group ahead of the MFMAs
    // that consume them, and the tile barrier sits BEFORE the last group's MFMAs, so the first
    // fragments of the next tile are fetched under 16 MFMAs (1024 issue cycles) as well. A wave
    // therefore never waits on LDS latency with an empty matrix pipe; it parks only for barrier skew.
    struct Frag { f32x4 a0, a1, b0, b1; };
    const int frag_off_a = (wm * 64 + li) * NT_LD + hi * 4;
    const int frag_off_b = NT_TILE + (wn * 64 + li) * NT_LD + hi * 4;
    auto fread = [&](int buf, int q) {
        const float *base = smem + buf * 2 * NT_TILE;
        Frag f;
        f.a0 = ld4(base + frag_off_a + q * 8);
        f.a1 = ld4(base + frag_off_a + 32 * NT_LD + q * 8);
        f.b0 = ld4(base + frag_off_b + q * 8);
        f.b1 = ld4(base + frag_off_b + 32 * NT_LD + q * 8);
        return f;
    };
    auto mma16 = [&](const Frag &f) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a0[s], f.b0[s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a0[s], f.b1[s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a1[s], f.b0[s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a1[s], f.b1[s], acc[1][1], 0, 0, 0);
        }
    };

    const int nk = (K + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    Frag f0 = fread(0, 0);
    for (int t = 0; t < nk; ++t) {
        const bool more = (t + 1) < nk;
        const int buf = t & 1;
        if (more) gload((t + 1) * BK);
        // sched_barrier(0) pins "issue the next group's ds_reads, THEN this group's 16 MFMAs":
        // left alone, hipcc sinks the reads to just before their first use to save 16 VGPRs.
        Frag f1 = fread(buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma16(f0);
        __builtin_amdgcn_sched_barrier(0);
        Frag f2 = fread(buf, 2);
        __builtin_amdgcn_sched_barrier(0);
        mma16(f1);
        __builtin_amdgcn_sched_barrier(0);
        Frag f3 = fread(buf, 3);
        __builtin_amdgcn_sched_barrier(0);
        mma16(f2);
        __builtin_amdgcn_sched_barrier(0);
        if (more) lstore(buf ^ 1);
        __syncthreads();
        if (more) f0 = fread(buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mma16(f3);
        __builtin_amdgcn_sched_barrier(0);
    }

    // epilogue: acc reg r of lane (li,hi) is row (r&3)+8*(r>>2)+4*hi, column li of the 32x32 tile.
    // Rows are clamped (not branched) for the addend/mask loads so all 16 loads of a sub-tile are
    // issued back to back; only the stores are predicated.
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = n0 + wn * 64 + b * 32 + li;
        const bool cok = col < N;
        const int colc = cok ? col : N - 1;
        const float bv = bias ? bias[colc] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int rbase = m0 + wm * 64 + a * 32 + 4 * hi;
            float add[16], msk[16];
            if (addend) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = min(rbase + (r & 3) + 8 * (r >> 2), M - 1);
                    add[r] = addend[(int64_t)row * ldc + colc];
                }
            }
            if (mask_src) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = min(rbase + (r & 3) + 8 * (r >> 2), M - 1);
                    msk[r] = mask_src[(int64_t)row * ldc + colc];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2);
                float v = acc[a][b][r] + bv;
                if (addend) v += add[r];
                if (relu) v = v > 0.f ? v : 0.f;
                if (es.drop.thresh) v *= drop_keep((uint64_t)row * (uint64_t)N + (uint64_t)col, es.drop);
                if (mask_src) v = msk[r] > 0.f ? v * es.mask_scale : 0.f;
                if (cok && row < M) C[(int64_t)row * ldc + col] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// NT, persistent 256x256 (the fast path; K % 32 == 0)
//
// Why this shape. Ablations (tools/ubench/gemm_ablate.cpp) showed the 128x128 kernels pay ~10 % for
// operand staging even when the data is never waited for: a 128x128x32 step moves 32 KB per 1.05
// MFLOP = 8 B/clk/CU at full MFMA rate, against a ~10-11 B/clk/CU vector-memory path. A 256x256
// tile halves the bytes per FLOP (3.9 B/clk/CU) and needs 25 % fewer LDS fragment reads per MFMA.
//
//  * one persistent block of 8 waves per CU (grid = 256), waves 4(m) x 2(n), each 64x128 = 2x4
//    MFMA 32x32 accumulators (128 acc VGPRs);
//  * operands go HBM/L2 -> LDS by LDS-DMA (global_load_lds, 16 B/lane): no staging VGPRs, no
//    ds_write pass. LDS-DMA writes lane-linear, so the tile image is unpadded [256 pos][32 floats]
//    and bank conflicts are removed by an XOR swizzle applied to the SOURCE address and to the
//    fragment reads: 16-B chunk c of position p is stored at chunk c ^ ((p >> 1) & 7);
//  * the B image is column-interleaved: position 32b+li of a wave's 128 columns holds column
//    4li+b, so the four 32-wide MFMA sub-tiles of a lane are 4 CONSECUTIVE output columns and
//    the epilogue moves 16 B per lane (bias/addend/mask loads and the store);
//  * the k-loop runs across work items (the next item's first stage is in flight while the
//    epilogue of the current one drains); fragments are read one k-group ahead and the stage
//    barrier sits before the last group's MFMAs;
//  * tile quantisation: every XCD plans its own tiles (row tiles x, x+8, ...; all column tiles of a
//    row tile together). Full rounds are dealt to its 32 blocks; the REMAINDER tiles are split
//    along K into g = 32/R pieces whose raw accumulators go to fp32 slabs, summed in fixed order
//    (deterministic) by nt_fixup_kernel, which also applies the epilogue. Small bags (fewer tiles
//    than CUs) are parallelised by the same mechanism.
// ------------------------------------------------------------------------------------------
// (PB = 256, the tile edge, PB_BLOCKS_PER_XCD = 32 and PB_GRID: h2_arith.h)
constexpr int PB_TILE = PB * BK;                                // floats per operand stage
constexpr int PB_SMEM = 2 * 2 * PB_TILE * (int)sizeof(float);   // 131,072 B: one block per CU
#ifndef TOAD_PB_GMAX
#define TOAD_PB_GMAX 16
#endif
constexpr int PB_GMAX = TOAD_PB_GMAX;                           // max K-split of a remainder tile

typedef __attribute__((address_space(1))) const void *gptr_t;      // (lptr_t: h2_arith.h)

struct NtPlan { int mt_x, tiles, rounds, rem, g; };
// K-slices an XCD would cut its remainder tiles into on its own: as many as it has idle workgroups, at most nk / PB_GMAX, and - every slice costs a
// 256 KB slab written and read back by the fix-up - at most ~64 slabs per launch (measured, tools/ab_n.sh: 2,000 patches = 16 remainder tiles run 7 %
// faster with 4 slices than with 16; a 256-patch bag (2 tiles on one XCD) still wants all 16; from 10k patches on the per-XCD bound is the tighter one).
__host__ __device__ inline int nt_natural_g(int rem, int rem_all, int nk) {
    int g = rem > 0 ? PB_BLOCKS_PER_XCD / rem : 0;
    if (g > nk) g = nk;
    if (g > PB_GMAX) g = PB_GMAX;
    if (g > 2) {
        int cap = rem_all > 0 ? 64 / rem_all : g;
        if (cap < 2) cap = 2;
        if (g > cap) g = cap;
    }
    return g;
}
__host__ __device__ inline NtPlan nt_plan(int xcd, int tiles_m, int tiles_n, int nk) {
    NtPlan p;
    p.mt_x = (tiles_m - xcd + kNumXCD - 1) / kNumXCD;
    p.tiles = p.mt_x * tiles_n;
    p.rounds = p.tiles / PB_BLOCKS_PER_XCD;
    p.rem = p.tiles - p.rounds * PB_BLOCKS_PER_XCD;
    int rem_all = 0;
    for (int x = 0; x < kNumXCD; ++x) rem_all += (((tiles_m - x + kNumXCD - 1) / kNumXCD) * tiles_n) % PB_BLOCKS_PER_XCD;
    int g = nt_natural_g(p.rem, rem_all, nk);
    // Round 6: no XCD slices finer than the SLOWEST XCD makes useful. The launch lasts as long as its slowest XCD: rounds + 1/g tile times. When one
    // XCD holds a few more tiles than the others (16,500 rows x 512 columns: XCD 0 has 18 tiles -> whole tiles, the other seven 16 -> two slices each)
    // the seven finish early and idle, and their slices still cost slabs and the fix-up LAUNCH: that shape ran 11 % slower than 20,000 rows
    // (profiles/r06q_size_sweep.txt). Each XCD takes the smallest g that still ends with the slowest one (exact integer arithmetic in units of
    // 1 / lcm(1..16) tile times). Whether a remainder tile is split at all (g > 1) stays a function of the tile counts only for every nk >= 2 (a
    // one-stage reduction, nk = 1, cannot be split: such a dgrad does not read the ReLU bit image - nt_route, gemm_f32.hip; tests/test_relu_bits_plan.py).
    if (g > 1) {
        constexpr int LCM = 720720;
        int t_max = 0;
        for (int x = 0; x < kNumXCD; ++x) {
            const int t = ((tiles_m - x + kNumXCD - 1) / kNumXCD) * tiles_n, r = t / PB_BLOCKS_PER_XCD, m = t - r * PB_BLOCKS_PER_XCD;
            const int gx = nt_natural_g(m, rem_all, nk);
            const int tx = r * LCM + (m > 0 ? LCM / gx : 0);
            if (tx > t_max) t_max = tx;
        }
        int gg = 1;
        while (gg < g && p.rounds * LCM + LCM / gg > t_max) ++gg;
        g = gg;
    }
    p.g = g;
    return p;
}
// item q of an XCD's work list (its tiles, row-major over the row tiles this XCD owns) -> the row tile it computes; the column tile is q % tiles_n.
// Host and device: the persistent kernel places its tiles with it and the host-side bit-image query (nt_bits_tile_map, gemm_f32.hip) reports them.
__host__ __device__ inline int nt_row_tile(int q, int tiles_n, int xcd) { return (q / tiles_n) * kNumXCD + xcd; }

// shared by the GEMM (direct tiles) and the fix-up kernel (slab sums): v = one float4 of 4 consecutive columns.
// NOTE: bias/addend/mask are passed to the kernels as DIRECT pointer arguments. Inside a by-value struct
// hipcc does not infer the global address space, emits FLAT loads, and a pending FLAT access makes it
// put `s_waitcnt vmcnt(0) lgkmcnt(0)` in front of every LDS access that follows (found the hard way).
__device__ __forceinline__ f32x4 apply_epilogue(f32x4 v, const EpiScalars &e, const float *add_p, const float *msk_p, f32x4 bv,
                                                uint64_t flat_idx) {
    v += bv;
    if (add_p) v += ld4(add_p);
    if (e.relu) { v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f; v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f; }
    if (e.drop.thresh) {               // forward dropout after the activation
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= drop_keep(flat_idx + k, e.drop);
    }
    if (msk_p) {                       // backward: relu (and dropout) mask of the saved activation, times 1/(1-p)
        const f32x4 m = ld4(msk_p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = m[k] > 0.f ? v[k] * e.mask_scale : 0.f;
    }
    return v;
}

// same, with the addend / mask vectors already loaded
__device__ __forceinline__ f32x4 apply_epilogue_v(f32x4 v, const EpiScalars &e, f32x4 av, bool has_add, f32x4 mv, bool has_msk, f32x4 bv,
                                                  uint64_t flat_idx) {
    v += bv;
    if (has_add) v += av;
    if (e.relu) { v[0] = v[0] > 0.f ? v[0] : 0.f; v[1] = v[1] > 0.f ? v[1] : 0.f; v[2] = v[2] > 0.f ? v[2] : 0.f; v[3] = v[3] > 0.f ? v[3] : 0.f; }
    if (e.drop.thresh) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= drop_keep(flat_idx + k, e.drop);
    }
    if (has_msk) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = mv[k] > 0.f ? v[k] * e.mask_scale : 0.f;
    }
    return v;
}


