// gemm_stream.inc — part of the extractor's translation unit conv.hip (included inside namespace toad after gemm_narrow.inc, whose
// weight-plane format, ConvGeom and GATHER_* modes it shares).
// ------------------------------------------------------------------------------------------
// Narrow-N NT kernel with a STREAMED A operand (round 3).   C = act(A' W^T + bias + addend), N tile = 64 or 128 columns.
//
// The narrow kernel of gemm_narrow.inc stages raw fp32 A rows in LDS next to the weight planes. Its tiles give every wave only 32
// output rows, so each wave re-reads the whole 64/128-column weight fragment set for 12 MFMAs, and A crosses LDS twice (DMA in,
// fragment read out): at 16 waves per CU that is ~1,600 LDS cycles per k16 round against ~1,540 matrix-pipe cycles, plus one
// workgroup barrier per 32-deep stage (24 MFMAs per wave). The extractor's narrow convolutions ran at 0.33-0.46 of the power-capped
// matrix rate (profiles/r03k_extractor_kernel_stats.md).
//
// Here A never enters LDS. A 32x32x16 MFMA wants from lane (li, hi) eight consecutive k of row li - 32 contiguous bytes of the
// fp32 activation row - so every lane loads its own fragment straight from global memory into registers (two 16-B loads, TWO k16
// steps ahead: 1x1 convolutions read A exactly once, every load is an HBM miss), splits it into the two fp16 pieces there and feeds
// the matrix pipe. LDS holds only the pre-split weight planes: two buffers of two k-stages each, one barrier per FOUR k16 steps; the
// next buffer is filled through registers, a quarter per step, each piece riding two steps between its load and its LDS write (a
// weight piece is an L2 hit, 300-500 ns - longer than one step). Not by LDS-DMA: hipcc does not count DMA issued from inline
// assembly, so every wait it places for an A fragment would also drain the DMA issued just before it. Wave tile = 64 x 128
// (<RA, NB> = <2, 4>) or 64 x 64 (<2, 2>; 128 x 64 does not fit 256 registers next to the loads in flight): every weight fragment
// read from LDS feeds 2 row sub-tiles (6 MFMAs), LDS traffic per MFMA is 2.5x lower, and no A fragment is converted twice. 4 waves
// per workgroup, 2 (<2, 4>) or 3 (<2, 2>) workgroups per CU. k-stages are walked in pairs: an odd count gets one zero-weight stage.
//
// What this kernel is NOT good at: its loads are fragment-shaped - the 32 lanes of a fragment are 32 different rows, so every 16-B
// load is its own tag lookup and the vector L1 delivers ~16 B/clk instead of 64 (measured: DESIGN.md 10). Layers that read A once
// (1x1, the stem) are HBM-bound before that matters; a 3x3 puts 9x the activation through that path, which is why every stride-1
// 3x3 runs on the halo kernel below and only the two stride-2 ones here.
//
// Implicit convolution (MODE = GATHER_CONV): row m = output pixel, K = (ky, kx, c); a k-stage lies inside one tap, so per tap each
// lane holds ONE offset (its pixel shifted by the tap) and ONE scale. The k-stages run channel-chunk OUTER, tap INNER (the weight
// planes are split in that order, split_planes_narrow_h2_kernel's `taps` - the order the halo kernel needs, shared so that both take
// the same planes; it also puts the nine reads of a 128-B piece one stage apart instead of 2-8). Taps that fall outside the image
// read the (always valid) centre pixel and are multiplied by a scale of ZERO in the split (x * 0 -> h = m = 0), which costs nothing -
// the split multiplies by the operand's power-of-two scale anyway. GATHER_STEM: the 7x7/2 stem on the space-to-depth image (4 window
// rows x 48 floats). The reference computes these layers with cudnn convolutions (models/resnet_custom.py:19-119).
// ------------------------------------------------------------------------------------------
template <int RA, int NB> struct StreamCfg {
    static constexpr int WAVES = 4, THREADS = 256;
    static constexpr int TM = WAVES * RA * 32, TN = NB * 32;
    static constexpr int PL_BYTES = TN * BK * 2;               // one plane of one k-stage
    static constexpr int ST_BYTES = 2 * PL_BYTES;              // one k-stage: h plane, m plane (contiguous in the split image)
    static constexpr int KS = 2;                               // k-stages per LDS buffer
    static constexpr int BUF = KS * ST_BYTES, SMEM = 2 * BUF;  // <2,4>: 64 KB, <2,2>: 32 KB
    static constexpr int WG_PER_CU = RA * NB <= 4 ? 3 : 2;     // 64 accumulator registers per lane leave room for a third workgroup
};

// The epilogue of the streamed / halo kernels: wave `wave` of the block holds rows wave * RA * 32 ... of the tile at (m0, n0); lane (li, hi)
// holds columns NB * li ... of every 32-column block pair. acc = (sA * t_col) * (A . B^T).
template <int RA, int NB>
__device__ __forceinline__ void stream_epilogue(const f32x16 (&acc)[RA][NB], int m0, int n0, int wave, int li, int hi, int kea, const float *__restrict__ bias,
                                                const float *__restrict__ binv, const float *addend, float *C, int64_t ldc, int M, int N, int relu, float &amx) {
    typedef float fvec __attribute__((ext_vector_type(NB)));
    constexpr int EG = 4;                // rows per batch: consecutive rows of the tile (r = 4j .. 4j + 3), residual loads issued back to back
    int lic = NB * li, hi4 = 4 * hi;
    asm volatile("" : "+v"(lic), "+v"(hi4));
    const int col = n0 + lic;
    const bool cok = col < N;
    fvec bv, iv;
#pragma unroll
    for (int e = 0; e < NB; ++e) { bv[e] = 0.f; iv[e] = 1.f; }
    if (bias && cok) bv = *reinterpret_cast<const fvec *>(bias + col);
    if (cok) iv = *reinterpret_cast<const fvec *>(binv + col);
    const float f1 = h2_descale_first(kea);          // (acc * f1) * iv[c] = acc / (sA * t_col), two exact power-of-two factors
#pragma unroll
    for (int e = 0; e < NB; ++e) { const float ive = iv[e]; iv[e] = h2_descale_second(kea, -h2_exp_of_pow2(ive)); }
    asm volatile("" : "+v"(bv), "+v"(iv));
    const float floorv = relu ? 0.f : -__builtin_inff();
    const int colc = cok ? col : 0;
    auto rows = [&](auto add_tag) __attribute__((always_inline)) {
        constexpr bool HAS_ADD = decltype(add_tag)::value;
#pragma unroll
        for (int a = 0; a < RA; ++a) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row0 = m0 + wave * (RA * 32) + a * 32 + 8 * j + hi4;       // rows row0 .. row0 + 3 <-> accumulator registers 4j .. 4j + 3
                fvec av[EG];
                if (HAS_ADD) {
#pragma unroll
                    for (int g = 0; g < EG; ++g) av[g] = *reinterpret_cast<const fvec *>(addend + (int64_t)min(row0 + g, M - 1) * ldc + colc);
                    __builtin_amdgcn_sched_barrier(0);
                }
                float *dst = C + (int64_t)row0 * ldc + col;
#pragma unroll
                for (int g = 0; g < EG; ++g) {
                    fvec v;
#pragma unroll
                    for (int e = 0; e < NB; ++e) v[e] = acc[a][e][4 * j + g];
                    v = (v * f1) * iv + bv;
                    if (HAS_ADD) v += av[g];
#pragma unroll
                    for (int e = 0; e < NB; ++e) { const float ve = v[e]; v[e] = __builtin_fmaxf(ve, floorv); }
                    if (cok && row0 + g < M) {
#pragma unroll
                        for (int e = 0; e < NB; ++e) { const float ve = v[e]; amx = __builtin_fmaxf(amx, __builtin_fabsf(ve)); }
                        __builtin_nontemporal_store(v, reinterpret_cast<fvec *>(dst + (int64_t)g * ldc));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (addend) rows(std::true_type{}); else rows(std::false_type{});
}

// ------------------------------------------------------------------------------------------
// The stem with nn.MaxPool2d(3, 2, 1) in its epilogue (MODE = GATHER_STEM_POOL; models/resnet_custom.py:96-99 as one kernel, round 4).
// The stem's output (B x 128 x 128 x 64 fp32: 2.15 GB per 512 tiles) was written once and read once by a streaming pool kernel - 4.3 GB
// of HBM traffic around a tensor nobody else wants. Here a tile is two whole image rows (Wo = 128: rows 2t and 2t + 1 of one image, waves
// 0-1 / 2-3), and the pooled row t = max over conv rows 2t - 1 .. 2t + 1, columns 2x - 1 .. 2x + 1 is formed before anything is stored:
//   horizontally in registers - a lane holds four consecutive pixels of two channels per accumulator group; the one neighbour pixel a
//     window needs from the previous group sits in the partner lane (lane ^ 32), the previous wave's last pixel comes through LDS;
//   vertically through LDS - waves 0-1 park their pooled row (16 KB), waves 2-3 combine it with their own and with the CARRY, the pooled
//     conv row 2t - 1 the previous tile left in LDS, store the result (64 pixels x 64 channels, 256-byte runs) and leave their row as the
//     next carry.
// A workgroup therefore walks image rows top to bottom: it owns a contiguous range of tiles (images back to back), preceded by the tile above
// the range computed for its carry only (~2 % more matrix work); a tile that starts an image takes zeros for the carry - every window holds a
// real pixel and post-ReLU values are >= 0, so zero padding cannot win. Values are the max-pool of exactly the stem's outputs: bit-identical
// to the two-kernel path.
constexpr int STEM_POOL_LDS = 64 * 64 * 4 + 4 * 64 * 4;               // carry + one edge pixel per wave (the parked row borrows the weight buffer the tile just finished with)
// Workgroup barrier for exchanges that go through LDS only: waits for this wave's LDS operations, NOT for its global loads / stores.
// __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier - in the pooled stem kernels that made every tile wait for a full HBM round
// trip of the pooled row it had just stored (and of the next window's loads) at each of the epilogue's barriers.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// RC (stem_halo.inc, round 6): the carried row lives in REGISTERS - it is written and read by the same lane of waves 2-3 (cr[((a * 4 + j) * 2 + w) * 2 + c]), so it
// needs no LDS at all; `lds` then holds only the edge pixels (1 KB).
// `mid()` runs between the two halves - after the accumulators have been folded into the pooled row (they are dead from there on), before the vertical combine:
// stem_halo.inc issues the next tile's window loads there (round 6).
struct StemNoMid { __device__ __forceinline__ void operator()() const {} };
template <int RA, int NB, bool RC = false, typename Mid = StemNoMid>
__device__ __forceinline__ void stem_pool_epilogue(const f32x16 (&acc)[RA][NB], char *lds, float *rowA, int wave, int li, int hi, int kea, const float *__restrict__ bias,
                                                   const float *__restrict__ binv, float *Yp, int64_t prow, bool store_out, bool top, float &amx, float (&cr)[32],
                                                   Mid mid = Mid{}) {
    static_assert(RA == 2 && NB == 2 && StreamCfg<RA, NB>::BUF >= 64 * 64 * 4, "the pooled stem epilogue is written for the 64 x 64 wave tile");
    // rowA: 16 KB = the weight buffer whose chunk was this tile's last (the next tile's first chunk already sits in the other one; this one is
    // refilled from the next tile's first step on - hence the barrier at the end). Three workgroups per CU keep fitting (49 KB each): the stem is
    // bound by its fragment-shaped loads, and with two it ran 1,270 us per 512 tiles instead of 896 + 552 for the two kernels.
    float *carry = reinterpret_cast<float *>(lds), *edge = RC ? carry : carry + 64 * 64;
    typedef float f2 __attribute__((ext_vector_type(2)));
    const int col = 2 * li;
    const f2 bv = bias ? *reinterpret_cast<const f2 *>(bias + col) : f2{0.f, 0.f};
    f2 iv = *reinterpret_cast<const f2 *>(binv + col);
    const float f1 = h2_descale_first(kea);
    iv[0] = h2_descale_second(kea, -h2_exp_of_pow2(iv[0])); iv[1] = h2_descale_second(kea, -h2_exp_of_pow2(iv[1]));
    auto conv = [&](int a, int r) __attribute__((always_inline)) {        // relu(stem) of accumulator register r of row sub-tile a, channels col, col + 1
        f2 t = {acc[a][0][r], acc[a][1][r]};
        t = (t * f1) * iv + bv;
        t[0] = __builtin_fmaxf(t[0], 0.f); t[1] = __builtin_fmaxf(t[1], 0.f);
        return t;
    };
    // the pixel left of each four-pixel group is the last pixel of the previous group: held by the partner lane (lane ^ 32), or - first group of
    // an odd wave - the previous wave's last pixel, which comes through LDS
    if (hi == 1) *reinterpret_cast<f2 *>(edge + wave * 64 + col) = conv(1, 15);
    lds_barrier();
    f2 prev_a = {0.f, 0.f};                                      // image edge: padding (never wins against values >= 0)
    if (wave & 1) prev_a = *reinterpret_cast<const f2 *>(edge + (wave - 1) * 64 + col);
    const int px0 = (wave & 1) * 32 + 2 * hi;
    // hp[a][j][w]: pooled pixel px0 + a * 16 + 4 j + w of this image row (horizontal 3-window, stride 2); one row sub-tile at a time (registers)
    f2 hp[2][4][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        f2 v[4][4], r[4];        // v[j][g]: pixel (wave & 1) * 64 + a * 32 + 8 j + 4 hi + g
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v[j][g] = conv(a, 4 * j + g);
                amx = __builtin_fmaxf(amx, __builtin_fmaxf(v[j][g][0], v[j][g][1]));
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[j][0] = __shfl_xor(v[j][3][0], 32); r[j][1] = __shfl_xor(v[j][3][1], 32); }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f2 nb = hi ? r[j] : (j > 0 ? r[j - 1] : prev_a);
            hp[a][j][0][0] = __builtin_fmaxf(nb[0], __builtin_fmaxf(v[j][0][0], v[j][1][0]));
            hp[a][j][0][1] = __builtin_fmaxf(nb[1], __builtin_fmaxf(v[j][0][1], v[j][1][1]));
            hp[a][j][1][0] = __builtin_fmaxf(v[j][1][0], __builtin_fmaxf(v[j][2][0], v[j][3][0]));
            hp[a][j][1][1] = __builtin_fmaxf(v[j][1][1], __builtin_fmaxf(v[j][2][1], v[j][3][1]));
        }
        prev_a = r[3];
        if (wave < 2) {                                          // conv row 2t: park the pooled row for waves 2-3
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int w = 0; w < 2; ++w) *reinterpret_cast<f2 *>(rowA + (px0 + a * 16 + 4 * j + w) * 64 + col) = hp[a][j][w];
        }
    }
    mid();
    lds_barrier();
    if (wave >= 2) {                                             // conv row 2t + 1: combine with row 2t and the carry (row 2t - 1), store, become the carry
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const int px = px0 + a * 16 + 4 * j + w;
                    const int ci = ((a * 4 + j) * 2 + w) * 2;
                    if (store_out) {
                        const f2 ra = *reinterpret_cast<const f2 *>(rowA + px * 64 + col);
                        f2 rc;
                        if (RC) rc = top ? f2{0.f, 0.f} : f2{cr[ci], cr[ci + 1]};
                        else rc = top ? f2{0.f, 0.f} : *reinterpret_cast<const f2 *>(carry + px * 64 + col);
                        f2 o;
                        o[0] = __builtin_fmaxf(__builtin_fmaxf(ra[0], rc[0]), hp[a][j][w][0]);
                        o[1] = __builtin_fmaxf(__builtin_fmaxf(ra[1], rc[1]), hp[a][j][w][1]);
                        __builtin_nontemporal_store(o, reinterpret_cast<f2 *>(Yp + (prow * 64 + px) * 64 + col));
                    }
                    if (RC) { cr[ci] = hp[a][j][w][0]; cr[ci + 1] = hp[a][j][w][1]; }
                    else *reinterpret_cast<f2 *>(carry + px * 64 + col) = hp[a][j][w];
                }
    }
    lds_barrier();                                             // rowA is a weight buffer again
}

template <int RA, int NB, int MODE>
__global__ __launch_bounds__(256, (RA * NB <= 4 ? 3 : 2)) void gemm_nt_h2_stream_kernel(
    const float *__restrict__ A, int64_t lda, const float *__restrict__ a_gmax, const unsigned short *__restrict__ Bp,
    const float *__restrict__ binv, float *C, int64_t ldc, int M, int N, int K, const float *__restrict__ bias, int relu,
    const float *addend, ConvGeom cg, float *y_gmax, int tiles_m, int tiles_n) {
    using Cfg = StreamCfg<RA, NB>;
    constexpr int TM = Cfg::TM, TN = Cfg::TN, KS = Cfg::KS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hi = lane >> 5;
    const int nkr = K / BK, nk = (nkr + 1) & ~1, cpk = nk / KS; // real k-stages; stages walked (an odd count is padded with a zero-weight stage); weight chunks per tile
    constexpr bool STEM = MODE == GATHER_STEM || MODE == GATHER_STEM_POOL, POOLED = MODE == GATHER_STEM_POOL;

    // ---- work list: XCD x owns a contiguous range of tiles (row-major over (tile_m, tile_n)); slot s of the XCD's blocks takes
    // tiles s, s + bpx, ... of that range, so concurrently running tiles are neighbours in M (taps / column tiles share L2 lines)
    const int bpx = gridDim.x / kNumXCD;
    const int xcd = blockIdx.x % kNumXCD, slot = blockIdx.x / kNumXCD;
    const int tiles = tiles_m * tiles_n;
    const int t_lo = (int)(((int64_t)tiles * xcd) / kNumXCD), t_hi = (int)(((int64_t)tiles * (xcd + 1)) / kNumXCD);
    // POOLED: every workgroup takes a CONTIGUOUS range of tiles (= image row pairs, images back to back), so the carried row is always at hand;
    // item 0 is the tile above the range, computed for its carry only (2 % more matrix work at 43 tiles per workgroup)
    const int tpi = POOLED ? cg.Ho / 2 : 1;                              // tiles per image
    const int p_lo = POOLED ? (int)(((int64_t)tiles_m * blockIdx.x) / gridDim.x) : 0, p_hi = POOLED ? (int)(((int64_t)tiles_m * (blockIdx.x + 1)) / gridDim.x) : 0;
    if (POOLED ? p_hi <= p_lo : t_hi - t_lo <= slot) return;
    const int n_items = POOLED ? p_hi - p_lo + 1 : (t_hi - t_lo - slot + bpx - 1) / bpx;
    auto item_tile = [&](int i) { return POOLED ? max(p_lo + i - 1, 0) : t_lo + slot + i * bpx; };

    const char *Ab = reinterpret_cast<const char *>(A), *Bpb = reinterpret_cast<const char *>(Bp);
    const unsigned lane16 = lane * 16u;
    // weight chunk = k-stages 2c, 2c + 1 of column tile tn: BUF contiguous bytes of the split image. Piece p (1 KB) of the NEXT chunk is
    // moved by wave w in step j of the current one, p = (4 j + w) * PPS + i
    constexpr int PPS = Cfg::BUF / 1024 / 16;
    // Each piece rides in registers for TWO steps (loaded in step j - 2, written to LDS in step j): a weight piece is an L2 hit, 300-500 ns,
    // longer than one k16 step; with the store in the step of the load every step waited for it.
    f32x4 bst[2][PPS];
    // source of weight chunk number gi of this block's chunk sequence (tiles in order, cpk chunks each; past the end: the last one again)
    auto chunk_src = [&](int gi) __attribute__((always_inline)) {
        gi = min(gi, n_items * cpk - 1);
        const int it = gi / cpk, ck = gi - it * cpk;
        return Bpb + (int64_t)((item_tile(it) % tiles_n) * nk + ck * KS) * Cfg::ST_BYTES;
    };
    auto b_load = [&](const char *src, int j, int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPS; ++i) bst[slot][i] = ld4(reinterpret_cast<const float *>(src + ((4 * j + wave) * PPS + i) * 1024 + lane16));
    };
    auto b_store = [&](int buf, int j, int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPS; ++i)
            *reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(smem) + buf * Cfg::BUF + ((4 * j + wave) * PPS + i) * 1024 + lane16) = bst[slot][i];
    };

    // ---- A addressing: the cursor of the k16 step being LOADED runs one step ahead of the one being multiplied
    const int kea = __builtin_amdgcn_readfirstlane(h2_exp_from_amax(a_gmax[0]));     // ONE power-of-two scale for the whole operand (gemm_narrow.inc)
    const float sA = h2_pow2(kea);
    unsigned aoff[RA];                   // per-lane byte offset of the lane's row (CONV: of pixel (oy*s - p, ox*s - p), may wrap below 0) + hi * 32
    int ayx[MODE == GATHER_CONV ? RA : 1];
    unsigned voff[RA];                   // offset the loads of the current tap use
    float sa[RA];                        // scale the split of those loads uses (0 for a tap outside the image)
    struct Cur { int it, kt, s, ky, kx, c0; };
    auto set_rows = [&](int q) __attribute__((always_inline)) {
        const int m0 = (q / tiles_n) * TM;
#pragma unroll
        for (int a = 0; a < RA; ++a) {
            const int m = min(m0 + wave * (RA * 32) + a * 32 + li, M - 1);
            if (MODE == GATHER_CONV) {
                const int ox = m % cg.Wo, t = m / cg.Wo;
                const int oy = t % cg.Ho, b = t / cg.Ho;
                const int iy0 = oy * cg.stride - cg.pad, ix0 = ox * cg.stride - cg.pad;
                aoff[a] = (unsigned)((b * cg.H + iy0) * cg.W + ix0) * (unsigned)(cg.C * 4) + hi * 32;     // mod 2^32: a negative pixel index wraps and the tap offset brings it back
                ayx[a] = ((iy0 + 8) << 16) | (ix0 + 8);
            } else if (STEM) {                     // space-to-depth image Xs[b, Y, X, 12]: the window of pixel (oy, ox) starts at (oy, ox)
                const int ox = m % cg.Wo, t = m / cg.Wo;
                const int oy = t % cg.Ho, b = t / cg.Ho;
                aoff[a] = (unsigned)((b * cg.H + oy) * cg.W + ox) * 48u;
            } else {
                aoff[a] = (unsigned)m * (unsigned)(lda * 4) + hi * 32;
            }
            voff[a] = aoff[a];
            sa[a] = sA;
        }
    };
    auto set_tap = [&](const Cur &c) __attribute__((always_inline)) {
        if (MODE != GATHER_CONV) return;
        const unsigned toff = (unsigned)(((c.ky * cg.W + c.kx) * cg.C) * 4), coff = (unsigned)(((cg.pad * cg.W + cg.pad) * cg.C) * 4);
#pragma unroll
        for (int a = 0; a < RA; ++a) {
            const int iy = (ayx[a] >> 16) - 8 + c.ky, ix = (ayx[a] & 0xFFFF) - 8 + c.kx;
            const bool in = (unsigned)iy < (unsigned)cg.H && (unsigned)ix < (unsigned)cg.W;
            voff[a] = aoff[a] + (in ? toff : coff);
            sa[a] = in ? sA : 0.f;
        }
    };
    const int kh = MODE == GATHER_CONV ? K / (cg.kw * cg.C) : 1;
    auto cur_next = [&](Cur &c) __attribute__((always_inline)) {        // -> the next k16 step; a new tile / tap re-derives the per-lane offsets
        if (++c.s < 2) return;
        c.s = 0;
        if (++c.kt == nk) {
            c.kt = 0; c.ky = 0; c.kx = 0; c.c0 = 0;
            if (++c.it < n_items) { set_rows(item_tile(c.it)); set_tap(c); }
            return;
        }
        if (MODE == GATHER_CONV && c.kt < nkr) {                        // channel chunk outer, tap inner (the padding stage re-reads the last one: its weights are zero)
            if (++c.kx == cg.kw) { c.kx = 0; if (++c.ky == kh) { c.ky = 0; c.c0 += BK; } }
            set_tap(c);
        }
    };
    auto load_a = [&](const Cur &c, f32x4 (&f)[RA][2]) __attribute__((always_inline)) {
        if (STEM) {
            // K = 4 window rows x 48 contiguous floats: the lane's 32-B piece g8 of the K row lies in window row g8 / 6 at piece g8 % 6
            const int g8 = c.kt * 4 + c.s * 2 + hi, qy = (g8 * 43) >> 8;
            const unsigned so = (unsigned)((qy * (cg.W * 12) + (g8 - 6 * qy) * 8) * 4);
#pragma unroll
            for (int a = 0; a < RA; ++a) {
                const float *p = reinterpret_cast<const float *>(Ab + (size_t)(voff[a] + so));
                f[a][0] = ld4(p); f[a][1] = ld4(p + 4);
            }
        } else {
            const char *sb = Ab + (MODE == GATHER_CONV ? c.c0 + c.s * 16 : min(c.kt, nkr - 1) * BK + c.s * 16) * 4;
#pragma unroll
            for (int a = 0; a < RA; ++a) {
                const float *p = reinterpret_cast<const float *>(sb + (size_t)voff[a]);
                f[a][0] = ld4(p); f[a][1] = ld4(p + 4);
            }
        }
    };

    // ---- weight fragments (layout of split_planes_narrow_h2_kernel<NB>: 64-B rows per position 32 b + li, 16-B groups XOR-swizzled)
    const int swB = (li >> 2) & 3;
    auto read_b = [&](int buf, int ks, int s, int b, h16x8 (&q)[2]) __attribute__((always_inline)) {
        const char *base = reinterpret_cast<const char *>(smem) + buf * Cfg::BUF + ks * Cfg::ST_BYTES + li * 64 + b * 32 * 64 + ((2 * s + hi) ^ swB) * 16;
#pragma unroll
        for (int p = 0; p < 2; ++p) q[p] = *reinterpret_cast<const h16x8 *>(base + p * Cfg::PL_BYTES);
    };
    f32x16 acc[RA][NB];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < RA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    h16x8 ap[RA][2], an[RA][2];
    f32x4 fr[2][RA][2];                  // raw fp32 fragments in flight: fr[s] was loaded two steps before the step (.., s) that multiplies it
    float sf[2][MODE == GATHER_CONV ? RA : 1];       // CONV: the scale each of them is split with (zero for a tap outside the image)
    h16x8 bq[2], bn[2];
    auto load_ring = [&](const Cur &c, int slot) __attribute__((always_inline)) {
        load_a(c, fr[slot]);
        if (MODE == GATHER_CONV) {
#pragma unroll
            for (int a = 0; a < RA; ++a) sf[slot][a] = sa[a];
        }
    };
    auto convert1 = [&](int slot, int a) __attribute__((always_inline)) {
        const float x[8] = {fr[slot][a][0][0], fr[slot][a][0][1], fr[slot][a][0][2], fr[slot][a][0][3],
                            fr[slot][a][1][0], fr[slot][a][1][1], fr[slot][a][1][2], fr[slot][a][1][3]};
        h2_split8(x, MODE == GATHER_CONV ? sf[slot][a] : sA, an[a][0], an[a][1]);
    };
    auto mma = [&](int b) __attribute__((always_inline)) {              // three terms (m.h, h.m, h.h), small ones first; row sub-tiles alternate
#define TOAD_T(PA, PB_) \
        _Pragma("unroll") for (int a = 0; a < RA; ++a) \
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ap[a][PA], bq[PB_], acc[a][b], 0, 0, 0);
        TOAD_T(1, 0) TOAD_T(0, 1) TOAD_T(0, 0)
#undef TOAD_T
    };

    float amx = 0.f;                     // abs-max of everything this lane stores (all tiles of the block): one atomic per block at the end
    auto epilogue = [&](int m0, int n0) __attribute__((always_inline)) {
        stream_epilogue<RA, NB>(acc, m0, n0, wave, li, hi, kea, bias, binv, addend, C, ldc, M, N, relu, amx);
    };

    // ---- main loop
    Cur nc{0, 0, 0, 0, 0, 0};
    const int total_steps = n_items * nk * 2;
    set_rows(item_tile(0));
    set_tap(nc);
    load_ring(nc, 0);                                    // step 0
    if (total_steps > 1) cur_next(nc);
    load_ring(nc, 1);                                    // step 1
    {                                                    // first weight chunk, all 16 pieces at once; pieces 0, 1 of the second one set out
        const char *src = chunk_src(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { b_load(src, j, 0); b_store(0, j, 0); }
        const char *src1 = chunk_src(1);
        b_load(src1, 0, 0); b_load(src1, 1, 1);
    }
    zero_acc();
#pragma unroll
    for (int a = 0; a < RA; ++a) convert1(0, a);
#pragma unroll
    for (int a = 0; a < RA; ++a) { ap[a][0] = an[a][0]; ap[a][1] = an[a][1]; }
    __syncthreads();
    int gstep = 0, gchunk = 0;
    // one k16 step (ks, S): the loads of the step after next and this step's quarter of the next weight chunk go out first, the NB
    // column blocks follow (weight fragments one block ahead), the split of the NEXT step's rows - loaded a whole step ago - is
    // spread over the last blocks, where it runs in the shadow of this wave's own MFMAs
    auto step = [&](int buf, int ks, auto s_tag, const char *lsrc) __attribute__((always_inline)) {
        constexpr int S = decltype(s_tag)::value;
        const int j = ks * 2 + S;
        if (gstep + 2 < total_steps) cur_next(nc);      // (the last two steps re-load valid rows whose result is never used)
        load_ring(nc, S);
        read_b(buf, ks, S, 0, bq);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) read_b(buf, ks, S, b + 1, bn);
            __builtin_amdgcn_sched_barrier(0);
            mma(b);
            constexpr int FIRST = NB > RA ? NB - RA : 0;             // the last RA blocks split one row sub-tile each
            constexpr int PER = NB > RA ? 1 : RA / NB;
            if (b >= FIRST) {
#pragma unroll
                for (int u = 0; u < PER; ++u) convert1(S ^ 1, (b - FIRST) * PER + u);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (b + 1 < NB) { bq[0] = bn[0]; bq[1] = bn[1]; }
        }
        b_store(buf ^ 1, j, S);                         // piece j of the next chunk (loaded two steps ago) ...
        b_load(lsrc, (j + 2) & 3, S);                   // ... and its registers take the piece two steps on
#pragma unroll
        for (int a = 0; a < RA; ++a) { ap[a][0] = an[a][0]; ap[a][1] = an[a][1]; }
        ++gstep;
    };
    for (int it = 0; it < n_items; ++it) {
        const int q = item_tile(it);
        const int tn = q % tiles_n;
        for (int ck = 0; ck < cpk; ++ck, ++gchunk) {
            const int buf = gchunk & 1;
            // the next weight chunk (of this tile, of the next one, or - at the very end - the last one again) goes to the other buffer:
            // nobody reads that any more (barrier below)
            const char *n1 = chunk_src(gchunk + 1), *n2 = chunk_src(gchunk + 2);
            step(buf, 0, std::integral_constant<int, 0>{}, n1);     // stores piece 0 of chunk + 1, loads its piece 2
            step(buf, 0, std::integral_constant<int, 1>{}, n1);     //        piece 1,                      piece 3
            step(buf, 1, std::integral_constant<int, 0>{}, n2);     //        piece 2, loads piece 0 of chunk + 2
            step(buf, 1, std::integral_constant<int, 1>{}, n2);     //        piece 3,       piece 1
            __syncthreads();
        }
        if constexpr (POOLED) {
            // q = image * tpi + t: the pooled row of tile t is row t of the image's pooled plane. Item 0 leaves the carry only; a tile that starts
            // an image reads zeros for the carry (every window holds a real pixel and post-ReLU values are >= 0: zero padding cannot win)
            float no_cr[32];                       // (the streamed kernel keeps its carried row in LDS: three workgroups per CU, no registers to spare)
            stem_pool_epilogue<RA, NB>(acc, reinterpret_cast<char *>(smem) + Cfg::SMEM, reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + ((gchunk - 1) & 1) * Cfg::BUF),
                                       wave, li, hi, kea, bias, binv, C, (int64_t)q, it != 0, q % tpi == 0, amx, no_cr);
        } else {
            epilogue((q / tiles_n) * TM, tn * TN);
        }
        zero_acc();
    }
    if (y_gmax) {
        __shared__ float s_amx[4];
        amx = h2_wave_max(amx);
        if (lane == 0) s_amx[wave] = amx;
        __syncthreads();
        if (tid == 0) h2_atomic_amax(y_gmax, __builtin_fmaxf(__builtin_fmaxf(s_amx[0], s_amx[1]), __builtin_fmaxf(s_amx[2], s_amx[3])));
    }
}

// ------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolutions with the activation HALO resident in LDS (round 3).
//
// Streaming every tap's fragments from global memory (above) puts 9x the activation through the vector L1, 16 bytes per tag lookup:
// lanes of an MFMA A fragment are 32 different rows, so a wave's load touches 32 cache lines and the L1 delivers ~16 B/clk instead
// of 64 (the streamed layer1 conv2 ran 726 us for 23 MB per CU = 16 B/clk exactly, with HBM fetching only 1.2x the tensor and the
// matrix pipe 30 % busy; cdna_hip_programming.md's "fragment-shaped loads" finding). The nine taps of a 256-pixel tile read the same
// (TH + 2) x (W + 2) pixels, TH = 256 / W. So per 32-channel chunk the workgroup copies that halo ONCE into LDS - by LDS-DMA in whole
// 128-B pixel rows, 8 lanes per pixel, i.e. fully coalesced, 1.3-1.5x the tile's bytes instead of 9x - with zeros written where
// the halo leaves the image. Each wave then splits the pixel rows it fetched IN PLACE into the two fp16 pieces (row = 64 B of h,
// 64 B of m: the same 128 bytes; one wave-wide ds_read_b128 takes a whole 8-pixel group out before the two ds_write_b64 put it
// back), so every element is converted once per tile instead of once per tap, and all nine taps take ready MFMA operands from LDS
// with ds_read_b128 (256 B/clk per CU): lane (li, hi) of row sub-tile a reads 16 B of h and 16 B of m of halo pixel (ty + ky, tx + kx).
// 16-B slots are XOR-swizzled with (pixel >> 1) & 7, the conflict-free pattern of ds_read_b128's lane groups for 128-B rows
// (MI355X_MICROARCH.md, LDS). k-stage = one tap of one chunk (the
// weight planes are split chunk-outer, tap-inner as for the streamed kernel); weights go through a two-stage ring filled through
// registers, one barrier per stage. One halo buffer: the refill per chunk is exposed to this workgroup and covered by the other
// one on the CU. Same split, same MFMA order, same epilogue as the streamed kernel.
// Shapes: kh = kw = 3, stride 1, pad 1, W a power of two in 8..128 dividing 256, H % (256 / W) == 0, C % 32 == 0 - every conv2 of
// ResNet-50's stride-1 bottlenecks (models/resnet_custom.py:25-27, 42-44); the two stride-2 ones stay on the streamed kernel.
// ------------------------------------------------------------------------------------------
template <int NB> struct HaloCfg {
    static constexpr int RA = 2, WAVES = 4, THREADS = 256, TM = 256, TN = NB * 32;
    static constexpr int PL_BYTES = TN * BK * 2, ST_BYTES = 2 * PL_BYTES;      // one k-stage of weights: h plane, m plane
    static constexpr int B_RING = 2 * ST_BYTES;
    static constexpr int PPS = ST_BYTES / 1024 / WAVES / 2;                    // 1-KB weight pieces per wave per k16 step: 1 (NB = 2) or 2 (NB = 4)
    static constexpr int halo_pixels(int W) { return (256 / W + 2) * (W + 2); }
    static constexpr int halo_bytes(int W) { return (halo_pixels(W) + 7) / 8 * 1024; }
    static constexpr int smem(int W) { return halo_bytes(W) + B_RING + 16; }
};

template <int NB>
__global__ __launch_bounds__(256, 2) void conv3x3_h2_halo_kernel(
    const float *__restrict__ X, const float *__restrict__ a_gmax, const unsigned short *__restrict__ Bp, const float *__restrict__ binv,
    float *Y, int64_t ldc, int M, int N, int K, const float *__restrict__ bias, int relu, const float *addend, ConvGeom cg, float *y_gmax,
    int tiles_m, int tiles_n, int halo_bytes) {
    using Cfg = HaloCfg<NB>;
    constexpr int RA = Cfg::RA, TM = Cfg::TM, TN = Cfg::TN;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char *const lds = reinterpret_cast<char *>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hi = lane >> 5;
    const int W = cg.W, H = cg.H, C = cg.C, Wh = W + 2;
    const int wsh = 31 - __builtin_clz(W);                       // W = 1 << wsh
    const int HP = (TM / W + 2) * Wh;                            // halo pixels
    const int hmagic = (65536 + Wh - 1) / Wh;                    // hp / Wh == (hp * hmagic) >> 16 for hp < 1024 (Wh <= 130)
    const int nchunk = C / BK, nk = K / BK;                      // K = 9 C: nk = 9 * nchunk stages, chunk-outer / tap-inner

    const int bpx = gridDim.x / kNumXCD;
    const int xcd = blockIdx.x % kNumXCD, slot = blockIdx.x / kNumXCD;
    const int tiles = tiles_m * tiles_n;
    const int t_lo = (int)(((int64_t)tiles * xcd) / kNumXCD), t_hi = (int)(((int64_t)tiles * (xcd + 1)) / kNumXCD);
    if (t_hi - t_lo <= slot) return;
    const int n_items = (t_hi - t_lo - slot + bpx - 1) / bpx;
    auto item_tile = [&](int i) { return t_lo + slot + i * bpx; };

    const char *Xb = reinterpret_cast<const char *>(X), *Bpb = reinterpret_cast<const char *>(Bp);
    const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lane16 = lane * 16u;
    char *const bring = lds + halo_bytes;
    const int kea = __builtin_amdgcn_readfirstlane(h2_exp_from_amax(a_gmax[0]));     // ONE power-of-two scale for the whole operand (gemm_narrow.inc)
    const float sA = h2_pow2(kea);
    auto dma1 = [&](const char *sbase, unsigned voff, unsigned lds_byte) __attribute__((always_inline)) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_byte) : "memory");
    };
    // halo of tile (image b, rows y0 .. y0 + TH - 1), channel chunk cc -> LDS. Group g = 8 halo pixels = 1 KB = one wave-wide DMA:
    // lane -> pixel 8 g + lane / 8, physical 16-B piece lane % 8 = logical piece ^ ((pixel >> 1) & 7)
    auto fill_halo = [&](int b, int y0, int cc) __attribute__((always_inline)) {
        const int ngroups = (HP + 7) >> 3;
        const unsigned img = (unsigned)(b * H) * (unsigned)W;                               // pixel index of the image's (0, 0)
        for (int g = wave; g < ngroups; g += Cfg::WAVES) {
            const int hp = g * 8 + (lane >> 3);
            const int hy = (hp * hmagic) >> 16, hx = hp - hy * Wh;
            const int y = y0 - 1 + hy, x = hx - 1;
            const int piece = (lane & 7) ^ ((hp >> 1) & 7);
            const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;      // (pixels past HP in the last group: y >= y0 + TH + 1 may still be inside - harmless)
            if (in) {
                dma1(Xb + cc * (BK * 4), (img + (unsigned)(y * W + x)) * (unsigned)(C * 4) + piece * 16, lds_base + g * 1024);
            } else {
                *reinterpret_cast<f32x4 *>(lds + g * 1024 + lane16) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    // in-place split of the groups THIS wave fetched (its own vmcnt(0) has made them visible to it): raw piece j (floats 4j .. 4j + 3 of
    // the pixel's 32) -> halves 4j .. 4j + 3 of h (16-B slot j / 2) and of m (slot 4 + j / 2), slots swizzled like the raw pieces were
    auto split_halo = [&]() __attribute__((always_inline)) {
        const int ngroups = (HP + 7) >> 3;
        for (int g = wave; g < ngroups; g += Cfg::WAVES) {
            const int hp = g * 8 + (lane >> 3), sw = (hp >> 1) & 7;
            const int j = (lane & 7) ^ sw;                                               // logical piece held at this lane's slot
            char *row = lds + hp * 128;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(lds + g * 1024 + lane16);
            unsigned h0, m0, h1, m1;
            h2_split2(v[0], v[1], sA, h0, m0);
            h2_split2(v[2], v[3], sA, h1, m1);
            const int oh = (((j >> 1) ^ sw) << 4) + ((j & 1) << 3);
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u32x2 *>(row + oh) = u32x2{h0, h1};
            *reinterpret_cast<u32x2 *>(row + (oh ^ 64)) = u32x2{m0, m1};
        }
    };
    // weights: stage st of column tile tn is ST_BYTES contiguous; piece p (1 KB) of the NEXT stage is moved by wave w in step s of
    // the current one, p = (2 w + s) * PPS + i  (2 steps x 4 waves x PPS pieces = one stage)
    // A piece rides in registers for two steps (one whole stage): loaded in step (st, s), written to LDS in step (st + 1, s) for stage st + 2.
    f32x4 bst[2][Cfg::PPS];
    auto stage_src = [&](int gs) __attribute__((always_inline)) {        // stage number gs of this block's stage sequence (past the end: the last one again)
        gs = min(gs, n_items * nk - 1);
        const int it = gs / nk, st = gs - it * nk;
        return Bpb + (int64_t)((item_tile(it) % tiles_n) * ((nk + 1) & ~1) + st) * Cfg::ST_BYTES;       // (planes hold an even number of stages per tile)
    };
    auto b_load = [&](const char *src, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < Cfg::PPS; ++i) bst[s][i] = ld4(reinterpret_cast<const float *>(src + ((2 * wave + s) * Cfg::PPS + i) * 1024 + lane16));
    };
    auto b_store = [&](int buf, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < Cfg::PPS; ++i) *reinterpret_cast<f32x4 *>(bring + buf * Cfg::ST_BYTES + ((2 * wave + s) * Cfg::PPS + i) * 1024 + lane16) = bst[s][i];
    };
    const int swB = (li >> 2) & 3;
    auto read_b = [&](int buf, int s, int b, h16x8 (&q)[2]) __attribute__((always_inline)) {
        const char *base = bring + buf * Cfg::ST_BYTES + li * 64 + b * 32 * 64 + ((2 * s + hi) ^ swB) * 16;
#pragma unroll
        for (int p = 0; p < 2; ++p) q[p] = *reinterpret_cast<const h16x8 *>(base + p * Cfg::PL_BYTES);
    };
    // A fragments: output pixel p = 64 wave + 32 a + li of the tile = (ty, tx); tap (ky, kx) reads halo pixel (ty + ky) * Wh + tx + kx
    int hp0[RA];
#pragma unroll
    for (int a = 0; a < RA; ++a) { const int p = wave * 64 + a * 32 + li; hp0[a] = (p >> wsh) * Wh + (p & (W - 1)); }
    auto read_a = [&](int tap_off, int s, h16x8 (&f)[RA][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < RA; ++a) {
            const int hp = hp0[a] + tap_off;
            const int o0 = hp * 128 + (((2 * s + hi) ^ ((hp >> 1) & 7)) << 4);
            f[a][0] = *reinterpret_cast<const h16x8 *>(lds + o0);               // h
            f[a][1] = *reinterpret_cast<const h16x8 *>(lds + (o0 ^ 64));        // m
        }
    };
    f32x16 acc[RA][NB];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < RA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    h16x8 ap[RA][2], an[RA][2];
    h16x8 bq[2], bn[2];
    auto mma = [&](int b) __attribute__((always_inline)) {
#define TOAD_T(PA, PB_) \
        _Pragma("unroll") for (int a = 0; a < RA; ++a) \
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ap[a][PA], bq[PB_], acc[a][b], 0, 0, 0);
        TOAD_T(1, 0) TOAD_T(0, 1) TOAD_T(0, 0)
#undef TOAD_T
    };
    float amx = 0.f;

    // one k16 step: this step's share of the next stage's weights and the NEXT step's A operands (same chunk: the halo stays) go out
    // first; nothing is converted here any more
    auto step = [&](int buf, int s, int next_tap_off, int next_s, bool have_next_a, const char *lsrc) __attribute__((always_inline)) {
        if (have_next_a) read_a(next_tap_off, next_s, an);
        read_b(buf, s, 0, bq);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) read_b(buf, s, b + 1, bn);
            __builtin_amdgcn_sched_barrier(0);
            mma(b);
            __builtin_amdgcn_sched_barrier(0);
            if (b + 1 < NB) { bq[0] = bn[0]; bq[1] = bn[1]; }
        }
        b_store(buf ^ 1, s);                             // piece s of the next stage (loaded a stage ago) ...
        b_load(lsrc, s);                                 // ... and its registers take piece s of the stage after that
        if (have_next_a) {
#pragma unroll
            for (int a = 0; a < RA; ++a) { ap[a][0] = an[a][0]; ap[a][1] = an[a][1]; }
        }
    };

    // first weight stage
    {
        const char *src = stage_src(0);
        b_load(src, 0); b_store(0, 0);
        b_load(src, 1); b_store(0, 1);
        const char *src1 = stage_src(1);
        b_load(src1, 0); b_load(src1, 1);
    }
    int gstage = 0;
    for (int it = 0; it < n_items; ++it) {
        const int q = item_tile(it);
        const int tn = q % tiles_n, m0 = (q / tiles_n) * TM;
        const int pix = m0 >> wsh;                               // global image-row index of the tile's first row: b * H + y0
        const int b = pix / H, y0 = pix - b * H;
        zero_acc();
        for (int cc = 0; cc < nchunk; ++cc) {
            __syncthreads();                                     // every wave is done with the previous halo (and the weights of stage gstage have landed)
            fill_halo(b, y0, cc);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            split_halo();
            __syncthreads();
            read_a(0, 0, ap);
            for (int tap = 0; tap < 9; ++tap, ++gstage) {
                const int buf = gstage & 1;
                // weights: this stage stores the pieces of stage + 1 and loads those of stage + 2 (next tap, chunk or tile; past the end: never read)
                const char *lsrc = stage_src(gstage + 2);
                const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;                       // tap / 3 for tap < 9
                const int t1 = tap + 1, ky1 = (t1 * 11) >> 5, kx1 = t1 - 3 * ky1;
                const int off = ky * Wh + kx, off1 = ky1 * Wh + kx1;
                step(buf, 0, off, 1, true, lsrc);
                step(buf, 1, off1, 0, tap < 8, lsrc);
                if (tap < 8) __syncthreads();                    // (after the last tap the chunk's / tile's barrier follows)
            }
        }
        stream_epilogue<RA, NB>(acc, m0, tn * TN, wave, li, hi, kea, bias, binv, addend, Y, ldc, M, N, relu, amx);
    }
    if (y_gmax) {
        float *s_amx = reinterpret_cast<float *>(bring + Cfg::B_RING);
        amx = h2_wave_max(amx);
        __syncthreads();
        if (lane == 0) s_amx[wave] = amx;
        __syncthreads();
        if (tid == 0) h2_atomic_amax(y_gmax, __builtin_fmaxf(__builtin_fmaxf(s_amx[0], s_amx[1]), __builtin_fmaxf(s_amx[2], s_amx[3])));
    }
}
