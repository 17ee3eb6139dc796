// gemm_h2.inc — part of the single translation unit gemm_f32.hip (included inside namespace toad): the SHIPPED GEMMs of the MIL path
// (forward, dgrad, wgrad) on the fp16 matrix pipe with TWO-piece operands.
// ------------------------------------------------------------------------------------------
// Arithmetic ("h2"): every fp32 operand element x is represented as  x*s = h + m  with
//   s  a power of two chosen so that max|x*s| lies in [2^13, 2^14)  (fp16 overflows at 2^16),
//   h  = rn_fp16(x*s)              (11 significand bits)
//   m  = rn_fp16(x*s - h)          (the residual is exact in fp32; 11 more bits + its own sign)
// so |x*s - h - m| <= 2^-22 |x*s| (2^-23.5 rms): the operand is carried at fp32 precision. A product keeps the three terms
//   h.h + h.m + m.h          (dropped: m.m <= 2^-22 relative, the same size as the representation error)
// on v_mfma_f32_32x32x16_f16 with fp32 accumulation. Emulated against fp64 (tools/split_emulation.py: K = 1024, normal /
// tiny-ReLU / heavy-tailed data) the result is as close to the exact value as the exact-fp32 fma chain and as the previous
// three-piece bf16 split (six terms) - at HALF the matrix-pipe work of the six-term form and with 2 VALU ops per split element
// instead of 5.5 (v_fma_mix{lo,hi}_f16: the fused multiply(-subtract)-round-pack is one instruction per piece, two per element).
//
// Scales. fp16 has 5 exponent bits, so operands are normalised by powers of two (exact):
//   * activations (the A operand of NT, both operands of TN) carry an abs-max array  amax[ceil(M/256)]  (bit patterns of
//     non-negative floats, one per block of 256 rows) that the PRODUCING kernel fills in its epilogue by atomic max (GEMM
//     epilogue / fix-up, pool backward) - or absmax_rows256_kernel for a tensor that comes from outside (the caller's bag).
//     NT uses the scale of its own 256-row tile (rows are independent there); TN (reduction over rows) uses the maximum of
//     the whole array.
//   * weights (the B operand of NT) are split once per call by split_planes_h2_kernel, one wave per weight row, each row
//     with its own scale; the epilogue multiplies the accumulator by 1/(s_tile t_col) as two exact power-of-two factors (h2_descale).
//   Elements far below the block maximum lose RELATIVE precision only below 2^-17 of it (m becomes subnormal: absolute error
//   <= 2^-39 of the block maximum), i.e. nothing a dot product can see.
// (Round 1's exact-fp32 / split-bf16 persistent kernels, from which the work decomposition, swizzles and the K-split tail descend, were
// removed from the library in round 4; this file and gemm_pt.inc hold the only persistent GEMMs.)
// ------------------------------------------------------------------------------------------
// (the vector typedefs, h2_exp_from_amax ... h2_descale_*, h2_split2 / h2_split8: h2_arith.h, shared with the extractor's kernels)
constexpr int H2_A_BYTES = PB * BK * 4;                          // 32,768
constexpr int H2_PLANE_BYTES = PB * BK * 2;                      // 16,384
constexpr int H2_B_BYTES = 2 * H2_PLANE_BYTES;                   // 32,768: both planes of one stage
constexpr int H2_A_SLOTS = 2, H2_B_SLOTS = 2;                    // A: fp16 plane image written by the block itself; B: LDS-DMA of the pre-split planes
constexpr int H2_B_BASE = H2_A_SLOTS * H2_A_BYTES;
constexpr int H2_SMEM = H2_B_BASE + H2_B_SLOTS * H2_B_BYTES;
constexpr int H2_SMEM_PT = 3 * H2_A_BYTES + H2_B_SLOTS * H2_B_BYTES;   // plane-tiled A: three DMA slots for A + two for B = 163,840 B, all of LDS
constexpr int H2_SMEM_RUN = H2_SMEM + 512 + 512 * 32;                             // self-measuring fp32 A (AMODE 3): + wave maxima, redo exponents, one parked raw octet per thread = 147,968 B
// half-height tiles (TM = 128): A slots of 128 rows (16 KB) and THREE B slots (the weight planes of stage s+2 are requested while stage s computes)
constexpr int H2_SMEM_HALF = 2 * (H2_A_BYTES / 2) + 3 * H2_B_BYTES;               // 131,072 B
constexpr int H2_SMEM_HALF_RUN = H2_SMEM_HALF + 512 + 512 * 32;                   // 147,968 B
static_assert(H2_ROWBLK == PB, "one abs-max entry per NT tile row");

__host__ __device__ inline int64_t h2_nblk(int64_t rows) { return (rows + H2_ROWBLK - 1) / H2_ROWBLK; }

// amax[b] = max |X[r, 0:K]| over rows r of block b (256 rows). grid = (4 or 16, nblk): 64 or 16 rows per workgroup (a short
// operand is a latency chain of row batches, not a bandwidth problem); `amax` zeroed by the caller.
__global__ __launch_bounds__(256) void absmax_rows256_kernel(const float *__restrict__ X, int64_t ld, int M, int K,
                                                              float *__restrict__ amax) {
    const int rpb = H2_ROWBLK / gridDim.x;               // rows per workgroup: 64 (grid.x = 4), or 16 (grid.x = 16) for operands of at most 2,048 rows
    const int r0 = blockIdx.y * H2_ROWBLK + blockIdx.x * rpb, r1 = min(M, r0 + rpb);
    const int k4 = K >> 2;
    float mx = 0.f;
    for (int r = r0; r < r1; r += 4) {                   // 4 independent 16-B loads in flight per lane (clamped rows repeat: harmless for a max)
        for (int c = threadIdx.x; c < k4; c += 256) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(X + (int64_t)min(r + u, r1 - 1) * ld + c * 4));
#pragma unroll
            for (int u = 0; u < 4; ++u) mx = __builtin_fmaxf(mx, h2_absmax4(v[u]));
        }
    }
    mx = h2_wave_max(mx);
    if ((threadIdx.x & 63) == 0 && r0 < r1) h2_atomic_amax(amax + blockIdx.y, mx);
}

// ---- weight operand -> two fp16 planes in LDS stage order + per-row inverse scales ---------------------------------------
// Bp[tile][kstage][plane 0..1][pos 0..255][phys chunk 0..3][8 fp16]  <-  B[n, k] = src[n * sn + k * sk]; binv[n] = 1 / t_n.
// One wave per weight row n (a column of the product): pass 1 reduces the row's abs-max, pass 2 splits it with the row's scale.
// Up to 6 operands per launch (the fused step prepares all weight operands of a slide in one launch).
// TRANSPOSED sources (sn == 1: the dgrad operands B[n, k] = W[k, n] read in place) take another thread mapping since round 6: row n of B is a
// COLUMN of W, so with a wave per row every 4-byte load touched a cache line of its own (134 MB of L2 requests for 2.6 MB of weights: ~10 of
// the launch's 12.4 us). There a workgroup owns 16 consecutive rows n - one 64-byte line of every W row - thread t = (row t & 15, k-chunk
// lane t >> 4): 16 lanes share each line, the row maxima meet through LDS. Same values, same planes.
struct H2SplitDesc { const float *src; int64_t sn, sk; unsigned short *planes; float *binv; int N, K, tiles_n, wave0; };
struct H2SplitBatch { H2SplitDesc d[6]; int n; int total_waves; float *zero; int zero_n; float *zero2; int zero2_n; };

// Side job: the launch also zeroes `zero[0..zero_n)` - the abs-max arrays the following kernels fill by atomic max - so a
// forward or backward pass needs no memset launches (each hipMemsetAsync is one or two ~5 us fill kernels).
__global__ __launch_bounds__(256) void split_planes_h2_kernel(H2SplitBatch batch) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    for (int t = blockIdx.x * 256 + threadIdx.x; t < batch.zero_n; t += gridDim.x * 256) batch.zero[t] = 0.f;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < batch.zero2_n; t += gridDim.x * 256) batch.zero2[t] = 0.f;
    if (gw >= batch.total_waves) return;
    int di = 0;
#pragma unroll
    for (int i = 1; i < 6; ++i) if (i < batch.n && gw >= batch.d[i].wave0) di = i;
    // select the descriptor fields without dynamic indexing of the by-value struct (that would go through scratch)
    const float *src = batch.d[0].src; int64_t sn = batch.d[0].sn, sk = batch.d[0].sk; unsigned short *planes = batch.d[0].planes;
    float *binv = batch.d[0].binv; int N = batch.d[0].N, K = batch.d[0].K, wave0 = batch.d[0].wave0;
#pragma unroll
    for (int i = 1; i < 6; ++i)
        if (di == i) { src = batch.d[i].src; sn = batch.d[i].sn; sk = batch.d[i].sk; planes = batch.d[i].planes; binv = batch.d[i].binv;
                       N = batch.d[i].N; K = batch.d[i].K; wave0 = batch.d[i].wave0; }
    const int nk = K / BK, nchunks = K / 8;
    if (sn == 1 && sk != 1) {                       // transposed source: 16 rows per workgroup (see above); workgroup-uniform branch
        __shared__ float s_mx[4][16];
        const int n0 = ((gw - wave0) >> 2) * 16, nl = threadIdx.x & 15, kq = threadIdx.x >> 4;       // kq 0..15
        const int n = n0 + nl;
        const bool real = n < N;
        const float *col = src + (real ? n : 0);
        const int tile = n / PB, cc = n % PB, r = cc & 127;
        const int pos = (cc & 128) + (r >> 2) + 32 * (r & 3);
        auto put = [&](int q, const float (&x)[8], float s) __attribute__((always_inline)) {
            h16x8 h, m;
            h2_split8(x, s, h, m);
            const int stage = q >> 2, chunk = q & 3;
            const int phys = chunk ^ ((pos >> 2) & 3);
            unsigned short *dst = planes + ((int64_t)(tile * nk + stage) * 2) * (PB * BK) + pos * BK + phys * 8;
            *reinterpret_cast<h16x8 *>(dst) = h;
            *reinterpret_cast<h16x8 *>(dst + PB * BK) = m;
        };
        constexpr int MAXQ = 8;                         // chunks per thread held in registers: K <= 1024 (every operand of the MIL step)
        if (nchunks <= 16 * MAXQ) {
            // ONE round trip: the thread's whole share of the column block is loaded up front (unconditional loads, clamped chunk index) and
            // stays in registers between the abs-max pass and the split. The loop form below re-read every element for the split and, not being
            // unrolled, waited for each chunk's eight loads before issuing the next: 2 x 6 dependent L2 round trips for the 768-deep dgrad
            // operand, on 64 workgroups, while every other workgroup of the launch had long finished (the launch took 9.6 us; round 6).
            float x[MAXQ][8];
#pragma unroll
            for (int i = 0; i < MAXQ; ++i) {
                const int qc = min(kq + 16 * i, nchunks - 1);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[i][e] = col[(int64_t)(qc * 8 + e) * sk];
            }
            float mx = 0.f;
#pragma unroll
            for (int i = 0; i < MAXQ; ++i) {
                const bool ok = real && kq + 16 * i < nchunks;
#pragma unroll
                for (int e = 0; e < 8; ++e) { x[i][e] = ok ? x[i][e] : 0.f; mx = __builtin_fmaxf(mx, __builtin_fabsf(x[i][e])); }
            }
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16));
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32));
            if (lane < 16) s_mx[threadIdx.x >> 6][lane] = mx;
            __syncthreads();
            mx = __builtin_fmaxf(__builtin_fmaxf(s_mx[0][nl], s_mx[1][nl]), __builtin_fmaxf(s_mx[2][nl], s_mx[3][nl]));
            const int kexp = h2_exp_from_amax(mx);
            const float s = h2_pow2(kexp);
            if (kq == 0) binv[n] = h2_pow2(-kexp);
#pragma unroll
            for (int i = 0; i < MAXQ; ++i)
                if (kq + 16 * i < nchunks) put(kq + 16 * i, x[i], s);
            return;
        }
        float mx = 0.f;
        if (real) {
            for (int q = kq; q < nchunks; q += 16) {
#pragma unroll
                for (int e = 0; e < 8; ++e) mx = __builtin_fmaxf(mx, __builtin_fabsf(col[(int64_t)(q * 8 + e) * sk]));
            }
        }
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16));
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32));
        if (lane < 16) s_mx[threadIdx.x >> 6][lane] = mx;
        __syncthreads();
        mx = __builtin_fmaxf(__builtin_fmaxf(s_mx[0][nl], s_mx[1][nl]), __builtin_fmaxf(s_mx[2][nl], s_mx[3][nl]));
        const int kexp = h2_exp_from_amax(mx);
        const float s = h2_pow2(kexp);
        if (kq == 0) binv[n] = h2_pow2(-kexp);
        for (int q = kq; q < nchunks; q += 16) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = real ? col[(int64_t)(q * 8 + e) * sk] : 0.f;
            put(q, x, s);
        }
        return;
    }
    const int n = gw - wave0;                       // row of B, 0 .. tiles_n*256 - 1 (rows >= N are zero padding)
    const bool real = n < N;
    const float *row = src + (int64_t)(real ? n : 0) * sn;
    auto load8 = [&](int q, float (&x)[8]) {
        if (sk == 1) {
            const f32x4 a = ld4(row + q * 8), b = ld4(row + q * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[4 + e] = b[e]; }
        } else {                                        // transposed source (dgrad: B = W^T read in place)
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = row[(int64_t)(q * 8 + e) * sk];
        }
    };
    const int tile = n / PB, cc = n % PB, r = cc & 127;
    const int pos = (cc & 128) + (r >> 2) + 32 * (r & 3);       // column-interleaved position (see gemm_nt_f32_big_kernel)
    auto put = [&](int q, const float (&x)[8], float s) __attribute__((always_inline)) {
        h16x8 h, m;
        h2_split8(x, s, h, m);
        const int stage = q >> 2, chunk = q & 3;
        const int phys = chunk ^ ((pos >> 2) & 3);
        unsigned short *dst = planes + ((int64_t)(tile * nk + stage) * 2) * (PB * BK) + pos * BK + phys * 8;
        *reinterpret_cast<h16x8 *>(dst) = h;
        *reinterpret_cast<h16x8 *>(dst + PB * BK) = m;
    };
    if (sk == 1 && nchunks <= 128) {                // K <= 1024, contiguous rows: the row stays in registers between the abs-max pass and the split (one round trip)
        float x[2][8];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qc = min(lane + 64 * i, nchunks - 1);
            const f32x4 a = ld4(row + qc * 8), b = ld4(row + qc * 8 + 4);
            const bool ok = real && lane + 64 * i < nchunks;
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[i][e] = ok ? a[e] : 0.f; x[i][4 + e] = ok ? b[e] : 0.f; }
        }
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) mx = __builtin_fmaxf(mx, __builtin_fabsf(x[i][e]));
        mx = h2_wave_max(mx);
        const int kexp = h2_exp_from_amax(mx);
        const float s = h2_pow2(kexp);
        if (lane == 0) binv[n] = h2_pow2(-kexp);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + 64 * i < nchunks) put(lane + 64 * i, x[i], s);
        return;
    }
    float mx = 0.f;
    if (real) {
        for (int q = lane; q < nchunks; q += 64) {
            float x[8];
            load8(q, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) mx = __builtin_fmaxf(mx, __builtin_fabsf(x[e]));
        }
    }
    mx = h2_wave_max(mx);
    const int kexp = h2_exp_from_amax(mx);
    const float s = h2_pow2(kexp);
    if (lane == 0) binv[n] = h2_pow2(-kexp);
    for (int q = lane; q < nchunks; q += 64) {
        float x[8];
        if (real) load8(q, x);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = 0.f;
        }
        put(q, x, s);
    }
}

// ------------------------------------------------------------------------------------------
// NT, persistent 256x256, h2 arithmetic.   C = epi( (A . B^T) ), A fp32 [M,K] + a_amax, B = pre-split planes + binv
// stage = 32 k: A as a 32 KB fp16 plane image written by the block itself (convert-once, below) + 2 x 16 KB B planes by LDS-DMA;
// two slots each = 128 KB of LDS. History (DESIGN.md 4, profiles/r02_pmc_gemm.md): the first h2 kernel staged raw fp32 A rows by
// LDS-DMA through a 3-slot ring and let every wave split its own fragments in lock-step; counters showed the matrix pipe 40 % busy
// with the waves parked or issue-stalled the rest of the time. What is here instead: A converted once per element, and the two
// waves of every SIMD alternating LOAD and COMPUTE phases (main loop).
// y_amax (optional): abs-max of the stored outputs per 256-row block, for the next GEMM that consumes C.
// ------------------------------------------------------------------------------------------
// Optional "pool addend" (pool_T > 0, the dgrad of the stacked attention Linear): instead of reading a materialised
//   dH_pool[r, c] = sum_t p[r,t] dM[t,c],  p[r,t] = exp(A_raw[r,t] - max_t) / sum_t          (models/model_toad.py:97-98 backward)
// from HBM (N x L floats written by the pooling backward and read here), the epilogue recomputes it from A_raw [M,T], the
// softmax stats [T,2] and dM [T,N]: two exponentials per row and 2T FMAs per element instead of a 410 MB round trip per
// 100k-patch slide.
__device__ __forceinline__ float h2_fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// POOL = true: the pooling addend is recomputed (no `addend` pointer then); ADD = true: an addend buffer is read (per-op API
// only; two rows per batch instead of four); MASK = 1: the fp32 relu_src is read, MASK = 2: its one-bit-per-element image
// (`mask_src` then points at the 64-bit words the forward GEMM of that layer wrote through `bits_out`: lane-private, 8 KB per tile
// instead of 256 KB - the row-batched fp32 mask loads exposed a full HBM latency eight times per tile). Compile-time variants keep each epilogue inside
// the register budget without spilling (the accumulators alone are 128 of the 256 VGPRs; a scratch reload inside the loop
// would be a VMEM wait) and make every epilogue load unconditionally issued AND consumed: hipcc's wait insertion is path
// insensitive, so a load guarded by a run-time flag at its issue and again at its use counts as "pending" at the loop
// back-edge and draws a vmcnt(0) in front of the next step's ds_reads.
// A16 = true: A is an fp16 matrix in memory (lda in halves; feature bags stored as fp16). Its elements ARE first pieces (h = x, m = 0,
// scale 1), so the staging copies octets instead of splitting them, only the h plane of A exists, and a product is two MFMA
// terms (h.m_w + h.h_w): exactly what the fp32 path computes for the same values, without its third term (which is zero).
// AMODE = 2 ("PT"): A is a plane-tiled tensor (pt_split_kernel below, or - Stage 2 - a producing GEMM's epilogue): the (h, m) fp16 planes of
// every 256-row x 32-column stage lie in memory in the LDS stage order, so the whole A stage arrives by LDS-DMA exactly like the
// weight planes: no register staging, no splitting, no plane writes in this kernel. Three A slots (96 KB) + two B slots = 160 KB:
// the A stream comes from HBM and gets two steps of latency cover, the weights (L2-resident) one.
// AMODE = 3 ("RUN", round 4): fp32 A whose abs-max array does NOT exist yet - the caller's bag in the first Linear. Instead of a separate pass over
// the bag (absmax_rows256_kernel: 410 MB read, 67 us per 100k-patch slide) the kernel measures every 256 x 32 stage while it stages it: each wave
// reduces the 16 raw elements per lane it holds for stage s+1 (one k-step before they are split), the eight wave maxima meet in 64 bytes of LDS
// across the step's barrier, every wave forms the same running maximum. An item (tile, or K-slice of a remainder tile) takes its scale from its
// FIRST stage with RUN_MARGIN = 3 extra bits of room: that stage's maximum lands in [2^10, 2^11) instead of [2^13, 2^14), fp16 is finite up to
// 65504 < 2^16, so the later stages of the item may exceed the first by a factor of 16 (running maximum in [2^14, 2^15): the poison test below) before
// anything can overflow - and a two-piece split is as exact
// at 2^15 as at 2^10 (what moves is the level below which second pieces go subnormal: 2^-14 instead of 2^-17 of the maximum, an absolute error
// <= 2^-36 of it). The accumulators are never rescaled (every way of doing that in registers made hipcc spill an accumulator on every step of
// the main path). An item whose running maximum does outgrow the room (an outlier column behind small leading columns) is POISONED: its
// accumulators may hold infinities, its epilogue is skipped, and after the last item the workgroup runs the poisoned items a second time
// (pass 1 of the loop below) with the exponent of their now known true maximum. The item's final maximum goes to a_amax_out by atomic max (the
// weight gradient of the layer scales the bag with the maximum of that array), a K-slice's exponent to slab_ke[workgroup] (the fix-up aligns the
// slabs). Results equal the a_amax path's to the last bit except where an element more than 2^14 below its stage's scale decides a rounding.
// Cost: both octets of a stage are split in LOAD(s,1) and their successors loaded there (half a step less latency cover for the bag's rows).
// TM = 128 (round 6): HALF-HEIGHT tiles for short operands (at most PB_GRID tiles of 128 x 256, i.e. M <= 16,384 at N = 512). A 10,000-row bag is
// 40 x 2 tiles of 256 x 256 on 256 CUs: the K-split that spread them (2-3 slices per tile) wrote every tile as raw slabs and needed a fix-up
// launch per GEMM - five launches, 26 % of the 10k-patch step (profiles/r06a_*). With 128 x 256 tiles the same bag is 79 x 2 = 158 whole-K items,
// one per workgroup: no slabs, no fix-up. Same 8 waves (4 x 2), each now 32 x 128 (acc[1][4]: 12 MFMAs per k16 step against 10 ds_read_b128), one
// staged octet per thread and stage instead of two; the plane image keeps its 256-row geometry (the upper half stays unused). A tile's operand
// scale still comes from its 256-row block of the abs-max array (two tiles share a slot), the ReLU bit image keeps its per-256-row-block layout
// (gemm_h2_epilogue.inc: epi_vwave / epi_a0). Instantiated for the MIL step's epilogues only (no residual addend, no plane-tiled A), and for the
// fp16 bags of the ragged multi-slide calls (AMODE 1: the plain forward; one 16-byte load per staged octet): the concatenation's first Linear then
// runs on the tile plan of the fp32 call on the up-cast bags - the same sums in the same order - and loses its K-split fix-up launch like it.
constexpr int RUN_MARGIN = 3;
template <bool POOL, bool ADD, int MASK, int AMODE = 0, int TM = PB>
__global__ __launch_bounds__(512, 2) void gemm_nt_h2_big_kernel(
    const float *__restrict__ A, int64_t lda, const float *__restrict__ a_amax, const unsigned short *__restrict__ Bp,
    const float *__restrict__ binv, float *C, int64_t ldc, int M, int N, int K, const float *__restrict__ bias, EpiScalars es,
    const float *addend, const float *__restrict__ mask_src, const float *__restrict__ pool_araw, const float *__restrict__ pool_stats,
    const float *__restrict__ pool_dM, int pool_T, float *__restrict__ slabs, float *y_amax, unsigned long long *__restrict__ bits_out,
    int tiles_m, int tiles_n, int a_stride, int y_stride, float *a_amax_out, int *__restrict__ slab_ke) {
    // a_stride / y_stride: 1 = abs-max ARRAYS (one entry per 256-row block); 0 = ONE scalar for the whole tensor (the extractor:
    // its convolutions gather rows from arbitrary pixels, so its activations carry a tensor-wide abs-max, gemm_narrow.inc)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool A16 = AMODE == 1, APT = AMODE == 2, ARUN = AMODE == 3;
    constexpr int NA = TM / 128;                                 // 32-row sub-tiles per wave = octets a thread stages per stage (2, or 1 for half-height tiles)
    constexpr int WROWS = TM / 4;                                // rows per wave row group (64 / 32)
    static_assert(TM == PB || (TM == 128 && !ADD && !APT), "half-height tiles: fp32 or fp16 A, no addend buffer");
    constexpr int A_LD = A16 ? 1 : 2;                            // 16-byte loads per staged octet (8 halves / 8 floats)
    constexpr int A_SLOTS = APT ? 3 : 2;
    // LDS geometry of the A plane image: [plane][k-group 0..3][row ^ (k-group << 2)] 16-byte entries, TM rows per k-group
    constexpr int A_KG_BYTES = TM * 16, A_PLANE_BYTES = 4 * A_KG_BYTES, A_SLOT_BYTES = 2 * A_PLANE_BYTES;      // 256 rows: 4,096 / 16,384 / 32,768
    static_assert(TM != PB || (A_SLOT_BYTES == H2_A_BYTES && A_PLANE_BYTES == H2_PLANE_BYTES), "full-height geometry unchanged");
    // B ring. Two slots (stage s+1 requested while stage s computes: two barrier intervals of latency cover) are enough when an interval is 24
    // MFMAs long; with half-height tiles an interval is 12 MFMAs (~0.2 us) and the L2 -> LDS latency of the weight planes (~0.8 us under load)
    // stalled every step at the vmcnt in front of its last barrier (profiles/r06c: 1.8 us per 128-row stage against 2.1 per 256-row stage).
    // Three slots there: stage s+2 is requested in LOAD(s, 0) and waited for at the end of LOAD(s+1, 1), six intervals later.
    constexpr int NB = TM == PB ? 2 : 3;
    constexpr int B_BASE = A_SLOTS * A_SLOT_BYTES;               // byte offset of the B slots (H2_B_BASE for the full-height two-slot modes)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, hi = lane >> 5;
    const int nk = K / BK;

    // ---- work list (identical to gemm_nt_f32_big_kernel)
    const int xcd = blockIdx.x % kNumXCD, j = blockIdx.x / kNumXCD;
    NtPlan pl = nt_plan(xcd, tiles_m, tiles_n, nk);
    if (TM != PB) pl.g = pl.rem > 0 ? 1 : 0;                     // half-height tiles are launched one whole-K item per workgroup: never K-split
    // Staggered start (es.stagger > 0, in 10 ns ticks of s_memrealtime: the tile period the host expects). Tiles take equal time, so all 256
    // workgroups run in phase: every CU multiplies while HBM idles, then every CU streams its 256 KB tile (+ 256 KB of residual) while the
    // matrix pipes idle - a short-K GEMM with a residual is the SUM of its matrix time and its memory time. Delaying workgroup j of an XCD
    // by (j mod 32) / 32 of a period spreads the phases; they stay spread (equal periods), and the chip overlaps one CU's epilogue with
    // another's main loop. Used by the extractor's short-K GEMMs (ext_linear); the MIL step's K >= 512 GEMMs are bound by the power cap, not by
    // this (profiles/r03r_nt_stagger.txt).
    if (es.stagger > 0) {
        const long long wait = ((long long)es.stagger * (j & 31)) >> 5, t_in = (long long)__builtin_amdgcn_s_memrealtime();
        while ((long long)__builtin_amdgcn_s_memrealtime() - t_in < wait) __builtin_amdgcn_s_sleep(16);
    }
    const bool has_part = j < pl.rem * pl.g;
    const int n_items = pl.rounds + (has_part ? 1 : 0);
    if (n_items == 0) return;
    const int part_tile = pl.g ? pl.rounds * PB_BLOCKS_PER_XCD + j / pl.g : 0;
    const int part = pl.g ? j % pl.g : 0;
    const int part_k0 = pl.g ? (part * nk) / pl.g : 0, part_k1 = pl.g ? ((part + 1) * nk) / pl.g : 0;
    auto item_tile = [&](int i) { return i < pl.rounds ? j + i * PB_BLOCKS_PER_XCD : part_tile; };
    auto item_k0 = [&](int i) { return i < pl.rounds ? 0 : part_k0; };
    auto item_k1 = [&](int i) { return i < pl.rounds ? nk : part_k1; };
    const int total = pl.rounds * nk + (has_part ? part_k1 - part_k0 : 0);

    // ---- staging
    const char *Ab = reinterpret_cast<const char *>(A), *Bpb = reinterpret_cast<const char *>(Bp);
    const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;
    unsigned aoff[2];
    const unsigned lane16 = lane * 16u;
    auto dma1 = [&](const char *sbase, unsigned voff, unsigned lds_byte) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_byte) : "memory");
    };
    // tile q of this XCD -> first row / column, column-tile index, exponent of the A scale of its 256-row block
    struct Tile { int m0, n0, tn, ke, tmi; };
    auto tile_of = [&](int q) {
        const int tmt = nt_row_tile(q, tiles_n, xcd);              // row tile (TM rows); tmi = the 256-row block its rows lie in (abs-max slot)
        const int tmi = TM == PB ? tmt : (tmt * TM) / PB;
        return Tile{tmt * TM, (q % tiles_n) * PB, q % tiles_n, (A16 || ARUN) ? 0 : h2_exp_from_amax(a_amax[tmi * a_stride]), tmi};
    };
    auto dma_b1 = [&](int slot, int kt, int tn, int i) {           // one 1 KiB piece of the linear copy of the pre-swizzled planes
        dma1(Bpb + (int64_t)(tn * nk + kt) * H2_B_BYTES + wave * 4096 + i * 1024, lane16,
             lds_base + B_BASE + (unsigned)slot * H2_B_BYTES + wave * 4096 + i * 1024);
    };
    auto dma_b = [&](int slot, int kt, int tn) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dma_b1(slot, kt, tn, i);
    };
    // PT: stage (row tile tmi, k-stage kt) of A = 32 KB contiguous (h plane, m plane), copied linearly; this wave moves 4 KB of it
    auto dma_a = [&](int slot, int kt, int tmi) {
        const char *src = Ab + ((int64_t)tmi * nk + kt) * (int64_t)H2_A_BYTES + wave * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) dma1(src + i * 1024, lane16, lds_base + (unsigned)slot * H2_A_BYTES + wave * 4096 + i * 1024);
    };

    // ---- fragment addressing
    // A is converted ONCE per element (round-2 ablation: every wave splitting its own raw fragments duplicated the work across
    // the two waves that share a row, and the LDS-DMA of raw fp32 + the splits were ~45 % of the kernel): a stage is 256 rows x
    // 32 k = 1024 octets of 8 k; thread t stages octets t and t + 512 (row (t>>2) + 128e, k-group t&3: four lanes cover one
    // row's 128 B), loads them straight into registers one stage ahead, splits them into the (h, m) fp16 octets = one MFMA
    // fragment entry each, and writes the plane image [plane][k-group][row ^ (k-group<<2)] (16-B entries; the XOR spreads the four
    // k-groups of a row over distinct banks for the writers and only permutes rows inside the 32-row block a reader fetches).
    const int swB = (li >> 2) & 3;
    const int bposb = B_BASE + (wn * 128 + li) * 64;                         // bytes, + plane*16384 + b*32*64
    const int kgrp_w = tid & 3;
    const unsigned wa_off = (unsigned)(kgrp_w * A_KG_BYTES + (((tid >> 2) ^ (kgrp_w << 2)) * 16));          // + e*128*16
    const unsigned ra_off0 = (unsigned)(hi * A_KG_BYTES + (((wm * WROWS + li) ^ (hi << 2)) * 16));             // k16 step 0: k-group hi
    const unsigned ra_off1 = (unsigned)((2 + hi) * A_KG_BYTES + (((wm * WROWS + li) ^ ((2 + hi) << 2)) * 16)); // k16 step 1: k-group 2 + hi
    // PT image of a stage (as it lies in memory): [plane][row 0..255][phys group 0..3][8 halves], phys = k-group ^ ((row >> 2) & 3)
    const unsigned rowA = (unsigned)(wm * 64 + li), swA = (rowA >> 2) & 3u;
    const unsigned rp_off0 = rowA * 64u + (((unsigned)hi) ^ swA) * 16u, rp_off1 = rowA * 64u + ((2u + (unsigned)hi) ^ swA) * 16u;
    auto read_a = [&](int slot, int s, h16x8 (&d)[NA][2]) {
        if (APT) {
            const char *base = reinterpret_cast<const char *>(smem) + slot * H2_A_BYTES + (s ? rp_off1 : rp_off0);
#pragma unroll
            for (int a = 0; a < NA; ++a) {           // sub-tile a: rows + 32 (the swizzle term (row >> 2) & 3 is unchanged)
                d[a][0] = *reinterpret_cast<const h16x8 *>(base + a * 2048);
                d[a][1] = *reinterpret_cast<const h16x8 *>(base + H2_PLANE_BYTES + a * 2048);
            }
            return;
        }
        const char *base = reinterpret_cast<const char *>(smem) + slot * A_SLOT_BYTES + (s ? ra_off1 : ra_off0);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            d[a][0] = *reinterpret_cast<const h16x8 *>(base + a * 512);
            if (!A16) d[a][1] = *reinterpret_cast<const h16x8 *>(base + A_PLANE_BYTES + a * 512);
        }
    };
    auto read_b = [&](int slot, int s, int b, h16x8 (&q)[2]) {
        const char *base = reinterpret_cast<const char *>(smem) + slot * H2_B_BYTES + bposb + b * 32 * 64 +
                           ((2 * s + hi) ^ swB) * 16;
#pragma unroll
        for (int p = 0; p < 2; ++p) q[p] = *reinterpret_cast<const h16x8 *>(base + p * H2_PLANE_BYTES);
    };
    f32x4 pa[2][2];                                                          // staged raw A: [octet e][lo/hi 4 floats]
    auto store_oct = [&](int slot, int e, float sc, f32x4 lo, f32x4 hi4v) {      // split one octet (8 floats) and write it to the plane image as octet e
        if (A16) {                                                           // the octet is already 8 halves
            char *dst16 = reinterpret_cast<char *>(smem) + slot * A_SLOT_BYTES + wa_off + e * (128 * 16);
            *reinterpret_cast<f32x4 *>(dst16) = lo;
            return;
        }
        const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi4v[0], hi4v[1], hi4v[2], hi4v[3]};
        h16x8 h, mm;
        h2_split8(x, sc, h, mm);
        char *dst = reinterpret_cast<char *>(smem) + slot * A_SLOT_BYTES + wa_off + e * (128 * 16);
        *reinterpret_cast<h16x8 *>(dst) = h;
        *reinterpret_cast<h16x8 *>(dst + A_PLANE_BYTES) = mm;
    };
    auto store_a = [&](int slot, int e, float sc) { store_oct(slot, e, sc, pa[e][0], pa[e][1]); };   // the staged octet e
    f32x16 acc[NA][4];
    auto zero_acc = [&]() {
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    // All fragments of one k16 step live in registers (A: 2 sub-tiles x 2 planes, B: 4 x 2 = 48 VGPRs): a wave's LOAD phase
    // fills them, its COMPUTE phase is 24 MFMAs and nothing else.
    h16x8 fa[NA][2], fb[4][2];
    auto read_frags = [&](int slot_a, int slot_b, int s) {
        read_a(slot_a, s, fa);
#pragma unroll
        for (int b = 0; b < 4; ++b) read_b(slot_b, s, b, fb[b]);
    };
    // three terms per product, small ones first; issue order keeps two MFMAs on one accumulator four issues apart
    auto compute = [&]() {
#define TOAD_T(B_, PA, PB_) \
        acc[0][B_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][PA], fb[B_][PB_], acc[0][B_], 0, 0, 0); \
        if (NA > 1) acc[NA - 1][B_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[NA - 1][PA], fb[B_][PB_], acc[NA - 1][B_], 0, 0, 0);
        if (A16) {
            TOAD_T(0, 0, 1) TOAD_T(1, 0, 1) TOAD_T(2, 0, 1) TOAD_T(3, 0, 1) TOAD_T(0, 0, 0) TOAD_T(1, 0, 0) TOAD_T(2, 0, 0) TOAD_T(3, 0, 0)
        } else if (NA == 1) {       // one sub-tile: all four column blocks per term, so that two MFMAs on one accumulator stay four issues apart
            TOAD_T(0, 1, 0) TOAD_T(1, 1, 0) TOAD_T(2, 1, 0) TOAD_T(3, 1, 0) TOAD_T(0, 0, 1) TOAD_T(1, 0, 1) TOAD_T(2, 0, 1) TOAD_T(3, 0, 1)
            TOAD_T(0, 0, 0) TOAD_T(1, 0, 0) TOAD_T(2, 0, 0) TOAD_T(3, 0, 0)
        } else {
            TOAD_T(0, 1, 0) TOAD_T(1, 1, 0) TOAD_T(0, 0, 1) TOAD_T(1, 0, 1) TOAD_T(0, 0, 0) TOAD_T(1, 0, 0)
            TOAD_T(2, 1, 0) TOAD_T(3, 1, 0) TOAD_T(2, 0, 1) TOAD_T(3, 0, 1) TOAD_T(2, 0, 0) TOAD_T(3, 0, 0)
        }
#undef TOAD_T
    };
    // ---- epilogue. acc holds (s_tile * t_col) * (A . B^T): rescaled by two exact power-of-two multiplies, then the usual chain.
    auto epilogue = [&](int m0, int n0, int tn, bool partial, int kexp) __attribute__((always_inline)) {
        constexpr int EPI_TILE_ROWS = TM, EPI_NA = NA, EPI_WROWS = WROWS;
        const int epi_rb = (m0 & (PB - 1)) + wm * WROWS;                      // the wave's first row inside its 256-row block
        const int epi_vwave = (epi_rb >> 6) * 2 + wn, epi_a0 = (epi_rb >> 5) & 1;  // (TM = 256: = wave, 0)
        float *epi_slab = slabs + (int64_t)blockIdx.x * PB * PB + wn * 128;
#include "gemm_h2_epilogue.inc"
    };

    // ---- main loop: the two waves of every SIMD alternate roles.
    // Round-2 counters showed why the lock-step version of this kernel kept the matrix pipe only ~40 % busy: the two waves a
    // 512-thread workgroup puts on one SIMD ran the same instruction mix at the same time, so their MFMA bursts collided and their
    // LDS reads / splits / address arithmetic (about as many issue cycles per stage as the MFMAs) left the pipe idle for both.
    // Here waves 0-3 (one per SIMD) and waves 4-7 (their partners) run the SAME program half a k16 step apart: a LOAD phase
    // (read the 48 fragment registers of the next k16 step from LDS, do a share of the staging of the stages ahead), a barrier,
    // a COMPUTE phase (24 back-to-back MFMAs, nothing else), a barrier. Group 1 takes one extra barrier first, so between any
    // two barriers one wave of each SIMD computes while its partner loads.
    //
    // Staging per stage s (k-stage of 32): B planes of stage s+1 by LDS-DMA (issued in LOAD(s,0), waited for at the end of
    // LOAD(s,1), three segments later); A rows of stage s+2 into registers (octet 0 in LOAD(s,0), octet 1 in LOAD(s,1)), split
    // and written to the plane image of stage s+2... one stage later (LOAD(s+1,.)), i.e. a full stage of latency cover.
    // LDS hazards (segments = barrier intervals, stage s is read in segments 4s..4s+3 counting both groups): slot (s+1)&1 was
    // last read in segment 4s-1 and is written in 4s..4s+3, first read in 4s+4.
    // A pass walks a LIST of this workgroup's items: pass 0 all of them (list position = item index); pass 1 - RUN mode only, and only when an
    // item was poisoned - the poisoned ones (list position i = the i-th set bit of redo_mask).
    int pass = 0;
    unsigned long long redo_mask = 0ull;               // RUN: items of pass 0 whose scale turned out too small
    auto L = [&](int i) {
        if (!ARUN || pass == 0) return i;
        unsigned long long m = redo_mask;
        for (int b = 0; b < i; ++b) m &= m - 1;
        return m ? (int)__builtin_ctzll(m) : 0;
    };
    struct Cursor { int it, kt, kend; };
    auto advance = [&](Cursor &c) {                    // -> true when the cursor entered a new item
        if (++c.kt != c.kend) return false;
        ++c.it; c.kt = item_k0(L(c.it)); c.kend = item_k1(L(c.it));
        return true;
    };
    // raw barrier (a __syncthreads() fence would also drain the A loads that are meant to stay in flight); the scheduling
    // fences keep MFMAs and splits on their own side of it
    auto barrier = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    const int grp = wave >> 2;
    // PACED: the LOAD / COMPUTE alternation of the two wave groups, locked by four barriers per step. It pays when a COMPUTE interval (24 MFMAs) is at
    // least as long as a LOAD interval. With half-height tiles a COMPUTE interval is 12 MFMAs (384 cycles) against the same ten fragment reads, the
    // splits, plane writes and LDS-DMA requests: the LOAD intervals set the pace and the barriers SERIALISE the two groups' LOAD work instead of hiding
    // it (PMC: waves parked 47 % of their cycles, profiles/r06j_pmc2_step_10k.txt). There the waves run free - ONE data barrier per step (this step's
    // plane writes / LDS-DMA before the next step's reads, this step's reads before the next step's writes) and the two waves of a SIMD interleave
    // by themselves: 2-8 % per kernel (profiles/r06n_half_tile_ablation.txt, which also shows that no single staging component owns the stage).
    constexpr bool PACED = TM == PB;
    auto pace = [&]() { if (PACED) barrier(); else __builtin_amdgcn_sched_barrier(0); };
    auto set_aoff1 = [&](int e, int m0) {
        aoff[e] = (unsigned)min(m0 + (tid >> 2) + 128 * e, M - 1) * (unsigned)(lda * (A16 ? 2 : 4)) + kgrp_w * (A16 ? 16 : 32);
    };
    auto load_a1 = [&](int e, int kt) {
        const float *src = reinterpret_cast<const float *>(Ab + kt * (BK * (A16 ? 2 : 4)) + aoff[e]);
        pa[e][0] = ld4(src);
        if (!A16) pa[e][1] = ld4(src + 4);
    };
    // RUN mode: the running maximum of the item being staged, its exponent (ke_next; ke_cur = the exponent the accumulators are in), whether
    // it has outgrown the room above its first stage (poisoned), and the list of poisoned items for the second pass
    constexpr int RUN_BASE = B_BASE + NB * H2_B_BYTES;                                          // behind the B slots (= H2_SMEM for full-height tiles)
    float *run_scr = reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + RUN_BASE);     // [stage parity | item end][8 waves]
    int *redo_ke = reinterpret_cast<int *>(run_scr + 32);                                       // [64] exponent of a poisoned item's true maximum
    char *run_park = reinterpret_cast<char *>(smem) + RUN_BASE + 512;                           // [512 threads][32 B]: octet 0 of an item's first stage, raw
    float run_tmax = 0.f, run_tmax_prev = 0.f;          // per LANE: max |x| over the elements this lane staged for the item being staged / the one before
    int ke_cur = 0, ke_next = 0;
    constexpr bool E1 = NA > 1;                         // a thread stages a second octet (rows + 128) per stage
    auto pa_lane_max = [&]() {                          // max |x| over the raw elements this lane holds (16, or 8 for half-height tiles)
        const float m0_ = __builtin_fmaxf(h2_absmax4(pa[0][0]), h2_absmax4(pa[0][1]));
        return E1 ? __builtin_fmaxf(m0_, __builtin_fmaxf(h2_absmax4(pa[1][0]), h2_absmax4(pa[1][1]))) : m0_;
    };
    auto run_local_max = [&]() { return h2_wave_max_dpp(pa_lane_max()); };     // ... over the wave
    auto run_stage_max = [&](int par) {                 // wave-uniform by construction: handed to the scalar unit (the loop runs at the VGPR limit)
        const f32x4 r0 = ld4(run_scr + par * 8), r1 = ld4(run_scr + par * 8 + 4);
        const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(r0[0], r0[1]), __builtin_fmaxf(r0[2], r0[3])),
                                        __builtin_fmaxf(__builtin_fmaxf(r1[0], r1[1]), __builtin_fmaxf(r1[2], r1[3])));
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, m)));
    };
    int total_p = total;                               // k-steps of the pass
    for (; pass < (ARUN ? 2 : 1); ++pass) {
    if (ARUN && pass == 1) {
        // both wave groups have passed the same number of barriers here (the prologue's extra one of group 1 is balanced by group 0's at the
        // last item), so a plain barrier lines them up; it also orders thread 0's redo_ke writes before everybody's reads
        if (redo_mask == 0ull) break;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        total_p = 0;
        for (unsigned long long m = redo_mask; m; m &= m - 1) { const int it = (int)__builtin_ctzll(m); total_p += item_k1(it) - item_k0(it); }
    }
    const int total = total_p;                         // (shadows the plan's total inside the pass)
    Cursor c0{0, item_k0(L(0)), item_k1(L(0))}, c1 = c0;
    bool c1_first = false;                             // the stage c1 points at opens an item
    Tile t0 = tile_of(item_tile(L(0))), t1 = t0;
    // prologue: stage 0 complete in slot 0; stage 1 on its way (registers, or - PT - the second A slot)
    int aoff_m0[2] = {t0.m0, t0.m0};                   // tile row the per-lane A offsets of octet e currently describe
    zero_acc();
    if (APT) {
        dma_a(0, c0.kt, t0.tmi);
        dma_b(0, c0.kt, t0.tn);
        if (total > 1) {
            if (advance(c1)) t1 = tile_of(item_tile(L(c1.it)));
            dma_a(1, c1.kt, t1.tmi);
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // A(0), B(0) landed; A(1) stays in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    } else {
        set_aoff1(0, t0.m0); if (E1) set_aoff1(1, t0.m0);
        load_a1(0, c0.kt); if (E1) load_a1(1, c0.kt);
        dma_b(0, c0.kt, t0.tn);
        if (ARUN) {                                    // stage 0's own maximum decides the first item's scale: one exchange before the groups separate
            const float m = run_local_max();
            if (lane == 0) run_scr[wave] = m;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            run_tmax = pa_lane_max();
            ke_cur = ke_next = pass ? redo_ke[L(0)] : h2_exp_from_amax(run_stage_max(0)) - RUN_MARGIN;
            t0.ke = ke_cur;
        }
        store_a(0, 0, h2_pow2(t0.ke));
        if (E1) store_a(0, 1, h2_pow2(t0.ke));
        if (total > 1) {
            if (advance(c1)) { t1 = tile_of(item_tile(L(c1.it))); c1_first = true; }
            if (t1.m0 != t0.m0) { set_aoff1(0, t1.m0); if (E1) set_aoff1(1, t1.m0); aoff_m0[0] = aoff_m0[1] = t1.m0; }
        }
        if (NB == 3 && total > 1) dma_b(1, c1.kt, t1.tn);  // three B slots: stage 1's planes are requested here, every later stage two steps ahead
        load_a1(0, c1.kt); if (E1) load_a1(1, c1.kt);      // (a repeat of stage 0 when there is only one stage)
        if (NB == 3) {                                     // B(0) has landed; B(1) (4 requests per wave, when there is a stage 1) and the stage-1 loads (2; 1 for fp16 A) stay in flight
            if (total > 1) { if (A_LD == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); }
            else if (A_LD == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        } else if (A16 || !E1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // B(0) has landed; the stage-1 loads (4; 2 for fp16 A or one octet) stay in flight
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    barrier();
    if (PACED && grp == 1) barrier();                  // group 1 runs one segment behind
    Cursor c2 = c1; Tile t2 = t1;                      // stage step + 2: the rows being loaded (registers / third A slot)
    int sa = 0;                                        // PT: A slot of stage `step` (step % 3); half-height tiles: B slot of stage `step` (same ring arithmetic)
    for (int step = 0; step < total; ++step) {
        const int sb = step & 1;
        const int sbb = NB == 3 ? sa : sb;                 // B slot of stage `step`
        const bool more = (step + 1) < total, more2 = (step + 2) < total;
        const float s_nxt = h2_pow2(t1.ke);
        bool c2_first = false;
        if (more2 && advance(c2)) { t2 = tile_of(item_tile(L(c2.it))); c2_first = true; }
        const int sa2 = sa == 0 ? 2 : sa - 1;          // (step + 2) % 3
        const int slot_a = APT ? sa : sb;
        // ===== LOAD(step, 0)
        // RUN: an item's scale is fixed by its first stage, so a stage INSIDE an item is split on the a_amax path's schedule (octet 0 here, octet 1 in
        // LOAD(step,1), their successors loaded behind them: a full step of latency cover) and only folded into the lane's running maximum. The stage
        // that OPENS an item (run_boundary, once per tile) cannot be split before the eight wave maxima have crossed this step's barrier: its octet 0
        // is parked raw in LDS here (the lane reads it back itself in LOAD(step,1)), so that the loads stay in ONE code path at their usual places -
        // with loads in both branches hipcc kept the staged rows in different registers per path and guarded the merge with vmcnt(0) on every step.
        const bool run_boundary = ARUN && more && c1_first;                // (a flag carried with the cursor: no plan arithmetic on the step's path)
        const bool run_last = ARUN && (c0.kt + 1 == c0.kend);             // this step completes the item the accumulators belong to
        if (ARUN) {                                    // (in front of the fragment reads: measured 5 us faster per 100k-patch bag than behind them)
            if (run_boundary) { run_tmax_prev = run_tmax; run_tmax = 0.f; }
            run_tmax = __builtin_fmaxf(run_tmax, __builtin_fmaxf(h2_absmax4(pa[0][0]), h2_absmax4(pa[0][1])));
        }
        if (ARUN && run_boundary) {
            // (opaque to the optimiser: otherwise hipcc hoists this path's |x| of the SECOND octet above the branch, and the wait for those
            //  loads - issued half a step ago - lands on every step of the common path)
            f32x4 q0 = pa[E1 ? 1 : 0][0], q1 = pa[E1 ? 1 : 0][1];              // (one octet per stage: run_tmax already holds it)
            asm volatile("" : "+v"(q0), "+v"(q1));
            const float m = h2_wave_max_dpp(__builtin_fmaxf(run_tmax, __builtin_fmaxf(h2_absmax4(q0), h2_absmax4(q1))));
            if (lane == 0) run_scr[((step + 1) & 1) * 8 + wave] = m;
            *reinterpret_cast<f32x4 *>(run_park + tid * 32) = pa[0][0];
            *reinterpret_cast<f32x4 *>(run_park + tid * 32 + 16) = pa[0][1];
        }
        read_frags(slot_a, sbb, 0);
        if (APT) {
            // B(step+1) first, then A(step+2): the vmcnt(4) below then covers B(step+1) and the older A(step+1). Slot (step+2) % 3 held
            // stage step-1, whose last reader (group 1, LOAD(step-1, 1)) finished before the barrier that opened this segment.
            if (more) dma_b(sb ^ 1, c1.kt, t1.tn);
            if (more2) dma_a(sa2, c2.kt, t2.tmi);
        } else {
            // octet 0 of stage step+1 (unconditional: see gemm_tn_h2_big_kernel - also at a RUN boundary, where it is split with the OLD item's
            // exponent; LOAD(step,1) overwrites those entries with the parked octet under the right one before anybody reads them)
            store_a(sb ^ 1, 0, ARUN ? h2_pow2(ke_next) : s_nxt);
            if (NB == 3) { if (more2) dma_b(sa2, c2.kt, t2.tn); }          // slot (step + 2) % 3 held stage step-1: its last reader finished before the barrier that opened this segment
            else if (more) dma_b(sb ^ 1, c1.kt, t1.tn);
            // (tried: the four requests between the MFMAs of COMPUTE(step, 0) instead - an LDS-DMA issue costs a wave ~85 cycles and this interval
            //  carries all of the staging; neutral within the box-to-box spread, profiles/r06k_*, so the simpler placement stays)
            if (t2.m0 != aoff_m0[0]) { set_aoff1(0, t2.m0); aoff_m0[0] = t2.m0; }
            load_a1(0, c2.kt);
        }
        pace();
        // ===== COMPUTE(step, 0)
        compute();
        pace();
        // ===== LOAD(step, 1)
        if (ARUN && run_boundary) {                    // (again in front of the fragment reads)
            // stage step+1 opens an item: every wave forms the same stage maximum from the eight wave maxima the groups wrote in their LOAD(step,0)
            // segments; with RUN_MARGIN bits of room it sets the item's exponent (pass 1: the exponent of the item's known true maximum). The
            // parked octet 0 comes back and is split with it; octet 1 follows in the common code below.
            ke_next = pass ? redo_ke[L(c1.it)] : h2_exp_from_amax(run_stage_max((step + 1) & 1)) - RUN_MARGIN;
            const f32x4 p0 = *reinterpret_cast<const f32x4 *>(run_park + tid * 32), p1 = *reinterpret_cast<const f32x4 *>(run_park + tid * 32 + 16);
            store_oct(sb ^ 1, 0, h2_pow2(ke_next), p0, p1);
        }
        if (ARUN && E1) run_tmax = __builtin_fmaxf(run_tmax, __builtin_fmaxf(h2_absmax4(pa[1][0]), h2_absmax4(pa[1][1])));
        if (ARUN && run_last) {
            // the finished item's maximum over this wave's lanes, for the exchange at the item's end (all its stages were folded long ago; its
            // successor's first stage has been going into a fresh run_tmax since LOAD(step,0))
            const float m = h2_wave_max_dpp(run_boundary ? run_tmax_prev : run_tmax);
            if (lane == 0) run_scr[16 + wave] = m;
        }
        read_frags(slot_a, sbb, 1);
        if (APT) {
            if (more2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // A(step+2) may stay in flight
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            if (E1) {
                store_a(sb ^ 1, 1, ARUN ? h2_pow2(ke_next) : s_nxt);
                if (t2.m0 != aoff_m0[1]) { set_aoff1(1, t2.m0); aoff_m0[1] = t2.m0; }
                load_a1(1, c2.kt);
            }
            if (NB == 3) {          // B(step+1) (requested a step ago) done; this step's B(step+2) requests (4 per wave, if any) and A loads (2; 1 for fp16 A) stay in flight
                if (more2) { if (A_LD == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); }
                else if (A_LD == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            } else if (A16 || !E1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // B(step+1) (and older stores) done; the A loads (4 / 2) stay in flight
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
        pace();
        // ===== COMPUTE(step, 1)
        compute();
        barrier();
        if (++c0.kt == c0.kend) {
            // Group 0 finishes an item one segment before group 1. Back to back, each epilogue would stall the other group at the
            // next barrier (exposed time = both epilogues). Group 0 instead idles for ONE segment (the barrier below pairs with
            // group 1's last COMPUTE), the two epilogues then run in the same segment and share the SIMDs like ordinary waves, and
            // group 1 drops back to one segment behind with the barrier after its epilogue (it pairs with group 0's LOAD(step+1,0)).
            if (PACED && grp == 0) barrier();
            const bool part_item = L(c0.it) >= pl.rounds && pl.g > 1;                // (an unsplit remainder tile is an ordinary tile)
            bool skip = false;
            if (ARUN) {
                // the item's true maximum: the eight wave maxima written in LOAD(step,1) of this step (both groups are past the barrier that follows
                // it). It must fit under fp16's last finite value 65,504 with the item's exponent - up to [2^14, 2^15) is allowed - else the item is
                // poisoned: its accumulators may hold infinities, the epilogue is skipped and pass 1 repeats the item with the right exponent
                const float fin = run_stage_max(2);
                skip = pass == 0 && h2_exp_from_amax(fin) < ke_cur - 1;
                if (skip) redo_mask |= 1ull << c0.it;
                if (tid == 0) {
                    h2_atomic_amax(a_amax_out + t0.tmi, fin);
                    if (skip) redo_ke[c0.it] = h2_exp_from_amax(fin);
                    else if (part_item) slab_ke[blockIdx.x] = ke_cur;
                }
                t0.ke = ke_cur;
            }
            if (!skip) epilogue(t0.m0, t0.n0, t0.tn, part_item, t0.ke);
            zero_acc();
            if (ARUN) ke_cur = ke_next;
            if (PACED && grp == 1 && more) barrier();
            ++c0.it; c0.kt = item_k0(L(c0.it)); c0.kend = item_k1(L(c0.it));
        }
        t0 = t1;
        if (more2) { c1 = c2; t1 = t2; c1_first = c2_first; }
        sa = sa == 2 ? 0 : sa + 1;
    }
    }   // pass
}

// Remainder tiles of the h2 kernel: C tile = epilogue( (sum of the g K-slice slabs) / (s_tile t_col) ), fixed order; same grid
// as nt_fixup_kernel. Also contributes to y_amax.
template <int R>          // rows per thread: 4 (16 rows per workgroup), or 1 when the launch has so few tiles that thread count matters more
__global__ __launch_bounds__(256) void nt_fixup_h2_kernel(const float *__restrict__ slabs, const float *__restrict__ a_amax,
                                                           const float *__restrict__ binv, float *C, int64_t ldc, int M, int N,
                                                           int K, const float *__restrict__ bias, EpiScalars es, const float *addend,
                                                           const float *__restrict__ mask_src, const float *__restrict__ pool_araw,
                                                           const float *__restrict__ pool_stats, const float *__restrict__ pool_dM, int pool_T,
                                                           float *y_amax, int tiles_m, int tiles_n, int a_stride, int y_stride,
                                                           const int *__restrict__ slab_ke) {
    // slab_ke (RUN mode of the GEMM, else NULL): the exponent each K-slice's partial sums were accumulated with; a slice whose own maximum was
    // smaller than the tile's carries a larger exponent and is brought to the tile's (kexp, from the completed abs-max array) by an exact factor
    __shared__ float s_max[4];
    const int xcd = blockIdx.z, tr = blockIdx.y;
    const NtPlan pl = nt_plan(xcd, tiles_m, tiles_n, K / BK);
    if (tr >= pl.rem || pl.g <= 1) return;                 // g == 1: the GEMM kernel wrote the tile itself
    const int q = pl.rounds * PB_BLOCKS_PER_XCD + tr;
    const int tmi = (q / tiles_n) * kNumXCD + xcd;
    const int m0 = tmi * PB, n0 = (q % tiles_n) * PB;
    const int c4 = threadIdx.x & 63;
    const int col = n0 + c4 * 4;
    float amx = 0.f;
    if (col < N) {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (bias) bv = ld4(bias + col);
        const f32x4 iv = ld4(binv + col);
        const int kexp = a_amax ? h2_exp_from_amax(a_amax[tmi * a_stride]) : 0;      // NULL: an fp16 A operand (scale 1)
        const float f1 = h2_descale_first(kexp);
        f32x4 f2;
#pragma unroll
        for (int k = 0; k < 4; ++k) f2[k] = h2_descale_second(kexp, -h2_exp_of_pow2(iv[k]));
        f32x4 dm0 = {0.f, 0.f, 0.f, 0.f}, dm1 = {0.f, 0.f, 0.f, 0.f};
        float pmx0 = 0.f, pil0 = 0.f, pmx1 = 0.f, pil1 = 0.f;
        const int pool_stride = pool_T >> 8;             // > 0: per-row records + per-slide dM (the batched form, gemm_h2_epilogue.inc PBATCH)
        if (pool_T > 0 && !pool_stride) {
            dm0 = ld4(pool_dM + col); pmx0 = pool_stats[0]; pil0 = 1.f / pool_stats[1];
            if (pool_T > 1) { dm1 = ld4(pool_dM + N + col); pmx1 = pool_stats[2]; pil1 = 1.f / pool_stats[3]; }
        }
        // 16 rows per workgroup: a thread owns one 16-byte column group of FOUR rows (rows rg, rg + 4, rg + 8, rg + 12 of the block's 16)
        // and issues all of their loads - g slabs, mask, addend / raw scores - before the first use: the kernel is a chain of
        // dependent memory round trips (parameters -> slabs -> operands -> store), and with one row per thread it ran at 2.2 TB/s.
        const int rg = threadIdx.x >> 6;
        const float *sp0 = slabs + ((int64_t)(xcd + kNumXCD * (tr * pl.g)) * PB) * PB + c4 * 4;
        const int64_t sstride = (int64_t)kNumXCD * PB * PB;
        auto slab_f = [&](int p) { return slab_ke ? h2_pow2(max(kexp - slab_ke[xcd + kNumXCD * (tr * pl.g + p)], -126)) : 1.f; };
        f32x4 v[R], av[R], mv[R];
        int lrow[R];
        bool ok[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lrow[r] = blockIdx.x * (4 * R) + rg + 4 * r;
            ok[r] = (m0 + lrow[r]) < M;
            const int lr = ok[r] ? lrow[r] : 0;                          // clamped: loaded, never stored
            v[r] = ld4(sp0 + (int64_t)lr * PB);
            if (slab_ke) v[r] *= slab_f(0);
            const int64_t off = (int64_t)min(m0 + lr, M - 1) * ldc + col;
            av[r] = addend ? ld4(addend + off) : f32x4{0.f, 0.f, 0.f, 0.f};
            mv[r] = mask_src ? ld4(mask_src + off) : f32x4{1.f, 1.f, 1.f, 1.f};
            if (pool_stride) {
                av[r] = ld4(pool_araw + (int64_t)min(m0 + lr, M - 1) * 4);
            } else if (pool_T > 0) {
                const int64_t row = min(m0 + lr, M - 1);
                av[r][0] = pool_araw[row * pool_T];
                av[r][1] = pool_T > 1 ? pool_araw[row * 2 + 1] : 0.f;
            }
        }
        int p = 1;
        for (; p + 3 < pl.g; p += 4) {                                   // fixed order: deterministic; 16 slab loads in flight per step
            f32x4 t[4][R];
#pragma unroll
            for (int pp = 0; pp < 4; ++pp)
#pragma unroll
                for (int r = 0; r < R; ++r) t[pp][r] = ld4(sp0 + (p + pp) * sstride + (int64_t)(ok[r] ? lrow[r] : 0) * PB);
            if (slab_ke) {
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {
                    const float f = slab_f(p + pp);
#pragma unroll
                    for (int r = 0; r < R; ++r) t[pp][r] *= f;
                }
            }
#pragma unroll
            for (int pp = 0; pp < 4; ++pp)
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] += t[pp][r];
        }
        for (; p < pl.g; ++p) {
            f32x4 t[R];
#pragma unroll
            for (int r = 0; r < R; ++r) t[r] = ld4(sp0 + p * sstride + (int64_t)(ok[r] ? lrow[r] : 0) * PB);
            if (slab_ke) {
                const float f = slab_f(p);
#pragma unroll
                for (int r = 0; r < R; ++r) t[r] *= f;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] += t[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            f32x4 x = (v[r] * f1) * f2;
            f32x4 a = av[r];
            if (pool_stride) {
                const float *dmr = pool_dM + (int64_t)(int)h2_bits(av[r][2]) * pool_stride;
                a = av[r][0] * ld4(dmr + col) + av[r][1] * ld4(dmr + N + col);
            } else if (pool_T > 0) {
                a = (h2_fast_exp(av[r][0] - pmx0) * pil0) * dm0;
                if (pool_T > 1) a += (h2_fast_exp(av[r][1] - pmx1) * pil1) * dm1;
            }
            x = apply_epilogue_v(x, es, a, addend != nullptr || pool_T > 0, mv[r], mask_src != nullptr, bv,
                                 (uint64_t)(m0 + lrow[r]) * (uint64_t)N + (uint64_t)col);
            if (ok[r]) {
                amx = __builtin_fmaxf(amx, h2_absmax4(x));
                st4s(C + (int64_t)(m0 + lrow[r]) * ldc + col, x);
            }
        }
    }
    if (y_amax) {           // one atomic per workgroup (64 share a tile's slot; per wave it was 256, and contended device-scope atomics cost ~150 ns each)
        amx = h2_wave_max(amx);
        if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = amx;
        __syncthreads();
        if (threadIdx.x == 0)
            h2_atomic_amax(y_amax + tmi * y_stride, __builtin_fmaxf(__builtin_fmaxf(s_max[0], s_max[1]), __builtin_fmaxf(s_max[2], s_max[3])));
    }
}

// ------------------------------------------------------------------------------------------
// TN (wgrad), persistent 256x256, h2 arithmetic:  slab[s][I,J] = (sA sB) * sum_{m in split s} A[m,I] B[m,J]
//
// Same work decomposition, slabs and column sums as gemm_tn_f32_big_kernel. Both operands are activations and the reduction runs
// over ROWS, so an MFMA fragment is 8 consecutive rows of one column: the operands cannot be consumed as they lie in memory.
// Round-2 ablation of the first version (fp32 rows staged by LDS-DMA, every wave splitting its own fragments: 48 elements per lane
// per 16-deep step, 3x redundant across the waves that share a fragment) showed the splits alone cost 45 % of the kernel. This
// version converts each element ONCE: a stage is 32 rows x (256 A + 256 B columns); even waves stage A, odd waves B, wave pair
// rg the rows 8rg..8rg+7. A lane loads 8 rows x 4 columns straight into registers (8 x 16 B, one stage ahead), splits each
// column's 8 rows into the (h, m) fp16 octets = exactly one MFMA fragment entry, and writes them to the LDS plane image
// [k-group][fragment order] that every wave then reads with ds_read_b128 (12 per 16-deep step instead of 16 wider ones).
// 32 elements per lane per stage (64 VALU ops) against 48 MFMAs; 128 KB of LDS (2 stages x 2 planes x 32 KB) + 4 KB for the
// column sums, which are accumulated from the same registers.
// Step order (s_memtime phases, profiles/r02at): the next stage's loads issue between the MFMAs of the first 16-deep unit, its splits and
// plane writes are spread over the second unit, and the step barrier sits in front of the last six MFMAs (they cover the next fragment reads).
// ONE scale per operand: the maximum over the operand's amax array (every block reduces the two short arrays itself).
// scale_out[0..1] = 1/sA, 1/sB for slab_reduce_h2_kernel, which applies them while summing the splits.
// ------------------------------------------------------------------------------------------
constexpr int TN2_PLANE = 4 * 512 * 16;                 // bytes of one plane of one stage: 4 k-groups x 512 columns x 8 halves
constexpr int TN2_STAGE = 2 * TN2_PLANE;
constexpr int TN2_SMEM = 2 * TN2_STAGE + 4 * PB * 4;    // + column-sum scratch [4][256] floats

// B16 = true: the B operand (the saved INPUT of the layer: the feature bag) is an fp16 matrix (ldb in halves): its elements are first
// pieces with scale 1 (see gemm_nt_h2_big_kernel's A16), the odd waves transpose octets with byte permutes instead of splitting, only
// B's h plane exists and a product is two MFMA terms (m_a.h_b + h_a.h_b).
// ONE_ITEM (round 6, the batched launch below): the workgroup runs exactly one item (one_split, one_tile) of the product it was handed instead of
// walking the per-XCD plan; `write_scale` names the workgroup that publishes the operand scales for the slab reduction.
template <bool B16, bool ONE_ITEM>
__device__ __forceinline__ void gemm_tn_h2_body(
    const float *__restrict__ A, int64_t lda, const float *__restrict__ a_amax, const float *__restrict__ B, int64_t ldb,
    const float *__restrict__ b_amax, float *__restrict__ slab, float *__restrict__ colsum_slab, float *__restrict__ scale_out,
    int Mred, int I, int J, int rows_per_split, int ti, int tj, int nsplit, int one_split, int one_tile, bool write_scale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char *smem_b = reinterpret_cast<char *>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const int li = lane & 31, hi = lane >> 5;
    const int tiles = ti * tj;

    const int xcd = blockIdx.x % kNumXCD, jb = blockIdx.x / kNumXCD;
    const int splits_x = (nsplit - xcd + kNumXCD - 1) / kNumXCD;
    const int items_x = splits_x * tiles;
    const int n_items = ONE_ITEM ? 1 : (jb < items_x ? (items_x - jb + PB_BLOCKS_PER_XCD - 1) / PB_BLOCKS_PER_XCD : 0);
    // ---- operand scales: max over the amax arrays (block-wide, through the not yet used LDS)
    {
        const int nblk = (Mred + H2_ROWBLK - 1) / H2_ROWBLK;
        float ma = 0.f, mb = 0.f;
        for (int i = tid; i < nblk; i += 512) { ma = __builtin_fmaxf(ma, a_amax[i]); if (!B16) mb = __builtin_fmaxf(mb, b_amax[i]); }
        ma = h2_wave_max(ma); mb = h2_wave_max(mb);
        if (lane == 0) { smem[wave] = ma; smem[8 + wave] = mb; }
        __syncthreads();
    }
    float gma = 0.f, gmb = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { gma = __builtin_fmaxf(gma, smem[w]); gmb = __builtin_fmaxf(gmb, smem[8 + w]); }
    __syncthreads();                                          // scratch is read before any stage may be written over it
    const int kea = h2_exp_from_amax(gma), keb = B16 ? 0 : h2_exp_from_amax(gmb);
    if (write_scale && tid == 0) { scale_out[0] = h2_pow2(-kea); scale_out[1] = h2_pow2(-keb); }
    if (n_items == 0) return;
    auto item_split = [&](int i) { return ONE_ITEM ? one_split : ((jb + i * PB_BLOCKS_PER_XCD) / tiles) * kNumXCD + xcd; };
    auto item_tile = [&](int i) { return ONE_ITEM ? one_tile : (jb + i * PB_BLOCKS_PER_XCD) % tiles; };
    auto split_steps = [&](int sp) {
        const int mb = sp * rows_per_split, me = min(Mred, mb + rows_per_split);
        return (me - mb + BK - 1) / BK;
    };
    int total = 0;
    for (int i = 0; i < n_items; ++i) total += split_steps(item_split(i));

    // ---- staging role of this wave (wave-uniform): operand, its 8 rows of the stage, the lane's 4 columns
    const bool opB = (wave & 1) != 0;
    const int rg = wave >> 1;
    const char *srcb = opB ? reinterpret_cast<const char *>(B) : reinterpret_cast<const char *>(A);
    const bool half_src = B16 && opB;                         // this wave stages the fp16 operand
    const int64_t src_ld = (opB ? ldb : lda) * (half_src ? 2 : 4);
    const int src_cols = opB ? J : I;
    const float sS = h2_pow2(opB ? keb : kea);
    // plane-image position (16-B entries) of column c of the tile, in FRAGMENT order so that the readers' 32 lanes are contiguous:
    //   A column wi*64 + 2*li + a -> wi*64 + a*32 + li ;  B column wj*128 + 4*li + b -> 256 + wj*128 + b*32 + li
    // this lane stages columns 4*lane + j: j -> entry w_base + (A: (j&1)*32 + (j>>1) ; B: j*32)
    const unsigned w_base = (unsigned)(rg * 512 + (opB ? 256 + (lane >> 5) * 128 + (lane & 31) : (lane >> 4) * 64 + 2 * (lane & 15))) * 16u;
    const unsigned w_j1 = opB ? 32u * 16u : 32u * 16u, w_j2 = opB ? 64u * 16u : 16u, w_j3 = opB ? 96u * 16u : 33u * 16u;
    unsigned coff = 0;                                        // byte offset of the lane's 4 columns in a source row
    int st_i0 = 0, st_j0 = 0, st_mend = 0;
    auto set_item = [&](int i, int &mrow) {
        const int sp = item_split(i), tl = item_tile(i);
        st_i0 = (tl / tj) * PB; st_j0 = (tl % tj) * PB;
        mrow = sp * rows_per_split;
        st_mend = min(Mred, mrow + rows_per_split);
        coff = half_src ? (unsigned)min(st_j0 + 8 * (lane & 31), src_cols - 8) * 2u      // 8 halves = 16 B per row, lanes 0-31 (32-63 repeat them)
                        : (unsigned)min((opB ? st_j0 : st_i0) + 4 * lane, src_cols - 4) * 4u;
    };
    f32x4 px[8];
    auto stage_load = [&](int m, int r0, int r1) {
        // one code path for both roles: 16 B per lane per row (4 fp32 columns, or - fp16 operand - 8 columns in lanes 0-31). A role
        // branch here (8-byte loads for the fp16 rows) made hipcc serialise the loads behind path-insensitive waits.
        // scalar address work per row: one 64-bit base per stage, then a 32-bit clamped row offset (min, mul, add/addc) instead of a
        // full 64-bit row * stride + base chain (the kernel issued ~170 scalar instructions per stage)
        const char *pb = srcb + (int64_t)m * src_ld;
        const int lim = Mred - 1 - m;                         // last valid row of the operand, relative to the stage (>= 0)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < r0 || r >= r1) continue;
            const unsigned ro = (unsigned)min(rg * 8 + r, lim) * (unsigned)src_ld;
            px[r] = ld4(reinterpret_cast<const float *>(pb + ro + coff));
        }
    };
    float bs[4] = {0.f, 0.f, 0.f, 0.f}, fin[4] = {0.f, 0.f, 0.f, 0.f};
    // rows at or beyond `mend` count as zeros; the A-staging waves add their rows into the column sums
    auto stage_prep = [&](int m, int mend, bool cs) {
        if (m + 32 > mend) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (m + rg * 8 + r >= mend) px[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (cs && !opB) {
#pragma unroll
            for (int r = 0; r < 8; ++r) { bs[0] += px[r][0]; bs[1] += px[r][1]; bs[2] += px[r][2]; bs[3] += px[r][3]; }
        }
    };
    // split column j of the staged registers (8 rows = one fragment entry) and write it to the plane image of stage `buf`
    auto stage_col = [&](int buf, int j) {
        char *img = smem_b + buf * TN2_STAGE + w_base;
        if (half_src) {               // fp16 operand: this call transposes the lane's columns 2j, 2j+1 (word j of every row, halves 0 / 1)
            // tile column 8L + t (L = lane & 31) is B column wj*128 + 4*li + b with wj = L >> 4, li = 2*(L & 15) + (t >> 2), b = t & 3
            char *img16 = smem_b + buf * TN2_STAGE + (unsigned)(rg * 512 + 256 + ((lane & 31) >> 4) * 128 + 2 * (lane & 15) + (j >> 1)) * 16u;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                u32x4 hp;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (copy the vector elements to scalars first: __builtin_bit_cast applied directly to a vector-element expression
                    //  read element 0 whatever the index - hipcc 7.2)
                    const float f_lo = px[2 * e][j], f_hi = px[2 * e + 1][j];
                    hp[e] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, f_hi), __builtin_bit_cast(unsigned, f_lo),
                                                  tt ? 0x07060302u : 0x05040100u);
                }
                if (lane < 32) *reinterpret_cast<u32x4 *>(img16 + (2 * (j & 1) + tt) * 512) = hp;
            }
            return;
        }
        float x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = px[r][j];
        h16x8 h, mm;
        h2_split8(x, sS, h, mm);
        const unsigned o = j == 0 ? 0u : j == 1 ? w_j1 : j == 2 ? w_j2 : w_j3;
        *reinterpret_cast<h16x8 *>(img + o) = h;
        *reinterpret_cast<h16x8 *>(img + TN2_PLANE + o) = mm;
    };

    // ---- fragment reads: k-group 2s + hi of stage `buf`
    const unsigned ra_off = (unsigned)(hi * 512 + wi * 64 + li) * 16u, rb_off = (unsigned)(hi * 512 + 256 + wj * 128 + li) * 16u;
    auto read_a = [&](int buf, int s, h16x8 (&d)[2][2]) {
        const char *b = smem_b + buf * TN2_STAGE + s * (2 * 512 * 16) + ra_off;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            d[a][0] = *reinterpret_cast<const h16x8 *>(b + a * 512);
            d[a][1] = *reinterpret_cast<const h16x8 *>(b + TN2_PLANE + a * 512);
        }
    };
    auto read_b = [&](int buf, int s, int bb, h16x8 (&d)[2]) {
        const char *b = smem_b + buf * TN2_STAGE + s * (2 * 512 * 16) + rb_off + bb * 512;
        d[0] = *reinterpret_cast<const h16x8 *>(b);
        if (!B16) d[1] = *reinterpret_cast<const h16x8 *>(b + TN2_PLANE);
    };
    f32x16 acc[2][4];
    auto zero_acc = [&]() {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    auto mma6 = [&](int b, const h16x8 (&ap)[2][2], const h16x8 (&bq)[2]) {
#define TOAD_T(PA, PB_) \
        acc[0][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ap[0][PA], bq[PB_], acc[0][b], 0, 0, 0); \
        acc[1][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ap[1][PA], bq[PB_], acc[1][b], 0, 0, 0);
        TOAD_T(1, 0)
        if (!B16) { TOAD_T(0, 1) }
        TOAD_T(0, 0)
#undef TOAD_T
    };
    float *cs_scr = reinterpret_cast<float *>(smem_b + 2 * TN2_STAGE);
    auto epilogue = [&](int sp, int i0, int j0, bool with_colsum) {
        int li4 = 4 * li, hi4 = 4 * hi;
        asm volatile("" : "+v"(li4), "+v"(hi4));
        float *out = slab + (int64_t)sp * I * J;
        const int col = j0 + wj * 128 + li4;
        const bool cok = col < J;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wi * 64 + 2 * ((r & 3) + 8 * (r >> 2) + hi4) + a;
                f32x4 v = {acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
                if (cok && row < I) st4(out + (int64_t)row * J + col, v);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (with_colsum) {                  // block-uniform: the four A-staging waves hold the sums of their 8 rows of every stage
            if (!opB) st4(cs_scr + rg * PB + 4 * lane, f32x4{fin[0], fin[1], fin[2], fin[3]});
            __syncthreads();
            if (tid < PB && (i0 + tid) < I)
                colsum_slab[(int64_t)sp * I + i0 + tid] = (cs_scr[tid] + cs_scr[PB + tid]) + (cs_scr[2 * PB + tid] + cs_scr[3 * PB + tid]);
            __syncthreads();
        }
    };

    int it = 0, nit = 0;
    int m_stage = 0;
    set_item(0, m_stage);
    int cur_sp = item_split(0), cur_i0 = st_i0, cur_j0 = st_j0;
    int kt = 0, kend = split_steps(cur_sp);
    int nkt = 0, nkend = kend;
    bool cur_cs = colsum_slab != nullptr && cur_j0 == 0;
    stage_load(m_stage, 0, 8);
    zero_acc();
    stage_prep(m_stage, st_mend, cur_cs);
#pragma unroll
    for (int j = 0; j < 4; ++j) stage_col(0, j);
    __syncthreads();
    h16x8 ap[2][2], bq0[2], bq1[2];
    read_a(0, 0, ap);
    read_b(0, 0, 0, bq0);
    for (int step = 0; step < total; ++step) {
        const int buf = step & 1;
        const bool more = (step + 1) < total;
        bool new_item = false;
        if (more) {
            if (++nkt == nkend) { ++nit; nkt = 0; set_item(nit, m_stage); nkend = split_steps(item_split(nit)); new_item = true; }
            else m_stage += BK;
        }
        // ---- 16-deep step 0. The first fragments are already in registers (read behind the previous step's barrier), so the MFMAs
        // start at once; the next stage's global loads (a full k16 of MFMAs ahead of their use) issue between them instead of in
        // front of them - in front, both waves of a SIMD spent ~560 cycles per step issuing loads with the matrix pipe idle
        // (tools/tn_abl.sh, s_memtime phases).
        read_b(buf, 0, 1, bq1);
        mma6(0, ap, bq0);
        stage_load(m_stage, 0, 4);
        __builtin_amdgcn_sched_barrier(0);
        read_b(buf, 0, 2, bq0);
        mma6(1, ap, bq1);
        stage_load(m_stage, 4, 8);
        __builtin_amdgcn_sched_barrier(0);
        read_b(buf, 0, 3, bq1);
        mma6(2, ap, bq0);
        __builtin_amdgcn_sched_barrier(0);
        mma6(3, ap, bq1);
        read_a(buf, 1, ap);
        read_b(buf, 1, 0, bq0);
        __builtin_amdgcn_sched_barrier(0);
        // ---- 16-deep step 1, with the next stage's splits + plane writes spread over its units.
        // The item that owns the stage in registers: its column sums restart when it is a new item. All of it is unconditional
        // (after the last stage the registers hold a repeat that lands in the idle buffer): a conditional consumer lets the
        // compiler sink the loads next to it, behind the MFMAs they are meant to overlap.
        if (new_item || !more) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { fin[j] = bs[j]; bs[j] = 0.f; }
        }
        read_b(buf, 1, 1, bq1);
        mma6(0, ap, bq0);
        stage_prep(m_stage, st_mend, more && colsum_slab != nullptr && st_j0 == 0);
        stage_col(buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        read_b(buf, 1, 2, bq0);
        mma6(1, ap, bq1);
        stage_col(buf ^ 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        read_b(buf, 1, 3, bq1);
        mma6(2, ap, bq0);
        stage_col(buf ^ 1, 2);
        stage_col(buf ^ 1, 3);
        __builtin_amdgcn_sched_barrier(0);
        // The barrier sits in FRONT of the last unit (which only needs registers): the next stage's first fragments are read behind
        // it and their latency, and the barrier's skew, are covered by this unit's six MFMAs instead of an idle matrix pipe.
        __syncthreads();                    // next stage written everywhere; this stage's LDS reads are all done
        h16x8 apn[2][2];
        if (more) { read_a(buf ^ 1, 0, apn); read_b(buf ^ 1, 0, 0, bq0); }
        mma6(3, ap, bq1);
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
#pragma unroll
            for (int a = 0; a < 2; ++a) { ap[a][0] = apn[a][0]; ap[a][1] = apn[a][1]; }
        }
        if (++kt == kend) {
            epilogue(cur_sp, cur_i0, cur_j0, cur_cs);
            zero_acc();
            ++it;
            if (it < n_items) {
                cur_sp = item_split(it); kt = 0; kend = split_steps(cur_sp);
                cur_i0 = st_i0; cur_j0 = st_j0;
                cur_cs = colsum_slab != nullptr && cur_j0 == 0;
            }
        }
    }
}

template <bool B16 = false>
__global__ __launch_bounds__(512, 2) void gemm_tn_h2_big_kernel(
    const float *__restrict__ A, int64_t lda, const float *__restrict__ a_amax, const float *__restrict__ B, int64_t ldb,
    const float *__restrict__ b_amax, float *__restrict__ slab, float *__restrict__ colsum_slab, float *__restrict__ scale_out,
    int Mred, int I, int J, int rows_per_split, int ti, int tj, int nsplit) {
    gemm_tn_h2_body<B16, false>(A, lda, a_amax, B, ldb, b_amax, slab, colsum_slab, scale_out, Mred, I, J, rows_per_split, ti, tj, nsplit, 0, 0,
                                blockIdx.x == 0);
}

// Up to three weight gradients of ONE backward pass in one launch (round 6, calls of at most kTnBatchMaxRows = 262,144 rows). The three TN products of a slide
// (dWab = dP^T H, dW2 = dZ2^T H1, dW1 = dZ1^T X) reduce over the SAME rows, and their operands all still exist when the last dgrad has run, so the
// backward defers them to its end and hands them over together: items = row splits x (tiles of product 0 + 1 + 2), one item per workgroup
// (at most PB_GRID items), every item the same number of 32-row stages. Against three launches of the per-XCD plan this pays the launch, the
// operand-scale prologue and the pipeline fill once, and - the larger part - it needs FEWER row splits for the same number of busy CUs (18 tiles
// x 14 splits instead of 6 x 40, 4 x 63 and 8 x 32 at 10,000 rows): the raw 256 x 256 slabs every item writes and the reduction reads back are
// 66 MB per step instead of 196 MB (profiles/r06*: three launches 106 us + reduction 37 us -> one launch + reduction).
// Item k = split * tiles_all + tile (split-major: the items of one split share their operand rows in one XCD's L2); workgroup b runs item
// (b % 8) * 32 + b / 8, i.e. XCD x holds the contiguous items [32 x, 32 x + 32). Values are exactly those of gemm_tn_h2_big_kernel with the same
// rows_per_split (same stage order inside an item, same fixed-order slab sum).
// X16: product 2's B operand is the fp16 feature bag (gemm_tn_h2_body's B16: two MFMA terms per product, scale 1, no abs-max array), products
// 0 and 1 stay fp32; a workgroup picks its body by product (workgroup-uniform, both bodies share the LDS image and the register budget). The
// plan is the SAME as for three fp32 products, so products 0 and 1 are bitwise those of the fp32 launch and product 2 sums the same non-zero
// terms in the same order as the fp32 launch on the up-cast bag. (Its items finish after two thirds of the MFMA work of the others. A plan that
// gave them their own, 3/2 deeper row splits and the fp32 products the workgroups that frees was measured on the 10k ... 100k-row batches:
// every sum then runs in another order than on the fp32 route and dWab / dbab / dW1 moved by up to 1.6e-6 of their magnitude, beyond the
// 1e-6 the fp16 route promises against the fp32 one - tests/test_gpu_multi_x16.py - so the launch keeps one depth for all items.)
template <bool X16 = false>
__global__ __launch_bounds__(512, 2) void gemm_tn_h2_batch_kernel(
    const float *__restrict__ A0, const float *__restrict__ aam0, const float *__restrict__ B0, const float *__restrict__ bam0, float *__restrict__ slab0,
    float *__restrict__ cs0, float *__restrict__ sc0, int I0, int J0,
    const float *__restrict__ A1, const float *__restrict__ aam1, const float *__restrict__ B1, const float *__restrict__ bam1, float *__restrict__ slab1,
    float *__restrict__ cs1, float *__restrict__ sc1, int I1, int J1,
    const float *__restrict__ A2, const float *__restrict__ aam2, const float *__restrict__ B2, const float *__restrict__ bam2, float *__restrict__ slab2,
    float *__restrict__ cs2, float *__restrict__ sc2, int I2, int J2, int n_gemm, int Mred, int rows_per_split, int nsplit) {
    const int tj0 = (J0 + PB - 1) / PB, tj1 = (J1 + PB - 1) / PB, tj2 = (J2 + PB - 1) / PB;
    const int ti0 = (I0 + PB - 1) / PB, ti1 = (I1 + PB - 1) / PB, ti2 = (I2 + PB - 1) / PB;
    const int t0 = ti0 * tj0, t1 = n_gemm > 1 ? ti1 * tj1 : 0, t2 = n_gemm > 2 ? ti2 * tj2 : 0;
    const int tiles_all = t0 + t1 + t2;
    const int k = (blockIdx.x % kNumXCD) * PB_BLOCKS_PER_XCD + blockIdx.x / kNumXCD;
    if (k >= nsplit * tiles_all) return;
    const int split = k / tiles_all, tt = k - split * tiles_all;
    const int g = tt < t0 ? 0 : (tt < t0 + t1 ? 1 : 2);                      // workgroup-uniform
    const int tile = tt - (g == 0 ? 0 : (g == 1 ? t0 : t0 + t1));
    if (X16 && g == 2) {                                                     // the product on the fp16 bag (ldb in halves)
        gemm_tn_h2_body<true, true>(A2, I2, aam2, B2, J2, nullptr, slab2, cs2, sc2, Mred, I2, J2, rows_per_split, ti2, tj2, nsplit, split, tile,
                                    split == 0 && tile == 0);
        return;
    }
    const float *A = g == 0 ? A0 : (g == 1 ? A1 : A2), *aam = g == 0 ? aam0 : (g == 1 ? aam1 : aam2);
    const float *B = g == 0 ? B0 : (g == 1 ? B1 : B2), *bam = g == 0 ? bam0 : (g == 1 ? bam1 : bam2);
    float *slab = g == 0 ? slab0 : (g == 1 ? slab1 : slab2), *cs = g == 0 ? cs0 : (g == 1 ? cs1 : cs2), *sc = g == 0 ? sc0 : (g == 1 ? sc1 : sc2);
    const int I = g == 0 ? I0 : (g == 1 ? I1 : I2), J = g == 0 ? J0 : (g == 1 ? J1 : J2);
    const int ti = g == 0 ? ti0 : (g == 1 ? ti1 : ti2), tj = g == 0 ? tj0 : (g == 1 ? tj1 : tj2);
    gemm_tn_h2_body<false, true>(A, I, aam, B, J, bam, slab, cs, sc, Mred, I, J, rows_per_split, ti, tj, nsplit, split, tile, split == 0 && tile == 0);
}


// out[e] = beta*out[e] + (sum_s slab[s][e]) / (sA sB)   (fixed order -> run-to-run deterministic); the bias slabs behind the
// weight slabs are plain column sums of the fp32 operand and carry no scale.
__global__ __launch_bounds__(256) void slab_reduce_h2_kernel(const float *__restrict__ slab, float *out, int64_t n,
                                                              const float *__restrict__ slab2, float *out2, int64_t n2,
                                                              int nsplit, float beta, const float *__restrict__ scales) {
    const int64_t n4 = n >> 2, m4 = n2 >> 2;
    float f1, f2;
    h2_descale(-h2_exp_of_pow2(scales[0]), -h2_exp_of_pow2(scales[1]), f1, f2);      // scales = (2^-ka, 2^-kb)
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4 + m4; e += (int64_t)gridDim.x * blockDim.x) {
        const bool second = e >= n4;
        const float *src = second ? slab2 + (e - n4) * 4 : slab + e * 4;
        float *dst = second ? out2 + (e - n4) * 4 : out + e * 4;
        const int64_t stride = second ? n2 : n;
        f32x4 s = ld4(src);
        int k = 1;
        for (; k + 3 < nsplit; k += 4) {                                 // four slab loads in flight; the adds keep the fixed order
            const f32x4 t0 = ld4(src + (int64_t)k * stride), t1 = ld4(src + (int64_t)(k + 1) * stride),
                        t2 = ld4(src + (int64_t)(k + 2) * stride), t3 = ld4(src + (int64_t)(k + 3) * stride);
            s += t0; s += t1; s += t2; s += t3;
        }
        for (; k < nsplit; ++k) s += ld4(src + (int64_t)k * stride);
        if (!second) s = (s * f1) * f2;
        if (beta != 0.f) s += beta * ld4(dst);
        st4(dst, s);
    }
}

// Up to three slab reductions in ONE launch (the fused backward defers the reductions of its three weight gradients to the end:
// nothing but the optimiser reads them, and each was a ~5-12 us launch of its own). Same arithmetic and order as slab_reduce_h2_kernel.
struct SlabReduceDesc { const float *slab; float *out; int64_t n; const float *slab2; float *out2; int64_t n2; int nsplit; float beta;
                        const float *scales; int64_t e0; };                   // e0: first float4 of this reduction in the batch
struct SlabReduceBatch { SlabReduceDesc d[3]; int count; int64_t total4; };
__global__ __launch_bounds__(256) void slab_reduce_h2_batch_kernel(SlabReduceBatch b) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < b.total4; g += (int64_t)gridDim.x * blockDim.x) {
        const int i = (b.count > 2 && g >= b.d[2].e0) ? 2 : ((b.count > 1 && g >= b.d[1].e0) ? 1 : 0);
        const float *slab = i == 2 ? b.d[2].slab : i == 1 ? b.d[1].slab : b.d[0].slab;
        const float *slab2 = i == 2 ? b.d[2].slab2 : i == 1 ? b.d[1].slab2 : b.d[0].slab2;
        float *out = i == 2 ? b.d[2].out : i == 1 ? b.d[1].out : b.d[0].out;
        float *out2 = i == 2 ? b.d[2].out2 : i == 1 ? b.d[1].out2 : b.d[0].out2;
        const float *scales = i == 2 ? b.d[2].scales : i == 1 ? b.d[1].scales : b.d[0].scales;
        const int64_t n = i == 2 ? b.d[2].n : i == 1 ? b.d[1].n : b.d[0].n, n2 = i == 2 ? b.d[2].n2 : i == 1 ? b.d[1].n2 : b.d[0].n2;
        const int64_t e = g - (i == 2 ? b.d[2].e0 : i == 1 ? b.d[1].e0 : 0);
        const int nsplit = i == 2 ? b.d[2].nsplit : i == 1 ? b.d[1].nsplit : b.d[0].nsplit;
        const float beta = i == 2 ? b.d[2].beta : i == 1 ? b.d[1].beta : b.d[0].beta;
        const int64_t n4 = n >> 2;
        const bool second = e >= n4;
        const float *src = second ? slab2 + (e - n4) * 4 : slab + e * 4;
        float *dst = second ? out2 + (e - n4) * 4 : out + e * 4;
        const int64_t stride = second ? n2 : n;
        f32x4 s = ld4(src);
        int k = 1;
        for (; k + 3 < nsplit; k += 4) {
            const f32x4 t0 = ld4(src + (int64_t)k * stride), t1 = ld4(src + (int64_t)(k + 1) * stride),
                        t2 = ld4(src + (int64_t)(k + 2) * stride), t3 = ld4(src + (int64_t)(k + 3) * stride);
            s += t0; s += t1; s += t2; s += t3;
        }
        for (; k < nsplit; ++k) s += ld4(src + (int64_t)k * stride);
        if (!second) {
            float f1, f2;
            h2_descale(-h2_exp_of_pow2(scales[0]), -h2_exp_of_pow2(scales[1]), f1, f2);
            s = (s * f1) * f2;
        }
        if (beta != 0.f) s += beta * ld4(dst);
        st4(dst, s);
    }
}

