// stem_halo.inc — part of the extractor's translation unit conv.hip (included inside namespace toad after gemm_stream.inc, whose weight-plane
// format, StreamCfg<2, 2> fragment addressing and pooled epilogue it shares).
// ------------------------------------------------------------------------------------------
// The extractor's stem straight from the caller's NCHW tiles: nn.Conv2d(3, 64, 7, stride 2, pad 3) + folded BN + ReLU + nn.MaxPool2d(3, 2, 1)
// (models/resnet_custom.py:96-99) as ONE kernel, with the input window of a tile resident in LDS (round 4).
//
// Until here the stem took three launches: a space-to-depth gather of the tiles (400 us per 512 tiles), the streamed GEMM over that image
// (every lane loads its own 32-byte fragments: 768 bytes per output pixel through the vector L1's one-tag-per-lane path, 6.4 GB per 512
// tiles at ~16 B/clk/CU - the kernel was bound by that, not by its 0.43 ms of matrix work), and - until the pool moved into the GEMM's
// epilogue - a streaming pool pass. This kernel reads the tiles themselves, once, in whole image rows:
//   * a tile = two conv rows of one image (256 output pixels, as in GATHER_STEM_POOL). Its window is 10 image rows x 3 channels; the
//     workgroup loads them with 8-byte lane loads (a lane owns one pixel of the SPACE-TO-DEPTH form: 2 rows x 2 columns x 3 channels = the
//     12 floats that are one 48-byte run of the stem's K row), takes the tile's abs-max (ONE power-of-two scale per tile: every product of
//     the tile sees the same window), splits the values into the two fp16 pieces ONCE and writes them to LDS as a 5 x 131 x 12 image per piece;
//   * an MFMA A fragment (pixel ox, eight consecutive k) is then 16 contiguous bytes per piece at ((oy + qy) * 131 + ox) * 24 + piece * 16: two
//     ds_read_b64 (8-byte aligned; a b128 would need 16). Nothing is converted twice, no fragment comes from global memory;
//   * the weight planes ([64 x 192], 48 KB) are copied into LDS once per workgroup and stay;
//   * epilogue = stem_pool_epilogue (gemm_stream.inc): horizontal window in registers, vertical through LDS with the carried row.
// Two workgroups of four waves per CU (80 KB of LDS each, see below): the next tile's window is loaded into registers before the matrix
// loop and converted after the epilogue; fragments are read one k16 step ahead. K order = Wf's (qy, qx, ry, rx, c) - the planes of
// split_planes_narrow_h2_kernel<2> as for the streamed stem.
// Shapes: W = 256 (Wo = 128), H % 4 == 0 (Ho even). Other tiles take the three-kernel path.
// ------------------------------------------------------------------------------------------
constexpr int SH_WS = 131;                                   // space-to-depth pixels per row: Wo + 3
constexpr int SH_ROWS = 5;                                   // space-to-depth rows a tile of two conv rows reads
constexpr int SH_PLANE = ((SH_ROWS * SH_WS * 12 * 2 + 63) / 64) * 64;       // bytes of one piece's image (15,744)
constexpr int SH_W_BYTES = 6 * StreamCfg<2, 2>::ST_BYTES;    // all six k-stages of the [64, 192] weight planes: 49,152
constexpr int SH_HALO_OFF = SH_W_BYTES;
// Round 6: TWO workgroups per CU. With one (four waves, one per SIMD) the three phases of a tile were serial - matrix loop 4 us, pooled epilogue 2 us, loading +
// converting the next window 2.3 us (profiles/r04*: timing ablations) - and the matrix pipe idled half the time. A second workgroup fills those phases, and it fits
// because (i) the carried pooled row moved from LDS into registers (it is written and read by the same lane: stem_pool_epilogue<.., RC = true>), and (ii) the parked
// pooled row (16 KB) borrows the window's LDS, which is dead between the last fragment read of a tile and the conversion of the next window (the epilogue's first
// barrier separates the two uses, its last one the return): 49,152 + 31,488 + 1,024 + 64 = 81,728 B, two of which are the CU's 160 KB to within 384 bytes.
constexpr int SH_POOL_OFF = SH_HALO_OFF + 2 * SH_PLANE;      // the edge pixels (1 KB): stem_pool_epilogue<.., RC>'s `lds`
constexpr int SH_ROWA_OFF = SH_HALO_OFF;                     // the parked pooled row (16 KB) lies over the window planes (31,488 B)
constexpr int SH_SCR_OFF = SH_POOL_OFF + 4 * 64 * 4;         // four wave maxima
constexpr int SH_SMEM = SH_SCR_OFF + 64;
static_assert(2 * SH_PLANE >= 64 * 64 * 4 && 2 * SH_SMEM <= 160 * 1024, "two workgroups per CU");
constexpr int SH_TASKS = (SH_ROWS * SH_WS + 255) / 256;      // space-to-depth pixels per thread and tile: 3 (655 over 256 threads)

// Input forms of the window loader. The kernel body is one template; what differs is how a lane fetches and holds the 12 values of its space-to-depth pixel:
//   fp32 NCHW (stem_halo_pool_kernel<SH_F32>): six 8-byte loads (2 rows x 3 channel planes), held as 12 floats per task across the matrix loop;
//   uint8 NHWC (stem_halo_pool_kernel<SH_U8>): the tiles as an image decoder hands them over, [B, H, 256, 3] RGB. A pixel pair of one row is 6 contiguous
//     bytes at ((b H + iy) 256 + ix) 3 - a multiple of 6, so 2-byte aligned relative to the base and not 4-byte aligned in general: one 4-byte and one
//     2-byte load per row, held RAW (4 registers per task instead of 12) across the matrix loop. store_window converts them once, in front of the abs-max:
//     x = fmaf((float)u, a_c, b_c) with a_c = 1 / (255 std_c), b_c = -mean_c / std_c rounded to fp32 by the host - ToTensor + Normalize of the tiles the
//     reference's extractor is fed (the ImageNet statistics of the weights models/resnet_custom.py:121-124 loads). A tap outside the image is 0 in
//     NORMALISED space (Normalize, then the convolution's zero padding), not b_c: the spare upper half of the 2-byte load's register carries the
//     "outside" mark. From the abs-max on the two forms run the same code on the same values, so the results are bitwise those of the fp32 form
//     fed the normalised image.
//   uint8 region (stem_halo_pool_kernel<SH_U8_REGION>): the tiles are never cut out. One decoded image [Hr, Wr, 3] with a row pitch in bytes, and per tile
//     its top-left pixel (x_b, y_b) in an int32 array [B][2] on the device. The image index b = q / tpi is uniform over the workgroup, so the tile's base
//     region + y_b pitch + x_b 3 is a 64-bit SCALAR; the in-tile offset iy pitch + ix 3 stays 32-bit (the launcher refuses H pitch >= 2^31). The edge
//     predicate is the TILE's (iy in [0, H), ix in [0, 256)), not the region's: a tap outside the tile is 0 in normalised space even where the region has
//     pixels there, so tile b behaves exactly as region[y:y+H, x:x+256] cut out and given to the uint8 form - and no address outside the tile, hence none
//     outside the region, is ever read (the origins' bounds are the caller's duty). (y_b + iy) pitch + (x_b + ix) 3 has any parity, and it changes from
//     row to row with an odd pitch: the 4-byte and the 2-byte word are loaded through common.h's u32_a1 / u16_a1 - the same two loads per row and the same
//     4 registers per task as the uint8 form, on global memory the hardware takes a dword at any byte address (six byte loads assembled in registers compile
//     to the same two loads at -O3: there is no second form to choose from). The loads are plain, not nontemporal:
//     overlapping tiles (heat-map strides) read the same bytes again. From the raw words on it is the uint8 form's code.
//   uint8 region, 2 x 2 box (stem_halo_pool_kernel<SH_U8_REGION_BOX2>): a 40x scan read at the 20x-equivalent pitch. Tile b is the (2 H, 512) FOOTPRINT at its
//     origin, and pixel (iy, ix) of the (H, 256) tile the kernel works on is t[iy, ix, c] = (sum of the footprint's [2 iy + dy, 2 ix + dx, c], dy, dx in 0 .. 1,
//     + 2) >> 2: the mean rounded half up, the box filter of every `down` of this library. The pixel pair of tile row iy at columns ix, ix + 1 is footprint
//     rows 2 iy, 2 iy + 1, bytes [6 ix, 6 ix + 12) - three u32_a1 dwords per row (one 12-byte load), any byte address, any pitch parity, plain loads as above.
//     v_perm_b32 spreads each row's left and right pixels over two 16-bit fields per dword, the four contributions and the rounding 2 are added per field (at
//     most 1022: exact, nothing carries), and the six means are packed into the SAME raw[k][2 ry] / raw[k][2 ry + 1] words the region form loads, the
//     SH_U8_OUTSIDE mark included: store_window, the abs-max, the split, the matrix loop and the epilogue do not know of it, and the result is bitwise the
//     uint8 form on those box-filtered tiles. The edge predicate stays the TILE's, in shrunk coordinates (padding is the tile's; no byte outside a footprint
//     is read); the in-footprint offset 2 iy pitch + 6 ix stays 32-bit (the launcher refuses 2 H pitch >= 2^31). Not built: factors above 2, other filters,
//     and a shrink on the tile forms.
//   uint8 region LIST (stem_halo_pool_kernel<SH_U8_REGIONS>, <SH_U8_REGIONS_BOX2>): the slide as the decoder cut it, up to STEM_REGIONS_MAX regions of their own
//     base address and pitch, and per tile a triple (x_b, y_b, k_b) in an int32 array [B][3] on the device: the tile's top-left pixel in the coordinates of
//     region k_b. The descriptors {base, pitch} travel BY VALUE in the kernel argument (2 KB; no device table, no allocation): b is uniform over the
//     workgroup, so the triple is three readfirstlane'd loads and r[k_b] a scalar load from the kernarg segment at a scalar index - no search, no scratch.
//     The tile's base base_k + y_b pitch_k + 3 x_b is the 64-bit scalar of the region form, the in-tile offset stays 32-bit with pitch_k (the launcher
//     refuses shrink H pitch_k >= 2^31 for every k). Every call of the loader takes the descriptor of ITS tile - the carry item of a workgroup's range (the
//     tile above it) may lie in another region than the range's first tile. From the tile's base on it is the region form's code, the box form's for
//     shrink = 2: the TILE's edge predicate, no byte outside a tile (footprint), plain loads. That every triple has 0 <= k_b < n and keeps its tile inside
//     region k_b is the caller's duty, as for the origins.
constexpr unsigned SH_U8_OUTSIDE = 0xFFFF0000u;              // upper half of a row's 2-byte word: the pixel pair lies outside the image
typedef unsigned sh_u32_a2 __attribute__((aligned(2)));      // a 4-byte load from a 2-byte aligned address
constexpr int SH_F32 = 0, SH_U8 = 1, SH_U8_REGION = 2, SH_U8_REGION_BOX2 = 3, SH_U8_REGIONS = 4, SH_U8_REGIONS_BOX2 = 5;   // the FORM parameter of the kernel

// (the constants are the LAST kernel argument, an empty struct in the fp32 form: that form's argument layout, registers and code are the ones it had as a
//  plain kernel - 64 SGPRs, 242 VGPRs, no scratch; the uint8 form: 68 SGPRs, 218 VGPRs, no scratch; the region form, whose last argument also carries the
//  pitch and the origins: 70 SGPRs, 217 VGPRs, no scratch; the box form, same arguments: 88 SGPRs, 220 VGPRs, no scratch; all 81,728 B of LDS, two workgroups
//  per CU; the list forms, whose last argument carries the triples and the 128 descriptors: profiles/extract_regions_isa.md)
struct StemNoNorm {};
struct StemRegionArg { StemNorm nrm; int pitch; const int *origins; };      // origins: int32 [B][2] = (x, y) of each tile's top-left pixel
struct StemRegionsArg { StemNorm nrm; const int *tiles; StemRegionDesc r[STEM_REGIONS_MAX]; };      // tiles: int32 [B][3] = (x, y, k), in region k's coordinates
template <int FORM> struct StemLastArg { typedef StemNoNorm type; };
template <> struct StemLastArg<SH_U8> { typedef StemNorm type; };
template <> struct StemLastArg<SH_U8_REGION> { typedef StemRegionArg type; };
template <> struct StemLastArg<SH_U8_REGION_BOX2> { typedef StemRegionArg type; };
template <> struct StemLastArg<SH_U8_REGIONS> { typedef StemRegionsArg type; };
template <> struct StemLastArg<SH_U8_REGIONS_BOX2> { typedef StemRegionsArg type; };
template <int FORM>
__global__ __launch_bounds__(256, 2) void stem_halo_pool_kernel(const typename std::conditional<FORM != SH_F32, unsigned char, float>::type *__restrict__ Xv,
                                                                const unsigned short *__restrict__ Bp, const float *__restrict__ binv,
                                                                const float *__restrict__ bias, float *Yp, int B, int H, float *y_gmax, int tiles,
                                                                typename StemLastArg<FORM>::type nrm_arg) {
    constexpr bool U8 = FORM != SH_F32, LIST = FORM == SH_U8_REGIONS || FORM == SH_U8_REGIONS_BOX2, BOX2 = FORM == SH_U8_REGION_BOX2 || FORM == SH_U8_REGIONS_BOX2,
                   REGION = FORM == SH_U8_REGION || LIST || BOX2;
    using Cfg = StreamCfg<2, 2>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char *lds = reinterpret_cast<char *>(smem);
    const float *X = reinterpret_cast<const float *>(Xv);
    const unsigned char *X8 = reinterpret_cast<const unsigned char *>(Xv);
    StemNorm nrm{};
    if constexpr (REGION) nrm = nrm_arg.nrm;
    else if constexpr (U8) nrm = nrm_arg;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hi = lane >> 5;
    constexpr int W = 256;
    const int tpi = H / 4;                                   // tiles (conv row pairs) per image: Ho / 2
    const int p_lo = (int)(((int64_t)tiles * blockIdx.x) / gridDim.x), p_hi = (int)(((int64_t)tiles * (blockIdx.x + 1)) / gridDim.x);
    if (p_hi <= p_lo) return;
    const int n_items = p_hi - p_lo + 1;                     // item 0: the tile above the range, for its carry only (gemm_stream.inc)
    auto item_tile = [&](int i) { return max(p_lo + i - 1, 0); };

    // ---- the weight planes: 48 KB, once
    for (int o = tid * 16; o < SH_W_BYTES; o += 256 * 16)
        *reinterpret_cast<f32x4 *>(lds + o) = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(Bp) + o);

    // ---- window loader: task k of this thread = space-to-depth pixel (Yl, Xs) = divmod(tid + 256 k, 131) of the tile's 5 x 131 window
    typedef float f2 __attribute__((ext_vector_type(2)));
    int tk[SH_TASKS];                                        // task k of this thread: (Yl << 8) | Xs, or -1
#pragma unroll
    for (int k = 0; k < SH_TASKS; ++k) {
        const int task = tid + 256 * k, Yl = task / SH_WS;
        tk[k] = task < SH_ROWS * SH_WS ? (Yl << 8) | (task - Yl * SH_WS) : -1;
    }
    // raw[k][ry * 3 + c] = columns (2 Xs - 4, 2 Xs - 3) of image row 4 t - 4 + 2 Yl + ry, channel c (a local of the caller's scope: loop-local liveness)
    // what a task holds between its loads and store_window: fp32 - the 12 values; uint8 - per row ry the 4-byte word [2 ry] (c0 c1 c2 of column 0, c0 of
    // column 1) and the 2-byte word [2 ry + 1] (c1 c2 of column 1; upper half 0, or SH_U8_OUTSIDE)
    using Raw = typename std::conditional<U8, unsigned[SH_TASKS][4], f2[SH_TASKS][6]>::type;
    auto load_window = [&](int q, Raw &raw) __attribute__((always_inline)) {
        const int b = q / tpi, t = q - b * tpi;
        if constexpr (REGION) {
            int pitch, x_b, y_b;
            const unsigned char *reg8;
            if constexpr (LIST) {                                // the tile's own region: three uniform loads, then one descriptor from the kernarg segment at a scalar index
                x_b = __builtin_amdgcn_readfirstlane(nrm_arg.tiles[3 * b]), y_b = __builtin_amdgcn_readfirstlane(nrm_arg.tiles[3 * b + 1]);
                const int k_b = __builtin_amdgcn_readfirstlane(nrm_arg.tiles[3 * b + 2]);
                pitch = nrm_arg.r[k_b].pitch;
                reg8 = nrm_arg.r[k_b].base;
            } else {
                pitch = nrm_arg.pitch;
                x_b = __builtin_amdgcn_readfirstlane(nrm_arg.origins[2 * b]), y_b = __builtin_amdgcn_readfirstlane(nrm_arg.origins[2 * b + 1]);
                reg8 = X8;
            }
            const unsigned char *img8 = reg8 + ((int64_t)y_b * pitch + (int64_t)x_b * 3);
#pragma unroll
            for (int k = 0; k < SH_TASKS; ++k) {
                int tc = tk[k];
                asm volatile("" : "+v"(tc));                     // (laundered per call, as below)
                const int Yl = tc >> 8, Xs = tc & 255;
                const int ix = 2 * Xs - 4;
#pragma unroll
                for (int ry = 0; ry < 2; ++ry) {
                    const int iy = 4 * t - 4 + 2 * Yl + ry;
                    const bool ok = tc >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W;       // the TILE's edges: bytes [0, 6) of the pair end inside row iy of the tile
                    if constexpr (BOX2) {
                        // footprint rows 2 iy, 2 iy + 1, bytes [6 ix, 6 ix + 12): columns 2 ix .. 2 ix + 3, the last one 2 W - 1 at most
                        const unsigned char *p = img8 + ((unsigned)(2 * iy) * (unsigned)pitch + (unsigned)(ix * 6));      // (32-bit, unsigned: 2 H pitch < 2^31; only read where ok)
                        unsigned w[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
                        if (ok) {                                     // (one branch around the six loads: hipcc then merges a row's three into one 12-byte load)
#pragma unroll
                            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                                for (int j = 0; j < 3; ++j) w[dy][j] = *reinterpret_cast<const u32_a1 *>(p + (dy ? (unsigned)pitch : 0u) + 4 * j);
                        }
                        unsigned s[3] = {0x00020002u, 0x00020002u, 0x00020002u};
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy) {
                            s[0] += __builtin_amdgcn_perm(w[dy][1], w[dy][0], 0x0c010c00u) + __builtin_amdgcn_perm(w[dy][1], w[dy][0], 0x0c040c03u);     // (b0, b1) + (b3, b4)
                            s[1] += __builtin_amdgcn_perm(w[dy][1], w[dy][0], 0x0c060c02u) + __builtin_amdgcn_perm(w[dy][2], w[dy][1], 0x0c050c01u);     // (b2, b6) + (b5, b9)
                            s[2] += __builtin_amdgcn_perm(w[dy][2], w[dy][1], 0x0c040c03u) + __builtin_amdgcn_perm(w[dy][2], w[dy][1], 0x0c070c06u);     // (b7, b8) + (b10, b11)
                        }
                        // each half of s[i] is a box's sum + 2, at most 1022: bytes 0 and 2 of s[i] >> 2 are the two rounded means, whatever leaks into byte 1
                        raw[k][2 * ry] = __builtin_amdgcn_perm(s[1] >> 2, s[0] >> 2, 0x06040200u);
                        raw[k][2 * ry + 1] = ok ? __builtin_amdgcn_perm(0u, s[2] >> 2, 0x0c0c0200u) : SH_U8_OUTSIDE;
                    } else {
                    const unsigned char *p = img8 + ((unsigned)iy * (unsigned)pitch + (unsigned)(ix * 3));      // (32-bit, unsigned: H pitch < 2^31; only read where ok)
                    raw[k][2 * ry] = ok ? *reinterpret_cast<const u32_a1 *>(p) : 0u;
                    raw[k][2 * ry + 1] = ok ? (unsigned)*reinterpret_cast<const u16_a1 *>(p + 4) : SH_U8_OUTSIDE;
                    }
                }
            }
        } else if constexpr (U8) {
            const unsigned char *img8 = X8 + (int64_t)b * H * W * 3;
#pragma unroll
            for (int k = 0; k < SH_TASKS; ++k) {
                int tc = tk[k];
                asm volatile("" : "+v"(tc));                     // (laundered per call, as below)
                const int Yl = tc >> 8, Xs = tc & 255;
                const int ix = 2 * Xs - 4;
#pragma unroll
                for (int ry = 0; ry < 2; ++ry) {
                    const int iy = 4 * t - 4 + 2 * Yl + ry;
                    const bool ok = tc >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W;       // (ix even, W even: both columns or neither; bytes [0, 6) of the pair end inside row iy)
                    const unsigned char *p = img8 + ((int64_t)iy * W + ix) * 3;
                    raw[k][2 * ry] = ok ? __builtin_nontemporal_load(reinterpret_cast<const sh_u32_a2 *>(p)) : 0u;
                    raw[k][2 * ry + 1] = ok ? (unsigned)__builtin_nontemporal_load(reinterpret_cast<const unsigned short *>(p + 4)) : SH_U8_OUTSIDE;
                }
            }
        } else {
        const float *img = X + (int64_t)b * 3 * H * W;
        // (the packed task coordinates are laundered per call: offsets and edge predicates are then formed here, per tile - a few integer instructions - instead
        //  of being hoisted out of the tile loop, where ~25 registers of them lived across the matrix loop and, at 256 registers per wave, were spilled)
#pragma unroll
        for (int k = 0; k < SH_TASKS; ++k) {
            int tc = tk[k];
            asm volatile("" : "+v"(tc));
            const int Yl = tc >> 8, Xs = tc & 255;               // tc < 0: no such task (Yl = -1 fails the row test below)
            const int ix = 2 * Xs - 4;
#pragma unroll
            for (int ry = 0; ry < 2; ++ry) {
                const int iy = 4 * t - 4 + 2 * Yl + ry;
                const bool ok = tc >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    raw[k][ry * 3 + c] = ok ? __builtin_nontemporal_load(reinterpret_cast<const f2 *>(img + ((int64_t)c * H + iy) * W + ix)) : f2{0.f, 0.f};
            }
        }
        }
    };
    float *scr = reinterpret_cast<float *>(lds + SH_SCR_OFF);
    // abs-max of the loaded window -> the tile's exponent; split into the two pieces, written in K order (ry, rx, c) per pixel
    auto store_values = [&](f2 (&raw)[SH_TASKS][6]) __attribute__((always_inline)) {
        float mx = 0.f;
#pragma unroll
        for (int k = 0; k < SH_TASKS; ++k)
#pragma unroll
            for (int e = 0; e < 6; ++e) mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fabsf(raw[k][e][0]), __builtin_fabsf(raw[k][e][1])));
        mx = h2_wave_max_dpp(mx);                            // (DPP + readlane: the shuffle form keeps five lane-index registers alive across the tile loop)
        if (lane == 0) scr[wave] = mx;
        lds_barrier();                                       // (also: every wave is done with the previous tile's window and epilogue)
        const int ke = __builtin_amdgcn_readfirstlane(h2_exp_from_amax(__builtin_fmaxf(__builtin_fmaxf(scr[0], scr[1]), __builtin_fmaxf(scr[2], scr[3]))));
        const float s = h2_pow2(ke);
#pragma unroll
        for (int k = 0; k < SH_TASKS; ++k) {
            int tc = tk[k];
            asm volatile("" : "+v"(tc));
            const int task = (tc >> 8) * SH_WS + (tc & 255);
            if (tc >= 0) {
                // pixel's 12 values in K order: (ry 0: rx 0: c0 c1 c2, rx 1: c0 c1 c2), (ry 1: ...)
                float v[12];
#pragma unroll
                for (int ry = 0; ry < 2; ++ry)
#pragma unroll
                    for (int rx = 0; rx < 2; ++rx)
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[(ry * 2 + rx) * 3 + c] = raw[k][ry * 3 + c][rx];
                unsigned hu[6], mu[6];
#pragma unroll
                for (int e = 0; e < 6; ++e) h2_split2(v[2 * e], v[2 * e + 1], s, hu[e], mu[e]);
                char *dst = lds + SH_HALO_OFF + task * 24;
                typedef unsigned u2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    *reinterpret_cast<u2 *>(dst + 8 * e) = u2{hu[2 * e], hu[2 * e + 1]};
                    *reinterpret_cast<u2 *>(dst + SH_PLANE + 8 * e) = u2{mu[2 * e], mu[2 * e + 1]};
                }
            }
        }
        lds_barrier();
        return ke;
    };
    // uint8: the raw words -> the values the fp32 form would have loaded (same [ry * 3 + c][rx] layout), ONE rounding each (an explicit fma: the
    // library is built with -ffp-contract=fast, and neither contraction nor its absence may decide the bits); then the shared code
    auto store_window = [&](Raw &raw) __attribute__((always_inline)) {
        if constexpr (U8) {
            f2 cv[SH_TASKS][6];
#pragma unroll
            for (int k = 0; k < SH_TASKS; ++k)
#pragma unroll
                for (int ry = 0; ry < 2; ++ry) {
                    const unsigned lo = raw[k][2 * ry], hi = raw[k][2 * ry + 1];
                    const bool in = hi < SH_U8_OUTSIDE;
                    const unsigned u[2][3] = {{lo & 255u, (lo >> 8) & 255u, (lo >> 16) & 255u}, {lo >> 24, hi & 255u, (hi >> 8) & 255u}};
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int rx = 0; rx < 2; ++rx) cv[k][ry * 3 + c][rx] = in ? __builtin_fmaf((float)u[rx][c], nrm.a[c], nrm.b[c]) : 0.f;
                }
            return store_values(cv);
        } else {
            return store_values(raw);
        }
    };

    // ---- fragments. Wave w: conv row w >> 1 of the tile, pixels (w & 1) * 64 + a * 32 + li (a = 0, 1); columns = the 64 channels (2 blocks)
    const int oyl = wave >> 1, ox0 = (wave & 1) * 64 + li;
    const int swB = (li >> 2) & 3;
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    struct Frag { h16x8 a[2][2]; h16x8 b[2][2]; };          // [row sub-tile / column block][piece]
    // (the 12 x 3 per-step LDS addresses of the fragment reads are tile-invariant and stay hoisted: ~36 registers that save ~8 % of the kernel's time; what is
    //  laundered per tile instead - so that it is NOT kept alive across the matrix loop - are the epilogue's and the window code's lane coordinates)
    auto read_frags = [&](int n, Frag &f) __attribute__((always_inline)) {     // k16 step n = 2 kt + s: the lane's k group g8 = 2 n + hi -> window row g8 / 6, 16-byte piece g8 % 6
        const int g8 = 2 * n + hi, qy = (g8 * 43) >> 8, piece = g8 - 6 * qy;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const char *p = lds + SH_HALO_OFF + ((oyl + qy) * SH_WS + ox0 + a * 32) * 24 + piece * 16;
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) {
                const u2 lo = *reinterpret_cast<const u2 *>(p + pc * SH_PLANE), hi2 = *reinterpret_cast<const u2 *>(p + pc * SH_PLANE + 8);
                f.a[a][pc] = __builtin_bit_cast(h16x8, u32x4{lo[0], lo[1], hi2[0], hi2[1]});
            }
        }
        const int kt = n >> 1, s = n & 1;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const char *base = lds + kt * Cfg::ST_BYTES + li * 64 + b * 32 * 64 + ((2 * s + hi) ^ swB) * 16;
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) f.b[b][pc] = *reinterpret_cast<const h16x8 *>(base + pc * Cfg::PL_BYTES);
        }
    };
    f32x16 acc[2][2];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    auto mma = [&](const Frag &f) __attribute__((always_inline)) {              // three terms (m.h, h.m, h.h), small ones first - the order of every h2 kernel
#define TOAD_T(PA, PB_) \
        _Pragma("unroll") for (int b = 0; b < 2; ++b) \
            _Pragma("unroll") for (int a = 0; a < 2; ++a) \
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[a][PA], f.b[b][PB_], acc[a][b], 0, 0, 0);
        TOAD_T(1, 0) TOAD_T(0, 1) TOAD_T(0, 0)
#undef TOAD_T
    };

    float amx = 0.f;
    float carry_r[32];                                       // waves 2-3: the pooled conv row 2t + 1 of the previous tile (the carry)
#pragma unroll
    for (int i = 0; i < 32; ++i) carry_r[i] = 0.f;
    int ke;
    { Raw raw0; load_window(item_tile(0), raw0); ke = store_window(raw0); }                                  // (its first barrier also publishes the weight planes)
    for (int it = 0; it < n_items; ++it) {
        const int q = item_tile(it);
        zero_acc();
        Frag f0, f1;
        read_frags(0, f0);
#pragma unroll
        for (int n = 0; n < 12; n += 2) {
            read_frags(n + 1, f1);
            __builtin_amdgcn_sched_barrier(0);
            mma(f0);
            __builtin_amdgcn_sched_barrier(0);
            if (n + 2 < 12) read_frags(n + 2, f0);
            __builtin_amdgcn_sched_barrier(0);
            mma(f1);
            __builtin_amdgcn_sched_barrier(0);
        }
        // The next window's loads are issued in the MIDDLE of the epilogue, once the accumulators have been folded into the pooled row: they fly during the vertical
        // combine and the stores (and under the other workgroup's matrix loop), and their 36 registers coexist neither with the two fragment sets of the loop nor
        // with the accumulators - at two workgroups per CU a wave has 256 registers, not 512. (Measured against "in front of the epilogue" and "behind it": 728 /
        // 777 / 754 us and 780 / 790 / 812 us on two boxes - the other workgroup hides most of the latency either way; profiles/r07f_stem_variants.txt.)
        Raw raw;
        int li_e = li, hi_e = hi;                             // the epilogue's lane coordinates, laundered (see read_frags)
        asm volatile("" : "+v"(li_e), "+v"(hi_e));
        const bool more = it + 1 < n_items;
        const int qn = item_tile(more ? it + 1 : it);
        auto mid = [&]() __attribute__((always_inline)) { if (more) load_window(qn, raw); };
        stem_pool_epilogue<2, 2, true>(acc, lds + SH_POOL_OFF, reinterpret_cast<float *>(lds + SH_ROWA_OFF), wave, li_e, hi_e, ke, bias, binv, Yp, (int64_t)q, it != 0,
                                       q % tpi == 0, amx, carry_r, mid);
        if (more) ke = store_window(raw);
    }
    if (y_gmax) {
        amx = h2_wave_max(amx);
        if (lane == 0) scr[wave] = amx;
        __syncthreads();
        if (tid == 0) h2_atomic_amax(y_gmax, __builtin_fmaxf(__builtin_fmaxf(scr[0], scr[1]), __builtin_fmaxf(scr[2], scr[3])));
    }
}
