// heatmap.hip — the attention heat map of a decoded uint8 region, rendered where the region lies: the stage behind the tiles-by-origin calls and the mirror
// image of tissue.hip (include/toad_hip.h, "attention heat map"). Everything is integer arithmetic, so the canvas has one right answer.
//
//   tile table  tile_q int32 [ny][nx]: -1 = the tile is absent, otherwise its score quantised to 0 .. 65535.
//   cell value  cells are cell x cell pixels, anchored at the region's (0, 0) as in tissue.hip. With n the present tiles that cover a cell and S the sum of
//               their q,   idx = (2 S + 257 n) / (514 n)  if n > 0, else -1:  255 mean(q) / 65535 rounded half up (65535 = 255 * 257), in 0 .. 255.
//   canvas      down in {1, 2, 4}; Ho = Hr / down, Wo = Wr / down, partial boxes at the right and the bottom edge are dropped. Per channel
//               m = (sum of the down x down box + down^2 / 2) / down^2;  the output byte is m where the box's cell has idx = -1, elsewhere
//               (alpha lut[idx][c] + (256 - alpha) m + 128) >> 8  with alpha in [0, 256]. down divides every cell size: a box lies in one cell.
//
//   per pixel   (toad_region_heat_blend_px_u8) the same canvas with the colour index and the alpha decided per canvas pixel: with smooth = 1 the index is
//               the bilinear tent between cell centres, in doubled coordinates so that it stays in integers - along x  p = 2 down ox + down - cell,
//               g0 = floor(p / (2 cell)), f = p - 2 cell g0, weights 2 cell - f for cell g0 and f for g0 + 1, the same along y; a neighbour outside the
//               table or without a value counts as the pixel's own cell;  idx_px = (sum wy wx v + 2 cell^2) >> (2 log2(cell) + 2). With a mask plane
//               [Hm][Wm] of mask_down x mask_down boxes a pixel is blended only where mask[(down oy) / mask_down][(down ox) / mask_down] > mask_thresh;
//               the pixels of the partial boxes the plane dropped are not. Coverage and mask edges stay sharp: only the colour inside is interpolated.
//
//   overview    (toad_region_heat_thumb_u8) the per-pixel canvas at down in {8, 16, 32} with down <= cell, so that a box still lies in one cell: the
//               slide overview of an 80k x 80k region without a full-size canvas in between.
//
//   window      (toad_region_heat_window_u8) any of the canvases above for a region that is the window at (wx, wy) of the image the table and the mask plane
//               describe: own cell, tent and mask coordinates from x + wx, y + wy, everything else - addresses, box means, the work split - the window's own.
//               A tent neighbour inside the table counts also where it lies outside the window: canvases put together from strips or blocks show no seams.
//               wx, wy are multiples of max(4, down), so that a lane's 4 x 4 block and a canvas box lie in one cell and one mask pixel as before.
//
//   blur        (toad_heat_cells_blur) the cell table smoothed before it is rendered: a normalised convolution with a symmetric separable integer kernel
//               of radius 1 .. 16 cells, absent cells and cells outside the table carrying no weight, absent cells staying absent.
//
//   list        (toad_region_heat_windows_u8) N windows of one slide, each with its own region, place and canvas, in one launch per 32 windows: every
//               canvas byte for byte the window entry's.
//
//   pyramid     (toad_region_heat_pyramid_u8) several of the six window canvases in one call, each byte for byte the window entry's: every level is defined
//               from the region's own box sums, never from the level above, and box sums nest, so one read of the region serves them all.
//
//   pyramid list (toad_region_heat_pyramid_windows_u8) both at once: N windows of one slide, several levels each, in one launch per 16 windows; every canvas
//               byte for byte the pyramid entry's.
//
// Eight kernels:
//   heat_pyramid_list_kernel<RB,MASK>      heat_pyramid_kernel over a LIST of windows: descriptors by value, the same body (heat_pyramid_body.inc).
//   heat_blend_px_list_kernel<DOWN,SMOOTH,MASK>, heat_thumb_list_kernel<DOWN>   the two single-level kernels below over a LIST of windows of one slide:
//                                          descriptors by value in the kernel argument, a workgroup finds its window and runs the same body.
//   heat_pyramid_kernel<RB,MASK>           two or more levels from one read: 1, 2, 4 finished in the lane, 8, 16, 32 in heat_thumb_kernel's tail.
//   heat_cells_blur_kernel                 a 16 x 64 tile of the cell table and its halo in LDS, a row pass and a column pass inside the workgroup.
//   heat_thumb_kernel<DOWN,WINDOW>        the overview canvas: the same streaming pass with a box's lanes and waves reduced, one thread per canvas pixel blends.
//   heat_cells_kernel                      one thread per cell: the covering tiles' index ranges in closed form from the lattice in cell units, a loop over them.
//   heat_blend_px_kernel<DOWN,SMOOTH,MASK>  one streaming pass over the region: read uint8, write uint8. <DOWN,0,false> is the flat canvas (one colour and one
//                                           alpha per cell: both entry points launch it); the others decide the index, the colour and the alpha per canvas pixel.
#include "region_u8.h"

namespace toad {

// All lattice arguments in cell units. Tile j covers cell row gy iff cy0 + j csy <= gy < cy0 + j csy + ch: with t = gy - cy0 >= 0 that is
// j in [t >= ch ? (t - ch) / csy + 1 : 0,  min(t / csy, ny - 1)], and the same along x. The launcher bounds ceil(ch / csy) ceil(cw / csx) by 4096, so
// 2 S + 257 n < 2^31. The table is small and cached. Every element of cells is written by exactly one thread: nothing is zeroed, nothing is atomic.
__global__ __launch_bounds__(256) void heat_cells_kernel(const int *__restrict__ tile_q, int nx, int ny, int cx0, int cy0, int ch, int cw, int csx, int csy,
                                                         int Gy, int Gx, int *__restrict__ cells) {
    const uint64_t total = (uint64_t)Gy * Gx;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const int gy = (int)(t / (unsigned)Gx), gx = (int)(t - (uint64_t)gy * Gx);
        const int ty = gy - cy0, tx = gx - cx0;
        int idx = -1;
        if (ty >= 0 && tx >= 0) {
            const int j0 = ty >= ch ? (ty - ch) / csy + 1 : 0, j1 = min(ty / csy, ny - 1);
            const int i0 = tx >= cw ? (tx - cw) / csx + 1 : 0, i1 = min(tx / csx, nx - 1);
            int n = 0, s = 0;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    const int q = tile_q[(int64_t)j * nx + i];
                    if (q >= 0) { s += min(q, 65535); ++n; }
                }
            if (n > 0) idx = (2 * s + 257 * n) / (514 * n);
        }
        cells[t] = idx;
    }
}

// ---- the Gaussian blur of the cell table: toad_heat_cells_blur ----
// A normalised convolution in integers (include/toad_hip.h): out = (2 N + D) / (2 D) with N = sum w[|dy|] w[|dx|] min(v, 255) and D = sum w[|dy|] w[|dx|]
// over the cells of the (2 r + 1)^2 window that lie inside the table and hold a value, -1 where the cell itself holds none. A workgroup owns a tile of
// BLUR_TH x BLUR_TW cells. Its window of (TH + 2 r) x (TW + 2 r) cells goes to LDS as  min(v, 255) | 1 << 20  for a value and 0 for a cell that is absent
// or outside the table, so that one multiply-add per tap sums N1 and D1 of the row pass in ONE dword, N1 | D1 << 20: N1 <= 255 * 1024 < 2^20 and
// D1 <= 1024. The row pass (a wave per window row, a lane per tile column) leaves (TH + 2 r) x TW such dwords in LDS, the column pass takes them apart
// again: N <= 255 * 1024^2 and 2 N + D < 2^31. Lanes read consecutive dwords in both passes. The taps are kernel arguments, zero beyond r; the tap
// loops are unrolled with a uniform exit at r so that every tap is read from a scalar register. Nothing outside [0, Gy) x [0, Gx) is read, every
// element of out is written once by one thread, there is no atomic. 30 KB of LDS, sized for r = 16.
constexpr int BLUR_R = 16, BLUR_TH = 16, BLUR_TW = 64, BLUR_IW = BLUR_TW + 2 * BLUR_R, BLUR_IH = BLUR_TH + 2 * BLUR_R;
struct HeatBlurTaps { int w[BLUR_R + 1]; };

__global__ __launch_bounds__(256) void heat_cells_blur_kernel(const int *__restrict__ cells, int Gy, int Gx, const HeatBlurTaps taps, int r, unsigned ntx,
                                                              int *__restrict__ out) {
    __shared__ unsigned in_s[BLUR_IH * BLUR_IW], mid_s[BLUR_IH * BLUR_TW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tx0 = (int64_t)(blockIdx.x % ntx) * BLUR_TW, ty0 = (int64_t)(blockIdx.x / ntx) * BLUR_TH;
    const int rows = BLUR_TH + 2 * r, cols = BLUR_TW + 2 * r;
    for (int row = wave; row < rows; row += 4) {
        const int64_t gy = ty0 - r + row;
        const bool iny = gy >= 0 && gy < Gy;
        for (int c = lane; c < cols; c += 64) {
            const int64_t gx = tx0 - r + c;
            const int v = iny && gx >= 0 && gx < Gx ? cells[gy * Gx + gx] : -1;
            in_s[row * BLUR_IW + c] = v >= 0 ? (unsigned)min(v, 255) | (1u << 20) : 0u;
        }
    }
    __syncthreads();
    for (int row = wave; row < rows; row += 4) {                     // the row pass: N1 | D1 << 20 of window row `row` at tile column `lane`
        const unsigned *p = in_s + row * BLUR_IW + r + lane;
        unsigned s = (unsigned)taps.w[0] * p[0];
#pragma unroll
        for (int d = 1; d <= BLUR_R; ++d) {
            if (d > r) break;
            s += (unsigned)taps.w[d] * (p[-d] + p[d]);
        }
        mid_s[row * BLUR_TW + lane] = s;
    }
    __syncthreads();
    const int64_t gx = tx0 + lane;
#pragma unroll
    for (int k = 0; k < BLUR_TH / 4; ++k) {                          // the column pass: tile row y, tile column `lane`
        const int y = wave * (BLUR_TH / 4) + k;
        const int64_t gy = ty0 + y;
        if (gy >= Gy || gx >= Gx) continue;
        int res = -1;
        if (in_s[(y + r) * BLUR_IW + r + lane] != 0u) {
            const unsigned *q = mid_s + (y + r) * BLUR_TW + lane;
            unsigned N = (unsigned)taps.w[0] * (q[0] & 0xFFFFFu), D = (unsigned)taps.w[0] * (q[0] >> 20);
#pragma unroll
            for (int d = 1; d <= BLUR_R; ++d) {
                if (d > r) break;
                const unsigned a = q[-d * BLUR_TW], b = q[d * BLUR_TW];
                N += (unsigned)taps.w[d] * ((a & 0xFFFFFu) + (b & 0xFFFFFu));
                D += (unsigned)taps.w[d] * ((a >> 20) + (b >> 20));
            }
            res = (int)((2u * N + D) / (2u * D));                  // the cell itself counts and w[0] >= 1: D >= 1
        }
        out[gy * Gx + gx] = res;
    }
}

// One lane's DOWN rows of 4 pixels (three little-endian dwords a row: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3) -> its 4 / DOWN output pixels, 12 / DOWN
// bytes packed in the same order into o. a[c] = alpha' lut[idx][c] + 128 and beta = 256 - alpha', with alpha' = 0 on a cell without a value, so that
// the byte is (a[c] + beta m) >> 8 everywhere: at most 256 * 255 + 128 < 2^16, which is why two bytes of a dword go through one 32-bit multiply-add.
template <int DOWN>
__device__ __forceinline__ void heat_px4(const unsigned (&w)[DOWN][3], const unsigned (&a)[3], unsigned beta, unsigned (&o)[3]) {
    if constexpr (DOWN == 1) {
        const unsigned rb = a[0] | (a[2] << 16), gr = a[1] | (a[0] << 16), bg = a[2] | (a[1] << 16);      // (even byte, odd byte) pairs of the three dwords
        const unsigned ev[3] = {rb, gr, bg}, od[3] = {gr, bg, rb};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = ((((w[0][k] & 0x00FF00FFu) * beta + ev[k]) >> 8) & 0x00FF00FFu) | ((((w[0][k] >> 8) & 0x00FF00FFu) * beta + od[k]) & 0xFF00FF00u);
    } else {
        constexpr int SH = DOWN == 2 ? 2 : 4;                        // log2(DOWN^2)
        unsigned b[12];                                              // the 12 column sums over the DOWN rows, each at most 4 * 255
        column_sums<DOWN>(w, b);
        o[0] = o[1] = o[2] = 0;
#pragma unroll
        for (int p = 0; p < 4 / DOWN; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned s = 0;
#pragma unroll
                for (int d = 0; d < DOWN; ++d) s += b[3 * (p * DOWN + d) + c];
                const unsigned m = (s + (1u << (SH - 1))) >> SH;
                o[(3 * p + c) >> 2] |= ((a[c] + beta * m) >> 8) << (8 * ((3 * p + c) & 3));
            }
    }
}

// a full lane's 12 / DOWN output bytes at any byte address: 12 as three dwords (hipcc merges them), 6 as a dword and a half word, 3 as a half word and a byte
template <int DOWN>
__device__ __forceinline__ void heat_store4(unsigned char *d, const unsigned (&o)[3]) {
    if constexpr (DOWN == 1) {
        *reinterpret_cast<u32_a1 *>(d) = o[0]; *reinterpret_cast<u32_a1 *>(d + 4) = o[1]; *reinterpret_cast<u32_a1 *>(d + 8) = o[2];
    } else if constexpr (DOWN == 2) {
        *reinterpret_cast<u32_a1 *>(d) = o[0]; *reinterpret_cast<u16_a1 *>(d + 4) = (unsigned short)o[1];
    } else {
        *reinterpret_cast<u16_a1 *>(d) = (unsigned short)o[0]; d[2] = (unsigned char)(o[0] >> 16);
    }
}

// ---- the blend pass: toad_region_heat_blend_u8 (no tent, no mask) and toad_region_heat_blend_px_u8 ----
struct HeatPxArgs {
    const unsigned char *region; int64_t pitch; int Hi, Wi;
    const int *cells; int Gy, Gx, shift;
    int alpha;
    const unsigned char *mask; int64_t mask_pitch; int Hm, Wm, mshift, mask_thresh;
    unsigned char *out; int64_t out_pitch; unsigned nchunks;
    int wx, wy;                                                      // the region's pixel (0, 0) in the image that cells and mask describe
};

// heat_px4 with a colour col[p] (0x00bbggrr, as in the LDS table) and an alpha al[p] of its own for each of the row's NP = 4 / DOWN output pixels. At
// DOWN == 1 a pixel's r and b go through one multiply-add as 0x00bb00rr and its g through another: alpha c + 128 + (256 - alpha) m < 2^16 as before, and
// the three output dwords are put together from the second byte of every half.
template <int DOWN>
__device__ __forceinline__ void heat_px4_each(const unsigned (&w)[DOWN][3], const unsigned (&col)[4 / DOWN], const unsigned (&al)[4 / DOWN], unsigned (&o)[3]) {
    if constexpr (DOWN == 1) {
        const unsigned w0 = w[0][0], w1 = w[0][1], w2 = w[0][2];
        const unsigned rb[4] = {w0 & 0x00FF00FFu, (w0 >> 24) | ((w1 << 8) & 0x00FF0000u), ((w1 >> 16) & 0xFFu) | ((w2 & 0xFFu) << 16), (w2 >> 8) & 0x00FF00FFu};
        const unsigned g[4] = {(w0 >> 8) & 0xFFu, w1 & 0xFFu, w1 >> 24, (w2 >> 16) & 0xFFu};
        unsigned RB[4], G[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned beta = 256u - al[p];
            RB[p] = rb[p] * beta + (col[p] & 0x00FF00FFu) * al[p] + 0x00800080u;
            G[p] = g[p] * beta + ((col[p] >> 8) & 0xFFu) * al[p] + 128u;
        }
        o[0] = ((RB[0] >> 8) & 0x00FF00FFu) | (G[0] & 0xFF00u) | ((RB[1] << 16) & 0xFF000000u);                              // r0 g0 b0 r1
        o[1] = ((G[1] >> 8) & 0xFFu) | ((RB[1] >> 16) & 0xFF00u) | ((RB[2] << 8) & 0x00FF0000u) | ((G[2] << 16) & 0xFF000000u);      // g1 b1 r2 g2
        o[2] = (RB[2] >> 24) | (RB[3] & 0xFF00FF00u) | ((G[3] << 8) & 0x00FF0000u);                                          // b2 r3 g3 b3
    } else {
        constexpr int SH = DOWN == 2 ? 2 : 4;                        // log2(DOWN^2)
        unsigned b[12];
        column_sums<DOWN>(w, b);
        o[0] = o[1] = o[2] = 0;
#pragma unroll
        for (int p = 0; p < 4 / DOWN; ++p) {
            const unsigned beta = 256u - al[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned s = 0;
#pragma unroll
                for (int d = 0; d < DOWN; ++d) s += b[3 * (p * DOWN + d) + c];
                const unsigned m = (s + (1u << (SH - 1))) >> SH;
                o[(3 * p + c) >> 2] |= ((al[p] * ((col[p] >> (8 * c)) & 255u) + 128u + beta * m) >> 8) << (8 * ((3 * p + c) & 3));
            }
        }
    }
}

// n of the NB = 4, 2 or 1 mask bytes at p exist: those bytes as a little-endian word, 0 for the others (0 is above no threshold: not tissue). Touches
// nothing beyond the n bytes.
template <int NB>
__device__ __forceinline__ unsigned load_mask(const unsigned char *p, int n) {
    if (n == NB) {
        if constexpr (NB == 4) return *reinterpret_cast<const u32_a1 *>(p);
        else if constexpr (NB == 2) return *reinterpret_cast<const u16_a1 *>(p);
        else return p[0];
    }
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < NB - 1; ++k)
        if (k < n) v |= (unsigned)p[k] << (8 * k);
    return v;
}

// The work split and its addresses are region_u8.h's, on strips of 16 rows (4 a wave, 12 dwords a lane in flight) over the Hi = DOWN Ho rows and
// Wi = DOWN Wo columns of the region that some output pixel consumes; nothing outside them is touched. What differs here: a lane owns a 4-pixel-wide,
// DOWN-row-high block and writes its 4 / DOWN output pixels - 12, 6 or 3 bytes - as dword, half-word and byte stores at any byte address (the row base
// oy out_pitch is 64-bit like y pitch); off the plain path it takes the wide stores only where x + 4 <= Wi and byte stores for the 1 to 3 pixels of the
// lane the row ends in. x is a multiple of 4 and the wave's first row one too, so with cell >= 4 a lane's 4 x 4 pixels lie in ONE cell: one load of the
// own cell per lane, lookups in the 256 colours the workgroup has packed into 1 KB of LDS. The variants differ only in blend_row, in how a row's colours
// and alphas come about. SMOOTH 0 without a mask is the flat canvas: the own cell's colour and alpha for all of the lane's pixels, through heat_px4. The
// others decide per canvas pixel, through heat_px4_each:
//   index   SMOOTH 0: the cell's own. SMOOTH 1 (cell >= 8): the 4 x 4 pixels also lie in one QUADRANT of the cell - 2 x .. 2 x + 8 holds no cell centre,
//           those are multiples of 8 in doubled coordinates - so g0 is the lane's: four neighbour loads, f steps by 2 DOWN from pixel to pixel. SMOOTH 2
//           (cell == 4): the lane's pixels are the whole width of the cell and straddle its centre: nine loads, g0 and f compile-time constants of the
//           pixel. Either way the tent is separable: H[r][j] = 2 cell v[r][0] + fx_j (v[r][1] - v[r][0]) per neighbour row and pixel column, then
//           S = 2 cell H[0][j] + fy_i (H[1][j] - H[0][j]). A neighbour outside the table or without a value is replaced by the own cell; where that has none
//           either the pixel is not blended, and max(own, 0) only keeps the lookup inside the table.
//   tissue  tis[r] = the mask bytes of region row y0 + r under the lane's 4 pixels, one byte a pixel: mask_down >= 4 is ONE byte for the whole block
//           (mask_down is a power of two and x, y0 are multiples of 4), 2 two rows of two bytes, 1 four dwords. Outside Hm x Wm the byte is 0.
//   alpha   al = alpha where own >= 0 and the byte is above the threshold, else 0: no branch.
// lut_s: the workgroup's 256 packed colours. No barrier in here: the caller has filled lut_s.
template <int DOWN, int SMOOTH, bool MASK>
__device__ __forceinline__ void heat_px_lane(const HeatPxArgs &a, const unsigned *lut_s, unsigned chunk, unsigned rb, int wave, int lane) {
    constexpr int RW = 4, ORW = RW / DOWN, NP = 4 / DOWN, OB = 12 / DOWN;      // rows per wave, output rows per wave, output pixels and bytes per lane and output row
    constexpr bool FLAT = SMOOTH == 0 && !MASK;
    const unsigned x = chunk * 256u + (unsigned)lane * 4u, off = 3u * x, ooff = off / DOWN;
    const int64_t y0 = (int64_t)rb * 16 + wave * RW;               // first row of this wave (may lie below Hi: then it writes nothing)
    if (y0 >= a.Hi) return;
    const bool live = x < (unsigned)a.Wi;
    const unsigned sx = x + (unsigned)a.wx;                        // the block's corner in the table's image: multiples of 4 like x and y0
    const int64_t sy0 = y0 + a.wy;
    const int gy = (int)(sy0 >> a.shift), gx = (int)(sx >> a.shift);
    const int own = live ? min(a.cells[(int64_t)gy * a.Gx + gx], 255) : -1;

    unsigned ua[3], ubeta;                                         // FLAT: heat_px4's a[] and beta, alpha' = 0 on a cell without a value
    int idx[NP][NP];                                                 // otherwise: the colour index of each of the lane's canvas pixels
    if constexpr (FLAT) {
        const unsigned col = lut_s[max(own, 0)], al = own >= 0 ? (unsigned)a.alpha : 0u;
        ubeta = 256u - al;
#pragma unroll
        for (int c = 0; c < 3; ++c) ua[c] = al * ((col >> (8 * c)) & 255u) + 128u;
    } else if constexpr (SMOOTH == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = 0; j < NP; ++j) idx[i][j] = max(own, 0);
    } else {
        constexpr int NB = SMOOTH == 2 ? 3 : 2;                      // the neighbourhood: NB x NB cells from (by, bx)
        const int cell = 1 << a.shift, c2 = 2 * cell;
        int bx, by, fx0 = 0, fy0 = 0;
        if constexpr (SMOOTH == 1) {
            const int px = (int)(2u * sx) + DOWN - cell;             // wx + Wr < 2^30, so 2 sx fits on every live lane
            const int64_t py = 2 * sy0 + DOWN - cell;
            bx = px >> (a.shift + 1); fx0 = px & (c2 - 1);
            by = (int)(py >> (a.shift + 1)); fy0 = (int)(py & (c2 - 1));
        } else {
            bx = gx - 1; by = gy - 1;
        }
        int v[NB][NB];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int yy = by + r, xx = bx + c;
                const bool in = live && yy >= 0 && yy < a.Gy && xx >= 0 && xx < a.Gx;
                const int t = in ? a.cells[(int64_t)yy * a.Gx + xx] : -1;
                v[r][c] = t >= 0 ? min(t, 255) : max(own, 0);
            }
        int H[NB][NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int pj = 2 * DOWN * j + DOWN - 4;                  // SMOOTH 2: the pixel's doubled offset from the cell's centre
            const int ca = SMOOTH == 2 && pj >= 0 ? 1 : 0, fx = SMOOTH == 2 ? (pj & 7) : fx0 + 2 * DOWN * j;
#pragma unroll
            for (int r = 0; r < NB; ++r) H[r][j] = c2 * v[r][ca] + fx * (v[r][ca + 1] - v[r][ca]);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pi = 2 * DOWN * i + DOWN - 4;
            const int ra = SMOOTH == 2 && pi >= 0 ? 1 : 0, fy = SMOOTH == 2 ? (pi & 7) : fy0 + 2 * DOWN * i;
#pragma unroll
            for (int j = 0; j < NP; ++j) idx[i][j] = (c2 * H[ra][j] + fy * (H[ra + 1][j] - H[ra][j]) + 2 * cell * cell) >> (2 * a.shift + 2);
        }
    }

    unsigned tis[RW] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    int thr = -1;                                                    // without a mask every byte is above it
    if constexpr (MASK) {
        thr = a.mask_thresh;
        const unsigned mx = sx >> a.mshift;
        const int64_t my = sy0 >> a.mshift;
        const int have = live && mx < (unsigned)a.Wm ? a.Wm - (int)mx : 0;      // mask columns from mx on that exist
        const unsigned char *mp = a.mask + my * a.mask_pitch + mx;
        if (a.mshift >= 2) {
            const unsigned t = load_mask<1>(mp, my < a.Hm ? min(have, 1) : 0) * 0x01010101u;
#pragma unroll
            for (int r = 0; r < RW; ++r) tis[r] = t;
        } else if (DOWN <= 2 && a.mshift == 1) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const unsigned t = load_mask<2>(mp + r * a.mask_pitch, my + r < a.Hm ? min(have, 2) : 0);
                tis[2 * r] = tis[2 * r + 1] = (t & 0xFFu) * 0x0101u | (t >> 8) * 0x01010000u;
            }
        } else if (DOWN == 1) {
#pragma unroll
            for (int r = 0; r < RW; ++r) tis[r] = load_mask<4>(mp + r * a.mask_pitch, my + r < a.Hm ? min(have, 4) : 0);
        }
    }

    const unsigned char *src = a.region + y0 * a.pitch + off;
    unsigned char *dst = a.out + (y0 / DOWN) * a.out_pitch + ooff;
    // output row q of the lane from its DOWN region rows
    auto blend_row = [&](int q, const unsigned (&w)[DOWN][3], unsigned (&o)[3]) {
        if constexpr (FLAT) {
            heat_px4<DOWN>(w, ua, ubeta, o);
        } else {
            unsigned col[NP], al[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                col[j] = lut_s[idx[q][j]];
                al[j] = own >= 0 && (int)((tis[DOWN * q] >> (8 * DOWN * j)) & 0xFFu) > thr ? (unsigned)a.alpha : 0u;
            }
            heat_px4_each<DOWN>(w, col, al, o);
        }
    };
    if (chunk * 256u + 256u <= (unsigned)a.Wi && y0 + RW <= a.Hi) {  // wave-uniform: all 768 bytes of all 4 rows are consumed
        unsigned w[ORW][DOWN][3];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) w[r / DOWN][r % DOWN][k] = *reinterpret_cast<const u32_a1 *>(src + r * a.pitch + 4 * k);
#pragma unroll
        for (int q = 0; q < ORW; ++q) {
            unsigned o[3];
            blend_row(q, w[q], o);
            heat_store4<DOWN>(dst + q * a.out_pitch, o);
        }
    } else {
        const int rows = (int)min((int64_t)ORW, (a.Hi - y0) / DOWN);  // output rows of this wave that exist: Hi and y0 are multiples of DOWN
        const int npx = live ? min(4, a.Wi - (int)x) : 0;            // pixels of this lane that are consumed: 0, DOWN, .., 4
        const int nout = 3 * npx / DOWN;                             // bytes to write per output row
        constexpr int UNROLL = FLAT ? 1 : ORW;                       // unrolled where blend_row uses q, so that it indexes registers
#pragma unroll UNROLL
        for (int q = 0; q < ORW; ++q) {
            if (q >= rows) break;
            unsigned w[DOWN][3];
#pragma unroll
            for (int r = 0; r < DOWN; ++r) load_px4(src + (q * DOWN + r) * a.pitch, npx, w[r]);
            unsigned o[3];
            blend_row(q, w, o);
            unsigned char *d = dst + q * a.out_pitch;
            if (npx == 4) {
                heat_store4<DOWN>(d, o);
            } else {
#pragma unroll
                for (int k = 0; k < OB; ++k)
                    if (k < nout) d[k] = (unsigned char)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// Bounded to 8 waves per SIMD: left alone, the two tent variants with a mask at DOWN == 1 take 65 registers and lose a wave for one register.
template <int DOWN, int SMOOTH, bool MASK>
__global__ __launch_bounds__(256, 8) void heat_blend_px_kernel(const HeatPxArgs a, const unsigned char *__restrict__ lut) {
    __shared__ unsigned lut_s[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    lut_s[tid] = (unsigned)lut[3 * tid] | ((unsigned)lut[3 * tid + 1] << 8) | ((unsigned)lut[3 * tid + 2] << 16);
    __syncthreads();
    heat_px_lane<DOWN, SMOOTH, MASK>(a, lut_s, blockIdx.x % a.nchunks, blockIdx.x / a.nchunks, wave, lane);
}

// ---- the overview canvas: toad_region_heat_thumb_u8, down in {8, 16, 32} ----
// sat_plane_kernel's DOWN >= 8 arm (tissue_seg.hip) with the three channel means kept and the blend in the tail. The work split and its addresses are
// region_u8.h's, on strips of RB = strip_rows(DOWN) rows (12 or 24 dwords a lane in flight): the DOWN / 4 lanes of a box are summed by DPP moves, the 2 or
// 4 waves of a box row meet in 3 KB of LDS behind the one barrier all 256 threads reach, and NB CPR = 64, 16 or 8 threads each finish one canvas pixel.
// Hi = DOWN Ho and Wi = DOWN Wo are the rows and columns some box consumes: nothing outside them is read. Wi is a multiple of DOWN >= 8, so a lane has
// all 4 of its pixels or none; a wave off the plain path holds zeros for what is not consumed, which is harmless because a box lies wholly inside
// Hi x Wi or wholly outside. A box lies in one cell (down <= cell) and in one mask pixel (mask_down a multiple of down), so the pixel's own cell, its
// tent (the formula of heat_px_lane's SMOOTH 1 at the box's corner: g0 and f are the pixel's) and its mask byte are single loads; smooth and the mask
// are run-time values because only these few threads look at them, and the colour comes straight from lut in global memory. Every canvas byte is
// written once, by one lane, with byte stores at any address; nothing outside oy out_pitch + [0, 3 Wo), oy < Ho, is written. WINDOW: the box's corner in
// the table's image is the region's plus (wx, wy) - a template parameter here and not in heat_blend_px_kernel, because here the two adds were measured:
// they sit in the dependent chain behind the barrier, where the few finishing threads wait for one load after the other, and cost the three older
// instantiations 1 to 3 % (tools/heatmap_bench.py --window --w0-only against the library as it was); the px kernels showed no difference.
// The body lies in heat_thumb_body.inc, which heat_thumb_list_kernel includes too.
template <int DOWN, bool WINDOW>
__global__ __launch_bounds__(256) void heat_thumb_kernel(const HeatPxArgs a, int smooth, const unsigned char *__restrict__ lut) {
    const unsigned bid = blockIdx.x;
#include "heat_thumb_body.inc"
}

// ---- a list of windows of one slide in one launch: toad_region_heat_windows_u8 ----
// The list forms of the two single-level kernels. The windows share the table, the mask plane, the colours, alpha and down - `shared`, whose region, out,
// extents and place are unused - and each has a descriptor of its own; the descriptors travel by value in the kernel argument, as HeatBlurTaps does: no
// device table, no upload. The grid is the windows' workgroups one after the other, descriptor k owning workgroups first[k] .. first[k + 1]; descriptors
// from n on carry first = 0xFFFFFFFF, above every workgroup index, so the search needs no n: five uniform steps of a binary search over the 32 prefixes,
// scalar loads from the kernarg segment, once per workgroup. From there on a workgroup is one of its window's: HeatPxArgs from the shared part and the
// descriptor, chunk and rb from its index inside the window, and the body the single-window kernel runs. The grid is exact: every workgroup has a window.
// Windows without a workgroup (Hr < down or Wr < down) never reach a descriptor.
constexpr int HEAT_LIST_MAX = 32;                                    // 32 descriptors of 56 bytes and the shared part: 1.9 KB of the 4 KB a kernel argument may have
struct HeatListWin {
    const unsigned char *region; int64_t pitch; unsigned char *out; int64_t out_pitch;
    int Hi, Wi, wx, wy; unsigned nchunks, first;
};
struct HeatListArgs { HeatPxArgs shared; HeatListWin w[HEAT_LIST_MAX]; };

// the window of workgroup `bid` -> its HeatPxArgs; local = the workgroup's index inside the window
__device__ __forceinline__ HeatPxArgs heat_list_window(const HeatListArgs &l, unsigned bid, unsigned &local) {
    static_assert(HEAT_LIST_MAX == 32, "five steps search 32 prefixes");
    int k = 0;
#pragma unroll
    for (int step = HEAT_LIST_MAX / 2; step >= 1; step >>= 1)
        if (l.w[k + step].first <= bid) k += step;
    const HeatListWin &w = l.w[k];
    HeatPxArgs a = l.shared;
    a.region = w.region; a.pitch = w.pitch; a.Hi = w.Hi; a.Wi = w.Wi;
    a.out = w.out; a.out_pitch = w.out_pitch; a.nchunks = w.nchunks;
    a.wx = w.wx; a.wy = w.wy;
    local = bid - w.first;
    return a;
}

template <int DOWN, int SMOOTH, bool MASK>
__global__ __launch_bounds__(256, 8) void heat_blend_px_list_kernel(const HeatListArgs l, const unsigned char *__restrict__ lut) {
    __shared__ unsigned lut_s[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    lut_s[tid] = (unsigned)lut[3 * tid] | ((unsigned)lut[3 * tid + 1] << 8) | ((unsigned)lut[3 * tid + 2] << 16);
    __syncthreads();
    unsigned local;
    const HeatPxArgs a = heat_list_window(l, blockIdx.x, local);
    heat_px_lane<DOWN, SMOOTH, MASK>(a, lut_s, local % a.nchunks, local / a.nchunks, wave, lane);
}

template <int DOWN>
__global__ __launch_bounds__(256) void heat_thumb_list_kernel(const HeatListArgs l, int smooth, const unsigned char *__restrict__ lut) {
    constexpr bool WINDOW = true;
    unsigned bid;
    const HeatPxArgs a = heat_list_window(l, blockIdx.x, bid);
#include "heat_thumb_body.inc"
}

// ---- the pyramid: toad_region_heat_pyramid_u8, several of the six canvases from ONE read of the region ----
// Every level is defined from the region's own box sums, and box sums nest, so each canvas is byte for byte the one its own kernel above writes. The work
// split is region_u8.h's over the window's Hr x Wr on strips of RB = max(16, D) rows, D the largest level asked for: a lane holds RW = RB / 4 = 4 or 8
// rows of 4 pixels, 12 or 24 dwords in flight, loaded once; what does not exist reads as 0 and is never part of a box that is written.
//   1, 2, 4   finished in the lane from each of its 4 x 4 blocks: heat_px_lane's arithmetic through heat_px4_each, with the own cell, the four tent
//             neighbours and the mask bytes of a block loaded ONCE for its up to three levels. 2 x + 1 - cell .. 2 x + 4 - cell crosses no multiple of
//             2 cell (cell >= 8 under the tent), so g0 is the block's for every level and only f moves with the level: f = f_block + down + 2 down j.
//   8, 16, 32 heat_thumb_kernel's tail: the lane's column sums over its RW rows, 2, 4 and 8 lanes summed by three DPP moves, the waves of a box row
//             meeting in 4.5 KB of LDS behind the one barrier all 256 threads reach; threads 0 .. 127, 128 .. 159 and 192 .. 199 - three different
//             waves - each finish one canvas pixel of level 8, 16 and 32.
// levels and smooth are run-time, wave-uniform values; the template is the strip height and MASK. Each level keeps its own Ho x Wo: Ho[k] = 0 marks a
// level that was not asked for or is empty. Every canvas byte is written once by one lane, nothing outside oy pitch_k + [0, 3 Wo_k) is written, there is
// no atomic. The tent at cell == 4 (heat_px_lane's SMOOTH 2) is not done here: the launcher refuses it.
// The body lies in heat_pyramid_body.inc, which heat_pyramid_list_kernel includes too.
struct HeatPyrArgs {
    HeatPxArgs a;                                                    // Hi x Wi = Hr x Wr; out, out_pitch unused
    unsigned char *out[6]; int64_t pitch[6]; int Ho[6], Wo[6];
    unsigned levels; int smooth;
};

// One 4 x 4 block of a lane -> its 4 / DOWN rows of 4 / DOWN pixels of canvas log2(DOWN), where they exist. own, v, fxb, fyb, tis, thr: the block's.
template <int DOWN>
__device__ __forceinline__ void heat_pyr_fine(const HeatPyrArgs &p, const unsigned *lut_s, const unsigned (&w)[4][3], unsigned x, int64_t yg, int own,
                                              bool tent, const int (&v)[2][2], int fxb, int fyb, const unsigned (&tis)[4], int thr) {
    constexpr int K = DOWN == 1 ? 0 : DOWN == 2 ? 1 : 2, NP = 4 / DOWN, OB = 12 / DOWN;
    const int Ho = p.Ho[K];
    const int64_t oy0 = yg / DOWN;
    const int npx = min(4, p.Wo[K] * DOWN - (int)x);               // pixels of this lane the level consumes: <= 0, DOWN, .., 4
    if (npx <= 0 || oy0 >= Ho) return;
    int idx[NP][NP];
    if (!tent) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = 0; j < NP; ++j) idx[i][j] = max(own, 0);
    } else {
        const int cell = 1 << p.a.shift, c2 = 2 * cell;
        int H[2][NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int fx = fxb + DOWN + 2 * DOWN * j;
#pragma unroll
            for (int r = 0; r < 2; ++r) H[r][j] = c2 * v[r][0] + fx * (v[r][1] - v[r][0]);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int fy = fyb + DOWN + 2 * DOWN * i;
#pragma unroll
            for (int j = 0; j < NP; ++j) idx[i][j] = (c2 * H[0][j] + fy * (H[1][j] - H[0][j]) + 2 * cell * cell) >> (2 * p.a.shift + 2);
        }
    }
    unsigned char *dst = p.out[K] + oy0 * p.pitch[K] + 3u * x / DOWN;
    const int nout = 3 * npx / DOWN;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        if (oy0 + q >= Ho) break;
        unsigned wq[DOWN][3], col[NP], al[NP], o[3];
#pragma unroll
        for (int r = 0; r < DOWN; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) wq[r][k] = w[q * DOWN + r][k];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            col[j] = lut_s[idx[q][j]];
            al[j] = own >= 0 && (int)((tis[DOWN * q] >> (8 * DOWN * j)) & 0xFFu) > thr ? (unsigned)p.a.alpha : 0u;
        }
        heat_px4_each<DOWN>(wq, col, al, o);
        unsigned char *d = dst + q * p.pitch[K];
        if (npx == 4) {
            heat_store4<DOWN>(d, o);
        } else {
#pragma unroll
            for (int k = 0; k < OB; ++k)
                if (k < nout) d[k] = (unsigned char)(o[k >> 2] >> (8 * (k & 3)));
        }
    }
}

template <int RB, bool MASK>
__global__ __launch_bounds__(256) void heat_pyramid_kernel(const HeatPyrArgs p, const unsigned char *__restrict__ lut) {
    const unsigned bid = blockIdx.x;
    auto level_Ho = [&](int k) { return p.Ho[k]; };
    auto level_Wo = [&](int k) { return p.Wo[k]; };
    auto level_out = [&](int k) { return p.out[k]; };
    auto level_pitch = [&](int k) { return p.pitch[k]; };
#include "heat_pyramid_body.inc"
}

// ---- the pyramid of a list of windows of one slide in one launch: toad_region_heat_pyramid_windows_u8 ----
// The list form of heat_pyramid_kernel, as heat_blend_px_list_kernel is the list form of heat_blend_px_kernel. The windows share the table, the mask plane,
// the colours, alpha, smooth and the SET of levels - so D, the largest level, and RB are the list's - and each has a descriptor of its own: region, pitch,
// extent, place, six canvases and their pitches, nchunks and its first workgroup, 136 bytes against HeatListWin's 56. The descriptors travel by value in the
// kernel argument, 16 a launch; descriptors from n on carry first = 0xFFFFFFFF, so four uniform steps of a binary search over the 16 prefixes find a
// workgroup's window. It then forms the window's HeatPyrArgs: Ho[k] = Hr >> k and Wo[k] = Wr >> k for the levels asked for, and a level that is empty for
// THIS window gets extent 0 and leaves the window's set, exactly as the pyramid entry leaves it out on the host. From there on the body is
// heat_pyramid_kernel's. A window's workgroups are counted from its full Hr x Wr on strips of RB rows: the finer levels need the rows a coarse level
// drops. The grid is exact, and a window in which every level is empty never reaches a descriptor.
constexpr int HEAT_PYR_LIST_MAX = 16;                                // 16 descriptors of 136 bytes and the shared part: 2.3 KB of the 4 KB a kernel argument may have
struct HeatPyrListWin {
    const unsigned char *region; int64_t pitch; int Hr, Wr, wx, wy;
    unsigned char *out[6]; int64_t out_pitch[6]; unsigned nchunks, first;
};
struct HeatPyrListArgs { HeatPxArgs shared; unsigned levels; int smooth; HeatPyrListWin w[HEAT_PYR_LIST_MAX]; };
static_assert(sizeof(HeatPyrListWin) == 136 && sizeof(HeatPyrListArgs) + sizeof(const unsigned char *) <= 4096, "the descriptors and lut must fit a kernel argument");

template <int RB, bool MASK>
__global__ __launch_bounds__(256) void heat_pyramid_list_kernel(const HeatPyrListArgs l, const unsigned char *__restrict__ lut) {
    static_assert(HEAT_PYR_LIST_MAX == 16, "four steps search 16 prefixes");
    int win = 0;
#pragma unroll
    for (int step = HEAT_PYR_LIST_MAX / 2; step >= 1; step >>= 1)
        if (l.w[win + step].first <= blockIdx.x) win += step;
    const HeatPyrListWin &lw = l.w[win];
    HeatPyrArgs p;
    p.a = l.shared;
    p.a.region = lw.region; p.a.pitch = lw.pitch; p.a.Hi = lw.Hr; p.a.Wi = lw.Wr;
    p.a.nchunks = lw.nchunks; p.a.wx = lw.wx; p.a.wy = lw.wy;
    p.levels = 0; p.smooth = l.smooth;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int Ho = lw.Hr >> k, Wo = lw.Wr >> k;
        const bool has = (l.levels >> k & 1u) && Ho != 0 && Wo != 0;
        p.out[k] = lw.out[k]; p.pitch[k] = lw.out_pitch[k];
        p.Ho[k] = has ? Ho : 0; p.Wo[k] = has ? Wo : 0;
        if (has) p.levels |= 1u << k;
    }
    const unsigned bid = blockIdx.x - lw.first;
    // the tail's level by a per-thread index: the extents again from the descriptor, the canvas from the kernel argument where it lies
    const unsigned has = p.levels;
    auto level_Ho = [&](int k) { return has >> k & 1u ? lw.Hr >> k : 0; };
    auto level_Wo = [&](int k) { return has >> k & 1u ? lw.Wr >> k : 0; };
    auto level_out = [&](int k) { return lw.out[k]; };
    auto level_pitch = [&](int k) { return lw.out_pitch[k]; };
#include "heat_pyramid_body.inc"
}

}  // namespace toad

using namespace toad;

extern "C" int toad_heat_cells(const int *tile_q, int nx, int ny, int cell, int x0, int y0, int H, int W, int sx, int sy, int Gy, int Gx, int *cells,
                               void *stream) {
    const char *what = "toad_heat_cells";
    if (!tile_q || !cells) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_lattice_units(what, cell, x0, y0, H, W, sx, sy, nx, ny, Gy, Gx)) return rc;
    const int64_t cover = (((int64_t)H + sy - 1) / sy) * (((int64_t)W + sx - 1) / sx);
    if (cover > 4096) {
        set_error("%s: coverage ceil(H / sy) * ceil(W / sx) = %lld exceeds 4096 tiles per cell (the int32 sum of their scores)", what, (long long)cover);
        return TOAD_ESHAPE;
    }
    if (int rc = check_lattice_extent(what, cell, x0, y0, H, W, sx, sy, nx, ny, Gy, Gx)) return rc;
    if (!aligned4(tile_q) || !aligned4(cells)) { set_error("%s: tile_q and cells (int32) must be 4-byte aligned", what); return TOAD_EALIGN; }
    const uint64_t g = ((uint64_t)Gy * Gx + 255) / 256;
    hipLaunchKernelGGL(heat_cells_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, tile_q, nx, ny, x0 / cell, y0 / cell,
                       H / cell, W / cell, sx / cell, sy / cell, Gy, Gx, cells);
    return check_launch(what);
}

extern "C" int toad_heat_cells_blur(const int *cells, int Gy, int Gx, const int *taps, int radius, int *out, void *stream) {
    const char *what = "toad_heat_cells_blur";
    if (!cells || !out) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (Gy < 1 || Gx < 1 || (int64_t)Gy * Gx >= ((int64_t)1 << 31)) {
        set_error("%s: bad shape Gy=%d Gx=%d (both >= 1, Gy * Gx < 2^31)", what, Gy, Gx);
        return TOAD_ESHAPE;
    }
    if (radius < 1 || radius > BLUR_R) { set_error("%s: radius = %d must lie in 1 .. %d cells", what, radius, BLUR_R); return TOAD_ESHAPE; }
    if (!taps) { set_error("%s: null taps (a HOST array of radius + 1 ints)", what); return TOAD_EINVAL; }
    HeatBlurTaps t = {};
    int64_t sum = 0;
    for (int d = 0; d <= radius; ++d) {
        if (taps[d] < (d == 0 ? 1 : 0) || taps[d] > 1024) {
            set_error("%s: taps[%d] = %d (taps[0] >= 1, every tap >= 0, taps[0] + 2 * sum of the others <= 1024)", what, d, taps[d]);
            return TOAD_EINVAL;
        }
        t.w[d] = taps[d];
        sum += d == 0 ? taps[d] : 2 * (int64_t)taps[d];
    }
    if (sum > 1024) {
        set_error("%s: the taps sum to %lld: taps[0] + 2 * sum of the others must not exceed 1024 (2 N + D in int32)", what, (long long)sum);
        return TOAD_EINVAL;
    }
    if (out == cells) { set_error("%s: out must not be cells (a cell is read by its neighbours' threads)", what); return TOAD_EINVAL; }
    if (!aligned4(cells) || !aligned4(out)) { set_error("%s: cells and out (int32) must be 4-byte aligned", what); return TOAD_EALIGN; }
    const int64_t ntx = ((int64_t)Gx + BLUR_TW - 1) / BLUR_TW, blocks = ntx * (((int64_t)Gy + BLUR_TH - 1) / BLUR_TH);      // < 2^21 + 2^27 + 2^25
    hipLaunchKernelGGL(heat_cells_blur_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cells, Gy, Gx, t, radius, (unsigned)ntx, out);
    return check_launch(what);
}

// The canvas checks that the window entry and the list entry both make, each with the one message: the list entry makes the ones about the shared arguments
// once and the others per window, under a `what` that names the window.
static int check_heat_alpha(const char *what, int alpha) {
    if (alpha >= 0 && alpha <= 256) return TOAD_OK;
    set_error("%s: alpha = %d must lie in [0, 256] (256 = the colour alone)", what, alpha);
    return TOAD_ESHAPE;
}
static int check_heat_window_down(const char *what, int down, int cell) {      // any of the six; from 8 on heat_thumb_kernel, whose box must lie in one cell
    if (down != 1 && down != 2 && down != 4 && down != 8 && down != 16 && down != 32) {
        set_error("%s: down = %d is not one of 1, 2, 4, 8, 16, 32", what, down);
        return TOAD_ESHAPE;
    }
    if (down >= 8 && down > cell) { set_error("%s: down = %d exceeds cell = %d (a canvas box must lie in one cell)", what, down, cell); return TOAD_ESHAPE; }
    return TOAD_OK;
}
static int check_heat_place(const char *what, bool window, int down, int wx, int wy, int Wr) {
    const int walign = down > 4 ? down : 4;                          // a lane's 4 x 4 block and a canvas box stay in one cell and in one mask pixel
    if (wx < 0 || wy < 0 || wx % walign || wy % walign) {
        set_error("%s: window (wx, wy) = (%d, %d) is negative or not a multiple of max(4, down) = %d (a lane's 4 x 4 block and a canvas box must lie in one "
                  "cell and in one mask pixel)", what, wx, wy, walign);
        return TOAD_ESHAPE;
    }
    if (window && (int64_t)wx + Wr >= (1ll << 30)) {
        set_error("%s: window too far right: wx + Wr = %lld must stay below 2^30 (doubled tent coordinates in 32 bits)", what, (long long)wx + Wr);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}
static int check_heat_smooth(const char *what, int smooth) {
    if (smooth == 0 || smooth == 1) return TOAD_OK;
    set_error("%s: smooth = %d must be 0 or 1", what, smooth);
    return TOAD_EINVAL;
}
// mshift = log2(mask_down), 0 without a plane. window: the plane is the image's, of any extent; otherwise it is exactly the region's (Hr x Wr).
static int check_heat_mask(const char *what, bool window, int down, int Hr, int Wr, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down,
                           int mask_thresh, int &mshift) {
    mshift = 0;
    if (!mask) return TOAD_OK;
    if (mask_down != 1 && mask_down != 2 && mask_down != 4 && mask_down != 8 && mask_down != 16 && mask_down != 32) {
        set_error("%s: mask_down = %d is not one of 1, 2, 4, 8, 16, 32", what, mask_down);
        return TOAD_ESHAPE;
    }
    if (mask_down % down) {
        set_error("%s: mask_down = %d is not a multiple of down = %d (a canvas box must lie in one mask pixel)", what, mask_down, down);
        return TOAD_ESHAPE;
    }
    if (window) {                                                    // what lies outside the plane is not tissue
        if (Hm < 0 || Wm < 0) { set_error("%s: Hm x Wm = %d x %d must not be negative", what, Hm, Wm); return TOAD_ESHAPE; }
    } else if (Hm != Hr / mask_down || Wm != Wr / mask_down) {
        set_error("%s: Hm x Wm = %d x %d is not (Hr / mask_down) x (Wr / mask_down) = %d x %d", what, Hm, Wm, Hr / mask_down, Wr / mask_down);
        return TOAD_ESHAPE;
    }
    if (int rc = check_plane_pitch(what, Wm, "mask_pitch", mask_pitch)) return rc;
    if (int rc = check_u8(what, "mask_thresh", mask_thresh)) return rc;
    while ((1 << mshift) < mask_down) ++mshift;
    return TOAD_OK;
}
static int check_heat_out_pitch(const char *what, int64_t out_pitch, int Wo) {
    if (out_pitch >= 3 * (int64_t)Wo) return TOAD_OK;
    set_error("%s: out_pitch %lld is less than a row of the canvas (3 Wo = %lld bytes)", what, (long long)out_pitch, 3ll * Wo);
    return TOAD_ESHAPE;
}
static int check_heat_table_holds(const char *what, int wx, int wy, int Hr, int Wr, int cell, int Gy, int Gx) {
    const int64_t gy_end = ((int64_t)wy + Hr + cell - 1) / cell, gx_end = ((int64_t)wx + Wr + cell - 1) / cell;
    if (gy_end <= Gy && gx_end <= Gx) return TOAD_OK;
    set_error("%s: the window ends at cell row %lld and cell column %lld, beyond the table's Gy x Gx = %d x %d (ceil((wy + Hr) / cell) <= Gy and "
              "ceil((wx + Wr) / cell) <= Gx)", what, (long long)gy_end, (long long)gx_end, Gy, Gx);
    return TOAD_ESHAPE;
}

// All three canvas entry points: every check in the order in which the first failing one wins, the geometry, the choice of the kernel. The flat entry passes
// smooth = 0 and mask = NULL, for which the smooth and mask checks are no-ops; `unaligned` names the planes its alignment message lets lie anywhere. `thumb`
// is the overview entry: down in {8, 16, 32} and at most the cell, strips of strip_rows(down) rows, heat_thumb_kernel<down>. `window` is the window entry
// (toad_region_heat_window_u8): the region is the window at (wx, wy) of the image that cells and mask describe, any of the six down values picks its
// kernel, the table and the plane need only hold the window; the other three pass wx = wy = 0 and demand a table and a plane of exactly the region's extent.
static int launch_heat_blend(const char *what, const char *unaligned, bool thumb, bool window, const unsigned char *region, int64_t pitch, int Hr, int Wr, int wx, int wy,
                             const int *cells, int Gy, int Gx, int cell, const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask,
                             int64_t mask_pitch, int Hm, int Wm, int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream) {
    if (!region || !cells || !lut || !out) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_hw(what, "Hr", Hr, "Wr", Wr)) return rc;
    if (int rc = check_heat_alpha(what, alpha)) return rc;
    if (window) {
        if (int rc = check_heat_window_down(what, down, cell)) return rc;
        thumb = down >= 8;
    } else if (thumb) {
        if (down != 8 && down != 16 && down != 32) { set_error("%s: down = %d is not one of 8, 16, 32", what, down); return TOAD_ESHAPE; }
        if (down > cell) {
            set_error("%s: down = %d exceeds cell = %d (a canvas box must lie in one cell)", what, down, cell);
            return TOAD_ESHAPE;
        }
    } else if (down != 1 && down != 2 && down != 4) {
        set_error("%s: down = %d is not one of 1, 2, 4", what, down);
        return TOAD_ESHAPE;
    }
    if (int rc = check_heat_place(what, window, down, wx, wy, Wr)) return rc;
    if (int rc = check_heat_smooth(what, smooth)) return rc;
    if (int rc = check_region_pitch(what, pitch, Wr)) return rc;
    int mshift = 0;
    if (int rc = check_heat_mask(what, window, down, Hr, Wr, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, mshift)) return rc;
    const int Ho = Hr / down, Wo = Wr / down;
    if (int rc = check_heat_out_pitch(what, out_pitch, Wo)) return rc;
    if (window) {
        if (int rc = check_heat_table_holds(what, wx, wy, Hr, Wr, cell, Gy, Gx)) return rc;
    } else if (Gy != (int)(((int64_t)Hr + cell - 1) / cell) || Gx != (int)(((int64_t)Wr + cell - 1) / cell)) {
        set_error("%s: Gy x Gx = %d x %d is not ceil(Hr / cell) x ceil(Wr / cell) = %lld x %lld", what, Gy, Gx, ((long long)Hr + cell - 1) / cell,
                  ((long long)Wr + cell - 1) / cell);
        return TOAD_ESHAPE;
    }
    const int Hi = Ho * down, Wi = Wo * down;
    const int rb = thumb ? strip_rows(down) : 16;
    const int64_t nchunks = ((int64_t)Wi + 255) / 256, blocks = nchunks * (((int64_t)Hi + rb - 1) / rb);
    if (int rc = check_blocks(what, "region", blocks)) return rc;
    if (!aligned4(cells)) { set_error("%s: cells (int32 [Gy][Gx]) must be 4-byte aligned (%s may have any alignment)", what, unaligned); return TOAD_EALIGN; }
    if (Ho == 0 || Wo == 0) return TOAD_OK;
    int shift = 2;
    while ((1 << shift) < cell) ++shift;
    // the tent's variant: none; one quadrant per lane (cell >= 8); cell == 4, where at down == 4 a canvas pixel is a whole cell and the tent is the own value
    const int sm = !smooth || cell == down ? 0 : cell == 4 ? 2 : 1;
    const HeatPxArgs a = {region, pitch, Hi, Wi, cells, Gy, Gx, shift, alpha, mask, mask_pitch, Hm, Wm, mshift, mask_thresh, out, out_pitch, (unsigned)nchunks,
                          wx, wy};
    if (thumb) {                                                     // cell == down: the tent is the own value, its four loads are not needed
        const int tent = smooth && cell != down;
#define TOAD_THUMB(D, W) \
    case 2 * D + W: hipLaunchKernelGGL((heat_thumb_kernel<D, W != 0>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, tent, lut); break;
        switch (2 * down + (window ? 1 : 0)) { TOAD_THUMB(8, 0) TOAD_THUMB(16, 0) TOAD_THUMB(32, 0) TOAD_THUMB(8, 1) TOAD_THUMB(16, 1) TOAD_THUMB(32, 1) }
#undef TOAD_THUMB
        return check_launch(what);
    }
#define TOAD_HEAT(D, S, M) \
    case 8 * D + 2 * S + M: hipLaunchKernelGGL((heat_blend_px_kernel<D, S, M != 0>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, lut); break;
    switch (8 * down + 2 * sm + (mask ? 1 : 0)) {                    // <D, 0, 0> is the flat canvas; variant 2 does not occur at down == 4 (cell == down)
        TOAD_HEAT(1, 0, 0) TOAD_HEAT(1, 0, 1) TOAD_HEAT(1, 1, 0) TOAD_HEAT(1, 1, 1) TOAD_HEAT(1, 2, 0) TOAD_HEAT(1, 2, 1)
        TOAD_HEAT(2, 0, 0) TOAD_HEAT(2, 0, 1) TOAD_HEAT(2, 1, 0) TOAD_HEAT(2, 1, 1) TOAD_HEAT(2, 2, 0) TOAD_HEAT(2, 2, 1)
        TOAD_HEAT(4, 0, 0) TOAD_HEAT(4, 0, 1) TOAD_HEAT(4, 1, 0) TOAD_HEAT(4, 1, 1)
    }
#undef TOAD_HEAT
    return check_launch(what);
}

extern "C" int toad_region_heat_blend_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                                         const unsigned char *lut, int alpha, int down, unsigned char *out, int64_t out_pitch, void *stream) {
    return launch_heat_blend("toad_region_heat_blend_u8", "the region and the canvas", false, false, region, pitch, Hr, Wr, 0, 0, cells, Gy, Gx, cell, lut, alpha, down, 0, nullptr, 0, 0,
                             0, 0, 0, out, out_pitch, stream);
}

extern "C" int toad_region_heat_blend_px_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                                            const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch,
                                            int Hm, int Wm, int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream) {
    return launch_heat_blend("toad_region_heat_blend_px_u8", "the region, the mask and the canvas", false, false, region, pitch, Hr, Wr, 0, 0, cells, Gy, Gx, cell, lut, alpha, down,
                             smooth, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, out, out_pitch, stream);
}

extern "C" int toad_region_heat_thumb_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *cells, int Gy, int Gx, int cell,
                                         const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch,
                                         int Hm, int Wm, int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream) {
    return launch_heat_blend("toad_region_heat_thumb_u8", "the region, the mask and the canvas", true, false, region, pitch, Hr, Wr, 0, 0, cells, Gy, Gx, cell, lut, alpha, down,
                             smooth, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, out, out_pitch, stream);
}

extern "C" int toad_region_heat_window_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int wx, int wy, const int *cells, int Gy, int Gx, int cell,
                                          const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch,
                                          int Hm, int Wm, int mask_down, int mask_thresh, unsigned char *out, int64_t out_pitch, void *stream) {
    return launch_heat_blend("toad_region_heat_window_u8", "the region, the mask and the canvas", false, true, region, pitch, Hr, Wr, wx, wy, cells, Gy, Gx, cell, lut,
                             alpha, down, smooth, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, out, out_pitch, stream);
}

// The list entry: the window entry's checks of what the windows share, in its order; then window by window its checks of what each window has of its own,
// in its order, the first failing window winning under "window k:"; then the workgroup count of the whole list and the alignment of cells, where the
// window entry has them. Nothing is launched before all of that has passed. Two walks over the host array, no allocation: the first checks and counts,
// the second fills HEAT_LIST_MAX descriptors at a time and launches them. window(k) gives descriptor k of the caller's host array as a ToadHeatWindow, so that
// the pyramid list entry with ONE level is this very call; `vacant`: a window without a canvas pixel may come without a canvas address and pitch (that entry's
// rule, since such a level has no canvas; the windows entry checks an empty window like any other).
template <class Window>
static int launch_heat_windows(const char *what, bool vacant, Window window, bool have_windows, int n, const int *cells, int Gy, int Gx, int cell,
                               const unsigned char *lut, int alpha, int down, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down,
                               int mask_thresh, void *stream) {
    if (n < 0) { set_error("%s: n = %d windows", what, n); return TOAD_EINVAL; }
    if (!cells || !lut || (n > 0 && !have_windows)) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_heat_alpha(what, alpha)) return rc;
    if (int rc = check_heat_window_down(what, down, cell)) return rc;
    if (int rc = check_heat_smooth(what, smooth)) return rc;
    int mshift = 0;
    if (int rc = check_heat_mask(what, true, down, 0, 0, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, mshift)) return rc;
    const bool thumb = down >= 8;
    const int rb = thumb ? strip_rows(down) : 16;
    // a window's workgroups: 0 where it has no canvas pixel
    auto geometry = [&](const ToadHeatWindow &w, int &Hi, int &Wi, int64_t &nchunks) {
        Hi = w.Hr / down * down; Wi = w.Wr / down * down;
        nchunks = ((int64_t)Wi + 255) / 256;
        return nchunks * (((int64_t)Hi + rb - 1) / rb);
    };
    int64_t blocks = 0;
    int dshift = 0;
    while ((1 << dshift) < down) ++dshift;
    for (int k = 0; k < n; ++k) {
        const ToadHeatWindow w = window(k);
        char who[80];
        snprintf(who, sizeof who, "window %d: %s", k, what);
        const bool canvas = !vacant || ((w.Hr >> dshift) != 0 && (w.Wr >> dshift) != 0);
        if (!w.region || (canvas && !w.out)) { set_error("%s: null pointer", who); return TOAD_EINVAL; }
        if (int rc = check_hw(who, "Hr", w.Hr, "Wr", w.Wr)) return rc;
        if (int rc = check_heat_place(who, true, down, w.wx, w.wy, w.Wr)) return rc;
        if (int rc = check_region_pitch(who, w.pitch, w.Wr)) return rc;
        if (canvas)
            if (int rc = check_heat_out_pitch(who, w.out_pitch, w.Wr / down)) return rc;
        if (int rc = check_heat_table_holds(who, w.wx, w.wy, w.Hr, w.Wr, cell, Gy, Gx)) return rc;
        int Hi, Wi;
        int64_t nchunks;
        blocks += geometry(w, Hi, Wi, nchunks);                      // one window: below 2^50; the sum is refused as soon as it reaches 2^31
        if (int rc = check_blocks(what, "list of regions", blocks)) return rc;
    }
    if (!aligned4(cells)) {
        set_error("%s: cells (int32 [Gy][Gx]) must be 4-byte aligned (the regions, the mask and the canvases may have any alignment)", what);
        return TOAD_EALIGN;
    }
    if (blocks == 0) return TOAD_OK;
    int shift = 2;
    while ((1 << shift) < cell) ++shift;
    const int sm = !smooth || cell == down ? 0 : cell == 4 ? 2 : 1;  // the tent's variant, as in launch_heat_blend
    const int tent = smooth && cell != down;
    HeatListArgs l = {};
    l.shared = {nullptr, 0, 0, 0, cells, Gy, Gx, shift, alpha, mask, mask_pitch, Hm, Wm, mshift, mask_thresh, nullptr, 0, 0u, 0, 0};
    for (int k = 0; k < n;) {
        int m = 0;
        unsigned grid = 0;
        for (; k < n && m < HEAT_LIST_MAX; ++k) {
            const ToadHeatWindow w = window(k);
            int Hi, Wi;
            int64_t nchunks;
            const int64_t b = geometry(w, Hi, Wi, nchunks);
            if (b == 0) continue;
            l.w[m++] = {w.region, w.pitch, w.out, w.out_pitch, Hi, Wi, w.wx, w.wy, (unsigned)nchunks, grid};
            grid += (unsigned)b;
        }
        if (m == 0) break;
        for (int j = m; j < HEAT_LIST_MAX; ++j) { l.w[j] = {}; l.w[j].first = 0xFFFFFFFFu; }      // above every workgroup index: the search stops short of them
        if (thumb) {
#define TOAD_THUMB_LIST(D) case D: hipLaunchKernelGGL((heat_thumb_list_kernel<D>), dim3(grid), dim3(256), 0, (hipStream_t)stream, l, tent, lut); break;
            switch (down) { TOAD_THUMB_LIST(8) TOAD_THUMB_LIST(16) TOAD_THUMB_LIST(32) }
#undef TOAD_THUMB_LIST
        } else {
#define TOAD_HEAT_LIST(D, S, M) \
    case 8 * D + 2 * S + M: hipLaunchKernelGGL((heat_blend_px_list_kernel<D, S, M != 0>), dim3(grid), dim3(256), 0, (hipStream_t)stream, l, lut); break;
            switch (8 * down + 2 * sm + (mask ? 1 : 0)) {            // the 16 shapes of launch_heat_blend
                TOAD_HEAT_LIST(1, 0, 0) TOAD_HEAT_LIST(1, 0, 1) TOAD_HEAT_LIST(1, 1, 0) TOAD_HEAT_LIST(1, 1, 1) TOAD_HEAT_LIST(1, 2, 0) TOAD_HEAT_LIST(1, 2, 1)
                TOAD_HEAT_LIST(2, 0, 0) TOAD_HEAT_LIST(2, 0, 1) TOAD_HEAT_LIST(2, 1, 0) TOAD_HEAT_LIST(2, 1, 1) TOAD_HEAT_LIST(2, 2, 0) TOAD_HEAT_LIST(2, 2, 1)
                TOAD_HEAT_LIST(4, 0, 0) TOAD_HEAT_LIST(4, 0, 1) TOAD_HEAT_LIST(4, 1, 0) TOAD_HEAT_LIST(4, 1, 1)
            }
#undef TOAD_HEAT_LIST
        }
        if (int rc = check_launch(what)) return rc;
    }
    return TOAD_OK;
}

extern "C" int toad_region_heat_windows_u8(const ToadHeatWindow *windows, int n, const int *cells, int Gy, int Gx, int cell, const unsigned char *lut, int alpha,
                                           int down, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down, int mask_thresh,
                                           void *stream) {
    return launch_heat_windows("toad_region_heat_windows_u8", false, [&](int k) { return windows[k]; }, windows != nullptr, n, cells, Gy, Gx, cell, lut, alpha, down,
                               smooth, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, stream);
}

// The checks of a set of levels that the pyramid entry and its list form both make, each with the one message. kmax = log2 of D, the largest level.
static int check_heat_levels(const char *what, unsigned levels, int cell, int &kmax, int &nlev) {
    if (levels == 0 || levels > 63u) {
        set_error("%s: levels = 0x%x is not a non-empty set of bits 0 .. 5 (bit k asks for down = 2^k, down in 1 .. 32)", what, levels);
        return TOAD_ESHAPE;
    }
    kmax = 0; nlev = 0;
    for (int k = 0; k < 6; ++k)
        if (levels >> k & 1u) { kmax = k; ++nlev; }
    if ((1 << kmax) >= 8 && (1 << kmax) > cell) {
        set_error("%s: down = %d, the largest level, exceeds cell = %d (a canvas box must lie in one cell)", what, 1 << kmax, cell);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}
static int check_heat_pyr_place(const char *what, int D, int wx, int wy, int Wr) {
    const int walign = D > 4 ? D : 4;
    if (wx < 0 || wy < 0 || wx % walign || wy % walign) {
        set_error("%s: window (wx, wy) = (%d, %d) is negative or not a multiple of max(4, down) = %d, down the largest level (a lane's 4 x 4 block and a "
                  "canvas box must lie in one cell and in one mask pixel)", what, wx, wy, walign);
        return TOAD_ESHAPE;
    }
    if ((int64_t)wx + Wr >= (1ll << 30)) {
        set_error("%s: window too far right: wx + Wr = %lld must stay below 2^30 (doubled tent coordinates in 32 bits)", what, (long long)wx + Wr);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}
static int check_heat_pyr_smooth(const char *what, int smooth, int cell) {     // two or more levels
    if (smooth != 0 && smooth != 1) { set_error("%s: smooth = %d must be 0 or 1", what, smooth); return TOAD_EINVAL; }
    if (smooth && cell == 4) {
        set_error("%s: smooth at cell = 4 is not done for more than one level (the nine-neighbour tent: render those levels one by one)", what);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}
static int check_heat_pyr_mask(const char *what, int D, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm, int mask_down, int mask_thresh, int &mshift) {
    mshift = 0;
    if (!mask) return TOAD_OK;
    if (mask_down != 1 && mask_down != 2 && mask_down != 4 && mask_down != 8 && mask_down != 16 && mask_down != 32) {
        set_error("%s: mask_down = %d is not one of 1, 2, 4, 8, 16, 32", what, mask_down);
        return TOAD_ESHAPE;
    }
    if (mask_down % D) {
        set_error("%s: mask_down = %d is not a multiple of down = %d, the largest level (a canvas box must lie in one mask pixel)", what, mask_down, D);
        return TOAD_ESHAPE;
    }
    if (Hm < 0 || Wm < 0) { set_error("%s: Hm x Wm = %d x %d must not be negative", what, Hm, Wm); return TOAD_ESHAPE; }
    if (int rc = check_plane_pitch(what, Wm, "mask_pitch", mask_pitch)) return rc;
    if (int rc = check_u8(what, "mask_thresh", mask_thresh)) return rc;
    while ((1 << mshift) < mask_down) ++mshift;
    return TOAD_OK;
}
static int check_heat_pyr_out_pitch(const char *what, int k, int64_t out_pitch, int Wr) {
    if (out_pitch >= 3 * (int64_t)(Wr >> k)) return TOAD_OK;
    set_error("%s: out_pitches[%d] = %lld is less than a row of the canvas of down = %d (3 Wo = %lld bytes)", what, k, (long long)out_pitch, 1 << k, 3ll * (Wr >> k));
    return TOAD_ESHAPE;
}

// The pyramid entry: the window entry's checks in the window entry's order, taken over the set of levels - D, the largest, stands where `down` stood, and the
// checks of the set and of its canvases where the down check sat. One level is the window entry itself; two or more are ONE launch of heat_pyramid_kernel.
extern "C" int toad_region_heat_pyramid_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int wx, int wy, const int *cells, int Gy, int Gx, int cell,
                                           const unsigned char *lut, int alpha, unsigned levels, int smooth, const unsigned char *mask, int64_t mask_pitch,
                                           int Hm, int Wm, int mask_down, int mask_thresh, unsigned char *const *outs, const int64_t *out_pitches, void *stream) {
    const char *what = "toad_region_heat_pyramid_u8";
    if (!region || !cells || !lut || !outs || !out_pitches) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_hw(what, "Hr", Hr, "Wr", Wr)) return rc;
    if (alpha < 0 || alpha > 256) { set_error("%s: alpha = %d must lie in [0, 256] (256 = the colour alone)", what, alpha); return TOAD_ESHAPE; }
    int kmax = 0, nlev = 0;
    if (int rc = check_heat_levels(what, levels, cell, kmax, nlev)) return rc;
    const int D = 1 << kmax;
    for (int k = 0; k < 6; ++k)
        if ((levels >> k & 1u) && !outs[k]) { set_error("%s: null pointer (outs[%d], the canvas of down = %d)", what, k, 1 << k); return TOAD_EINVAL; }
    if (nlev == 1)                                                   // the same kernel, the same bytes, the same time
        return launch_heat_blend(what, "the region, the mask and the canvases", false, true, region, pitch, Hr, Wr, wx, wy, cells, Gy, Gx, cell, lut, alpha, D, smooth,
                                 mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, outs[kmax], out_pitches[kmax], stream);
    if (int rc = check_heat_pyr_place(what, D, wx, wy, Wr)) return rc;
    if (int rc = check_heat_pyr_smooth(what, smooth, cell)) return rc;
    if (int rc = check_region_pitch(what, pitch, Wr)) return rc;
    int mshift = 0;
    if (int rc = check_heat_pyr_mask(what, D, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, mshift)) return rc;
    for (int k = 0; k < 6; ++k)
        if (levels >> k & 1u)
            if (int rc = check_heat_pyr_out_pitch(what, k, out_pitches[k], Wr)) return rc;
    if (int rc = check_heat_table_holds(what, wx, wy, Hr, Wr, cell, Gy, Gx)) return rc;
    const int rb = strip_rows(D);
    const int64_t nchunks = ((int64_t)Wr + 255) / 256, blocks = nchunks * (((int64_t)Hr + rb - 1) / rb);
    if (int rc = check_blocks(what, "region", blocks)) return rc;
    if (!aligned4(cells)) {
        set_error("%s: cells (int32 [Gy][Gx]) must be 4-byte aligned (the region, the mask and the canvases may have any alignment)", what);
        return TOAD_EALIGN;
    }
    int shift = 2;
    while ((1 << shift) < cell) ++shift;
    HeatPyrArgs p = {};
    p.a = {region, pitch, Hr, Wr, cells, Gy, Gx, shift, alpha, mask, mask_pitch, Hm, Wm, mshift, mask_thresh, nullptr, 0, (unsigned)nchunks, wx, wy};
    p.smooth = smooth;
    for (int k = 0; k < 6; ++k) {
        const int Ho = Hr >> k, Wo = Wr >> k;
        if (!(levels >> k & 1u) || Ho == 0 || Wo == 0) continue;     // an empty level writes nothing; the others are still rendered
        p.levels |= 1u << k;
        p.out[k] = outs[k]; p.pitch[k] = out_pitches[k]; p.Ho[k] = Ho; p.Wo[k] = Wo;
    }
    if (p.levels == 0) return TOAD_OK;
#define TOAD_PYR(R, M) hipLaunchKernelGGL((heat_pyramid_kernel<R, M>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, lut)
    if (rb == 32) { if (mask) TOAD_PYR(32, true); else TOAD_PYR(32, false); }
    else { if (mask) TOAD_PYR(16, true); else TOAD_PYR(16, false); }
#undef TOAD_PYR
    return check_launch(what);
}

// The pyramid list entry: the list entry's walk over the pyramid entry's checks. What the windows share first, in the pyramid entry's order and with its
// messages; then window by window what each has of its own, the first failing window winning under "window k:"; then the workgroup count of the whole list
// and the alignment of cells. A level that is empty for a window has no canvas there: neither its address nor its pitch is looked at. One level is the list
// entry itself; two or more are one launch of heat_pyramid_list_kernel per HEAT_PYR_LIST_MAX windows that have a canvas pixel. Two walks, no allocation.
extern "C" int toad_region_heat_pyramid_windows_u8(const ToadHeatPyramidWindow *windows, int n, const int *cells, int Gy, int Gx, int cell, const unsigned char *lut,
                                                   int alpha, unsigned levels, int smooth, const unsigned char *mask, int64_t mask_pitch, int Hm, int Wm,
                                                   int mask_down, int mask_thresh, void *stream) {
    const char *what = "toad_region_heat_pyramid_windows_u8";
    if (n < 0) { set_error("%s: n = %d windows", what, n); return TOAD_EINVAL; }
    if (!cells || !lut || (n > 0 && !windows)) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_heat_alpha(what, alpha)) return rc;
    int kmax = 0, nlev = 0;
    if (int rc = check_heat_levels(what, levels, cell, kmax, nlev)) return rc;
    const int D = 1 << kmax;
    if (nlev == 1) {                                                 // the same kernels, the same bytes; its shared checks are the window entry's, as the pyramid entry's are
        auto window = [&](int k) {
            const ToadHeatPyramidWindow &w = windows[k];
            return ToadHeatWindow{w.region, w.pitch, w.Hr, w.Wr, w.wx, w.wy, w.outs[kmax], w.out_pitches[kmax]};
        };
        return launch_heat_windows(what, true, window, windows != nullptr, n, cells, Gy, Gx, cell, lut, alpha, D, smooth, mask, mask_pitch, Hm, Wm, mask_down,
                                   mask_thresh, stream);
    }
    if (int rc = check_heat_pyr_smooth(what, smooth, cell)) return rc;
    int mshift = 0;
    if (int rc = check_heat_pyr_mask(what, D, mask, mask_pitch, Hm, Wm, mask_down, mask_thresh, mshift)) return rc;
    const int rb = strip_rows(D);
    // the levels window w has a canvas pixel at, and its workgroups: 0 where it has none
    auto geometry = [&](const ToadHeatPyramidWindow &w, unsigned &has, int64_t &nchunks) {
        has = 0;
        for (int j = 0; j < 6; ++j)
            if ((levels >> j & 1u) && (w.Hr >> j) != 0 && (w.Wr >> j) != 0) has |= 1u << j;
        nchunks = ((int64_t)w.Wr + 255) / 256;
        return has ? nchunks * (((int64_t)w.Hr + rb - 1) / rb) : (int64_t)0;
    };
    int64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        const ToadHeatPyramidWindow &w = windows[k];
        char who[80];
        snprintf(who, sizeof who, "window %d: %s", k, what);
        unsigned has;
        int64_t nchunks;
        if (!w.region) { set_error("%s: null pointer", who); return TOAD_EINVAL; }
        geometry(w, has, nchunks);
        for (int j = 0; j < 6; ++j)
            if ((has >> j & 1u) && !w.outs[j]) { set_error("%s: null pointer (outs[%d], the canvas of down = %d)", who, j, 1 << j); return TOAD_EINVAL; }
        if (int rc = check_hw(who, "Hr", w.Hr, "Wr", w.Wr)) return rc;
        if (int rc = check_heat_pyr_place(who, D, w.wx, w.wy, w.Wr)) return rc;
        if (int rc = check_region_pitch(who, w.pitch, w.Wr)) return rc;
        for (int j = 0; j < 6; ++j)
            if (has >> j & 1u)
                if (int rc = check_heat_pyr_out_pitch(who, j, w.out_pitches[j], w.Wr)) return rc;
        if (int rc = check_heat_table_holds(who, w.wx, w.wy, w.Hr, w.Wr, cell, Gy, Gx)) return rc;
        blocks += geometry(w, has, nchunks);                         // one window: below 2^50; the sum is refused as soon as it reaches 2^31
        if (int rc = check_blocks(what, "list of regions", blocks)) return rc;
    }
    if (!aligned4(cells)) {
        set_error("%s: cells (int32 [Gy][Gx]) must be 4-byte aligned (the regions, the mask and the canvases may have any alignment)", what);
        return TOAD_EALIGN;
    }
    if (blocks == 0) return TOAD_OK;
    int shift = 2;
    while ((1 << shift) < cell) ++shift;
    HeatPyrListArgs l = {};
    l.shared = {nullptr, 0, 0, 0, cells, Gy, Gx, shift, alpha, mask, mask_pitch, Hm, Wm, mshift, mask_thresh, nullptr, 0, 0u, 0, 0};
    l.levels = levels; l.smooth = smooth;
    for (int k = 0; k < n;) {
        int m = 0;
        unsigned grid = 0;
        for (; k < n && m < HEAT_PYR_LIST_MAX; ++k) {
            const ToadHeatPyramidWindow &w = windows[k];
            unsigned has;
            int64_t nchunks;
            const int64_t b = geometry(w, has, nchunks);
            if (b == 0) continue;
            HeatPyrListWin &d = l.w[m++];
            d = {};
            d.region = w.region; d.pitch = w.pitch; d.Hr = w.Hr; d.Wr = w.Wr; d.wx = w.wx; d.wy = w.wy; d.nchunks = (unsigned)nchunks; d.first = grid;
            for (int j = 0; j < 6; ++j)
                if (has >> j & 1u) { d.out[j] = w.outs[j]; d.out_pitch[j] = w.out_pitches[j]; }
            grid += (unsigned)b;
        }
        if (m == 0) break;
        for (int j = m; j < HEAT_PYR_LIST_MAX; ++j) { l.w[j] = {}; l.w[j].first = 0xFFFFFFFFu; }      // above every workgroup index: the search stops short of them
#define TOAD_PYR_LIST(R, M) hipLaunchKernelGGL((heat_pyramid_list_kernel<R, M>), dim3(grid), dim3(256), 0, (hipStream_t)stream, l, lut)
        if (rb == 32) { if (mask) TOAD_PYR_LIST(32, true); else TOAD_PYR_LIST(32, false); }
        else { if (mask) TOAD_PYR_LIST(16, true); else TOAD_PYR_LIST(16, false); }
#undef TOAD_PYR_LIST
        if (int rc = check_launch(what)) return rc;
    }
    return TOAD_OK;
}
