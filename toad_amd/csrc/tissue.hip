// tissue.hip — which tiles of a decoded uint8 region hold tissue: the stage in front of the tiles-by-origin calls (include/toad_hip.h, "tissue selection").
//
// The pixel predicate, integers only, no rounding anywhere: with mx = max(r, g, b) and mn = min(r, g, b),
//     tissue(r, g, b)  <=>  mx >= val_min  and  255 (mx - mn) > sat_thresh mx.
// That is "HSV saturation (mx - mn) / mx above sat_thresh on the 8-bit scale" written without the division. It is NOT OpenCV's rounded S channel
// (round(255 (mx - mn) / mx) > sat_thresh): the two differ where the quotient rounds up across the threshold. mx == 0 is never tissue (0 > 0 is false);
// val_min removes black scanner margins, whose JPEG noise - (1, 0, 0) - is fully "saturated".
//
// Two kernels:
//   tissue_cells_kernel<CELL>   one streaming pass over the region -> int32 counts [Gy][Gx], the tissue pixels of every CELL x CELL cell of the partition
//                               anchored at the region's (0, 0); Gy = ceil(Hr / CELL), Gx = ceil(Wr / CELL). Partial cells at the right and the bottom
//                               edge count the pixels that exist.
//   tissue_tile_counts_kernel   one thread per tile of a lattice whose origin, tile shape and strides are multiples of the cell: the tile is an exact
//                               union of whole cells, and its count the sum of theirs. Strides below the tile size (heat-map lattices) re-read cells.
// Why cells and not one kernel per lattice: the region pass is the 100 MB one and does not depend on the lattice, the tile sums read a table 3 CELL^2 times
// smaller (74 KB for a 4096 x 8192 region at CELL = 64), and overlapping tiles cost nothing extra in the pass over the pixels.
#include "common.h"

namespace toad {

// the region form's words (stem_halo.inc declares the same types for its own loads): a dword from any byte address - base, pitch and 3 x have any parity
typedef unsigned ts_u32_a1 __attribute__((aligned(1)));

// 255 (mx - mn) > sat mx  <=>  (255 - sat) mx - 255 mn - 1 >= 0, an exact rearrangement in integers; with mx - vmin >= 0 that is "the OR of the two
// differences has its sign bit clear". All products are below 2^16: 24-bit multiplies (the full-rate ones).
__device__ __forceinline__ int tissue_px(int r, int g, int b, int sat, int vmin) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    return (int)((((__mul24(mx, 255 - sat) - 1 - __mul24(mn, 255)) | (mx - vmin)) >= 0));
}

// the 12 bytes of 4 pixels as three little-endian dwords: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
__device__ __forceinline__ int tissue_px4(unsigned w0, unsigned w1, unsigned w2, int sat, int vmin) {
    return tissue_px(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, sat, vmin) + tissue_px(w0 >> 24, w1 & 255, (w1 >> 8) & 255, sat, vmin) +
           tissue_px((w1 >> 16) & 255, w1 >> 24, w2 & 255, sat, vmin) + tissue_px((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24, sat, vmin);
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
// every lane of each aligned group of LANES lanes (1, 2, 4, 8, 16: inside a 16-lane DPP row) ends with the group's sum; all 64 lanes must be active
template <int LANES>
__device__ __forceinline__ int lanes_allreduce_sum(int v) {
    if constexpr (LANES >= 2) v += dpp_mov_i<0xB1>(v);    // quad_perm [1,0,3,2]
    if constexpr (LANES >= 4) v += dpp_mov_i<0x4E>(v);    // quad_perm [2,3,0,1]
    if constexpr (LANES >= 8) v += dpp_mov_i<0x141>(v);   // row_half_mirror
    if constexpr (LANES >= 16) v += dpp_mov_i<0x140>(v);  // row_mirror
    return v;
}

// Work split. Lanes run along x: a lane takes 4 pixels = 12 contiguous bytes as three dwords, a wave 256 pixels = 768 contiguous bytes of one row, so a
// cell is CELL / 4 adjacent lanes. A workgroup of 4 waves takes one 256-pixel column chunk of RB = max(CELL, 16) rows, RB / 4 consecutive rows per wave
// (4, 4, 4, 8, 16 rows for CELL = 4 .. 64): the row loop is unrolled, so a wave has 12 to 48 dwords per lane in flight, and the grid - one workgroup per
// (row block, chunk), chunks adjacent - is 8,192 workgroups (CELL <= 16) or 4,096 / 2,048 (CELL = 32 / 64) on a 4096 x 8192 region. Per-lane counts stay in
// a register over the rows; the CELL / 4 lanes of a cell are summed by DPP moves; the up to 4 waves that share a band meet in 1 KB of LDS, and one lane per
// cell stores its count with a plain store. Every element of counts is written by exactly one lane of one workgroup: nothing is zeroed, nothing is atomic.
//
// Addresses: the row base y pitch is a 64-bit scalar, the in-row byte offset chunk 768 + lane 12 is 32-bit (the launcher refuses 3 Wr >= 2^31). No byte
// outside y pitch + [0, 3 Wr), y in [0, Hr), is read: a wave whose 768 bytes end inside the row, over rows that all exist, runs the plain path; any other
// wave loops over the rows that exist, and per lane takes the three dwords only where offset + 12 <= 3 Wr, byte loads for the 1 to 3 pixels of the lane
// the row ends in, and nothing beyond (the last row of a pitched view may be the end of its allocation).
template <int CELL>
__global__ __launch_bounds__(256) void tissue_cells_kernel(const unsigned char *__restrict__ region, int64_t pitch, int Hr, int Wr, int sat, int vmin,
                                                           int *__restrict__ counts, int Gy, int Gx, unsigned nchunks) {
    constexpr int RB = CELL > 16 ? CELL : 16, RW = RB / 4;          // rows per workgroup, per wave
    constexpr int NB = RB / CELL, WPB = 4 / NB;                    // bands per workgroup, waves per band
    constexpr int LANES = CELL / 4, CPR = 64 / LANES;              // lanes per cell, cells per chunk
    __shared__ int part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned chunk = blockIdx.x % nchunks, rb = blockIdx.x / nchunks;
    const unsigned row_bytes = 3u * (unsigned)Wr, off = chunk * 768u + (unsigned)lane * 12u;
    const int64_t y0 = (int64_t)rb * RB + wave * RW;               // first row of this wave (may lie below the region: then it counts nothing)
    const unsigned char *base = region + y0 * pitch;
    int cnt = 0;
    if (chunk * 768u + 768u <= row_bytes && y0 + RW <= Hr) {       // wave-uniform: all 768 bytes of all RW rows exist
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const unsigned char *p = base + r * pitch + off;
            cnt += tissue_px4(*reinterpret_cast<const ts_u32_a1 *>(p), *reinterpret_cast<const ts_u32_a1 *>(p + 4), *reinterpret_cast<const ts_u32_a1 *>(p + 8),
                              sat, vmin);
        }
    } else {
        const int rows = (int)min((int64_t)RW, (int64_t)Hr - y0);  // <= 0 below the region
        for (int r = 0; r < rows; ++r) {
            const unsigned char *p = base + r * pitch + off;
            if (off + 12u <= row_bytes) {
                cnt += tissue_px4(*reinterpret_cast<const ts_u32_a1 *>(p), *reinterpret_cast<const ts_u32_a1 *>(p + 4),
                                  *reinterpret_cast<const ts_u32_a1 *>(p + 8), sat, vmin);
            } else if (off < row_bytes) {                          // the lane the row ends in: 1, 2 or 3 whole pixels, byte by byte
                const int npx = (int)(row_bytes - off) / 3;
                for (int k = 0; k < npx; ++k) cnt += tissue_px(p[3 * k], p[3 * k + 1], p[3 * k + 2], sat, vmin);
            }
        }
    }
    cnt = lanes_allreduce_sum<LANES>(cnt);
    part[wave][lane] = cnt;
    __syncthreads();
    if (tid < NB * CPR) {
        const int band = tid / CPR, c = tid - band * CPR;
        int s = 0;
#pragma unroll
        for (int k = 0; k < WPB; ++k) s += part[band * WPB + k][c * LANES];
        const int64_t gy = (int64_t)rb * NB + band;
        const unsigned gx = chunk * CPR + c;
        if (gy < Gy && gx < (unsigned)Gx) counts[gy * Gx + gx] = s;
    }
}

// All lattice arguments in CELL units. One thread per tile (j, i), row-major; the cell table is small and cached, so the strided reads of neighbouring
// threads are not worth a smarter layout (a 16 x 32 lattice of 256 x 256 tiles at CELL = 64 reads 8,192 ints).
__global__ __launch_bounds__(256) void tissue_tile_counts_kernel(const int *__restrict__ counts, int Gx, int cx0, int cy0, int ch, int cw, int csx, int csy,
                                                                 int nx, int ny, int *__restrict__ tile_counts) {
    const uint64_t total = (uint64_t)nx * ny;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const int64_t j = (int64_t)(t / (unsigned)nx), i = (int64_t)(t - (uint64_t)j * nx);
        const int *p = counts + (cy0 + j * csy) * Gx + cx0 + i * csx;
        int s = 0;
        for (int a = 0; a < ch; ++a)
            for (int b = 0; b < cw; ++b) s += p[(int64_t)a * Gx + b];
        tile_counts[t] = s;
    }
}

static bool cell_ok(int cell) { return cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64; }
static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace toad

using namespace toad;

extern "C" int toad_region_tissue_cells_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int cell, int sat_thresh, int val_min, int *counts,
                                           void *stream) {
    const char *what = "toad_region_tissue_cells_u8";
    if (!region || !counts) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (sat_thresh < 0 || sat_thresh > 255 || val_min < 0 || val_min > 255) {
        set_error("%s: sat_thresh = %d and val_min = %d must lie in [0, 255] (the 8-bit scale)", what, sat_thresh, val_min);
        return TOAD_EINVAL;
    }
    if (!cell_ok(cell)) { set_error("%s: cell = %d is not one of 4, 8, 16, 32, 64", what, cell); return TOAD_ESHAPE; }
    if (Hr <= 0 || Wr <= 0) { set_error("%s: bad shape (Hr = %d, Wr = %d)", what, Hr, Wr); return TOAD_ESHAPE; }
    if (pitch < 3 * (int64_t)Wr) { set_error("%s: pitch %lld is less than a row of the region (3 Wr = %lld bytes)", what, (long long)pitch, 3ll * Wr); return TOAD_ESHAPE; }
    if (3 * (int64_t)Wr >= (1ll << 31)) { set_error("%s: region too wide: 3 Wr must stay below 2^31 (32-bit offsets inside a row)", what); return TOAD_ESHAPE; }
    const int rb = cell > 16 ? cell : 16;
    const int64_t nchunks = ((int64_t)Wr + 255) / 256, blocks = nchunks * (((int64_t)Hr + rb - 1) / rb);
    if (blocks >= (1ll << 31)) { set_error("%s: region too large: %lld workgroups", what, (long long)blocks); return TOAD_ESHAPE; }
    if (!aligned4(counts)) { set_error("%s: counts (int32 [Gy][Gx]) must be 4-byte aligned (the region may have any alignment)", what); return TOAD_EALIGN; }
    const int Gy = (int)(((int64_t)Hr + cell - 1) / cell), Gx = (int)(((int64_t)Wr + cell - 1) / cell);
    hipStream_t st = (hipStream_t)stream;
#define TOAD_TISSUE_LAUNCH(C) \
    hipLaunchKernelGGL(tissue_cells_kernel<C>, dim3((unsigned)blocks), dim3(256), 0, st, region, pitch, Hr, Wr, sat_thresh, val_min, counts, Gy, Gx, (unsigned)nchunks)
    switch (cell) {
        case 4: TOAD_TISSUE_LAUNCH(4); break;
        case 8: TOAD_TISSUE_LAUNCH(8); break;
        case 16: TOAD_TISSUE_LAUNCH(16); break;
        case 32: TOAD_TISSUE_LAUNCH(32); break;
        default: TOAD_TISSUE_LAUNCH(64); break;
    }
#undef TOAD_TISSUE_LAUNCH
    return check_launch(what);
}

extern "C" int toad_tissue_tile_counts(const int *counts, int Gy, int Gx, int cell, int x0, int y0, int H, int W, int sx, int sy, int nx, int ny,
                                       int *tile_counts, void *stream) {
    const char *what = "toad_tissue_tile_counts";
    if (!counts || !tile_counts) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (!cell_ok(cell)) { set_error("%s: cell = %d is not one of 4, 8, 16, 32, 64", what, cell); return TOAD_ESHAPE; }
    if (Gy <= 0 || Gx <= 0 || nx <= 0 || ny <= 0 || H <= 0 || W <= 0 || sx <= 0 || sy <= 0) {
        set_error("%s: bad shape (Gy, Gx, nx, ny, H, W, sx, sy must all be positive)", what);
        return TOAD_ESHAPE;
    }
    const int vals[6] = {x0, y0, H, W, sx, sy};
    const char *names[6] = {"x0", "y0", "H", "W", "sx", "sy"};
    for (int k = 0; k < 6; ++k)
        if (vals[k] < 0 || vals[k] % cell) {
            set_error("%s: %s = %d is negative or not a multiple of cell = %d (a tile must be a union of whole cells)", what, names[k], vals[k], cell);
            return TOAD_ESHAPE;
        }
    if ((int64_t)H * W >= (1ll << 31)) { set_error("%s: bad shape: H * W must stay below 2^31 (int32 counts)", what); return TOAD_ESHAPE; }
    const int64_t x_end = x0 + (int64_t)(nx - 1) * sx + W, y_end = y0 + (int64_t)(ny - 1) * sy + H;
    if (x_end > (int64_t)Gx * cell || y_end > (int64_t)Gy * cell) {
        set_error("%s: the lattice's last tile ends at (x, y) = (%lld, %lld), outside the %d x %d cells of %d pixels (Gy x Gx)", what, (long long)x_end,
                  (long long)y_end, Gy, Gx, cell);
        return TOAD_ESHAPE;
    }
    if (!aligned4(counts) || !aligned4(tile_counts)) { set_error("%s: counts and tile_counts (int32) must be 4-byte aligned", what); return TOAD_EALIGN; }
    const uint64_t g = ((uint64_t)nx * ny + 255) / 256;
    hipLaunchKernelGGL(tissue_tile_counts_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, counts, Gx, x0 / cell, y0 / cell,
                       H / cell, W / cell, sx / cell, sy / cell, nx, ny, tile_counts);
    return check_launch(what);
}
