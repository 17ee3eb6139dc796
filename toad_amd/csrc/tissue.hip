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
#include "region_u8.h"

namespace toad {

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

// The work split, its addresses and the cell-count tail are region_u8.h's; what this kernel adds is the predicate. A wave off the plain path takes its
// rows through load_px4 and counts all 4 pixels of the lane, absent ones included: load_px4 gives them as zeros, and an all-zero pixel is never tissue,
// whatever sat and vmin are - tissue_px(0, 0, 0, ..) has -1 in its first term.
template <int CELL>
__global__ __launch_bounds__(256) void tissue_cells_kernel(const unsigned char *__restrict__ region, int64_t pitch, int Hr, int Wr, int sat, int vmin,
                                                           int *__restrict__ counts, int Gy, int Gx, unsigned nchunks) {
    constexpr int RB = CellStrip<CELL>::RB, RW = CellStrip<CELL>::RW;
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
            cnt += tissue_px4(*reinterpret_cast<const u32_a1 *>(p), *reinterpret_cast<const u32_a1 *>(p + 4), *reinterpret_cast<const u32_a1 *>(p + 8), sat, vmin);
        }
    } else {
        const int rows = (int)min((int64_t)RW, (int64_t)Hr - y0);  // <= 0 below the region
        const int npx = off < row_bytes ? min(4, (int)((row_bytes - off) / 3u)) : 0;       // pixels of this lane that exist
        for (int r = 0; r < rows; ++r) {
            unsigned w[3];
            load_px4(base + r * pitch + off, npx, w);
            cnt += tissue_px4(w[0], w[1], w[2], sat, vmin);
        }
    }
    store_cell_counts<CELL>(cnt, part, rb, chunk, counts, Gy, Gx);
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
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_hw(what, "Hr", Hr, "Wr", Wr)) return rc;
    if (int rc = check_region_pitch(what, pitch, Wr)) return rc;
    const int rb = strip_rows(cell);
    const int64_t nchunks = ((int64_t)Wr + 255) / 256, blocks = nchunks * (((int64_t)Hr + rb - 1) / rb);
    if (int rc = check_blocks(what, "region", blocks)) return rc;
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
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_lattice_units(what, cell, x0, y0, H, W, sx, sy, nx, ny, Gy, Gx)) return rc;
    if ((int64_t)H * W >= (1ll << 31)) { set_error("%s: bad shape: H * W must stay below 2^31 (int32 counts)", what); return TOAD_ESHAPE; }
    if (int rc = check_lattice_extent(what, cell, x0, y0, H, W, sx, sy, nx, ny, Gy, Gx)) return rc;
    if (!aligned4(counts) || !aligned4(tile_counts)) { set_error("%s: counts and tile_counts (int32) must be 4-byte aligned", what); return TOAD_EALIGN; }
    const uint64_t g = ((uint64_t)nx * ny + 255) / 256;
    hipLaunchKernelGGL(tissue_tile_counts_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, counts, Gx, x0 / cell, y0 / cell,
                       H / cell, W / cell, sx / cell, sy / cell, nx, ny, tile_counts);
    return check_launch(what);
}
