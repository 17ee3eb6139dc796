// region_u8.h — what the kernels over a decoded uint8 region and over its byte planes share (tissue.hip, tissue_seg.hip, tissue_morph.hip, heatmap.hip):
// the strip work split and its loads, the cell-count tail, and the launchers' argument checks. The unaligned word types, the integer DPP all-reduce and
// aligned4 are common.h's (stem_halo.inc uses the types too).
//
// Work split. Lanes run along x: a lane takes 4 pixels = 12 contiguous bytes as three dwords, a wave 256 pixels = 768 contiguous bytes of one row. A
// workgroup of 4 waves takes one 256-pixel column chunk of RB = strip_rows(n) = max(n, 16) rows (n the cell or the box size), RB / 4 consecutive rows per
// wave (4, 4, 4, 8, 16 rows for n = 4 .. 64): the row loop is unrolled, so a wave has 12 to 48 dwords per lane in flight, and the grid - one workgroup per
// (row block, chunk), chunks adjacent - is 8,192 workgroups (n <= 16) or 4,096 / 2,048 (n = 32 / 64) on a 4096 x 8192 region. A plane kernel is the same
// with one byte per pixel: a lane takes one dword.
//
// Addresses: the row base y pitch is a 64-bit scalar, the in-row byte offset chunk 768 + lane 12 is 32-bit (check_region_pitch refuses 3 Wr >= 2^31). No
// byte outside y pitch + [0, 3 W), y in [0, H), is read, H x W being the rows and columns the kernel consumes: a wave whose 768 bytes end inside the row,
// over rows that all exist, runs the plain path - unrolled dword loads, written out in each kernel; any other wave goes row by row over the rows that exist
// and takes each lane's pixels through load_px4, which touches nothing beyond the pixels it is told exist (the last row of a pitched view may be the end
// of its allocation). sat_plane_kernel alone has load_px4's body written out, for a measured reason given there.
#pragma once
#include "common.h"

namespace toad {

constexpr int strip_rows(int n) { return n > 16 ? n : 16; }         // RB: the rows of a workgroup's strip, for kernels and launchers alike

// npx of a lane's 4 pixels of a row exist, the 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 as three little-endian dwords: npx == 4 takes the three
// dwords, npx in 1 .. 3 (the lane the row ends in) 3 npx byte loads, and whatever does not exist is 0 (npx <= 0: all of it, and p is not touched).
__device__ __forceinline__ void load_px4(const unsigned char *p, int npx, unsigned (&w)[3]) {
    if (npx == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = *reinterpret_cast<const u32_a1 *>(p + 4 * k);
    } else {
        w[0] = w[1] = w[2] = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k < 3 * npx) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    }
}

// b[k] = the sum over ROWS rows of byte k of a lane's three dwords: the 12 column sums, two to a dword while they add up (ROWS * 255 < 2^16)
template <int ROWS>
__device__ __forceinline__ void column_sums(const unsigned (&w)[ROWS][3], unsigned (&b)[12]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsigned ev = 0, od = 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { ev += w[r][k] & 0x00FF00FFu; od += (w[r][k] >> 8) & 0x00FF00FFu; }
        b[4 * k] = ev & 0xFFFFu; b[4 * k + 1] = od & 0xFFFFu; b[4 * k + 2] = ev >> 16; b[4 * k + 3] = od >> 16;
    }
}

// The strip of a kernel that counts per CELL x CELL cell: a cell is CELL / 4 adjacent lanes, and a strip holds RB / CELL bands of cells.
template <int CELL>
struct CellStrip {
    static constexpr int RB = strip_rows(CELL), RW = RB / 4;         // rows per workgroup, per wave
    static constexpr int NB = RB / CELL, WPB = 4 / NB;               // bands per workgroup, waves per band
    static constexpr int LANES = CELL / 4, CPR = 64 / LANES;         // lanes per cell, cells per chunk
};
// The tail of such a kernel, cnt being the lane's count over its wave's rows: the CELL / 4 lanes of a cell are summed by DPP moves, the up to 4 waves that
// share a band meet in 1 KB of LDS, and one lane per cell stores its count with a plain store. Every element of counts is written by exactly one lane of
// one workgroup: nothing is zeroed, nothing is atomic. All 256 threads must arrive.
template <int CELL>
__device__ __forceinline__ void store_cell_counts(int cnt, int (&part)[4][64], unsigned rb, unsigned chunk, int *__restrict__ counts, int Gy, int Gx) {
    using S = CellStrip<CELL>;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    part[wave][lane] = lanes_allreduce_sum<S::LANES>(cnt);
    __syncthreads();
    if (tid < S::NB * S::CPR) {
        const int band = tid / S::CPR, c = tid - band * S::CPR;
        int s = 0;
#pragma unroll
        for (int k = 0; k < S::WPB; ++k) s += part[band * S::WPB + k][c * S::LANES];
        const int64_t gy = (int64_t)rb * S::NB + band;
        const unsigned gx = chunk * S::CPR + c;
        if (gy < Gy && gx < (unsigned)Gx) counts[gy * Gx + gx] = s;
    }
}

// ---- the launchers' argument checks: each returns TOAD_OK or the code it has already explained through set_error ("if (int rc = ...) return rc;") ----
static int check_hw(const char *what, const char *hname, int H, const char *wname, int W) {      // "Hr", "Wr" of a region; "Hp", "Wp" of a plane
    if (H > 0 && W > 0) return TOAD_OK;
    set_error("%s: bad shape (%s = %d, %s = %d)", what, hname, H, wname, W);
    return TOAD_ESHAPE;
}
static int check_region_pitch(const char *what, int64_t pitch, int Wr) {
    if (pitch < 3 * (int64_t)Wr) { set_error("%s: pitch %lld is less than a row of the region (3 Wr = %lld bytes)", what, (long long)pitch, 3ll * Wr); return TOAD_ESHAPE; }
    if (3 * (int64_t)Wr >= (1ll << 31)) { set_error("%s: region too wide: 3 Wr must stay below 2^31 (32-bit offsets inside a row)", what); return TOAD_ESHAPE; }
    return TOAD_OK;
}
static int check_plane_pitch(const char *what, int Wp, const char *name, int64_t pitch) {      // name: "pitch", "plane_pitch", "dst_pitch" - the caller's argument
    if (pitch >= (int64_t)Wp) return TOAD_OK;
    set_error("%s: %s %lld is less than a row of the plane (Wp = %d bytes)", what, name, (long long)pitch, Wp);
    return TOAD_ESHAPE;
}
static int check_plane_pitches(const char *what, int Wp, int64_t src_pitch, int64_t dst_pitch) {
    if (src_pitch >= (int64_t)Wp && dst_pitch >= (int64_t)Wp) return TOAD_OK;
    set_error("%s: src_pitch %lld or dst_pitch %lld is less than a row of the plane (Wp = %d bytes)", what, (long long)src_pitch, (long long)dst_pitch, Wp);
    return TOAD_ESHAPE;
}
static int check_cell(const char *what, int cell) {
    if (cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64) return TOAD_OK;
    set_error("%s: cell = %d is not one of 4, 8, 16, 32, 64", what, cell);
    return TOAD_ESHAPE;
}
static int check_u8(const char *what, const char *name, int v) {
    if (v >= 0 && v <= 255) return TOAD_OK;
    set_error("%s: %s = %d must lie in [0, 255] (the 8-bit scale)", what, name, v);
    return TOAD_EINVAL;
}
static int check_blocks(const char *what, const char *of, int64_t blocks) {      // of: "region" or "plane"
    if (blocks < (1ll << 31)) return TOAD_OK;
    set_error("%s: %s too large: %lld workgroups", what, of, (long long)blocks);
    return TOAD_ESHAPE;
}
// a lattice of tiles over a table of Gy x Gx cells: everything positive, the six lattice numbers multiples of the cell ...
static int check_lattice_units(const char *what, int cell, int x0, int y0, int H, int W, int sx, int sy, int nx, int ny, int Gy, int Gx) {
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
    return TOAD_OK;
}
// ... and its last tile inside the table
static int check_lattice_extent(const char *what, int cell, int x0, int y0, int H, int W, int sx, int sy, int nx, int ny, int Gy, int Gx) {
    const int64_t x_end = x0 + (int64_t)(nx - 1) * sx + W, y_end = y0 + (int64_t)(ny - 1) * sy + H;
    if (x_end <= (int64_t)Gx * cell && y_end <= (int64_t)Gy * cell) return TOAD_OK;
    set_error("%s: the lattice's last tile ends at (x, y) = (%lld, %lld), outside the %d x %d cells of %d pixels (Gy x Gx)", what, (long long)x_end,
              (long long)y_end, Gy, Gx, cell);
    return TOAD_ESHAPE;
}
static int check_no_overlap(const char *what, const unsigned char *src, int64_t src_pitch, const unsigned char *dst, int64_t dst_pitch, int Hp, int Wp) {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (uintptr_t)(Hp - 1) * (uintptr_t)src_pitch + (uintptr_t)Wp;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)(Hp - 1) * (uintptr_t)dst_pitch + (uintptr_t)Wp;
    if (!(s0 < d1 && d0 < s1)) return TOAD_OK;
    set_error("%s: src and dst overlap (a window reads what a neighbour has written)", what);
    return TOAD_EINVAL;
}
// the labels and areas of a plane's components: Hp Wp below 2^30, both arrays 4-byte aligned; `other` is the byte plane of the call, which need not be
static int check_labels(const char *what, int Hp, int Wp, const int *labels, const int *area, const char *other) {
    if ((int64_t)Hp * Wp >= (1ll << 30)) {
        set_error("%s: plane too large: Hp * Wp = %lld must stay below 2^30 (int32 labels, the border bit of area)", what, (long long)Hp * Wp);
        return TOAD_ESHAPE;
    }
    if (aligned4(labels) && aligned4(area)) return TOAD_OK;
    set_error("%s: labels (int32 [Hp][Wp]) and area (int32 [Hp * Wp]) must be 4-byte aligned (%s may have any alignment)", what, other);
    return TOAD_EALIGN;
}

}  // namespace toad
