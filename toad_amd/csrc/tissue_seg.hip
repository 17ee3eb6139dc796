// tissue_seg.hip — tissue selection as CLAM does it: a saturation plane of a box-filtered level, median-filtered, thresholded (by the caller's value or by
// Otsu's, which the host takes from the histogram this file counts), summed per cell (include/toad_hip.h, "segmented tissue selection"). The second
// selector next to tissue.hip, which stays as it is. Everything is integer arithmetic, so every plane, histogram and count has one right answer.
//
//   box filter  down in {1, 2, 4, 8, 16, 32}; Hp = Hr / down, Wp = Wr / down, partial boxes at the right and the bottom edge are dropped (as in
//               heat_blend_kernel). Per channel m = (sum of the down x down box + down^2 / 2) / down^2.
//   saturation  on the mean pixel, mx = max(r, g, b), mn = min(r, g, b):  S = (255 (mx - mn) + (mx >> 1)) / mx, that is 255 (mx - mn) / mx rounded half
//               up, and S = 0 where mx == 0 or mx < val_min. It is NOT claimed to be bit-equal to OpenCV's COLOR_RGB2HSV S channel (OpenCV rounds
//               a table-driven fixed-point quotient of its own).
//   median      k in {1, 3, 5, 7}: the (k k) / 2-th of the sorted k x k window around each plane pixel, coordinates clamped to the plane (replicate
//               border, as cv2.medianBlur); k = 1 is the identity. Any Hp, Wp >= 1, planes smaller than the window included.
//   histogram   hist[v] = the number of pixels of the median plane equal to v, int32 [256].
//   cells       counts[gy][gx] = the pixels > thresh (THRESH_BINARY) of every cell x cell cell of a plane, cells anchored at (0, 0), partial edge cells
//               counting the pixels that exist - the table toad_tissue_tile_counts sums over a lattice given in plane units.
//
// Four kernels:
//   sat_plane_kernel<DOWN>    one streaming pass over the region (the 100 MB one) -> the uint8 saturation plane.
//   sat_plane_list_kernel<DOWN>   the same pass over a LIST of windows (strips or blocks of a slide, each into its rows and columns of one plane): descriptors
//                             by value, the same body (sat_plane_body.inc).
//   plane_median_kernel<K>    a 64 x 4 output tile and its K - 1 halo staged in LDS as bytes, the rank taken by bisection over the 8 value bits.
//   plane_cells_kernel<CELL>  tissue_cells_kernel's work split on one byte per pixel.
#include "region_u8.h"

namespace toad {

// S = (255 (mx - mn) + (mx >> 1)) / mx exactly, for all 32,896 pairs mn <= mx: the numerator n is below 2^16 and the divisor below 2^8, so the float
// quotient n * rcp(mx) is off by less than 2^-6 and its truncation by at most one in either direction; one remainder test each way corrects it. mx == 0
// divides 0 by 1. val_min: S = 0 below it.
__device__ __forceinline__ unsigned sat_byte(int r, int g, int b, int vmin) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    const int d = max(mx, 1), n = __mul24(255, mx - mn) + (mx >> 1);
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int rem = n - __mul24(q, d);
    q += (rem >= d) - (rem < 0);
    return mx >= vmin ? (unsigned)q : 0u;
}

// byte k of the 12 bytes of 4 pixels held as three little-endian dwords: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
__device__ __forceinline__ int sg_byte(const unsigned (&w)[3], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// The work split and its addresses are region_u8.h's, on strips of RB = strip_rows(DOWN) rows (12 or 24 dwords a lane in flight). The kernel carries three
// channel sums where tissue_cells_kernel carries one count:
//   DOWN = 1, 2   a lane owns its boxes: 4 outputs a row, or 2 outputs every second row, stored as a dword / a half word at any byte address;
//   DOWN = 4      a lane's 4 x 4 pixels are one box: one byte a lane;
//   DOWN >= 8     the DOWN / 4 lanes of a box are summed by DPP moves, the 2 or 4 waves of a box row meet in 3 KB of LDS, one lane per box stores.
// Hi = DOWN Hp and Wi = DOWN Wp are the rows and columns some box consumes: nothing outside them is read (a dropped partial box needs no reading at all),
// so no byte outside y pitch + [0, 3 Wr), y < Hr, is. A wave off the plain path holds zeros for the rows and pixels that are not consumed (a lane has
// 1 to 3 pixels with DOWN <= 2 only: Wi is a multiple of DOWN). Zeros are harmless: a box lies wholly inside Hi x Wi or wholly outside. Every plane byte is
// written by exactly one lane, once; nothing outside y plane_pitch + [0, Wp), y < Hp, is written.
// The one exception to "edge loads go through load_px4": the loop below is load_px4's body, statement for statement, but for the zeroing of w[r], which
// stands in front of the r < rows test (rows that do not exist must be zeros too) and not in the byte-load arm. With the helper called instead, hipcc
// lays sat_plane_kernel<1> out differently and its PLAIN path - the same instructions - ran 0.8 % slower on a 4096 x 8192 region in 6 of 6 alternating
// runs, the parent's own runs spreading by 0.2 % (profiles/r13a_region_refactor_ab.md, "sat_plane_kernel through load_px4"). Written out, DOWN = 1 and 2
// compile to the parent's code. The body lies in sat_plane_body.inc, which sat_plane_list_kernel includes too (an included file and not a device
// function, for the same reason: profiles/tissue_strips_isa.md compares the six instantiations with what the kernel compiled to when the body stood here).
template <int DOWN>
__global__ __launch_bounds__(256) void sat_plane_kernel(const unsigned char *__restrict__ region, int64_t pitch, int Hi, int Wi, int vmin,
                                                        unsigned char *__restrict__ plane, int64_t ppitch, unsigned nchunks) {
    const unsigned bid = blockIdx.x;
#include "sat_plane_body.inc"
}

// ---- a list of windows in one launch: toad_regions_saturation_u8 ----
// The list form of sat_plane_kernel, built as heat_blend_px_list_kernel is (heatmap.hip): the windows share DOWN and vmin and each has a descriptor of its
// own; the descriptors travel by value in the kernel argument - no device table, no upload. The grid is the windows' workgroups one after the other,
// descriptor k owning workgroups first[k] .. first[k + 1]; descriptors from n on carry first = 0xFFFFFFFF, above every workgroup index, so the search needs
// no n: five uniform steps of a binary search over the 32 prefixes, scalar loads from the kernel argument, once per workgroup. From there on a workgroup is
// one of its window's: chunk and rb from its index inside the window, and the body sat_plane_kernel runs. The grid is exact: every workgroup has a window.
// Windows without a workgroup (Hr < down or Wr < down) never reach a descriptor. No atomics, no scratch, and the LDS of the single form.
constexpr int SAT_LIST_MAX = 32;                                     // 32 descriptors of 48 bytes and vmin: 1.5 KB of the 4 KB a kernel argument may have
struct SatListWin {
    const unsigned char *region; int64_t pitch; unsigned char *plane; int64_t ppitch;
    int Hi, Wi; unsigned nchunks, first;
};
struct SatListArgs { SatListWin w[SAT_LIST_MAX]; };
static_assert(sizeof(SatListArgs) + sizeof(int) <= 4096, "the descriptors travel in the kernel argument");

template <int DOWN>
__global__ __launch_bounds__(256) void sat_plane_list_kernel(const SatListArgs l, int vmin) {
    static_assert(SAT_LIST_MAX == 32, "five steps search 32 prefixes");
    int k = 0;
#pragma unroll
    for (int step = SAT_LIST_MAX / 2; step >= 1; step >>= 1)
        if (l.w[k + step].first <= blockIdx.x) k += step;
    const SatListWin &win = l.w[k];
    const unsigned char *__restrict__ region = win.region;
    unsigned char *__restrict__ plane = win.plane;
    const int64_t pitch = win.pitch, ppitch = win.ppitch;
    const int Hi = win.Hi, Wi = win.Wi;
    const unsigned nchunks = win.nchunks, bid = blockIdx.x - win.first;
#include "sat_plane_body.inc"
}

// Per byte of x: bit 7 of the result is set iff the byte >= the byte of t at that place (unsigned); the other bits are garbage. d compares the low 7
// bits - (x | 0x80) - (t & 0x7f) cannot borrow across bytes - and where the top bits differ (e) the top bit of x decides: a bit-field insert.
__device__ __forceinline__ unsigned bytes_ge(unsigned x, unsigned t, unsigned t7) {
    const unsigned d = (x | 0x80808080u) - t7, e = x ^ t;
    return (e & x) | (~e & d);
}

// A workgroup of 4 waves takes a 64 x 4 tile of outputs, one row a wave, one output a lane (a small plane - 512 x 256 at down = 16 - still fills the
// chip). The tile and its halo, (3 + K) rows of 72 bytes = plane columns [x0 - 4, x0 + 68), are staged in LDS as bytes with CLAMPED coordinates, one dword
// a thread, so nothing afterwards branches on the border: a dword load at any byte address where its 4 columns lie inside the plane, 4 clamped byte loads
// elsewhere - no byte outside y src_pitch + [0, Wp), y < Hp, is read. A lane then reads its window as K rows of three neighbouring DWORDS (not bytes: no
// 4-way same-dword traffic), and a byte alignment turns them into the 8 bytes that start at its window's first column. LDS banks: the 32 lanes of a
// ds_read_b32 group read at most 11 consecutive dwords of one row - distinct banks, equal addresses broadcast; the staging stores are 32 consecutive
// dwords of a 19-dword-pitch array but for one wrap, so at most 2-way on a handful of banks.
// The rank: bisection over the 8 value bits. With m = K K / 2 the median is the largest v with #(window < v) <= m, built from the top bit down; a
// candidate is kept iff #(window >= candidate) >= K K - m. The count is a byte-parallel compare (bytes_ge) and a popcount per dword, masked to the
// window's K bytes: about 6 K ceil(K / 4) operations a bit, no scratch, the window held in 2 K registers.
// The histogram: each workgroup counts its outputs in 1 KB of LDS and adds its non-zero bins to hist with INTEGER atomics - integer adds commute, so the
// result does not depend on the order in which workgroups arrive. No float atomics anywhere.
template <int K>
__global__ __launch_bounds__(256) void plane_median_kernel(const unsigned char *__restrict__ src, int64_t spitch, int Hp, int Wp,
                                                           unsigned char *__restrict__ dst, int64_t dpitch, int *__restrict__ hist, unsigned ntx) {
    constexpr int R = K / 2, ROWS = 4 + K - 1, ROWDW = 19;         // 18 dwords of pixels and one of zeros, which the last lanes' third read lands in
    __shared__ unsigned tile[ROWS * ROWDW];
    __shared__ int lhist[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = (int)(tx * 64u);
    const int64_t y0 = (int64_t)ty * 4;
    if (hist) lhist[tid] = 0;
    if (tid < ROWS * ROWDW) {
        const int r = tid / ROWDW, c = tid - r * ROWDW;
        unsigned v = 0;
        if (c < 18) {
            const int64_t y = min(max(y0 + r - R, (int64_t)0), (int64_t)Hp - 1);
            const unsigned char *row = src + y * spitch;
            const int xs = x0 - 4 + 4 * c;
            if (xs >= 0 && xs + 4 <= Wp) {
                v = *reinterpret_cast<const u32_a1 *>(row + xs);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v |= (unsigned)row[min(max(xs + k, 0), Wp - 1)] << (8 * k);
            }
        }
        tile[tid] = v;
    }
    __syncthreads();
    const int bx = lane + 4 - R, d0 = bx >> 2, sh = bx & 3;        // the window's first column as a byte of the LDS row: dword and byte inside it
    unsigned lo[K], hi[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const unsigned *p = tile + (wave + r) * ROWDW + d0;
        const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
        lo[r] = __builtin_amdgcn_alignbyte(w1, w0, sh);
        hi[r] = __builtin_amdgcn_alignbyte(w2, w1, sh);
    }
    unsigned med;
    if constexpr (K == 1) {
        med = lo[0] & 255u;
    } else {
        constexpr unsigned MLO = K >= 4 ? 0x80808080u : 0x00808080u;                               // the window's K bytes of the 8
        constexpr unsigned MHI = K == 7 ? 0x00808080u : K == 5 ? 0x00000080u : 0u;
        constexpr int NEED = K * K - (K * K) / 2;
        med = 0;
#pragma unroll
        for (int bit = 7; bit >= 0; --bit) {
            const unsigned cand = med | (1u << bit), t = cand * 0x01010101u, t7 = t & 0x7F7F7F7Fu;
            int cnt = 0;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                cnt += __builtin_popcount(bytes_ge(lo[r], t, t7) & MLO);
                if constexpr (MHI != 0u) cnt += __builtin_popcount(bytes_ge(hi[r], t, t7) & MHI);
            }
            if (cnt >= NEED) med = cand;
        }
    }
    const int64_t y = y0 + wave;
    const int xo = x0 + lane;
    const bool live = y < Hp && xo < Wp;
    if (live) dst[y * dpitch + xo] = (unsigned char)med;
    if (hist) {                                                    // workgroup-uniform
        if (live) atomicAdd(&lhist[med], 1);
        __syncthreads();
        const int n = lhist[tid];
        if (n) atomicAdd(hist + tid, n);
    }
}

// tissue_cells_kernel on a one-byte plane (region_u8.h's work split with a dword a lane, and its cell-count tail). The bytes > thresh of a dword are its
// bytes >= thresh + 1 (t1, in 1 .. 255; the launcher passes on = 0 for thresh = 255, where nothing counts): one byte-parallel compare and a popcount. No
// byte outside y pitch + [0, Wp), y < Hp, is read: the lane the row ends in takes its 1 to 3 bytes one by one; absent bytes are 0, below every t1.
template <int CELL>
__global__ __launch_bounds__(256) void plane_cells_kernel(const unsigned char *__restrict__ plane, int64_t pitch, int Hp, int Wp, unsigned t1, int on,
                                                          int *__restrict__ counts, int Gy, int Gx, unsigned nchunks) {
    constexpr int RB = CellStrip<CELL>::RB, RW = CellStrip<CELL>::RW;
    __shared__ int part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned chunk = blockIdx.x % nchunks, rb = blockIdx.x / nchunks;
    const unsigned off = chunk * 256u + (unsigned)lane * 4u;
    const int64_t y0 = (int64_t)rb * RB + wave * RW;
    const unsigned char *base = plane + y0 * pitch + off;
    const unsigned t = t1 * 0x01010101u, t7 = t & 0x7F7F7F7Fu;
    int cnt = 0;
    if (chunk * 256u + 256u <= (unsigned)Wp && y0 + RW <= Hp) {    // wave-uniform: all 256 bytes of all RW rows exist
#pragma unroll
        for (int r = 0; r < RW; ++r) cnt += __builtin_popcount(bytes_ge(*reinterpret_cast<const u32_a1 *>(base + r * pitch), t, t7) & 0x80808080u);
    } else {
        const int rows = (int)min((int64_t)RW, (int64_t)Hp - y0);  // <= 0 below the plane
        const int nb = off < (unsigned)Wp ? min(4, Wp - (int)off) : 0;
        for (int r = 0; r < rows; ++r) {
            const unsigned char *p = base + r * pitch;
            unsigned v = 0;
            if (nb == 4) {
                v = *reinterpret_cast<const u32_a1 *>(p);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < nb) v |= (unsigned)p[k] << (8 * k);
            }
            cnt += __builtin_popcount(bytes_ge(v, t, t7) & 0x80808080u);
        }
    }
    store_cell_counts<CELL>(on ? cnt : 0, part, rb, chunk, counts, Gy, Gx);
}

static bool seg_down_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8 || d == 16 || d == 32; }

}  // namespace toad

using namespace toad;

extern "C" int toad_region_saturation_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, int down, int val_min, unsigned char *plane,
                                         int64_t plane_pitch, void *stream) {
    const char *what = "toad_region_saturation_u8";
    if (!region || !plane) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_u8(what, "val_min", val_min)) return rc;
    if (!seg_down_ok(down)) { set_error("%s: down = %d is not one of 1, 2, 4, 8, 16, 32", what, down); return TOAD_ESHAPE; }
    if (int rc = check_hw(what, "Hr", Hr, "Wr", Wr)) return rc;
    if (int rc = check_region_pitch(what, pitch, Wr)) return rc;
    const int Hp = Hr / down, Wp = Wr / down;
    if (int rc = check_plane_pitch(what, Wp, "plane_pitch", plane_pitch)) return rc;
    const int Hi = Hp * down, Wi = Wp * down, rb = strip_rows(down);
    const int64_t nchunks = ((int64_t)Wi + 255) / 256, blocks = nchunks * (((int64_t)Hi + rb - 1) / rb);
    if (int rc = check_blocks(what, "region", blocks)) return rc;
    if (Hp == 0 || Wp == 0) return TOAD_OK;
    hipStream_t st = (hipStream_t)stream;
#define TOAD_SAT_LAUNCH(D) \
    hipLaunchKernelGGL(sat_plane_kernel<D>, dim3((unsigned)blocks), dim3(256), 0, st, region, pitch, Hi, Wi, val_min, plane, plane_pitch, (unsigned)nchunks)
    switch (down) {
        case 1: TOAD_SAT_LAUNCH(1); break;
        case 2: TOAD_SAT_LAUNCH(2); break;
        case 4: TOAD_SAT_LAUNCH(4); break;
        case 8: TOAD_SAT_LAUNCH(8); break;
        case 16: TOAD_SAT_LAUNCH(16); break;
        default: TOAD_SAT_LAUNCH(32); break;
    }
#undef TOAD_SAT_LAUNCH
    return check_launch(what);
}

// The list entry: what the windows share first (val_min, down: the single entry's checks and messages), then window by window the single entry's checks of
// what each window has of its own, in its order, the first failing window winning under "window k:"; then the workgroup count of the whole list. Nothing is
// launched before all of that has passed. Two walks over the host array, no allocation: the first checks and counts, the second fills SAT_LIST_MAX
// descriptors at a time and launches them.
extern "C" int toad_regions_saturation_u8(const ToadSatWindow *windows, int n, int down, int val_min, void *stream) {
    const char *what = "toad_regions_saturation_u8";
    if (n > 0 && !windows) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (n < 0) { set_error("%s: n = %d windows", what, n); return TOAD_EINVAL; }
    if (int rc = check_u8(what, "val_min", val_min)) return rc;
    if (!seg_down_ok(down)) { set_error("%s: down = %d is not one of 1, 2, 4, 8, 16, 32", what, down); return TOAD_ESHAPE; }
    const int rb = strip_rows(down);
    // a window's workgroups: 0 where it has no plane pixel
    auto geometry = [&](const ToadSatWindow &w, int &Hi, int &Wi, int64_t &nchunks) {
        Hi = w.Hr / down * down; Wi = w.Wr / down * down;
        nchunks = ((int64_t)Wi + 255) / 256;
        return nchunks * (((int64_t)Hi + rb - 1) / rb);
    };
    int64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        const ToadSatWindow &w = windows[k];
        char who[80];
        snprintf(who, sizeof who, "window %d: %s", k, what);
        if (!w.region || !w.plane) { set_error("%s: null pointer", who); return TOAD_EINVAL; }
        if (int rc = check_hw(who, "Hr", w.Hr, "Wr", w.Wr)) return rc;
        if (int rc = check_region_pitch(who, w.pitch, w.Wr)) return rc;
        if (int rc = check_plane_pitch(who, w.Wr / down, "plane_pitch", w.plane_pitch)) return rc;
        int Hi, Wi;
        int64_t nchunks;
        blocks += geometry(w, Hi, Wi, nchunks);                      // one window: below 2^50 ...
        if (blocks > (1ll << 31)) blocks = 1ll << 31;                // ... and the sum saturates where it is refused
    }
    if (int rc = check_blocks(what, "list of regions", blocks)) return rc;
    if (blocks == 0) return TOAD_OK;
    SatListArgs l;
    for (int k = 0; k < n;) {
        int m = 0;
        unsigned grid = 0;
        for (; k < n && m < SAT_LIST_MAX; ++k) {
            const ToadSatWindow &w = windows[k];
            int Hi, Wi;
            int64_t nchunks;
            const int64_t b = geometry(w, Hi, Wi, nchunks);
            if (b == 0) continue;
            l.w[m++] = {w.region, w.pitch, w.plane, w.plane_pitch, Hi, Wi, (unsigned)nchunks, grid};
            grid += (unsigned)b;
        }
        if (m == 0) break;
        for (int j = m; j < SAT_LIST_MAX; ++j) { l.w[j] = {}; l.w[j].first = 0xFFFFFFFFu; }      // above every workgroup index: the search stops short of them
#define TOAD_SAT_LIST(D) case D: hipLaunchKernelGGL(sat_plane_list_kernel<D>, dim3(grid), dim3(256), 0, (hipStream_t)stream, l, val_min); break;
        switch (down) { TOAD_SAT_LIST(1) TOAD_SAT_LIST(2) TOAD_SAT_LIST(4) TOAD_SAT_LIST(8) TOAD_SAT_LIST(16) TOAD_SAT_LIST(32) }
#undef TOAD_SAT_LIST
        if (int rc = check_launch(what)) return rc;
    }
    return TOAD_OK;
}

extern "C" int toad_plane_median_u8(const unsigned char *src, int64_t src_pitch, int Hp, int Wp, int k, unsigned char *dst, int64_t dst_pitch, int *hist,
                                    void *stream) {
    const char *what = "toad_plane_median_u8";
    if (!src || !dst) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (k != 1 && k != 3 && k != 5 && k != 7) { set_error("%s: k = %d is not one of 1, 3, 5, 7", what, k); return TOAD_ESHAPE; }
    if (int rc = check_hw(what, "Hp", Hp, "Wp", Wp)) return rc;
    if (int rc = check_plane_pitches(what, Wp, src_pitch, dst_pitch)) return rc;
    if (int rc = check_no_overlap(what, src, src_pitch, dst, dst_pitch, Hp, Wp)) return rc;
    const int64_t ntx = ((int64_t)Wp + 63) / 64, blocks = ntx * (((int64_t)Hp + 3) / 4);
    if (int rc = check_blocks(what, "plane", blocks)) return rc;
    if (hist && !aligned4(hist)) { set_error("%s: hist (int32 [256]) must be 4-byte aligned (the planes may have any alignment)", what); return TOAD_EALIGN; }
    hipStream_t st = (hipStream_t)stream;
    if (hist && hipMemsetAsync(hist, 0, 256 * sizeof(int), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: zeroing hist failed", what);
        return TOAD_EINVAL;
    }
#define TOAD_MEDIAN_LAUNCH(KK) \
    hipLaunchKernelGGL(plane_median_kernel<KK>, dim3((unsigned)blocks), dim3(256), 0, st, src, src_pitch, Hp, Wp, dst, dst_pitch, hist, (unsigned)ntx)
    switch (k) {
        case 1: TOAD_MEDIAN_LAUNCH(1); break;
        case 3: TOAD_MEDIAN_LAUNCH(3); break;
        case 5: TOAD_MEDIAN_LAUNCH(5); break;
        default: TOAD_MEDIAN_LAUNCH(7); break;
    }
#undef TOAD_MEDIAN_LAUNCH
    return check_launch(what);
}

extern "C" int toad_plane_cells_u8(const unsigned char *plane, int64_t pitch, int Hp, int Wp, int cell, int thresh, int *counts, void *stream) {
    const char *what = "toad_plane_cells_u8";
    if (!plane || !counts) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_u8(what, "thresh", thresh)) return rc;
    if (int rc = check_cell(what, cell)) return rc;
    if (int rc = check_hw(what, "Hp", Hp, "Wp", Wp)) return rc;
    if (int rc = check_plane_pitch(what, Wp, "pitch", pitch)) return rc;
    const int rb = strip_rows(cell);
    const int64_t nchunks = ((int64_t)Wp + 255) / 256, blocks = nchunks * (((int64_t)Hp + rb - 1) / rb);
    if (int rc = check_blocks(what, "plane", blocks)) return rc;
    if (!aligned4(counts)) { set_error("%s: counts (int32 [Gy][Gx]) must be 4-byte aligned (the plane may have any alignment)", what); return TOAD_EALIGN; }
    const int Gy = (int)(((int64_t)Hp + cell - 1) / cell), Gx = (int)(((int64_t)Wp + cell - 1) / cell);
    const unsigned t1 = thresh < 255 ? (unsigned)thresh + 1u : 255u;
    const int on = thresh < 255;
    hipStream_t st = (hipStream_t)stream;
#define TOAD_PCELLS_LAUNCH(C) \
    hipLaunchKernelGGL(plane_cells_kernel<C>, dim3((unsigned)blocks), dim3(256), 0, st, plane, pitch, Hp, Wp, t1, on, counts, Gy, Gx, (unsigned)nchunks)
    switch (cell) {
        case 4: TOAD_PCELLS_LAUNCH(4); break;
        case 8: TOAD_PCELLS_LAUNCH(8); break;
        case 16: TOAD_PCELLS_LAUNCH(16); break;
        case 32: TOAD_PCELLS_LAUNCH(32); break;
        default: TOAD_PCELLS_LAUNCH(64); break;
    }
#undef TOAD_PCELLS_LAUNCH
    return check_launch(what);
}
