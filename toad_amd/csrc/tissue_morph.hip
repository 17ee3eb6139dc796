// tissue_morph.hip — the steps of CLAM's segmentTissue that follow the threshold: morphological closing of the tissue mask, then the area filters over its
// connected components and over the holes inside them (include/toad_hip.h, "segmented tissue selection", steps 6a to 6c). Everything is integer
// arithmetic on a plane of bytes, so every mask, label and area has one right answer.
//
//   closing     c in 0 .. 8, lo = c / 2, hi = c - 1 - c / 2: M0 = src > thresh; D[y][x] = OR of M0 over -lo <= dy, dx <= hi, M1[y][x] = AND of D over the
//               same offsets, both windows clipped to the plane. dst = 255 where M1, 0 elsewhere. c = 0, 1: M1 = M0.
//   components  selected = (plane > thresh) != background; 8-connected for background == 0, 4-connected for background == 1. labels[y][x] = the smallest
//               y Wp + x of the pixel's component, -1 where unselected; area[label] = the component's pixel count + 2^30 iff it touches the plane's outer
//               rows or columns, 0 at every other index.
//   selection   mode 0: dst = 255 iff label >= 0 and count >= limit; mode 1 (labels of the background): dst = 255 iff label < 0 or (count < limit and the
//               border bit is clear).
//
// Five kernels:
//   plane_close_kernel<C>  a 64 x 16 output tile and its 2 (C - 1) halo as bytes in LDS; four separable passes (row OR, column OR, row AND, column AND).
//   cc_local_kernel        union-find of a 64 x 16 tile in LDS; writes every pixel's parent as a global index and zeroes the tile's part of area.
//   cc_seam_kernel         one lane per pixel on the low side of a tile seam: merges the trees across the seam, diagonals included for connectivity 8.
//   cc_flatten_kernel      every pixel's root; counts and border bits summed per tile in LDS, then added to area[root] with integer atomics.
//   area_select_kernel     one byte per pixel from labels and area.
//
// The labelling is the label-equivalence (union-find) scheme: parent[i] <= i always, a root has parent[i] == i, and the root of a tree is its smallest
// index - the canonical label. The memory-model argument, which holds for the LDS phase and the global phases alike:
//   * a parent is only ever written by an atomic min (or, in the flatten pass, replaced by the root it already leads to), so parents only decrease and trees
//     only merge. Every value a parent ever held is a member of the pixel's component, at an index <= the pixel's.
//   * a stale read of a parent - from L1, from another XCD's view of L2 - therefore still names an ancestor or a former root of the same tree. find() may
//     stop at a pixel that has meanwhile stopped being a root; the link is made by a RETURNED device-scope atomicMin on that pixel's parent, which acts on the
//     true value: if it returns anything but the pixel itself the lane lost a race and continues from the value returned, which is smaller. Correctness
//     never depends on a load being fresh; freshness only shortens walks, which is why the find path of the seam pass loads with
//     __hip_atomic_load(relaxed, agent) - served by L2, not by a CU's L1, which no other CU's store ever refreshes.
//   * the only ordering between workgroups for plain data is a kernel boundary: local -> seam -> flatten are three launches on one stream.
// Hang safety: every loop strictly decreases an index (find: x <- parent[x] < x; union: max(a, b) decreases with every lost race), no lane waits for another
// workgroup, there is no grid-wide barrier, no cooperative launch and no float atomic. Counts and the border bit reach area[] by integer add and or, which
// commute: the result does not depend on the order of arrival.
#include "region_u8.h"

namespace toad {

constexpr int MT_W = 64, MT_H = 16, MT_PX = MT_W * MT_H;           // the tile of every kernel here: lanes along x, 4 rows a thread
constexpr int MT_BORDER = 1 << 30, MT_COUNT = MT_BORDER - 1;

// ---- closing ----------------------------------------------------------------------------------------------------------------------------------------------
// LDS frame: row r <-> plane row y0 - 2 lo + r, column q <-> plane column x0 - 2 lo + q; RH = 16 + 2 (C - 1) rows of RW = 64 + 2 (C - 1) bytes (30 x 78 at
// C = 8). The window is clipped to the PLANE, not the tile, so the dilated values the erosion reads at halo positions must be right: that is what the
// second ring of halo is for. Outside the plane M0 = 0 (the identity of OR) and D = 1 (the identity of AND) - clipping the window is leaving those out.
//   pass 0  a[r][q] = M0, all RH x RW                       pass 1  b[r][q] = OR a[r][q - lo .. q + hi],  q in [lo, RW - hi)
//   pass 2  a[r][q] = OR b[r - lo .. r + hi][q] (1 outside the plane), r in [lo, RH - hi), q as in pass 1
//   pass 3  b[r][q] = AND a[r][q - lo .. q + hi], q in [2 lo, 2 lo + 64)       pass 4  out = AND b[r - lo .. r + hi][q], r in [2 lo, 2 lo + 16)
// No byte outside src + y src_pitch + [0, Wp), y < Hp, is read and none outside dst + y dst_pitch + [0, Wp) written: every access tests its coordinates.
template <int C>
__global__ __launch_bounds__(256) void plane_close_kernel(const unsigned char *__restrict__ src, int64_t spitch, int Hp, int Wp, int thresh,
                                                          unsigned char *__restrict__ dst, int64_t dpitch, unsigned ntx) {
    constexpr int LO = C / 2, HI = C - 1 - C / 2, RH = MT_H + 2 * (C - 1), RW = MT_W + 2 * (C - 1), RP = (RW + 3) & ~3;
    __shared__ unsigned char a[RH * RP], b[RH * RP];
    const int tid = threadIdx.x;
    const unsigned tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int64_t ya = (int64_t)ty * MT_H - 2 * LO;                // plane row of LDS row 0
    const int xa = (int)(tx * MT_W) - 2 * LO;                      // plane column of LDS column 0
    for (int i = tid; i < RH * RW; i += 256) {
        const int r = i / RW, q = i - r * RW;
        const int64_t y = ya + r;
        const int x = xa + q;
        a[r * RP + q] = (y >= 0 && y < Hp && x >= 0 && x < Wp) ? (unsigned char)(src[y * spitch + x] > thresh) : (unsigned char)0;
    }
    if constexpr (C > 1) {
        constexpr int W1 = RW - LO - HI, H2 = RH - LO - HI;
        __syncthreads();
        for (int i = tid; i < RH * W1; i += 256) {
            const int r = i / W1, q = LO + (i - r * W1);
            unsigned v = 0;
#pragma unroll
            for (int d = -LO; d <= HI; ++d) v |= a[r * RP + q + d];
            b[r * RP + q] = (unsigned char)v;
        }
        __syncthreads();
        for (int i = tid; i < H2 * W1; i += 256) {
            const int r = LO + i / W1, q = LO + i % W1;
            const int64_t y = ya + r;
            const int x = xa + q;
            unsigned v = 0;
#pragma unroll
            for (int d = -LO; d <= HI; ++d) v |= b[(r + d) * RP + q];
            a[r * RP + q] = (y >= 0 && y < Hp && x >= 0 && x < Wp) ? (unsigned char)v : (unsigned char)1;
        }
        __syncthreads();
        for (int i = tid; i < H2 * MT_W; i += 256) {
            const int r = LO + i / MT_W, q = 2 * LO + i % MT_W;
            unsigned v = 1;
#pragma unroll
            for (int d = -LO; d <= HI; ++d) v &= a[r * RP + q + d];
            b[r * RP + q] = (unsigned char)v;
        }
    }
    __syncthreads();
    const int lx = tid & 63;
    const int x = (int)(tx * MT_W) + lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k;
        const int64_t y = (int64_t)ty * MT_H + ly;
        const int r = 2 * LO + ly, q = 2 * LO + lx;
        unsigned v;
        if constexpr (C > 1) {
            v = 1;
#pragma unroll
            for (int d = -LO; d <= HI; ++d) v &= b[(r + d) * RP + q];
        } else {
            v = a[r * RP + q];
        }
        if (y < Hp && x < Wp) dst[y * dpitch + x] = v ? (unsigned char)255 : (unsigned char)0;
    }
}

// ---- union-find -------------------------------------------------------------------------------------------------------------------------------------------
// find: follow parents while they decrease. The unsigned compare also stops at a negative value (an unselected pixel's -1), which no selected pixel's
// parent ever is: the walk cannot leave the array whatever it reads.
__device__ __forceinline__ int lds_find(const int *lab, int x) {
    for (;;) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
}
__device__ __forceinline__ int dev_find(const int *lab, int x) {
    for (;;) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
}
// union: link the larger root to the smaller with a returned atomic min. old == a: a was a root and now hangs below b. Otherwise a had a parent old < a
// already (and now min(old, b)): what remains is to merge old with b. max(a, b) strictly decreases from one round to the next.
__device__ __forceinline__ void lds_union(int *lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}
__device__ __forceinline__ void dev_union(int *lab, int a, int b) {
    for (;;) {
        a = dev_find(lab, a);
        b = dev_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);                     // device scope, returned
        if (old == a) return;
        a = old;
    }
}
__device__ __forceinline__ bool lds_selected(const int *lab, int l) { return __hip_atomic_load(lab + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0; }
__device__ __forceinline__ bool dev_selected(const int *lab, int g) { return __hip_atomic_load(lab + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0; }

// (a) A workgroup labels its 64 x 16 tile in 4 KB of LDS: lab[l] = l on selected pixels, -1 elsewhere (pixels outside the plane included); every selected
// pixel is united with its selected left, upper and - for connectivity 8 - upper-left and upper-right neighbours inside the tile. The local root is the
// smallest local index, and local and global indices are both row-major, so it is the smallest global index of the tile's part too. Every in-plane element
// of labels and of area is written: the parent (or -1), and 0.
__global__ __launch_bounds__(256) void cc_local_kernel(const unsigned char *__restrict__ plane, int64_t pitch, int Hp, int Wp, int thresh, int background,
                                                       int *__restrict__ labels, int *__restrict__ area, unsigned ntx) {
    __shared__ int lab[MT_PX];
    const int tid = threadIdx.x, lx = tid & 63;
    const unsigned tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = (int)(tx * MT_W), y0 = (int)(ty * MT_H), x = x0 + lx;
    unsigned sel = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly, l = ly * MT_W + lx;
        const bool inb = x < Wp && y < Hp;
        const bool s = inb && ((plane[(int64_t)y * pitch + x] > thresh) != (background != 0));
        sel |= (unsigned)s << k;
        lab[l] = s ? l : -1;
        if (inb) area[y * Wp + x] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, l = ly * MT_W + lx;
        if (!((sel >> k) & 1u)) continue;
        if (lx > 0 && lds_selected(lab, l - 1)) lds_union(lab, l, l - 1);
        if (ly > 0) {
            if (lds_selected(lab, l - MT_W)) lds_union(lab, l, l - MT_W);
            if (!background) {
                if (lx > 0 && lds_selected(lab, l - MT_W - 1)) lds_union(lab, l, l - MT_W - 1);
                if (lx < MT_W - 1 && lds_selected(lab, l - MT_W + 1)) lds_union(lab, l, l - MT_W + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly, l = ly * MT_W + lx;
        if (x < Wp && y < Hp) {
            int g = -1;
            if ((sel >> k) & 1u) {
                const int r = lds_find(lab, l);
                g = (y0 + (r >> 6)) * Wp + x0 + (r & 63);
            }
            labels[y * Wp + x] = g;
        }
    }
}

// (b) One lane per pixel on the low side of a seam. The first nvl = nv Hp lanes take the vertical seams - pixel (y, x), x = 64 (s + 1), with (y, x - 1) and,
// for connectivity 8, (y - 1, x - 1) and (y + 1, x - 1); the others the horizontal seams - pixel (y, x), y = 16 (s + 1), with (y - 1, x) and, for
// connectivity 8, (y - 1, x - 1) and (y - 1, x + 1). Every pair of neighbours that lie in different tiles is met by one of these, the diagonal pairs across
// the corner where four tiles meet included (some twice, which is harmless). Whether a pixel is selected never changes (-1 is written once, by (a)).
__global__ __launch_bounds__(256) void cc_seam_kernel(int *labels, int Hp, int Wp, int conn8, int nvl, int total) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= total) return;
    if (i < nvl) {
        const int s = i / Hp, y = i - s * Hp, x = MT_W * (s + 1), g = y * Wp + x;
        if (!dev_selected(labels, g)) return;
        if (dev_selected(labels, g - 1)) dev_union(labels, g, g - 1);
        if (conn8) {
            if (y > 0 && dev_selected(labels, g - Wp - 1)) dev_union(labels, g, g - Wp - 1);
            if (y < Hp - 1 && dev_selected(labels, g + Wp - 1)) dev_union(labels, g, g + Wp - 1);
        }
    } else {
        const int j = i - nvl, s = j / Wp, x = j - s * Wp, y = MT_H * (s + 1), g = y * Wp + x;
        if (!dev_selected(labels, g)) return;
        if (dev_selected(labels, g - Wp)) dev_union(labels, g, g - Wp);
        if (conn8) {
            if (x > 0 && dev_selected(labels, g - Wp - 1)) dev_union(labels, g, g - Wp - 1);
            if (x < Wp - 1 && dev_selected(labels, g - Wp + 1)) dev_union(labels, g, g - Wp + 1);
        }
    }
}

// (c) Every selected pixel adds itself to a bucket of its tile in LDS: the bucket of its parent where that lies in this tile (after (a) and (b) this is the
// pixel's local root - (b) changes the parents of roots only - but nothing here relies on it: any parent is a member of the same component), its own
// otherwise; a pixel on the plane's outer rows or columns also sets the bucket's border bit. The thread of every non-empty bucket then finds the root of
// its own pixel - one global walk per local component, not per pixel - adds the bucket's count to area[root] and ors the border bit in (integer atomics:
// Guideline 12, summed in LDS first), and leaves the root in LDS for the bucket's pixels to store. Counts stay below 2^30 = Hp Wp's bound, so the adds
// never carry into the border bit. Other workgroups overwrite parents with roots while this one walks them: a root is an ancestor like any other.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int *labels, int *area, int Hp, int Wp, unsigned ntx) {
    __shared__ int cnt[MT_PX], groot[MT_PX];
    const int tid = threadIdx.x, lx = tid & 63;
    const unsigned tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = (int)(tx * MT_W), y0 = (int)(ty * MT_H), x = x0 + lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[((tid >> 6) + 4 * k) * MT_W + lx] = 0;
    __syncthreads();
    int bucket[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly, l = ly * MT_W + lx;
        bucket[k] = -1;
        if (x < Wp && y < Hp) {
            const int p = __hip_atomic_load(labels + y * Wp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p >= 0) {
                const int py = p / Wp - y0, px = p - (p / Wp) * Wp - x0;
                const int bk = ((unsigned)py < (unsigned)MT_H && (unsigned)px < (unsigned)MT_W) ? py * MT_W + px : l;
                bucket[k] = bk;
                atomicAdd(cnt + bk, 1);
                if (y == 0 || y == Hp - 1 || x == 0 || x == Wp - 1) atomicOr(cnt + bk, MT_BORDER);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly, l = ly * MT_W + lx;
        const int c = cnt[l];
        if (c != 0) {                                              // then (y, x) is a selected pixel of the plane
            const int root = dev_find(labels, y * Wp + x);
            groot[l] = root;
            atomicAdd(area + root, c & MT_COUNT);
            if (c & MT_BORDER) atomicOr(area + root, MT_BORDER);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly;
        if (bucket[k] >= 0) labels[y * Wp + x] = groot[bucket[k]];
    }
}

__global__ __launch_bounds__(256) void area_select_kernel(const int *__restrict__ labels, const int *__restrict__ area, int Hp, int Wp, int mode, int limit,
                                                          unsigned char *__restrict__ dst, int64_t dpitch, unsigned ntx) {
    const int tid = threadIdx.x;
    const unsigned tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x = (int)(tx * MT_W) + (tid & 63);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = (int)(ty * MT_H) + (tid >> 6) + 4 * k;
        if (x < Wp && y < Hp) {
            const int l = labels[y * Wp + x];
            bool on = mode != 0;                                   // an unselected pixel: background in mode 0, tissue in mode 1
            if (l >= 0) {
                const int a = area[l];
                on = mode == 0 ? (a & MT_COUNT) >= limit : ((a & MT_COUNT) < limit && !(a & MT_BORDER));
            }
            dst[(int64_t)y * dpitch + x] = on ? (unsigned char)255 : (unsigned char)0;
        }
    }
}

}  // namespace toad

using namespace toad;

extern "C" int toad_plane_close_u8(const unsigned char *src, int64_t src_pitch, int Hp, int Wp, int thresh, int c, unsigned char *dst, int64_t dst_pitch,
                                   void *stream) {
    const char *what = "toad_plane_close_u8";
    if (!src || !dst) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_u8(what, "thresh", thresh)) return rc;
    if (c < 0 || c > 8) { set_error("%s: c = %d is not one of 0 .. 8", what, c); return TOAD_ESHAPE; }
    if (int rc = check_hw(what, "Hp", Hp, "Wp", Wp)) return rc;
    if (int rc = check_plane_pitches(what, Wp, src_pitch, dst_pitch)) return rc;
    if (int rc = check_no_overlap(what, src, src_pitch, dst, dst_pitch, Hp, Wp)) return rc;
    const int64_t ntx = ((int64_t)Wp + MT_W - 1) / MT_W, blocks = ntx * (((int64_t)Hp + MT_H - 1) / MT_H);
    if (int rc = check_blocks(what, "plane", blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
#define TOAD_CLOSE_LAUNCH(CC) \
    hipLaunchKernelGGL(plane_close_kernel<CC>, dim3((unsigned)blocks), dim3(256), 0, st, src, src_pitch, Hp, Wp, thresh, dst, dst_pitch, (unsigned)ntx)
    switch (c) {
        case 0: case 1: TOAD_CLOSE_LAUNCH(1); break;
        case 2: TOAD_CLOSE_LAUNCH(2); break;
        case 3: TOAD_CLOSE_LAUNCH(3); break;
        case 4: TOAD_CLOSE_LAUNCH(4); break;
        case 5: TOAD_CLOSE_LAUNCH(5); break;
        case 6: TOAD_CLOSE_LAUNCH(6); break;
        case 7: TOAD_CLOSE_LAUNCH(7); break;
        default: TOAD_CLOSE_LAUNCH(8); break;
    }
#undef TOAD_CLOSE_LAUNCH
    return check_launch(what);
}

extern "C" int toad_plane_components_u8(const unsigned char *plane, int64_t pitch, int Hp, int Wp, int thresh, int background, int *labels, int *area,
                                        void *stream) {
    const char *what = "toad_plane_components_u8";
    if (!plane || !labels || !area) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_u8(what, "thresh", thresh)) return rc;
    if (background != 0 && background != 1) { set_error("%s: background = %d must be 0 or 1", what, background); return TOAD_EINVAL; }
    if (int rc = check_hw(what, "Hp", Hp, "Wp", Wp)) return rc;
    if (int rc = check_plane_pitch(what, Wp, "pitch", pitch)) return rc;
    if (int rc = check_labels(what, Hp, Wp, labels, area, "the plane")) return rc;
    const int ntx = (Wp + MT_W - 1) / MT_W, nty = (Hp + MT_H - 1) / MT_H, blocks = ntx * nty;      // < 2^20
    const int nvl = (ntx - 1) * Hp, total = nvl + (nty - 1) * Wp;                                   // < 2^30 / 8
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)blocks), dim3(256), 0, st, plane, pitch, Hp, Wp, thresh, background, labels, area, (unsigned)ntx);
    if (total > 0)
        hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, labels, Hp, Wp, background == 0 ? 1 : 0, nvl, total);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)blocks), dim3(256), 0, st, labels, area, Hp, Wp, (unsigned)ntx);
    return check_launch(what);
}

extern "C" int toad_plane_area_select_u8(const int *labels, const int *area, int Hp, int Wp, int mode, int limit, unsigned char *dst, int64_t dst_pitch,
                                         void *stream) {
    const char *what = "toad_plane_area_select_u8";
    if (!labels || !area || !dst) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d must be 0 (drop small components) or 1 (fill small holes)", what, mode); return TOAD_EINVAL; }
    if (limit < 0) { set_error("%s: limit = %d must not be negative", what, limit); return TOAD_EINVAL; }
    if (int rc = check_hw(what, "Hp", Hp, "Wp", Wp)) return rc;
    if (int rc = check_plane_pitch(what, Wp, "dst_pitch", dst_pitch)) return rc;
    if (int rc = check_labels(what, Hp, Wp, labels, area, "dst")) return rc;
    const int ntx = (Wp + MT_W - 1) / MT_W, nty = (Hp + MT_H - 1) / MT_H;
    hipLaunchKernelGGL(area_select_kernel, dim3((unsigned)(ntx * nty)), dim3(256), 0, (hipStream_t)stream, labels, area, Hp, Wp, mode, limit, dst, dst_pitch,
                       (unsigned)ntx);
    return check_launch(what);
}
