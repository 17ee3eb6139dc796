// conv.hip — the truncated ResNet-50 feature extractor (models/resnet_custom.py:19-119 of the reference) in
// inference form, as the producer of the [N,1024] bags the MIL path consumes (BASELINE config 5).
//
// Design for gfx950: activations live in HBM as NHWC fp32, so every convolution is the NT product the MIL trunk
// already runs — Y[M, Cout] = act(cols[M, K] . Wf[Cout, K]^T + bf (+ residual)) with M = B*Ho*Wo pixels — in the
// same fp16 two-piece MFMA arithmetic (h2_arith.h; fp32-accurate, so the extractor keeps the 1e-4 parity bar):
// Cout >= 256 on the persistent 256x256 kernel, narrower layers, short-K residual expansions, the stem and the 3x3
// convolutions on the kernels of gemm_stream.inc (A streamed through registers; stride-1 3x3 with the activation halo
// in LDS) - those never materialise cols. Batch-norm (eval form) is folded into Wf / bf on the host; ReLU and the
// bottleneck's residual add ride in the GEMM epilogue. 1x1 stride-1 convolutions need no data movement at all (cols ==
// the NHWC activation); the explicit gathers below (16-B lanes, coalesced on the channel dimension) remain for strided
// 1x1 convolutions, for small batches of the 256-channel 3x3, and as API entry points.
//
// This is the extractor's translation unit (a launcher and its own kernels must share a TU without -fgpu-rdc), organised as:
//   h2_arith.h         the two-piece operand arithmetic and the persistent-grid constants, shared with the MIL unit (gemm_f32.hip)
//   gemm_narrow.inc    the narrow-N weight-plane format, convolution geometry and gather modes
//   gemm_stream.inc    narrow-N kernels: A streamed through registers; 3x3 convolutions with the activation halo in LDS
//   stem_halo.inc      stem + ReLU + max-pool as one kernel, straight from fp32 NCHW / uint8 NHWC tiles or a uint8 region
//   this file          the gathers and pools, the launchers of the kernels above with their kernel attributes (ext_cfg), the GEMM layer ext_* with
//                      the tensor-wide abs-max scalars, the 43-convolution sequencer trunc_fwd, the extern "C" entry points of include/toad_hip.h
// The wide GEMMs (Cout >= 256) are the one thing it takes from the MIL unit: launch_split_h2 / launch_nt_h2 and, as the last resort, launch_nt
// (common.h), each of which sets its own unit's kernel attributes.
#include "common.h"
#include "h2_arith.h"
#include "stem_u8.h"

#include <algorithm>
#include <mutex>
#include <type_traits>

namespace toad {

#include "gemm_narrow.inc"
#include "gemm_stream.inc"
#include "stem_halo.inc"

// ---- gathers ---------------------------------------------------------------------------------------------------
// cols[m, (ky*kw + kx)*C + c] = X[b, oy*s - p + ky, ox*s - p + kx, c]  (0 outside), m = (b*Ho + oy)*Wo + ox.
// One thread per 16-B chunk of a cols row; C % 4 == 0 so a chunk never straddles a tap.
__global__ __launch_bounds__(256) void im2col_nhwc_kernel(const float *__restrict__ X, float *__restrict__ cols, int B, int H,
                                                          int W, int C, int Ho, int Wo, int kh, int kw, int stride, int pad) {
    const uint32_t kq = (uint32_t)(kh * kw * C) >> 2, cq = (uint32_t)C >> 2;
    const uint64_t total = (uint64_t)B * Ho * Wo * kq;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t m = (uint32_t)(i / kq), j = (uint32_t)(i - (uint64_t)m * kq);
        const uint32_t tap = j / cq, c4 = j - tap * cq;
        const int ky = (int)(tap / (uint32_t)kw), kx = (int)(tap - (uint32_t)ky * kw);
        const uint32_t ox = m % (uint32_t)Wo, t = m / (uint32_t)Wo;
        const uint32_t oy = t % (uint32_t)Ho, b = t / (uint32_t)Ho;
        const int iy = (int)oy * stride - pad + ky, ix = (int)ox * stride - pad + kx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = ld4(X + (((uint64_t)b * H + iy) * W + ix) * C + 4 * c4);
        st4(cols + i * 4, v);
    }
}

// The stem: cols[m, c*49 + ky*7 + kx] (K = 147, zero-padded to Kp = 160) from NCHW tiles, 7x7 / stride 2 / pad 3.
// K keeps the reference's own weight order [Cout, Cin, kh, kw] (resnet_custom.py:62), so kx runs along W in memory.
__global__ __launch_bounds__(256) void im2col_stem_nchw_kernel(const float *__restrict__ X, float *__restrict__ cols, int B, int H,
                                                               int W, int Ho, int Wo) {
    constexpr uint32_t KQ = 40;        // 160 / 4
    const uint64_t total = (uint64_t)B * Ho * Wo * KQ;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t m = (uint32_t)(i / KQ), j = (uint32_t)(i - (uint64_t)m * KQ);
        const uint32_t ox = m % (uint32_t)Wo, t = m / (uint32_t)Wo;
        const uint32_t oy = t % (uint32_t)Ho, b = t / (uint32_t)Ho;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t k = 4 * j + e;
            float x = 0.f;
            if (k < 147) {
                const uint32_t c = k / 49, r = k - c * 49, ky = r / 7, kx = r - ky * 7;
                const int iy = (int)oy * 2 - 3 + (int)ky, ix = (int)ox * 2 - 3 + (int)kx;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) x = X[(((uint64_t)b * 3 + c) * H + iy) * W + ix];
            }
            v[e] = x;
        }
        st4(cols + i * 4, v);
    }
}

// Space-to-depth image of the stem: Xs[b, Y, X, (ry*2 + rx)*3 + c] = x[b, c, 2Y + ry - 4, 2X + rx - 4] (0 outside), Y < Ho + 3,
// X < Wo + 3. With it the 7x7 / stride-2 / pad-3 convolution (resnet_custom.py:62) becomes a 4x4 / stride-1 one whose K row
// for output pixel (oy, ox) is 4 window rows of 48 CONTIGUOUS floats (Xs[b, oy+qy, ox..ox+3, :]), i.e. something the GEMM's
// LDS-DMA can gather by itself: tap ky = 2*qy + ry - 1, kx = 2*qx + rx - 1 (the -1 slots carry zero weights). One thread per
// (b, Y, X): 12 reads that are pairwise adjacent in NCHW memory, 48 contiguous bytes written.
// gmax (optional): receives max |X| by atomic max (zeroed by the caller) - the image is the tiles' values plus zeros, so this IS the abs-max of the
// stem GEMM's operand and the separate pass over the tiles (74 us per 512 tiles) is not needed.
__global__ __launch_bounds__(256) void stem_s2d_kernel(const float *__restrict__ X, float *__restrict__ Xs, int B, int H, int W, int Hs, int Ws, float *gmax) {
    const uint64_t total = (uint64_t)B * Hs * Ws;
    float mx = 0.f;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t xs = (uint32_t)(i % (uint32_t)Ws), t = (uint32_t)(i / (uint32_t)Ws);
        const uint32_t ys = t % (uint32_t)Hs, b = t / (uint32_t)Hs;
        float v[12];
#pragma unroll
        for (int ry = 0; ry < 2; ++ry) {
            const int iy = 2 * (int)ys + ry - 4;
#pragma unroll
            for (int rx = 0; rx < 2; ++rx) {
                const int ix = 2 * (int)xs + rx - 4;
                const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[(ry * 2 + rx) * 3 + c] = ok ? X[(((uint64_t)b * 3 + c) * H + iy) * W + ix] : 0.f;
            }
        }
        float *dst = Xs + i * 12;
        st4(dst, f32x4{v[0], v[1], v[2], v[3]}); st4(dst + 4, f32x4{v[4], v[5], v[6], v[7]}); st4(dst + 8, f32x4{v[8], v[9], v[10], v[11]});
#pragma unroll
        for (int e = 0; e < 12; ++e) mx = __builtin_fmaxf(mx, __builtin_fabsf(v[e]));
    }
    if (gmax) {
        mx = h2_wave_max(mx);
        if ((threadIdx.x & 63) == 0 && mx > 0.f) h2_atomic_amax(gmax, mx);
    }
}

// nn.MaxPool2d(3, stride 2, padding 1) on NHWC (resnet_custom.py:66): padding never wins the max.
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc_kernel(const float *__restrict__ X, float *__restrict__ Y, int B, int H, int W,
                                                                int C, int Ho, int Wo) {
    const uint32_t cq = (uint32_t)C >> 2;
    const uint64_t total = (uint64_t)B * Ho * Wo * cq;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t m = (uint32_t)(i / cq), c4 = (uint32_t)(i - (uint64_t)m * cq);
        const uint32_t ox = m % (uint32_t)Wo, t = m / (uint32_t)Wo;
        const uint32_t oy = t % (uint32_t)Ho, b = t / (uint32_t)Ho;
        const float ninf = -__builtin_huge_valf();
        f32x4 best = {ninf, ninf, ninf, ninf};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = (int)oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = (int)ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const f32x4 v = ld4(X + (((uint64_t)b * H + iy) * W + ix) * C + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) best[e] = v[e] > best[e] ? v[e] : best[e];
            }
        }
        st4(Y + i * 4, best);
    }
}

// nn.AdaptiveAvgPool2d(1) + flatten (resnet_custom.py:70,104-105): feat[b, c] = mean over the HW pixels of X[b, :, c].
// Block = (tile b, 256 channels): 4 pixel groups x 64 lanes x 16 B; fixed-order LDS combine -> deterministic.
// H16: the bag row is stored as fp16, rn16 of the fp32 mean (feature stores kept in half precision: the *_x16 calls of the MIL path read it as stored).
template <bool H16>
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const float *__restrict__ X, void *__restrict__ feat_v, int HW, int C) {
    __shared__ f32x4 part[4][64];
    const int b = blockIdx.y, c0 = blockIdx.x * 256;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const bool live = c0 + 4 * lane < C;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float *p = X + (uint64_t)b * HW * C + c0 + 4 * lane;
        for (int px = grp; px < HW; px += 4) acc += ld4(p + (uint64_t)px * C);
    }
    part[grp][lane] = acc;
    __syncthreads();
    if (grp == 0 && live) {
        const f32x4 s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        const float inv = 1.f / (float)HW;
        const f32x4 m = s * inv;
        const uint64_t o = (uint64_t)b * C + c0 + 4 * lane;
        if constexpr (H16) {
            typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<h16x4 *>(reinterpret_cast<_Float16 *>(feat_v) + o) = h16x4{(_Float16)m[0], (_Float16)m[1], (_Float16)m[2], (_Float16)m[3]};
        } else {
            st4(reinterpret_cast<float *>(feat_v) + o, m);
        }
    }
}

// uint8 NHWC tiles [B, H, W, 3] (RGB, as an image decoder hands them over) -> the normalised fp32 NCHW tiles [B, 3, H, W] the reference model is fed:
// out[b, c, p] = fmaf((float)u[b, p, c], a_c, b_c), a_c = 1 / (255 std_c), b_c = -mean_c / std_c - ToTensor + Normalize in one rounding (the explicit fma:
// this library is built with -ffp-contract=fast). One thread per group of four pixels of one image: 12 source bytes (three 4-byte loads where the group's
// address allows it, byte loads otherwise - any base alignment, no read past the group), one 16-byte store per channel plane when HW % 4 == 0 (the
// planes are then 16-byte aligned like `out`), scalar stores otherwise and in a ragged last group.
// REGION: the tiles are read by origin from one decoded image (src = uint8 [Hr, Wr, 3] with a row pitch in bytes, origins = int32 [B][2] = (x, y) of tile b's
// top-left pixel): pixel p of tile b is at src + (y_b + p / W) pitch + (x_b + p % W) 3. A group that lies in one tile row is 12 contiguous bytes as above;
// one that wraps into the next row takes its pixels one by one. Only bytes of the tile are read; the values and the stores are those of the tile form.
// SHRINK == 2 (REGION only): tile b is the (2 H, 2 W) footprint at its origin and pixel p of the H x W tile the integer mean of its 2 x 2 box,
// (sum + 2) >> 2 - the tile toad::stem_halo_pool_kernel<SH_U8_REGION_BOX2> sees - read byte by byte (this is the staged route, not the hot one); the fma and
// the stores are the tile form's.
// LIST (REGION only): the tiles are read from a list of regions (src is not used): rg.tiles = int32 [B][3] = (x, y, k), the top-left pixel of tile b in the
// coordinates of region k, and rg.r[k] = {base, pitch} of that region, by value in the kernel argument like the stem's (stem_halo.inc). Here b differs from
// thread to thread, so the descriptor is read per lane; from the tile's base on the code is the region form's.
struct TilesNoRegion {};
struct TilesRegionArg { int64_t pitch; const int *origins; uint32_t W; };
struct TilesRegionsArg { const int *tiles; uint32_t W; StemRegionDesc r[STEM_REGIONS_MAX]; };
template <bool REGION, bool LIST> struct TilesLastArg { typedef TilesNoRegion type; };
template <> struct TilesLastArg<true, false> { typedef TilesRegionArg type; };
template <> struct TilesLastArg<true, true> { typedef TilesRegionsArg type; };
template <bool REGION, int SHRINK = 1, bool LIST = false>
__global__ __launch_bounds__(256) void tiles_u8_nhwc_to_nchw_kernel(const unsigned char *__restrict__ src, float *__restrict__ out, uint64_t B, uint32_t HW,
                                                                    StemNorm nrm, typename TilesLastArg<REGION, LIST>::type rg) {
    static_assert(REGION || !LIST, "a list of regions is a region form");
    const uint32_t gpi = (HW + 3) >> 2;                                   // groups per image
    const uint64_t total = B * gpi;
    const bool vec = (HW & 3u) == 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t b = i / gpi;
        const uint32_t p0 = (uint32_t)(i - b * gpi) * 4, np = HW - p0 < 4 ? HW - p0 : 4;
        const unsigned char *s, *tile = nullptr;
        bool one_run = true;                                              // the group's 3 np bytes are contiguous
        int64_t pitch = 0;                                                // the row pitch of the tile's region
        if constexpr (REGION) {
            const uint32_t y0 = p0 / rg.W, x0 = p0 - y0 * rg.W;
            if constexpr (LIST) {
                const int *t3 = rg.tiles + 3 * b;
                const StemRegionDesc &d = rg.r[t3[2]];
                pitch = d.pitch;
                tile = d.base + (uint64_t)(uint32_t)t3[1] * (uint64_t)pitch + (uint64_t)(uint32_t)t3[0] * 3;
            } else {
                pitch = rg.pitch;
                tile = src + (uint64_t)(uint32_t)rg.origins[2 * b + 1] * (uint64_t)pitch + (uint64_t)(uint32_t)rg.origins[2 * b] * 3;
            }
            s = tile + (uint64_t)y0 * (uint64_t)pitch + x0 * 3;
            one_run = x0 + np <= rg.W;
        } else {
            s = src + (b * HW + p0) * 3;
        }
        unsigned u[12];
        if constexpr (SHRINK == 2) {
            // pixel (ye, xe) of the tile = the mean, rounded half up, of the 2 x 2 box at rows 2 ye, 2 ye + 1, bytes [6 xe, 6 xe + 6) of the footprint
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t pe = p0 + e, ye = pe / rg.W, xe = pe - ye * rg.W;
                const unsigned char *q = tile + (uint64_t)(2 * ye) * (uint64_t)pitch + xe * 6;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    u[3 * e + c] = (uint32_t)e < np ? ((unsigned)q[c] + q[3 + c] + q[pitch + c] + q[pitch + 3 + c] + 2u) >> 2 : 0u;
            }
        } else if (!one_run) {
            if constexpr (REGION) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t pe = p0 + e, ye = pe / rg.W, xe = pe - ye * rg.W;
                    const unsigned char *q = tile + (uint64_t)ye * (uint64_t)pitch + xe * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) u[3 * e + c] = (uint32_t)e < np ? q[c] : 0u;
                }
            }
        } else if (np == 4 && (reinterpret_cast<uintptr_t>(s) & 3u) == 0) {
            const unsigned w0 = reinterpret_cast<const unsigned *>(s)[0], w1 = reinterpret_cast<const unsigned *>(s)[1], w2 = reinterpret_cast<const unsigned *>(s)[2];
#pragma unroll
            for (int e = 0; e < 4; ++e) { u[e] = (w0 >> (8 * e)) & 255u; u[4 + e] = (w1 >> (8 * e)) & 255u; u[8 + e] = (w2 >> (8 * e)) & 255u; }
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) u[e] = (uint32_t)e < 3 * np ? s[e] : 0u;
        }
        float *o = out + b * 3 * HW + p0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf((float)u[3 * e + c], nrm.a[c], nrm.b[c]);
            float *oc = o + (uint64_t)c * HW;
            if (vec) st4(oc, v);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) if ((uint32_t)e < np) oc[e] = v[e];
        }
    }
}

// ---- host side of the extractor's GEMMs ------------------------------------------------------------------------
// Residual GEMMs with a reduction of at most this many elements run on the narrow (streamed) tiles whatever their width: measured
// (tools/gemm_shape_bench.py, same box) M=262144 K=64 N=256 +residual 170 -> 133 us; K=128 equal, K=256 slower (A is re-split per
// 128-column tile)
constexpr int kNarrowResKmax = 64;
// One-time initialisation of this translation unit: the attributes (dynamic LDS sizes) of the extractor's own kernels, completed before the first
// launch of any of them from any thread (launch_narrow_t, stem_pool_from_tiles). The MIL kernels' attributes are gemm_f32.hip's (cfg()).
static std::once_flag g_ext_cfg_once;
static void ext_cfg() {
    std::call_once(g_ext_cfg_once, [] {
#define TOAD_ATTR(K, BYTES) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES)
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 2, GATHER_NONE>), (StreamCfg<2, 2>::SMEM));
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 4, GATHER_NONE>), (StreamCfg<2, 4>::SMEM));
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 2, GATHER_CONV>), (StreamCfg<2, 2>::SMEM));
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 4, GATHER_CONV>), (StreamCfg<2, 4>::SMEM));
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 2, GATHER_STEM>), (StreamCfg<2, 2>::SMEM));
        TOAD_ATTR((gemm_nt_h2_stream_kernel<2, 2, GATHER_STEM_POOL>), (StreamCfg<2, 2>::SMEM + STEM_POOL_LDS));
        TOAD_ATTR(stem_halo_pool_kernel<SH_F32>, SH_SMEM);
        TOAD_ATTR(stem_halo_pool_kernel<SH_U8>, SH_SMEM);
        TOAD_ATTR(stem_halo_pool_kernel<SH_U8_REGION>, SH_SMEM);
        TOAD_ATTR(stem_halo_pool_kernel<SH_U8_REGION_BOX2>, SH_SMEM);
        TOAD_ATTR(stem_halo_pool_kernel<SH_U8_REGIONS>, SH_SMEM);
        TOAD_ATTR(stem_halo_pool_kernel<SH_U8_REGIONS_BOX2>, SH_SMEM);
        TOAD_ATTR(conv3x3_h2_halo_kernel<2>, 160 * 1024);
        TOAD_ATTR(conv3x3_h2_halo_kernel<4>, 160 * 1024);
#undef TOAD_ATTR
    });
}

// max |x| over n floats -> out[0] (bit pattern of a non-negative float, zeroed here): the tensor-wide abs-max a narrow / extractor GEMM
// scales its A operand with when no producer handed one over (the per-op entry points; inside toad_resnet50_trunc_fwd_f32 every
// producer emits it)
__global__ __launch_bounds__(256) void gmax_kernel(const float *__restrict__ x, int64_t n4, float *__restrict__ out) {
    __shared__ float s[4];
    float mx = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        mx = __builtin_fmaxf(mx, h2_absmax4(__builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(x) + i)));
    mx = h2_wave_max(mx);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) h2_atomic_amax(out, __builtin_fmaxf(__builtin_fmaxf(s[0], s[1]), __builtin_fmaxf(s[2], s[3])));
}
int launch_gmax(const float *x, int64_t n, float *out, hipStream_t st, const char *what) {
    (void)hipMemsetAsync(out, 0, sizeof(float), st);
    int64_t grid = (n / 4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gmax_kernel, dim3((unsigned)grid), dim3(256), 0, st, x, n / 4, out);
    return check_launch(what);
}

// C[M,N] = act(A' W^T + bias + addend) with N <= 128 on the narrow kernels; A' = A[M,K] (MODE = GATHER_NONE) or the implicit
// im2col of the NHWC activation A described by cg. `ws` as for launch_nt (planes and inverse scales live behind the slab area).
// a_gmax: device scalar max |A| (of the whole activation); y_gmax (optional): receives max |C| by atomic max (zeroed by the caller).
template <int RA, int NB, int MODE>
static int launch_narrow_t(const float *A, int64_t lda, const float *a_gmax, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t M, int64_t N,
                           int64_t K, const float *bias, int relu, const float *addend, const ConvGeom &cg, float *y_gmax, void *ws,
                           hipStream_t st, const char *what) {
    ext_cfg();
    char *w = reinterpret_cast<char *>(ws) + (size_t)PB_GRID * PB * PB * sizeof(float);
    constexpr int TNW = NB * 32;         // tile width (RA only names the instantiation; the streamed kernels run 64-row wave tiles)
    const int tiles_n = (int)((N + TNW - 1) / TNW);
    unsigned short *planes = reinterpret_cast<unsigned short *>(w);
    float *binv;
    // the streamed kernel walks an implicit convolution's k-stages channel-chunk outer, tap inner (gemm_stream.inc): its planes are split in that order
    const int taps = MODE == GATHER_CONV ? (int)(K / cg.C) : 1;
    const int nk = (int)(K / BK), nkp = (nk + 1) & ~1;                  // the streamed kernel walks k-stages in pairs: an odd count gets a zero stage
    binv = reinterpret_cast<float *>(w + (size_t)tiles_n * TNW * (size_t)nkp * BK * 4);
    hipLaunchKernelGGL(split_planes_narrow_h2_kernel<NB>, dim3((tiles_n * TNW + 3) / 4), dim3(256), 0, st, W, ldw, planes, binv, (int)N, (int)K, tiles_n,
                       taps, cg.C, nkp);
    if (int rc = check_launch(what)) return rc;
    if (MODE == GATHER_CONV) {       // 3x3 / 1 / 1 with whole 256-pixel row blocks: the activation halo lives in LDS (gemm_stream.inc)
        const int W = cg.W, H = cg.H;
        const bool shape = cg.kw == 3 && K == 9 * (int64_t)cg.C && cg.stride == 1 && cg.pad == 1 && cg.Ho == H && cg.Wo == W && W >= 8 && W <= 128 &&
                           (W & (W - 1)) == 0 && H % (256 / W) == 0 && cg.C % BK == 0 && M % 256 == 0;
        if (shape) {
            using HCfg = HaloCfg<NB>;
            const int hb = HCfg::halo_bytes(W);
            hipLaunchKernelGGL(conv3x3_h2_halo_kernel<NB>, dim3(2 * PB_GRID), dim3(HCfg::THREADS), HCfg::smem(W), st, A, a_gmax, planes, binv, C, ldc, (int)M, (int)N,
                               (int)K, bias, relu, addend, cg, y_gmax, (int)(M / 256), tiles_n, hb);
            return check_launch(what);
        }
    }
    // A streamed through registers (gemm_stream.inc): wave tile 64 x 64 / 64 x 128
    constexpr int SRA = 2;
    using SCfg = StreamCfg<SRA, NB>;
    const int stiles_m = (int)((M + SCfg::TM - 1) / SCfg::TM);
    if constexpr (MODE == GATHER_STEM_POOL) {        // C = the POOLED output; every workgroup a contiguous range of row-pair tiles (ext_stem_conv checked the geometry)
        hipLaunchKernelGGL((gemm_nt_h2_stream_kernel<SRA, NB, MODE>), dim3(std::min(stiles_m, SCfg::WG_PER_CU * PB_GRID)), dim3(SCfg::THREADS), SCfg::SMEM + STEM_POOL_LDS, st,
                           A, lda, a_gmax, planes, binv, C, ldc, (int)M, (int)N, (int)K, bias, relu, addend, cg, y_gmax, stiles_m, tiles_n);
        return check_launch(what);
    }
    hipLaunchKernelGGL((gemm_nt_h2_stream_kernel<SRA, NB, MODE>), dim3(SCfg::WG_PER_CU * PB_GRID), dim3(SCfg::THREADS), SCfg::SMEM, st, A, lda, a_gmax, planes, binv,
                       C, ldc, (int)M, (int)N, (int)K, bias, relu, addend, cg, y_gmax, stiles_m, tiles_n);
    return check_launch(what);
}

static bool narrow_ok(int64_t M, int64_t N, int64_t K, int64_t ldc, const float *bias, const float *addend, void *ws) {
    const bool wide_ok = addend && K <= kNarrowResKmax;       // residual GEMMs with a short reduction: epilogue-bound, see DESIGN 10
    return ws && (N <= 128 || wide_ok) && N % 4 == 0 && K % BK == 0 && ldc % 4 == 0 && M < (1ll << 31) &&
           (!bias || aligned16(bias)) && (!addend || aligned16(addend));
}

// ---- the extractor's GEMMs (models/resnet_custom.py:19-119 as NHWC GEMMs, conv.hip): Y = act(X' W^T + bias + residual) -------------
// x_gmax: device scalar max |X| of the whole activation (NULL: measured here, one extra read); y_gmax: device scalar that receives
// max |Y| by atomic max (the caller zeroed it; NULL: not wanted). One tensor-wide power-of-two scale per activation: gemm_narrow.inc.
static float *ext_scratch_scalar(void *ws, int64_t M, int64_t N, int64_t K) {          // a float inside the workspace's abs-max area
    const size_t tiles_n = (size_t)((N + PB - 1) / PB), kpad = (size_t)((K + 2 * BK - 1) / (2 * BK) * (2 * BK));        // as toad_linear_ws_bytes
    return reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + (size_t)PB_GRID * PB * PB * sizeof(float) + tiles_n * PB * kpad * 6 + tiles_n * PB * sizeof(float)) + 8;
}
int ext_linear(const float *X, const float *x_gmax, const float *W, const float *bias, const float *residual, float *Y, float *y_gmax,
                     int64_t M, int64_t K, int64_t N, int act, void *ws, size_t ws_bytes, hipStream_t st, const char *what) {
    if (!X || !W || !Y) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (act != TOAD_ACT_NONE && act != TOAD_ACT_RELU) { set_error("%s: bad act %d", what, act); return TOAD_EINVAL; }
    if (M <= 0 || N <= 0 || K <= 0) { set_error("%s: non-positive dimension", what); return TOAD_EINVAL; }
    if (residual && (N % 4 != 0 || !aligned16(residual))) { set_error("%s: residual needs N %% 4 == 0 and 16-byte alignment", what); return TOAD_ESHAPE; }
    if (int rc = check_ws(ws, ws_bytes, M, N, K, what)) return rc;
    EpiScalars es{act == TOAD_ACT_RELU, 1.f, make_drop(0.f, 0)};
    const bool narrow = narrow_ok(M, N, K, N, bias, residual, ws) && (uint64_t)M * K * 4 < (1ull << 32);
    const bool big = !narrow && ws && h2_nt_ok(M, N, K, K, N);
    if ((narrow || big) && !x_gmax) {
        float *g = ext_scratch_scalar(ws, M, N, K);
        if (int rc = launch_gmax(X, M * K, g, st, what)) return rc;
        x_gmax = g;
    }
    if (narrow) {
        const ConvGeom none{0, 0, 0, 0, 0, 0, 0, 0};
        if (N <= 64) return launch_narrow_t<2, 2, GATHER_NONE>(X, K, x_gmax, W, K, Y, N, M, N, K, bias, es.relu, residual, none, y_gmax, ws, st, what);
        return launch_narrow_t<1, 4, GATHER_NONE>(X, K, x_gmax, W, K, Y, N, M, N, K, bias, es.relu, residual, none, y_gmax, ws, st, what);
    }
    if (big) {
        // wide outputs (1x1 expansions / downsamples, the 256-channel 3x3 after im2col): the persistent 256x256 kernel of the MIL path
        // with the tensor-wide scalars in place of its per-block abs-max arrays (stride 0)
        if (!aligned16(X) || !aligned16(W) || !aligned16(Y) || (bias && !aligned16(bias))) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
        char *w = reinterpret_cast<char *>(ws);
        float *slabs = reinterpret_cast<float *>(w);
        w += (size_t)PB_GRID * PB * PB * sizeof(float);
        unsigned short *planes = reinterpret_cast<unsigned short *>(w);
        w += h2_planes_bytes(N, K);
        float *binv = reinterpret_cast<float *>(w);
        const H2Operand op{W, K, 1, N, K, planes, binv};
        if (int rc = launch_split_h2(&op, 1, nullptr, 0, st, what)) return rc;
        // short reductions: a tile is a few k-steps of matrix work followed by 256-512 KB of epilogue traffic, and 256 workgroups in phase make
        // the GEMM the SUM of the two. Spread the starts over one expected tile period (10 ns ticks: ~1.95 us per k-step, ~8 us per 256 KB of
        // epilogue traffic; measured on the extractor's shapes, tools/ab/duo_ext_bench.py: -8..-10 % on the residual GEMMs, neutral from K = 1024)
        if (K <= 512 && M >= 32 * 1024) es.stagger = (int)std::min<int64_t>((K / BK) * 195 + (residual ? 1600 : 800), 3000);
        return launch_nt_h2(X, K, x_gmax, planes, binv, Y, N, M, N, K, bias, es, residual, nullptr, nullptr, H2Pool{nullptr, nullptr, nullptr, 0}, slabs,
                            y_gmax, nullptr, st, what, TOAD_X_F32, 0, 0);
    }
    if (int rc = launch_nt(X, K, W, K, Y, N, M, N, K, bias, es, residual, nullptr, ws, st, what)) return rc;
    return y_gmax ? launch_gmax(Y, M * N, y_gmax, st, what) : TOAD_OK;
}

int ext_conv_nhwc(const float *X, const float *x_gmax, const float *Wf, const float *bias, const float *residual, float *Y, float *y_gmax, int B,
                        int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, int act, void *ws, size_t ws_bytes, hipStream_t st,
                        const char *what) {
    if (!X || !Wf || !Y || !ws) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (act != TOAD_ACT_NONE && act != TOAD_ACT_RELU) { set_error("%s: bad act %d", what, act); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || pad > 8 || H + 8 >= 32768 || W + 8 >= 32768) { set_error("%s: bad geometry", what); return TOAD_ESHAPE; }
    if (Cin <= 0 || Cin % BK != 0) { set_error("%s: Cin must be a multiple of %d (use toad_im2col_nhwc_f32 + toad_linear_act_res_fwd_f32 otherwise)", what, BK); return TOAD_ESHAPE; }
    if (Cout <= 0 || Cout > 512 || Cout % 4 != 0) { set_error("%s: implicit path needs Cout <= 512, a multiple of 4 (use im2col + linear for wider layers)", what); return TOAD_ESHAPE; }
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    if (Ho < 1 || Wo < 1) { set_error("%s: empty output", what); return TOAD_ESHAPE; }
    const int64_t M = (int64_t)B * Ho * Wo, K = (int64_t)kh * kw * Cin;
    if ((uint64_t)B * H * W * Cin * 4 >= (1ull << 31) || M >= (1ll << 31)) { set_error("%s: activation too large for 32-bit offsets (split the batch)", what); return TOAD_ESHAPE; }
    if (!aligned16(X) || !aligned16(Wf) || !aligned16(Y)) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (int rc = check_ws(ws, ws_bytes, M, Cout, K, what)) return rc;
    if (!narrow_ok(M, Cout <= 128 ? Cout : 128, K, Cout, bias, residual, ws)) { set_error("%s: bias / residual must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (!x_gmax) {
        float *g = ext_scratch_scalar(ws, M, Cout, K);
        if (int rc = launch_gmax(X, (int64_t)B * H * W * Cin, g, st, what)) return rc;
        x_gmax = g;
    }
    const ConvGeom cg{H, W, Cin, Ho, Wo, kw, stride, pad};
    if (Cout <= 64)
        return launch_narrow_t<2, 2, GATHER_CONV>(X, 0, x_gmax, Wf, K, Y, Cout, M, Cout, K, bias, act == TOAD_ACT_RELU, residual, cg, y_gmax, ws, st, what);
    return launch_narrow_t<1, 4, GATHER_CONV>(X, 0, x_gmax, Wf, K, Y, Cout, M, Cout, K, bias, act == TOAD_ACT_RELU, residual, cg, y_gmax, ws, st, what);
}

bool stem_pool_ok(int Ho, int Wo, int act) { return Wo == 128 && Ho > 0 && Ho % 2 == 0 && act == TOAD_ACT_RELU; }   // the stem may take the 3x3/2 max-pool into its epilogue (gemm_stream.inc)
int ext_stem_conv(const float *Xs, const float *x_gmax, const float *Wf, const float *bias, float *Y, float *y_gmax, int B, int Ho, int Wo, int act,
                  void *ws, size_t ws_bytes, hipStream_t st, const char *what, bool pooled = false) {
    if (!Xs || !Wf || !Y || !ws) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (act != TOAD_ACT_NONE && act != TOAD_ACT_RELU) { set_error("%s: bad act %d", what, act); return TOAD_EINVAL; }
    if (B <= 0 || Ho <= 0 || Wo <= 0) { set_error("%s: bad geometry", what); return TOAD_ESHAPE; }
    const int Hs = Ho + 3, Ws = Wo + 3;
    const int64_t M = (int64_t)B * Ho * Wo;
    if ((uint64_t)B * Hs * Ws * 48 >= (1ull << 31) || M >= (1ll << 31)) { set_error("%s: batch too large for 32-bit offsets (split it)", what); return TOAD_ESHAPE; }
    if (!aligned16(Xs) || !aligned16(Wf) || !aligned16(Y)) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (int rc = check_ws(ws, ws_bytes, M, 64, 192, what)) return rc;
    if (!narrow_ok(M, 64, 192, 64, bias, nullptr, ws)) { set_error("%s: bias must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (!x_gmax) {
        float *g = ext_scratch_scalar(ws, M, 64, 192);
        if (int rc = launch_gmax(Xs, (int64_t)B * Hs * Ws * 12, g, st, what)) return rc;
        x_gmax = g;
    }
    const ConvGeom cg{Hs, Ws, 12, Ho, Wo, 0, 0, 0};
    if (pooled) {
        // the 3x3/2 max-pool in the stem's epilogue (gemm_stream.inc): a tile = two whole image rows, ReLU outputs
        if (!stem_pool_ok(Ho, Wo, act)) { set_error("%s: the pooled stem needs Wo = 128, an even Ho and ReLU", what); return TOAD_ESHAPE; }
        return launch_narrow_t<2, 2, GATHER_STEM_POOL>(Xs, 0, x_gmax, Wf, 192, Y, 64, M, 64, 192, bias, 1, nullptr, cg, y_gmax, ws, st, what);
    }
    return launch_narrow_t<2, 2, GATHER_STEM>(Xs, 0, x_gmax, Wf, 192, Y, 64, M, 64, 192, bias, act == TOAD_ACT_RELU, nullptr, cg, y_gmax, ws, st, what);
}

// The stem + ReLU + 3x3/2 max-pool straight from the tiles (stem_halo.inc): no space-to-depth image, no fragment loads from global memory. norm == NULL: fp32 NCHW
// tiles; otherwise uint8 NHWC tiles [B, H, 256, 3] and the six normalisation constants (stem_u8.h), checked before any device work. rg != NULL: the uint8 tiles
// are read by origin from rg->region (X is not used; no alignment requirement on the region); with shrink == 2 tile b is the (2 H, 512) footprint at its origin,
// box-filtered by the window loader (H, W stay the network tile's).
bool stem_nchw_pool_ok(int H, int W) { return W == 256 && H >= 4 && H % 4 == 0; }     // the shapes it takes
static int stem_pool_from_tiles(const void *X, bool u8, const float *norm, const float *Wf, const float *bias, float *Yp, float *y_gmax, int B, int H, int W, void *ws,
                                size_t ws_bytes, hipStream_t st, const char *what, const RegionSrc *rg = nullptr, int shrink = 1) {
    if (rg) X = rg->region;
    if (!X || (u8 && !norm) || !Wf || !Yp || !ws || (rg && !rg->origins)) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    const bool list = rg && rg->list;                                // a list of regions is checked in front of B and the tile shape (include/toad_hip.h)
    if (list) { if (int rc = check_region_u8(*rg, H, W, what, shrink)) return rc; }
    if (B <= 0 || !stem_nchw_pool_ok(H, W)) {
        set_error("%s: needs W = 256 and H %% 4 == 0 (other tiles: %stoad_stem_s2d_nchw_f32 + toad_stem_conv_s2d_f32 + toad_maxpool3x3s2_nhwc_f32)", what,
                  list ? "toad_tiles_u8_regions_to_nchw_f32 + " : rg ? "toad_tiles_u8_region_to_nchw_f32 + " : u8 ? "toad_tiles_u8_nhwc_to_nchw_f32 + " : "");
        return TOAD_ESHAPE;
    }
    if (rg && !list) { if (int rc = check_region_u8(*rg, H, W, what, shrink)) return rc; }
    const int64_t M = (int64_t)B * (H / 2) * 128;
    if (M >= (1ll << 31)) { set_error("%s: batch too large for 32-bit offsets (split it)", what); return TOAD_ESHAPE; }
    if (u8) { if (int rc = check_norm_u8(norm, what)) return rc; }
    if (u8 && !rg && (reinterpret_cast<uintptr_t>(X) & 1u) != 0) { set_error("%s: the uint8 tiles must be 2-byte aligned", what); return TOAD_EALIGN; }
    if ((!u8 && !aligned16(X)) || !aligned16(Wf) || !aligned16(Yp) || (bias && !aligned16(bias))) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (int rc = check_ws(ws, ws_bytes, M, 64, 192, what)) return rc;
    ext_cfg();
    char *w = reinterpret_cast<char *>(ws) + (size_t)PB_GRID * PB * PB * sizeof(float);
    unsigned short *planes = reinterpret_cast<unsigned short *>(w);
    float *binv = reinterpret_cast<float *>(w + (size_t)64 * 6 * BK * 4);
    hipLaunchKernelGGL(split_planes_narrow_h2_kernel<2>, dim3(16), dim3(256), 0, st, Wf, (int64_t)192, planes, binv, 64, 192, 1, 1, 12, 6);
    if (int rc = check_launch(what)) return rc;
    const int tiles = B * (H / 4);
    const dim3 grid(std::min(tiles, 2 * PB_GRID));                  // two workgroups per CU
    if (u8) {
        StemNorm nrm;
        for (int c = 0; c < 3; ++c) { nrm.a[c] = norm[c]; nrm.b[c] = norm[3 + c]; }
        if (list) {
            StemRegionsArg la;
            la.nrm = nrm; la.tiles = rg->origins;
            fill_region_descs(*rg, la.r);
            if (shrink == 2)
                hipLaunchKernelGGL(stem_halo_pool_kernel<SH_U8_REGIONS_BOX2>, grid, dim3(256), SH_SMEM, st, static_cast<const unsigned char *>(nullptr), planes, binv, bias, Yp, B, H,
                                   y_gmax, tiles, la);
            else
                hipLaunchKernelGGL(stem_halo_pool_kernel<SH_U8_REGIONS>, grid, dim3(256), SH_SMEM, st, static_cast<const unsigned char *>(nullptr), planes, binv, bias, Yp, B, H,
                                   y_gmax, tiles, la);
        } else if (rg && shrink == 2)
            hipLaunchKernelGGL(stem_halo_pool_kernel<SH_U8_REGION_BOX2>, grid, dim3(256), SH_SMEM, st, rg->region, planes, binv, bias, Yp, B, H, y_gmax, tiles,
                               StemRegionArg{nrm, (int)rg->pitch, rg->origins});
        else if (rg)
            hipLaunchKernelGGL(stem_halo_pool_kernel<SH_U8_REGION>, grid, dim3(256), SH_SMEM, st, rg->region, planes, binv, bias, Yp, B, H, y_gmax, tiles,
                               StemRegionArg{nrm, (int)rg->pitch, rg->origins});
        else
            hipLaunchKernelGGL(stem_halo_pool_kernel<SH_U8>, grid, dim3(256), SH_SMEM, st, reinterpret_cast<const unsigned char *>(X), planes, binv, bias, Yp, B, H, y_gmax, tiles, nrm);
    } else {
        hipLaunchKernelGGL(stem_halo_pool_kernel<SH_F32>, grid, dim3(256), SH_SMEM, st, reinterpret_cast<const float *>(X), planes, binv, bias, Yp, B, H, y_gmax, tiles, StemNoNorm{});
    }
    return check_launch(what);
}
int ext_stem_nchw_pool(const float *X, const float *Wf, const float *bias, float *Yp, float *y_gmax, int B, int H, int W, void *ws, size_t ws_bytes,
                       hipStream_t st, const char *what) {
    return stem_pool_from_tiles(X, false, nullptr, Wf, bias, Yp, y_gmax, B, H, W, ws, ws_bytes, st, what);
}
int ext_stem_nhwc_u8_pool(const unsigned char *X8, const float *norm, const float *Wf, const float *bias, float *Yp, float *y_gmax, int B, int H, int W,
                          void *ws, size_t ws_bytes, hipStream_t st, const char *what) {
    return stem_pool_from_tiles(X8, true, norm, Wf, bias, Yp, y_gmax, B, H, W, ws, ws_bytes, st, what);
}
int ext_stem_region_u8_pool(const RegionSrc &rg, const float *norm, const float *Wf, const float *bias, float *Yp, float *y_gmax, int B, int H, int W, void *ws,
                            size_t ws_bytes, hipStream_t st, const char *what, int shrink = 1) {
    return stem_pool_from_tiles(nullptr, true, norm, Wf, bias, Yp, y_gmax, B, H, W, ws, ws_bytes, st, what, &rg, shrink);
}

static int grid_for(uint64_t threads) {
    uint64_t g = (threads + 255) / 256;
    const uint64_t cap = 256 * 32;                     // 32 blocks per CU is plenty for a streaming gather
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

static inline int conv_out(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }

// ---- the network plan (shared by the workspace query and the sequencer) -----------------------------------------
struct ConvSpec { int cin, cout, k, stride, pad; };
constexpr int kNumConvs = 43;
struct NetPlan {
    ConvSpec conv[kNumConvs];
    size_t act_max, cols_max, gemm_ws;    // floats, floats, bytes
    int Hs, Ws, Hp, Wp;                   // stem and max-pool output sizes
};
static const int kPlanes[3] = {64, 128, 256}, kBlocks[3] = {3, 4, 6}, kStride[3] = {1, 2, 2};

static bool make_plan(int B, int H, int W, NetPlan &p) {
    if (B <= 0 || H < 1 || W < 1) return false;
    int n = 0;
    p.conv[n++] = {3, 64, 7, 2, 3};
    p.Hs = conv_out(H, 7, 2, 3); p.Ws = conv_out(W, 7, 2, 3);
    p.Hp = conv_out(p.Hs, 3, 2, 1); p.Wp = conv_out(p.Ws, 3, 2, 1);
    if (p.Hs < 1 || p.Ws < 1 || p.Hp < 1 || p.Wp < 1) return false;
    size_t act = (size_t)B * p.Hs * p.Ws * 64, cols = (size_t)B * (p.Hs + 3) * (p.Ws + 3) * 12, gws = toad_linear_ws_bytes((int64_t)B * p.Hs * p.Ws, 64, 192);
    auto upd = [&](size_t M, int cout, int K, bool gathered) {
        if (M * cout > act) act = M * cout;
        if (gathered && M * K > cols) cols = M * K;
        const size_t w = toad_linear_ws_bytes((int64_t)M, cout, K);
        if (w > gws) gws = w;
    };
    int h = p.Hp, w = p.Wp, inpl = 64;
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < kBlocks[l]; ++b) {
            const int s = b == 0 ? kStride[l] : 1, pl = kPlanes[l];
            const int ho = conv_out(h, 3, s, 1), wo = conv_out(w, 3, s, 1);
            p.conv[n++] = {inpl, pl, 1, 1, 0};     upd((size_t)B * h * w, pl, inpl, false);
            p.conv[n++] = {pl, pl, 3, s, 1};       upd((size_t)B * ho * wo, pl, 9 * pl, true);
            p.conv[n++] = {pl, 4 * pl, 1, 1, 0};   upd((size_t)B * ho * wo, 4 * pl, pl, false);
            if (b == 0) { p.conv[n++] = {inpl, 4 * pl, 1, s, 0}; upd((size_t)B * ho * wo, 4 * pl, inpl, s != 1); }
            inpl = 4 * pl; h = ho; w = wo;
        }
    p.act_max = act; p.cols_max = cols; p.gemm_ws = gws;
    return n == kNumConvs;
}

static inline size_t align2m(size_t x) { return (x + ((size_t)1 << 21) - 1) & ~(((size_t)1 << 21) - 1); }

}  // namespace toad

using namespace toad;

// ---- the per-op entry points of the extractor's GEMM layer --------------------------------------------------------
extern "C" int toad_linear_act_res_fwd_f32(const float *X, const float *W, const float *bias, const float *residual, float *Y,
                                            int64_t M, int64_t K, int64_t N, int act, void *ws, size_t ws_bytes, void *stream) {
    return ext_linear(X, nullptr, W, bias, residual, Y, nullptr, M, K, N, act, ws, ws_bytes, (hipStream_t)stream, "toad_linear_act_res_fwd_f32");
}

extern "C" int toad_conv_nhwc_f32(const float *X, const float *Wf, const float *bias, const float *residual, float *Y, int B, int H,
                                  int W, int Cin, int kh, int kw, int stride, int pad, int Cout, int act, void *ws, size_t ws_bytes,
                                  void *stream) {
    return ext_conv_nhwc(X, nullptr, Wf, bias, residual, Y, nullptr, B, H, W, Cin, kh, kw, stride, pad, Cout, act, ws, ws_bytes, (hipStream_t)stream,
                         "toad_conv_nhwc_f32");
}

extern "C" int toad_stem_conv_s2d_f32(const float *Xs, const float *Wf, const float *bias, float *Y, int B, int Ho, int Wo, int act,
                                      void *ws, size_t ws_bytes, void *stream) {
    return ext_stem_conv(Xs, nullptr, Wf, bias, Y, nullptr, B, Ho, Wo, act, ws, ws_bytes, (hipStream_t)stream, "toad_stem_conv_s2d_f32");
}
// The stem AND nn.MaxPool2d(3, 2, 1) as one kernel (models/resnet_custom.py:96-99): Yp [B, Ho/2, Wo/2, 64]. Shapes: Wo = 128, Ho a multiple of 32
// (256 x 256 tiles); others take toad_stem_conv_s2d_f32 + toad_maxpool3x3s2_nhwc_f32.
extern "C" int toad_stem_conv_pool_s2d_f32(const float *Xs, const float *Wf, const float *bias, float *Yp, int B, int Ho, int Wo, void *ws, size_t ws_bytes,
                                           void *stream) {
    return ext_stem_conv(Xs, nullptr, Wf, bias, Yp, nullptr, B, Ho, Wo, TOAD_ACT_RELU, ws, ws_bytes, (hipStream_t)stream, "toad_stem_conv_pool_s2d_f32", true);
}

extern "C" int toad_stem_pool_nchw_f32(const float *X, const float *Wf, const float *bias, float *Yp, int B, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    return ext_stem_nchw_pool(X, Wf, bias, Yp, nullptr, B, H, W, ws, ws_bytes, (hipStream_t)stream, "toad_stem_pool_nchw_f32");
}
extern "C" int toad_stem_pool_nhwc_u8(const unsigned char *tiles, const float *norm, const float *Wf, const float *bias, float *Yp, int B, int H, int W, void *ws,
                                      size_t ws_bytes, void *stream) {
    return ext_stem_nhwc_u8_pool(tiles, norm, Wf, bias, Yp, nullptr, B, H, W, ws, ws_bytes, (hipStream_t)stream, "toad_stem_pool_nhwc_u8");
}
extern "C" int toad_stem_pool_region_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, const float *Wf,
                                        const float *bias, float *Yp, int B, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    return ext_stem_region_u8_pool(RegionSrc{region, pitch, Hr, Wr, origins}, norm, Wf, bias, Yp, nullptr, B, H, W, ws, ws_bytes, (hipStream_t)stream,
                                   "toad_stem_pool_region_u8");
}
extern "C" int toad_stem_pool_region_box_u8(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, const float *Wf,
                                            const float *bias, float *Yp, int B, int H, int W, int shrink, void *ws, size_t ws_bytes, void *stream) {
    return ext_stem_region_u8_pool(RegionSrc{region, pitch, Hr, Wr, origins}, norm, Wf, bias, Yp, nullptr, B, H, W, ws, ws_bytes, (hipStream_t)stream,
                                   "toad_stem_pool_region_box_u8", shrink);
}
// toad_stem_pool_region_box_u8 for a list of regions (stem_u8.h: check_regions_u8)
extern "C" int toad_stem_pool_regions_u8(const ToadTileRegion *regions, int n, const int *tiles, const float *norm, const float *Wf, const float *bias, float *Yp,
                                         int B, int H, int W, int shrink, void *ws, size_t ws_bytes, void *stream) {
    return ext_stem_region_u8_pool(region_list_src(regions, n, tiles), norm, Wf, bias, Yp, nullptr, B, H, W, ws, ws_bytes, (hipStream_t)stream,
                                   "toad_stem_pool_regions_u8", shrink);
}

// ---- the gathers, pools and tile converters as entry points --------------------------------------------------------
extern "C" int toad_im2col_nhwc_f32(const float *X, float *cols, int B, int H, int W, int C, int kh, int kw, int stride,
                                     int pad, void *stream) {
    const char *what = "toad_im2col_nhwc_f32";
    if (!X || !cols) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0) { set_error("%s: bad shape (C must be a multiple of 4)", what); return TOAD_ESHAPE; }
    if (!aligned16(X) || !aligned16(cols)) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    const int Ho = conv_out(H, kh, stride, pad), Wo = conv_out(W, kw, stride, pad);
    if (Ho < 1 || Wo < 1 || (uint64_t)B * Ho * Wo >= (1ull << 32)) { set_error("%s: empty or oversized output", what); return TOAD_ESHAPE; }
    const uint64_t total = (uint64_t)B * Ho * Wo * (uint64_t)(kh * kw * C / 4);
    hipLaunchKernelGGL(im2col_nhwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, X, cols, B, H, W, C, Ho, Wo, kh, kw, stride, pad);
    return check_launch(what);
}

extern "C" int toad_im2col_stem_nchw_f32(const float *X, float *cols, int B, int H, int W, void *stream) {
    const char *what = "toad_im2col_stem_nchw_f32";
    if (!X || !cols) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (!aligned16(cols)) { set_error("%s: cols must be 16-byte aligned", what); return TOAD_EALIGN; }
    const int Ho = conv_out(H, 7, 2, 3), Wo = conv_out(W, 7, 2, 3);
    if (Ho < 1 || Wo < 1 || (uint64_t)B * Ho * Wo >= (1ull << 32)) { set_error("%s: empty or oversized output", what); return TOAD_ESHAPE; }
    hipLaunchKernelGGL(im2col_stem_nchw_kernel, dim3(grid_for((uint64_t)B * Ho * Wo * 40)), dim3(256), 0, (hipStream_t)stream, X, cols, B, H, W, Ho, Wo);
    return check_launch(what);
}

extern "C" int toad_stem_s2d_nchw_f32(const float *X, float *Xs, int B, int H, int W, void *stream) {
    const char *what = "toad_stem_s2d_nchw_f32";
    if (!X || !Xs) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (!aligned16(Xs)) { set_error("%s: Xs must be 16-byte aligned", what); return TOAD_EALIGN; }
    const int Hs = conv_out(H, 7, 2, 3) + 3, Ws = conv_out(W, 7, 2, 3) + 3;
    hipLaunchKernelGGL(stem_s2d_kernel, dim3(grid_for((uint64_t)B * Hs * Ws)), dim3(256), 0, (hipStream_t)stream, X, Xs, B, H, W, Hs, Ws, (float *)nullptr);
    return check_launch(what);
}

extern "C" int toad_maxpool3x3s2_nhwc_f32(const float *X, float *Y, int B, int H, int W, int C, void *stream) {
    const char *what = "toad_maxpool3x3s2_nhwc_f32";
    if (!X || !Y) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) { set_error("%s: bad shape (C must be a multiple of 4)", what); return TOAD_ESHAPE; }
    if (!aligned16(X) || !aligned16(Y)) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    const int Ho = conv_out(H, 3, 2, 1), Wo = conv_out(W, 3, 2, 1);
    if ((uint64_t)B * Ho * Wo >= (1ull << 32)) { set_error("%s: oversized output", what); return TOAD_ESHAPE; }
    hipLaunchKernelGGL(maxpool3x3s2_nhwc_kernel, dim3(grid_for((uint64_t)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, Y, B, H, W, C, Ho, Wo);
    return check_launch(what);
}

static int launch_avgpool(const float *X, void *feat, bool h16, int B, int HW, int C, hipStream_t st, const char *what) {
    if (!X || !feat) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || B > 65535 || HW <= 0 || C <= 0 || C % 4) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (!aligned16(X) || !aligned16(feat)) { set_error("%s: pointers must be 16-byte aligned", what); return TOAD_EALIGN; }
    if (h16) hipLaunchKernelGGL(avgpool_nhwc_kernel<true>, dim3((C + 255) / 256, B), dim3(256), 0, st, X, feat, HW, C);
    else hipLaunchKernelGGL(avgpool_nhwc_kernel<false>, dim3((C + 255) / 256, B), dim3(256), 0, st, X, feat, HW, C);
    return check_launch(what);
}
extern "C" int toad_avgpool_nhwc_f32(const float *X, float *feat, int B, int HW, int C, void *stream) {
    return launch_avgpool(X, feat, false, B, HW, C, (hipStream_t)stream, "toad_avgpool_nhwc_f32");
}

// the one launch behind the tile converters (arguments checked by the callers): contiguous tiles (rg == NULL), tiles by origin, or their box form (shrink == 2)
static int launch_tiles_to_nchw(const unsigned char *src, const RegionSrc *rg, int shrink, const float *norm, float *out, int B, int H, int W, hipStream_t st,
                                const char *what) {
    StemNorm nrm;
    for (int c = 0; c < 3; ++c) { nrm.a[c] = norm[c]; nrm.b[c] = norm[3 + c]; }
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const dim3 grid(grid_for((uint64_t)B * ((HW + 3) / 4)));
    if (!rg)
        hipLaunchKernelGGL(tiles_u8_nhwc_to_nchw_kernel<false>, grid, dim3(256), 0, st, src, out, (uint64_t)B, HW, nrm, TilesNoRegion{});
    else if (rg->list) {
        TilesRegionsArg la;
        la.tiles = rg->origins; la.W = (uint32_t)W;
        fill_region_descs(*rg, la.r);
        if (shrink == 2)
            hipLaunchKernelGGL((tiles_u8_nhwc_to_nchw_kernel<true, 2, true>), grid, dim3(256), 0, st, static_cast<const unsigned char *>(nullptr), out, (uint64_t)B, HW, nrm, la);
        else
            hipLaunchKernelGGL((tiles_u8_nhwc_to_nchw_kernel<true, 1, true>), grid, dim3(256), 0, st, static_cast<const unsigned char *>(nullptr), out, (uint64_t)B, HW, nrm, la);
    } else if (shrink == 2)
        hipLaunchKernelGGL((tiles_u8_nhwc_to_nchw_kernel<true, 2>), grid, dim3(256), 0, st, src, out, (uint64_t)B, HW, nrm, TilesRegionArg{rg->pitch, rg->origins, (uint32_t)W});
    else
        hipLaunchKernelGGL(tiles_u8_nhwc_to_nchw_kernel<true>, grid, dim3(256), 0, st, src, out, (uint64_t)B, HW, nrm, TilesRegionArg{rg->pitch, rg->origins, (uint32_t)W});
    return check_launch(what);
}

extern "C" int toad_tiles_u8_nhwc_to_nchw_f32(const unsigned char *tiles, const float *norm, float *out, int B, int H, int W, void *stream) {
    const char *what = "toad_tiles_u8_nhwc_to_nchw_f32";
    if (!tiles || !norm || !out) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (B <= 0 || H <= 0 || W <= 0 || (uint64_t)H * W >= (1ull << 31)) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (int rc = check_norm_u8(norm, what)) return rc;
    if (!aligned16(out)) { set_error("%s: out must be 16-byte aligned (the uint8 source may have any alignment)", what); return TOAD_EALIGN; }
    return launch_tiles_to_nchw(tiles, nullptr, 1, norm, out, B, H, W, (hipStream_t)stream, what);
}

// shrink == 2: H x W is the network tile, the (2 H, 2 W) footprint at each origin is box-filtered on the way (stem_u8.h: check_region_u8)
static int region_to_nchw(const RegionSrc &rg, const float *norm, float *out, int B, int H, int W, hipStream_t st, const char *what, int shrink = 1) {
    if (!norm || !out) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_region_u8(rg, H, W, what, shrink)) return rc;
    if (B <= 0 || (uint64_t)H * W >= (1ull << 31)) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (int rc = check_norm_u8(norm, what)) return rc;
    if (!aligned16(out)) { set_error("%s: out must be 16-byte aligned (the region may have any alignment)", what); return TOAD_EALIGN; }
    return launch_tiles_to_nchw(rg.region, &rg, shrink, norm, out, B, H, W, st, what);
}
extern "C" int toad_tiles_u8_region_box_to_nchw_f32(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, float *out, int B,
                                                    int H, int W, int shrink, void *stream) {
    return region_to_nchw(RegionSrc{region, pitch, Hr, Wr, origins}, norm, out, B, H, W, (hipStream_t)stream, "toad_tiles_u8_region_box_to_nchw_f32", shrink);
}
extern "C" int toad_tiles_u8_region_to_nchw_f32(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, float *out, int B,
                                                int H, int W, void *stream) {
    return region_to_nchw(RegionSrc{region, pitch, Hr, Wr, origins}, norm, out, B, H, W, (hipStream_t)stream, "toad_tiles_u8_region_to_nchw_f32");
}
// toad_tiles_u8_region_box_to_nchw_f32 for a list of regions
extern "C" int toad_tiles_u8_regions_to_nchw_f32(const ToadTileRegion *regions, int n, const int *tiles, const float *norm, float *out, int B, int H, int W,
                                                 int shrink, void *stream) {
    return region_to_nchw(region_list_src(regions, n, tiles), norm, out, B, H, W, (hipStream_t)stream, "toad_tiles_u8_regions_to_nchw_f32", shrink);
}

extern "C" size_t toad_resnet50_trunc_ws_bytes(int B, int H, int W) {
    NetPlan p;
    if (!make_plan(B, H, W, p)) return 0;
    return 4 * align2m(p.act_max * 4) + align2m(p.cols_max * 4) + align2m(p.gemm_ws) + align2m(4096) + ((size_t)1 << 21);
}

// The uint8 call's workspace: the fp32 call's, plus - only for tile shapes the one-kernel stem does not take - the staging image of the normalised fp32 NCHW
// tiles at its end.
extern "C" size_t toad_resnet50_trunc_u8_ws_bytes(int B, int H, int W) {
    const size_t base = toad_resnet50_trunc_ws_bytes(B, H, W);
    if (base == 0) return 0;
    return base + (stem_nchw_pool_ok(H, W) ? 0 : align2m((size_t)B * 3 * H * W * 4));
}

// weights[i] : folded conv i as [Cout, K] fp32 (K = kh*kw*Cin in (ky, kx, c) order; the stem is [64, 192] in the space-to-depth
//              order of toad_stem_conv_s2d_f32),
// biases[i]  : folded BN shift [Cout]; i runs in execution order (conv1, then per block conv1, conv2, conv3[, downsample]).
// The network behind the three entry points. tiles_u8 == NULL: fp32 NCHW tiles (arguments checked by trunc_entry below, for every form). Otherwise uint8 NHWC tiles with
// norm[6]: 256-wide tiles go straight into the stem kernel, others are converted into the staging image and take the fp32 call's three-kernel stem from there.
// rg != NULL: the uint8 tiles are read by origin from rg->region (tiles_u8 == rg->region), by the region forms of the same two kernels; shrink == 2: by their
// box forms, H x W being the network tile and (2 H, 2 W) the footprint at each origin.
// feat / feat16: either may be NULL; each one given receives the bag rows.
static int trunc_fwd(const float *tiles_nchw, const unsigned char *tiles_u8, const float *norm, const float *const *weights, const float *const *biases, float *feat,
                     void *feat16, const NetPlan &p, int B, int H, int W, void *ws, void *stream, const char *what, const RegionSrc *rg = nullptr, int shrink = 1) {
    hipStream_t st = (hipStream_t)stream;
    char *base = reinterpret_cast<char *>(ws);
    size_t off = align2m(reinterpret_cast<uintptr_t>(ws)) - reinterpret_cast<uintptr_t>(ws);
    auto take = [&](size_t bytes) { char *q = base + off; off += align2m(bytes); return q; };
    float *act[4];
    for (int i = 0; i < 4; ++i) act[i] = reinterpret_cast<float *>(take(p.act_max * 4));
    float *cols = reinterpret_cast<float *>(take(p.cols_max * 4));
    void *gws = take(p.gemm_ws);
    const size_t gcap = p.gemm_ws;
    // Tensor-wide abs-max scalars, one per activation the network produces (round 3): every GEMM epilogue maxes |output| into the slot of
    // its output, the consumer derives ONE power-of-two scale for its fp16 two-piece A operand from it (gemm_narrow.inc). Pools and the
    // im2col / space-to-depth gathers only move values (plus zeros), so their outputs share the producer's slot. All slots are zeroed
    // by one memset; nothing in the call measures an activation a second time.
    float *gm = reinterpret_cast<float *>(take(4096));
    (void)hipMemsetAsync(gm, 0, 4096, st);
    int gi = 0;
    auto slot = [&]() { return gm + (gi++); };
    // stem: 7x7/2 conv + BN + ReLU (resnet_custom.py:96-98), 3x3/2 max-pool (:99)
    float *g_in = slot();
    float *gx = slot();
    if (tiles_u8 && !stem_nchw_pool_ok(H, W)) {
        float *stage = reinterpret_cast<float *>(take((size_t)B * 3 * H * W * 4));
        if (rg) TOAD_TRY(region_to_nchw(*rg, norm, stage, B, H, W, st, what, shrink));
        else TOAD_TRY(toad_tiles_u8_nhwc_to_nchw_f32(tiles_u8, norm, stage, B, H, W, st));
        tiles_nchw = stage;
        tiles_u8 = nullptr;
    }
    // five stems, all leaving the pooled activation in act[1] and its abs-max in gx: three forms of the one-kernel stem (stem_halo.inc) for 256-wide
    // tiles (uint8 ones of another width were staged as fp32 above), two of the space-to-depth stem (gemm_stream.inc) for every other fp32 tile
    if (tiles_u8 && rg) {
        // uint8 tiles read by origin from the region (region form; shrink == 2: box form)
        TOAD_TRY(ext_stem_region_u8_pool(*rg, norm, weights[0], biases[0], act[1], gx, B, H, W, gws, gcap, st, what, shrink));
    } else if (tiles_u8) {
        // uint8 tiles, 256 wide: the same kernel body reads them as stored and normalises while it converts its window (stem_halo.inc, uint8 form)
        TOAD_TRY(ext_stem_nhwc_u8_pool(tiles_u8, norm, weights[0], biases[0], act[1], gx, B, H, W, gws, gcap, st, what));
    } else if (stem_nchw_pool_ok(H, W) && aligned16(tiles_nchw)) {
        // 256-wide tiles: stem + ReLU + max-pool as ONE kernel reading the NCHW tiles themselves (stem_halo.inc); per-tile operand scales, so not even
        // max |tiles| is measured
        TOAD_TRY(ext_stem_nchw_pool(tiles_nchw, weights[0], biases[0], act[1], gx, B, H, W, gws, gcap, st, what));
    } else {
        // 12-channel space-to-depth image (53 MB per 64 tiles); the gather also emits max |tiles| - the only measured tensor - into its slot
        if (!aligned16(cols)) { set_error("%s: internal: cols not aligned", what); return TOAD_EALIGN; }
        hipLaunchKernelGGL(stem_s2d_kernel, dim3(grid_for((uint64_t)B * (p.Hs + 3) * (p.Ws + 3))), dim3(256), 0, st, tiles_nchw, cols, B, H, W, p.Hs + 3, p.Ws + 3, g_in);
        TOAD_TRY(check_launch(what));
        if (stem_pool_ok(p.Hs, p.Ws, TOAD_ACT_RELU)) {      // tiles 256 wide: the max-pool rides in the stem's epilogue, the stem's own output is never stored
            TOAD_TRY(ext_stem_conv(cols, g_in, weights[0], biases[0], act[1], gx, B, p.Hs, p.Ws, TOAD_ACT_RELU, gws, gcap, st, what, true));
        } else {
            TOAD_TRY(ext_stem_conv(cols, g_in, weights[0], biases[0], act[0], gx, B, p.Hs, p.Ws, TOAD_ACT_RELU, gws, gcap, st, what));
            TOAD_TRY(toad_maxpool3x3s2_nhwc_f32(act[0], act[1], B, p.Hs, p.Ws, 64, st));      // max-pooling keeps the maximum: same slot
        }
    }
    float *x = act[1];                          // block input (abs-max scalar: gx)
    auto other = [&](float *a0, float *a1, float *a2) {          // a buffer different from the (up to) three in use
        for (int i = 0; i < 4; ++i) if (act[i] != a0 && act[i] != a1 && act[i] != a2) return act[i];
        return (float *)nullptr;
    };
    int h = p.Hp, w = p.Wp, inpl = 64, ci = 1;
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < kBlocks[l]; ++b) {
            const int s = b == 0 ? kStride[l] : 1, pl = kPlanes[l];
            const int ho = conv_out(h, 3, s, 1), wo = conv_out(w, 3, s, 1);
            const int64_t Mi = (int64_t)B * h * w, Mo = (int64_t)B * ho * wo;
            float *t1 = other(x, nullptr, nullptr);
            // conv1 1x1 + BN + ReLU (:38-40): cols == x
            float *g1 = slot();
            TOAD_TRY(ext_linear(x, gx, weights[ci], biases[ci], nullptr, t1, g1, Mi, inpl, pl, TOAD_ACT_RELU, gws, gcap, st, what));
            // conv2 3x3 stride s + BN + ReLU (:42-44)
            float *t2 = other(x, t1, nullptr);
            // implicit convolution (halo in LDS for stride 1, streamed taps for stride 2), no cols buffer: always for the narrow
            // layers; for 256 output channels (two 128-column tiles per 256 pixels) only when there are enough tiles to fill
            // the chip's 512 workgroup slots - otherwise im2col + the 256x256 kernel with its K-split is faster (measured at B = 64 vs 512)
            const bool implicit = pl <= 128 || (pl <= 256 && (Mo / 256) * ((pl + 127) / 128) >= 512);
            float *g2 = slot();
            if (implicit) {
                TOAD_TRY(ext_conv_nhwc(t1, g1, weights[ci + 1], biases[ci + 1], nullptr, t2, g2, B, h, w, pl, 3, 3, s, 1, pl, TOAD_ACT_RELU, gws, gcap, st, what));
            } else {
                TOAD_TRY(toad_im2col_nhwc_f32(t1, cols, B, h, w, pl, 3, 3, s, 1, st));
                TOAD_TRY(ext_linear(cols, g1, weights[ci + 1], biases[ci + 1], nullptr, t2, g2, Mo, 9 * pl, pl, TOAD_ACT_RELU, gws, gcap, st, what));
            }
            // residual: identity, or downsample = strided 1x1 conv + BN (:49-50, :79-85)
            const float *res = x;
            float *rbuf = nullptr;
            if (b == 0) {
                rbuf = t1;                       // t1 is dead once conv2 has consumed it
                const float *src = x;
                if (s != 1) { TOAD_TRY(toad_im2col_nhwc_f32(x, cols, B, h, w, inpl, 1, 1, s, 0, st)); src = cols; }
                TOAD_TRY(ext_linear(src, gx, weights[ci + 3], biases[ci + 3], nullptr, rbuf, nullptr, Mo, inpl, 4 * pl, TOAD_ACT_NONE, gws, gcap, st, what));
                res = rbuf;                      // (only ever an epilogue addend: nobody needs its abs-max)
            }
            // conv3 1x1 + BN, + residual, ReLU (:46-47, :52-53) in one epilogue
            float *y = other(x, t2, rbuf);
            float *gy = slot();
            TOAD_TRY(ext_linear(t2, g2, weights[ci + 2], biases[ci + 2], res, y, gy, Mo, pl, 4 * pl, TOAD_ACT_RELU, gws, gcap, st, what));
            ci += b == 0 ? 4 : 3;
            x = y; gx = gy; inpl = 4 * pl; h = ho; w = wo;
        }
    if (feat) TOAD_TRY(launch_avgpool(x, feat, false, B, h * w, inpl, st, what));
    if (feat16) TOAD_TRY(launch_avgpool(x, feat16, true, B, h * w, inpl, st, what));
    return TOAD_OK;
}

// What every entry in front of trunc_fwd checks, in the order the callers rely on (tests/test_abi_and_host.py): null pointers, the plan, the region
// (tiles by origin), the normalisation constants (uint8 forms), the workspace size, alignment, the 43 weight / bias slots. Then the network.
// u8 == false: fp32 NCHW tiles into feat; u8: uint8 tiles (tiles_u8, or rg->region by origin) into feat and / or feat16.
static int trunc_entry(bool u8, const float *tiles_nchw, const unsigned char *tiles_u8, const RegionSrc *rg, int shrink, const float *norm,
                       const float *const *weights, const float *const *biases, float *feat, void *feat16, int B, int H, int W, void *ws, size_t ws_bytes,
                       void *stream, const char *what) {
    const bool no_src = u8 ? (!tiles_u8 || (rg && !rg->origins) || !norm) : !tiles_nchw;
    if (no_src || !weights || !biases || (!feat && !feat16) || !ws) {
        set_error(u8 ? "%s: null pointer (feat and feat_f16 may not both be NULL)" : "%s: null pointer", what);
        return TOAD_EINVAL;
    }
    const bool list = rg && rg->list;                                // a list of regions is checked in front of the plan (include/toad_hip.h)
    RegionSrc seen{};                                                // ... once: the stem / the converter behind trunc_fwd take it as checked
    if (list) {
        TOAD_TRY(check_region_u8(*rg, H, W, what, shrink));
        seen = *rg; seen.checked = true; rg = &seen;
    }
    NetPlan p;
    if (!make_plan(B, H, W, p)) { set_error("%s: bad shape B=%d H=%d W=%d", what, B, H, W); return TOAD_ESHAPE; }
    if (rg && !list) TOAD_TRY(check_region_u8(*rg, H, W, what, shrink));
    if (u8) TOAD_TRY(check_norm_u8(norm, what));
    if (ws_bytes < (u8 ? toad_resnet50_trunc_u8_ws_bytes(B, H, W) : toad_resnet50_trunc_ws_bytes(B, H, W))) { set_error("%s: workspace too small", what); return TOAD_EWORKSPACE; }
    if (!aligned16(ws) || (feat && !aligned16(feat)) || (feat16 && !aligned16(feat16))) {
        set_error(u8 ? "%s: workspace / outputs must be 16-byte aligned" : "%s: workspace / output must be 16-byte aligned", what);
        return TOAD_EALIGN;
    }
    if (u8 && !rg && stem_nchw_pool_ok(H, W) && (reinterpret_cast<uintptr_t>(tiles_u8) & 1u) != 0) { set_error("%s: 256-wide uint8 tiles must be 2-byte aligned", what); return TOAD_EALIGN; }
    for (int i = 0; i < kNumConvs; ++i) if (!weights[i] || !biases[i]) { set_error("%s: null weight/bias slot %d", what, i); return TOAD_EINVAL; }
    return trunc_fwd(tiles_nchw, tiles_u8, norm, weights, biases, feat, feat16, p, B, H, W, ws, stream, what, rg, shrink);
}

extern "C" int toad_resnet50_trunc_fwd_f32(const float *tiles_nchw, const float *const *weights, const float *const *biases,
                                            float *feat, int B, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    return trunc_entry(false, tiles_nchw, nullptr, nullptr, 1, nullptr, weights, biases, feat, nullptr, B, H, W, ws, ws_bytes, stream, "toad_resnet50_trunc_fwd_f32");
}

extern "C" int toad_resnet50_trunc_fwd_u8(const unsigned char *tiles, const float *norm, const float *const *weights, const float *const *biases, float *feat,
                                           void *feat_f16, int B, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    return trunc_entry(true, nullptr, tiles, nullptr, 1, norm, weights, biases, feat, feat_f16, B, H, W, ws, ws_bytes, stream, "toad_resnet50_trunc_fwd_u8");
}

static int trunc_fwd_region(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm, const float *const *weights,
                            const float *const *biases, float *feat, void *feat_f16, int B, int H, int W, int shrink, void *ws, size_t ws_bytes, void *stream,
                            const char *what) {
    const RegionSrc rg{region, pitch, Hr, Wr, origins};
    return trunc_entry(true, nullptr, region, &rg, shrink, norm, weights, biases, feat, feat_f16, B, H, W, ws, ws_bytes, stream, what);
}
extern "C" int toad_resnet50_trunc_fwd_u8_region(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm,
                                                  const float *const *weights, const float *const *biases, float *feat, void *feat_f16, int B, int H, int W, void *ws,
                                                  size_t ws_bytes, void *stream) {
    return trunc_fwd_region(region, pitch, Hr, Wr, origins, norm, weights, biases, feat, feat_f16, B, H, W, 1, ws, ws_bytes, stream, "toad_resnet50_trunc_fwd_u8_region");
}
extern "C" int toad_resnet50_trunc_fwd_u8_region_box(const unsigned char *region, int64_t pitch, int Hr, int Wr, const int *origins, const float *norm,
                                                      const float *const *weights, const float *const *biases, float *feat, void *feat_f16, int B, int H, int W,
                                                      int shrink, void *ws, size_t ws_bytes, void *stream) {
    return trunc_fwd_region(region, pitch, Hr, Wr, origins, norm, weights, biases, feat, feat_f16, B, H, W, shrink, ws, ws_bytes, stream,
                            "toad_resnet50_trunc_fwd_u8_region_box");
}
// toad_resnet50_trunc_fwd_u8_region_box for a list of regions: the same network behind the list forms of the stem / the converter
extern "C" int toad_resnet50_trunc_fwd_u8_regions(const ToadTileRegion *regions, int n, const int *tiles, const float *norm, const float *const *weights,
                                                   const float *const *biases, float *feat, void *feat_f16, int B, int H, int W, int shrink, void *ws,
                                                   size_t ws_bytes, void *stream) {
    const RegionSrc rg = region_list_src(regions, n, tiles);
    return trunc_entry(true, nullptr, rg.region, &rg, shrink, norm, weights, biases, feat, feat_f16, B, H, W, ws, ws_bytes, stream, "toad_resnet50_trunc_fwd_u8_regions");
}
