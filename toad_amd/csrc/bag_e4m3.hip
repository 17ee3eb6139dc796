// bag_e4m3.hip — feature bags as 8-bit OCP e4m3fn codes with one power-of-two exponent per bag (include/toad_hip.h, "e4m3 bags"; the format is defined in
// toad_amd/ingest.py and DESIGN.md). Two streaming kernels: the decode that runs behind a bag's host-to-device copy, and the quantiser for the side that
// produces bags.
//
//   value(code) = (-1)^s * m * 2^-9 for e == 0, (-1)^s * (8 + m) * 2^(e - 10) otherwise, with s = c >> 7, e = (c >> 3) & 15, m = c & 7; c & 0x7F == 0x7F is
//   NaN, there is no infinity, the largest finite value is 448. A bag element is value(code) * 2^-exp, -7 <= exp <= 15.
//
// Decode. (c & 0x7F) << 7, read as an fp16 bit pattern, is the number value(|c|) * 2^-8: the four exponent bits land in the low four of fp16's five, the
// three significand bits in the top three of its ten, and e == 0 is a subnormal of both formats with the same significand. One fp16 multiplication by
// 2^(8 - exp) - a normal fp16 number for every exp of the range - gives the element, and it is EXACT: the product has a 4-bit significand and lies between
// 2^-24 and 57,344, so it is an fp16 number, subnormal ones included (kernels here run with fp16 and fp32 subnormals kept, the compiler's default). Two
// codes are decoded by one packed multiplication. The NaN code would come out as 480 * 2^-exp: its halves get the bits 0x7E00 ORed in. The fp32 output is
// the fp16 one converted, which is exact as well.
//
// Quantise, on y = |x| * 2^exp in fp32 (exact, or far below half the smallest code where it is not; an overflow to +Inf saturates like any y >= 448):
//   y >= 448 -> 0x7E, NaN -> 0x7F;  y >= 2^-6: the fp32 bits rounded to nearest-even at bit 20, minus the exponent bias difference (120 << 3);
//   y < 2^-6: the codes are the integers y * 2^9 = 0 .. 8, read off the low bits of y + 2^14 (whose ulp is 2^-9; the addition rounds to nearest-even).
// A tie goes to the even code in both branches, the sign bit of x is kept. fp16 input is converted to fp32 first, exactly: one rounding in all.
//
// Memory. A lane of the body takes 16 codes: one 16-byte load and two (fp16) or four (fp32) 16-byte stores, the quantiser the mirror image. The body starts
// at the first code whose address is 16-byte aligned and exists only if the other array is 16-byte aligned at that element too; what lies in front of it,
// behind it, or - where there is no body - the whole array goes element by element. No access is wider than what it moves, so no byte outside [0, n) of
// either array is touched. Element offsets are 64-bit. No LDS, no scratch, no atomics.
//
// Lists. The same two loops over a LIST of bags that lie back to back, each with its own exponent and its own split, in one launch, and the abs-max of
// each bag of such a list (the one kernel here with LDS, 16 bytes, and an integer atomic): "a LIST of bags" below.
#include "common.h"

#include <hip/hip_fp16.h>
#include <math.h>

namespace toad {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kE4m3ExpMin = -7, kE4m3ExpMax = 15;
constexpr int kE4m3Lane = 16;               // codes per lane of the body
constexpr int kE4m3Threads = 256;
constexpr int64_t kE4m3MaxBlocks = 256 * 8; // 8 blocks of 4 waves on each of the 256 CUs; longer arrays loop

// two codes, each in the HIGH byte of its half of x -> two fp16 numbers (bit patterns); scale2 = 2^(8 - exp) in both halves
__host__ __device__ __forceinline__ unsigned e4m3_pair_to_h2(unsigned x, unsigned scale2) {
    const unsigned sign = x & 0x80008000u, mag = (x & 0x7F007F00u) >> 1;
    const unsigned nan = (((mag + 0x00800080u) >> 14) & 0x00010001u) * 0x7E00u;          // mag + 0x80 reaches bit 14 for 0x3F80 (the NaN code) only
    const h16x2 v = __builtin_bit_cast(h16x2, mag) * __builtin_bit_cast(h16x2, scale2);
    return __builtin_bit_cast(unsigned, v) | nan | sign;
}
// the four codes of a little-endian word -> four fp16 numbers, in order
__host__ __device__ __forceinline__ void e4m3_word_to_h4(unsigned w, unsigned scale2, unsigned &h01, unsigned &h23) {
    h01 = e4m3_pair_to_h2(((w & 0xFFu) << 8) | ((w & 0xFF00u) << 16), scale2);
    h23 = e4m3_pair_to_h2(((w >> 8) & 0xFF00u) | (w & 0xFF000000u), scale2);
}
__host__ __device__ __forceinline__ float h16_bits_to_f32(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }
__host__ __device__ __forceinline__ unsigned e4m3_scale2(int exp) { const unsigned s = (unsigned)(23 - exp) << 10; return s | (s << 16); }

__host__ __device__ __forceinline__ void e4m3_store1(__half *out, int64_t i, unsigned h) { reinterpret_cast<unsigned short *>(out)[i] = (unsigned short)h; }
__host__ __device__ __forceinline__ void e4m3_store1(float *out, int64_t i, unsigned h) { out[i] = h16_bits_to_f32(h); }

// x -> code, scale = 2^exp
__host__ __device__ __forceinline__ unsigned e4m3_from_f32(float x, float scale) {
    const unsigned sign = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
    const float y = __builtin_fabsf(x) * scale;
    const unsigned u = __builtin_bit_cast(unsigned, y);
    unsigned c;
    if (u >= 0x43E00000u) c = u > 0x7F800000u ? 0x7Fu : 0x7Eu;                           // 448 and above, +Inf included; NaN
    else if (u < 0x3C800000u) c = __builtin_bit_cast(unsigned, y + 16384.0f) - 0x46800000u;   // below 2^-6: multiples of 2^-9
    else c = ((u + 0x7FFFFu + ((u >> 20) & 1u)) >> 20) - (120u << 3);
    return c | sign;
}
__host__ __device__ __forceinline__ float e4m3_load1(const float *x, int64_t i) { return x[i]; }
__host__ __device__ __forceinline__ float e4m3_load1(const __half *x, int64_t i) {
    return h16_bits_to_f32(reinterpret_cast<const unsigned short *>(x)[i]);
}
__host__ __device__ __forceinline__ unsigned e4m3_pack4(float a, float b, float c, float d, float scale) {
    return e4m3_from_f32(a, scale) | (e4m3_from_f32(b, scale) << 8) | (e4m3_from_f32(c, scale) << 16) | (e4m3_from_f32(d, scale) << 24);
}

// codes [n] -> out [n]. Body: nvec lanes' worth of 16 elements from element `head` on (codes + head and out + head both 16-byte aligned; nvec == 0 where
// that cannot be had); every other element one at a time.
template <typename OUT>
__global__ __launch_bounds__(kE4m3Threads) void bag_dequant_e4m3_kernel(const unsigned char *__restrict__ codes, OUT *__restrict__ out, int64_t n,
                                                                        int64_t head, int64_t nvec, int exp) {
    const unsigned scale2 = e4m3_scale2(exp);
    const int64_t gid = (int64_t)blockIdx.x * kE4m3Threads + threadIdx.x, stride = (int64_t)gridDim.x * kE4m3Threads;
#include "bag_dequant_e4m3_body.inc"
}

// x [n] -> codes [n]; head and nvec as above (codes + head and x + head both 16-byte aligned)
template <typename IN>
__global__ __launch_bounds__(kE4m3Threads) void bag_quant_e4m3_kernel(const IN *__restrict__ x, unsigned char *__restrict__ codes, int64_t n, int64_t head,
                                                                      int64_t nvec, int exp) {
    const float scale = __builtin_bit_cast(float, (unsigned)(127 + exp) << 23);
    const int64_t gid = (int64_t)blockIdx.x * kE4m3Threads + threadIdx.x, stride = (int64_t)gridDim.x * kE4m3Threads;
#include "bag_quant_e4m3_body.inc"
}

// ---- a LIST of bags in one launch (toad_bags_dequant_e4m3, toad_bags_quant_e4m3, toad_bags_absmax_bits): the bags lie back to back in one [R, k] array, each
// with its own exponent. Descriptors travel BY VALUE in the kernel argument, as in sat_plane_list_kernel (tissue_seg.hip): bag j of the launch owns the
// workgroups first .. first + nblocks; descriptors from the launch's count on carry first = 0xFFFFFFFF, above every workgroup index, so the search needs no
// count: six uniform steps of a binary search over the 64 prefixes, scalar loads from the kernel argument, once per workgroup. From there on a workgroup is
// one of its bag's and runs the loop of the single-bag kernel (the included body) with the bag's own head / body / tail split - a bag starts at any byte, so
// the split is per bag - over the bag's own workgroups. Empty bags never reach a descriptor. The grid is exact: every workgroup has a bag.
struct E4m3ListBag {
    int64_t off, n, nvec;            // first element of the bag in the concatenation, its elements, the lanes of its body
    unsigned first, nblocks;         // its workgroups
    int head, exp, bag, pad_;        // elements in front of its body; its exponent; its place in the caller's list (the abs-max slot)
};
struct E4m3ListArgs { E4m3ListBag b[TOAD_E4M3_LIST_MAX]; };
static_assert(sizeof(E4m3ListBag) == 48 && sizeof(E4m3ListArgs) + 2 * sizeof(void *) <= 4096, "the descriptors and two pointers travel in the kernel argument");

__device__ __forceinline__ const E4m3ListBag &e4m3_list_bag(const E4m3ListArgs &l) {
    static_assert(TOAD_E4M3_LIST_MAX == 64, "six steps search 64 prefixes");
    int k = 0;
#pragma unroll
    for (int step = TOAD_E4M3_LIST_MAX / 2; step >= 1; step >>= 1)
        if (l.b[k + step].first <= blockIdx.x) k += step;
    return l.b[k];
}

template <typename OUT>
__global__ __launch_bounds__(kE4m3Threads) void bags_dequant_e4m3_list_kernel(const E4m3ListArgs l, const unsigned char *__restrict__ cat_codes,
                                                                              OUT *__restrict__ cat_out) {
    const E4m3ListBag &w = e4m3_list_bag(l);
    const unsigned char *__restrict__ codes = cat_codes + w.off;
    OUT *__restrict__ out = cat_out + w.off;
    const int64_t n = w.n, head = w.head, nvec = w.nvec;
    const unsigned scale2 = e4m3_scale2(w.exp);
    const int64_t gid = (int64_t)(blockIdx.x - w.first) * kE4m3Threads + threadIdx.x, stride = (int64_t)w.nblocks * kE4m3Threads;
#include "bag_dequant_e4m3_body.inc"
}

template <typename IN>
__global__ __launch_bounds__(kE4m3Threads) void bags_quant_e4m3_list_kernel(const E4m3ListArgs l, const IN *__restrict__ cat_x,
                                                                            unsigned char *__restrict__ cat_codes) {
    const E4m3ListBag &w = e4m3_list_bag(l);
    const IN *__restrict__ x = cat_x + w.off;
    unsigned char *__restrict__ codes = cat_codes + w.off;
    const int64_t n = w.n, head = w.head, nvec = w.nvec;
    const float scale = __builtin_bit_cast(float, (unsigned)(127 + w.exp) << 23);
    const int64_t gid = (int64_t)(blockIdx.x - w.first) * kE4m3Threads + threadIdx.x, stride = (int64_t)w.nblocks * kE4m3Threads;
#include "bag_quant_e4m3_body.inc"
}

// amax_bits[bag] = the largest sign-cleared bit pattern of the bag's elements, as an fp32 pattern: an unsigned maximum, so the order of the reduction does
// not matter, +-Inf is 0x7F800000 and a NaN lies above it. fp16 patterns are ordered the same way, so their maximum is taken as 15-bit integers and
// up-cast ONCE, by the workgroup's first lane (exact, subnormals included; a NaN stays a NaN). Here the body is 16-BYTE lanes from the first 16-byte
// aligned element on (x is aligned to its element, so `head` whole elements lie in front of it), everything else element by element. A workgroup reduces in
// registers, across its four waves through 16 bytes of LDS, and issues at most ONE integer atomic max; the caller's array was zeroed on the stream before
// the launch (an all-zero bag, like an empty one, leaves its 0).
constexpr int64_t kE4m3AbsmaxMaxBlocks = 256;   // per bag: a bag's workgroups all meet in ONE atomic word
template <typename IN>
__global__ __launch_bounds__(kE4m3Threads) void bags_absmax_list_kernel(const E4m3ListArgs l, const IN *__restrict__ cat_x, unsigned *__restrict__ amax_bits) {
    constexpr int kPer = 16 / (int)sizeof(IN);
    const E4m3ListBag &w = e4m3_list_bag(l);
    const IN *__restrict__ x = cat_x + w.off;
    const int64_t n = w.n, head = w.head, nvec = w.nvec;
    const int64_t gid = (int64_t)(blockIdx.x - w.first) * kE4m3Threads + threadIdx.x, stride = (int64_t)w.nblocks * kE4m3Threads;
    unsigned m = 0;
    for (int64_t v = gid; v < nvec; v += stride) {
        const u32x4 a = *reinterpret_cast<const u32x4 *>(x + head + v * kPer);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (sizeof(IN) == 4) m = max(m, a[j] & 0x7FFFFFFFu);
            else m = max(max(m, a[j] & 0x7FFFu), (a[j] >> 16) & 0x7FFFu);
        }
    }
    const int64_t body = nvec * kPer, rest = n - body;
    for (int64_t r = gid; r < rest; r += stride) {
        const int64_t i = r < head ? r : r + body;
        if constexpr (sizeof(IN) == 4) m = max(m, reinterpret_cast<const unsigned *>(x)[i] & 0x7FFFFFFFu);
        else m = max(m, (unsigned)reinterpret_cast<const unsigned short *>(x)[i] & 0x7FFFu);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    __shared__ unsigned red[kE4m3Threads / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if constexpr (sizeof(IN) == 2) m = __builtin_bit_cast(unsigned, h16_bits_to_f32(m));
        if (m) atomicMax(amax_bits + w.bag, m);
    }
}

// the split of [0, n) for a code array at `codes` and a second array of `elem`-byte elements at `other`: head elements in front of the body, nvec lanes of 16
static void e4m3_split(const void *codes, const void *other, int elem, int64_t n, int64_t &head, int64_t &nvec) {
    head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(codes) & 15u)) & 15u);
    nvec = 0;
    if (head <= n && ((reinterpret_cast<uintptr_t>(other) + (uintptr_t)head * (uintptr_t)elem) & 15u) == 0) nvec = (n - head) / kE4m3Lane;
    if (nvec == 0) head = 0;
}
static unsigned e4m3_blocks(int64_t n, int64_t nvec) {
    const int64_t rest = n - nvec * kE4m3Lane, work = nvec > rest ? nvec : rest;
    const int64_t blocks = (work + kE4m3Threads - 1) / kE4m3Threads;
    return (unsigned)(blocks < 1 ? 1 : blocks > kE4m3MaxBlocks ? kE4m3MaxBlocks : blocks);
}
static int e4m3_check(const char *what, const void *a, const void *b, int64_t n, int exp) {
    if (!a || !b) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (n < 0) { set_error("%s: n = %lld must not be negative", what, (long long)n); return TOAD_EINVAL; }
    if (exp < kE4m3ExpMin || exp > kE4m3ExpMax) { set_error("%s: exp = %d outside %d .. %d", what, exp, kE4m3ExpMin, kE4m3ExpMax); return TOAD_EINVAL; }
    return TOAD_OK;
}

}  // namespace toad

using namespace toad;

extern "C" int toad_bag_dequant_e4m3(const void *codes, void *out, int out_f32, int64_t n, int exp, void *stream) {
    const char *what = "toad_bag_dequant_e4m3";
    if (int rc = e4m3_check(what, codes, out, n, exp)) return rc;
    const int elem = out_f32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(elem - 1)) { set_error("%s: out must be %d-byte aligned", what, elem); return TOAD_EALIGN; }
    if (n == 0) return TOAD_OK;
    int64_t head, nvec;
    e4m3_split(codes, out, elem, n, head, nvec);
    const dim3 grid(e4m3_blocks(n, nvec)), block(kE4m3Threads);
    if (out_f32)
        hipLaunchKernelGGL(bag_dequant_e4m3_kernel<float>, grid, block, 0, (hipStream_t)stream, (const unsigned char *)codes, (float *)out, n, head, nvec, exp);
    else
        hipLaunchKernelGGL(bag_dequant_e4m3_kernel<__half>, grid, block, 0, (hipStream_t)stream, (const unsigned char *)codes, (__half *)out, n, head, nvec, exp);
    return check_launch(what);
}

extern "C" int toad_bag_quant_e4m3(const void *x, int x_f16, void *codes, int64_t n, int exp, void *stream) {
    const char *what = "toad_bag_quant_e4m3";
    if (int rc = e4m3_check(what, x, codes, n, exp)) return rc;
    const int elem = x_f16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(x) & (uintptr_t)(elem - 1)) { set_error("%s: x must be %d-byte aligned", what, elem); return TOAD_EALIGN; }
    if (n == 0) return TOAD_OK;
    int64_t head, nvec;
    e4m3_split(codes, x, elem, n, head, nvec);
    const dim3 grid(e4m3_blocks(n, nvec)), block(kE4m3Threads);
    if (x_f16)
        hipLaunchKernelGGL(bag_quant_e4m3_kernel<__half>, grid, block, 0, (hipStream_t)stream, (const __half *)x, (unsigned char *)codes, n, head, nvec, exp);
    else
        hipLaunchKernelGGL(bag_quant_e4m3_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float *)x, (unsigned char *)codes, n, head, nvec, exp);
    return check_launch(what);
}

// ---- the list entries. What the bags share first (pointers, nb, k, the first offset), then bag by bag, the first failing bag winning under "bag i:"; then
// the alignment of the whole array. Nothing is launched before all of that has passed. Two walks over the host arrays, no allocation, no upload, no
// synchronisation: the first checks, the second fills TOAD_E4M3_LIST_MAX descriptors of non-empty bags at a time and launches them.
namespace toad {

static int e4m3_list_check(const char *what, const void *a, const void *b, int64_t k, const int64_t *row_offsets, const int *exps, bool need_exps, int nb) {
    if (!a || !b || !row_offsets || (need_exps && nb > 0 && !exps)) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (nb < 0) { set_error("%s: nb = %d bags", what, nb); return TOAD_EINVAL; }
    if (k <= 0) { set_error("%s: k = %lld must be positive", what, (long long)k); return TOAD_EINVAL; }
    if (row_offsets[0] != 0) { set_error("%s: row_offsets[0] = %lld must be 0", what, (long long)row_offsets[0]); return TOAD_EINVAL; }
    for (int i = 0; i < nb; ++i) {
        if (row_offsets[i + 1] < row_offsets[i]) {
            set_error("bag %d: %s: row_offsets decrease from %lld to %lld", i, what, (long long)row_offsets[i], (long long)row_offsets[i + 1]);
            return TOAD_EINVAL;
        }
        if (need_exps && (exps[i] < kE4m3ExpMin || exps[i] > kE4m3ExpMax)) {
            set_error("bag %d: %s: exp = %d outside %d .. %d", i, what, exps[i], kE4m3ExpMin, kE4m3ExpMax);
            return TOAD_EINVAL;
        }
    }
    if (row_offsets[nb] > (INT64_MAX >> 2) / k) {                    // R k elements of up to 4 bytes: offsets stay inside 64 bits
        set_error("%s: %lld rows of %lld elements", what, (long long)row_offsets[nb], (long long)k);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}

// the second walk: plan(off, n, d) fills head, nvec and nblocks of a non-empty bag's descriptor, launch(l, grid) launches one filled argument
template <typename Plan, typename Launch>
static int e4m3_list_run(const char *what, int64_t k, const int64_t *row_offsets, const int *exps, int nb, Plan plan, Launch launch) {
    E4m3ListArgs l;
    for (int i = 0; i < nb;) {
        int m = 0;
        unsigned grid = 0;
        for (; i < nb && m < TOAD_E4M3_LIST_MAX; ++i) {
            const int64_t n = (row_offsets[i + 1] - row_offsets[i]) * k;
            if (n == 0) continue;
            E4m3ListBag &d = l.b[m++];
            d = {};
            d.off = row_offsets[i] * k; d.n = n; d.first = grid; d.exp = exps ? exps[i] : 0; d.bag = i;
            plan(d);
            grid += d.nblocks;
        }
        if (m == 0) break;
        for (int j = m; j < TOAD_E4M3_LIST_MAX; ++j) { l.b[j] = {}; l.b[j].first = 0xFFFFFFFFu; }      // above every workgroup index: the search stops short of them
        launch(l, grid);
        if (int rc = check_launch(what)) return rc;
    }
    return TOAD_OK;
}

}  // namespace toad

extern "C" int toad_bags_dequant_e4m3(const void *codes, void *out, int out_f32, int64_t k, const int64_t *row_offsets, const int *exps, int nb,
                                      void *stream) {
    const char *what = "toad_bags_dequant_e4m3";
    if (int rc = e4m3_list_check(what, codes, out, k, row_offsets, exps, true, nb)) return rc;
    const int elem = out_f32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(elem - 1)) { set_error("%s: out must be %d-byte aligned", what, elem); return TOAD_EALIGN; }
    auto plan = [&](E4m3ListBag &d) {
        int64_t head;
        e4m3_split((const unsigned char *)codes + d.off, (const unsigned char *)out + d.off * elem, elem, d.n, head, d.nvec);
        d.head = (int)head; d.nblocks = e4m3_blocks(d.n, d.nvec);
    };
    auto launch = [&](const E4m3ListArgs &l, unsigned grid) {
        if (out_f32)
            hipLaunchKernelGGL(bags_dequant_e4m3_list_kernel<float>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const unsigned char *)codes, (float *)out);
        else
            hipLaunchKernelGGL(bags_dequant_e4m3_list_kernel<__half>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const unsigned char *)codes, (__half *)out);
    };
    return e4m3_list_run(what, k, row_offsets, exps, nb, plan, launch);
}

extern "C" int toad_bags_quant_e4m3(const void *x, int x_f16, void *codes, int64_t k, const int64_t *row_offsets, const int *exps, int nb, void *stream) {
    const char *what = "toad_bags_quant_e4m3";
    if (int rc = e4m3_list_check(what, x, codes, k, row_offsets, exps, true, nb)) return rc;
    const int elem = x_f16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(x) & (uintptr_t)(elem - 1)) { set_error("%s: x must be %d-byte aligned", what, elem); return TOAD_EALIGN; }
    auto plan = [&](E4m3ListBag &d) {
        int64_t head;
        e4m3_split((const unsigned char *)codes + d.off, (const unsigned char *)x + d.off * elem, elem, d.n, head, d.nvec);
        d.head = (int)head; d.nblocks = e4m3_blocks(d.n, d.nvec);
    };
    auto launch = [&](const E4m3ListArgs &l, unsigned grid) {
        if (x_f16)
            hipLaunchKernelGGL(bags_quant_e4m3_list_kernel<__half>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const __half *)x, (unsigned char *)codes);
        else
            hipLaunchKernelGGL(bags_quant_e4m3_list_kernel<float>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const float *)x, (unsigned char *)codes);
    };
    return e4m3_list_run(what, k, row_offsets, exps, nb, plan, launch);
}

extern "C" int toad_bags_absmax_bits(const void *x, int x_f16, uint32_t *amax_bits, int64_t k, const int64_t *row_offsets, int nb, void *stream) {
    const char *what = "toad_bags_absmax_bits";
    if (int rc = e4m3_list_check(what, x, amax_bits, k, row_offsets, nullptr, false, nb)) return rc;
    const int elem = x_f16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(x) & (uintptr_t)(elem - 1)) { set_error("%s: x must be %d-byte aligned", what, elem); return TOAD_EALIGN; }
    if (!aligned4(amax_bits)) { set_error("%s: amax_bits must be 4-byte aligned", what); return TOAD_EALIGN; }
    if (nb == 0) return TOAD_OK;
    // every slot starts at 0, whatever it held: the kernels only ever raise it (one fill on the stream, in front of the launches)
    if (hipMemsetAsync(amax_bits, 0, (size_t)nb * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return check_launch(what);
    const int per = 16 / elem;
    auto plan = [&](E4m3ListBag &d) {
        const uintptr_t at = reinterpret_cast<uintptr_t>(x) + (uintptr_t)d.off * (uintptr_t)elem;
        int64_t head = (int64_t)(((16u - (unsigned)(at & 15u)) & 15u) / (unsigned)elem);
        if (head > d.n) head = d.n;
        d.nvec = (d.n - head) / per;
        if (d.nvec == 0) head = 0;
        d.head = (int)head;
        const int64_t rest = d.n - d.nvec * per, work = d.nvec > rest ? d.nvec : rest, blocks = (work + kE4m3Threads - 1) / kE4m3Threads;
        d.nblocks = (unsigned)(blocks > kE4m3AbsmaxMaxBlocks ? kE4m3AbsmaxMaxBlocks : blocks);
    };
    auto launch = [&](const E4m3ListArgs &l, unsigned grid) {
        if (x_f16)
            hipLaunchKernelGGL(bags_absmax_list_kernel<__half>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const __half *)x, amax_bits);
        else
            hipLaunchKernelGGL(bags_absmax_list_kernel<float>, dim3(grid), dim3(kE4m3Threads), 0, (hipStream_t)stream, l, (const float *)x, amax_bits);
    };
    return e4m3_list_run(what, k, row_offsets, nullptr, nb, plan, launch);
}
