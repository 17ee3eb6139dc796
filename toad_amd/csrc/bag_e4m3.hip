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
    for (int64_t v = gid; v < nvec; v += stride) {
        const int64_t i = head + v * kE4m3Lane;
        const u32x4 w = *reinterpret_cast<const u32x4 *>(codes + i);
        unsigned h[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) e4m3_word_to_h4(w[j], scale2, h[2 * j], h[2 * j + 1]);
        if constexpr (sizeof(OUT) == 2) {
            u32x4 *o = reinterpret_cast<u32x4 *>(out + i);
            o[0] = u32x4{h[0], h[1], h[2], h[3]};
            o[1] = u32x4{h[4], h[5], h[6], h[7]};
        } else {
            f32x4 *o = reinterpret_cast<f32x4 *>(out + i);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = f32x4{h16_bits_to_f32(h[2 * j]), h16_bits_to_f32(h[2 * j] >> 16), h16_bits_to_f32(h[2 * j + 1]), h16_bits_to_f32(h[2 * j + 1] >> 16)};
        }
    }
    const int64_t body = nvec * kE4m3Lane, rest = n - body;
    for (int64_t r = gid; r < rest; r += stride) {
        const int64_t i = r < head ? r : r + body;
        e4m3_store1(out, i, e4m3_pair_to_h2((unsigned)codes[i] << 8, scale2));
    }
}

// x [n] -> codes [n]; head and nvec as above (codes + head and x + head both 16-byte aligned)
template <typename IN>
__global__ __launch_bounds__(kE4m3Threads) void bag_quant_e4m3_kernel(const IN *__restrict__ x, unsigned char *__restrict__ codes, int64_t n, int64_t head,
                                                                      int64_t nvec, int exp) {
    const float scale = __builtin_bit_cast(float, (unsigned)(127 + exp) << 23);
    const int64_t gid = (int64_t)blockIdx.x * kE4m3Threads + threadIdx.x, stride = (int64_t)gridDim.x * kE4m3Threads;
    for (int64_t v = gid; v < nvec; v += stride) {
        const int64_t i = head + v * kE4m3Lane;
        u32x4 c;
        if constexpr (sizeof(IN) == 4) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(x + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const f32x4 a = p[j]; c[j] = e4m3_pack4(a[0], a[1], a[2], a[3], scale); }
        } else {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(x + i);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4 a = p[q];
                c[2 * q] = e4m3_pack4(h16_bits_to_f32(a[0]), h16_bits_to_f32(a[0] >> 16), h16_bits_to_f32(a[1]), h16_bits_to_f32(a[1] >> 16), scale);
                c[2 * q + 1] = e4m3_pack4(h16_bits_to_f32(a[2]), h16_bits_to_f32(a[2] >> 16), h16_bits_to_f32(a[3]), h16_bits_to_f32(a[3] >> 16), scale);
            }
        }
        *reinterpret_cast<u32x4 *>(codes + i) = c;
    }
    const int64_t body = nvec * kE4m3Lane, rest = n - body;
    for (int64_t r = gid; r < rest; r += stride) {
        const int64_t i = r < head ? r : r + body;
        codes[i] = (unsigned char)e4m3_from_f32(e4m3_load1(x, i), scale);
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
