// h2_arith.h — the fp16 two-piece ("h2") operand arithmetic and the persistent-grid constants that BOTH kernel families of libtoad_hip.so use: the MIL
// GEMMs (gemm_f32.hip: gemm_h2.inc, gemm_pt.inc, ...) and the extractor's kernels (conv.hip: gemm_narrow.inc, gemm_stream.inc, stem_halo.inc). Besides
// common.h it is the only thing the two translation units share; gemm_h2.inc explains the arithmetic. Included after common.h.
#pragma once
#include "common.h"

namespace toad {

constexpr int BK = 32;                                          // depth of one k-stage of every GEMM
constexpr int PB = 256;                                         // tile edge
constexpr int PB_BLOCKS_PER_XCD = 32;
constexpr int PB_GRID = kNumXCD * PB_BLOCKS_PER_XCD;

typedef __attribute__((address_space(3))) void *lptr_t;

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// power-of-two exponent k with amax * 2^k in [2^13, 2^14); clamped so that 2^k and 2^-k are normal floats
__device__ __forceinline__ int h2_exp_from_amax(float amax) {
    const int e = __builtin_amdgcn_frexp_expf(amax);            // amax = f * 2^e, f in [0.5, 1); 0 -> 0
    int k = 14 - e;
    return k < -120 ? -120 : (k > 120 ? 120 : k);
}
// bits of a float passed BY VALUE: __builtin_bit_cast applied directly to an element of an ext_vector (v[k]) reads element 0 whatever k is
// (hipcc 7.2: the operand is a glvalue, and a vector element has no address of its own)
__device__ __forceinline__ unsigned h2_bits(float x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ float h2_pow2(int k) { return __builtin_bit_cast(float, (unsigned)(127 + k) << 23); }
// The accumulator holds 2^(ka+kb) times the product. Undoing that with one factor can leave the fp32 range (2^-240), and with
// two factors 2^-ka, 2^-kb in sequence the intermediate can (operands of magnitude 1e30 give 2^38 * 2^88); the combined exponent
// split into two halves cannot: f1 * f2 = 2^-(ka+kb), |exponent of each| <= 120, and acc * f1 lies between acc and the result.
__device__ __forceinline__ void h2_descale(int ka, int kb, float &f1, float &f2) {
    const int e = -(ka + kb), e1 = e >> 1;
    f1 = h2_pow2(e1);
    f2 = h2_pow2(e - e1);
}
// the same with a per-column kb and ONE shared first factor (keeps the epilogue at 4 VGPRs of scale): f1 = 2^((-ka) >> 1),
// f2[c] = 2^(-ka - e1 - kb[c]); f2 is only out of the normal range where the product itself is (clamped there).
__device__ __forceinline__ float h2_descale_first(int ka) { return h2_pow2((-ka) >> 1); }
__device__ __forceinline__ float h2_descale_second(int ka, int kb) {
    int e = -ka - ((-ka) >> 1) - kb;
    e = e < -126 ? -126 : (e > 127 ? 127 : e);
    return h2_pow2(e);
}
__device__ __forceinline__ int h2_exp_of_pow2(float p) { return (int)((__builtin_bit_cast(unsigned, p) >> 23) & 255u) - 127; }   // p = 2^k -> k

// split 8 fp32 (times the power of two s) into the fp16 planes h, m.
// Two instructions per element: v_fma_mix{lo,hi}_f16 computes fma(x, s, c) in fp32 (exact here: s is a power of two and the
// residual x*s - h is representable), rounds ONCE to fp16 and writes the low / high half of the destination, so
//   h = (rn16(a*s), rn16(b*s))            mixlo(a, s, 0); mixhi(b, s, 0)
//   m = (rn16(a*s - h.lo), rn16(b*s - h.hi))   mixlo(a, s, -h[15:0]); mixhi(b, s, -h[31:16])      (op_sel picks the fp16 half)
// hipcc emits exactly these instructions for the plain-C form below when its SLP vectoriser does not get in the way (probe in
// tools/ubench/h2_split_probe.hip); inside the big kernels it pairs the fp32 FMAs instead (7-8 ops per pair), hence the asm.
// The trailing `s_nop 1` covers the VALU-write -> MFMA-read wait states for a consumer scheduled right behind the block
// (the hazard recogniser does not look inside an asm statement). (The plain-C arm went with the other A/B switches in round 4: same results.)
__device__ __forceinline__ void h2_split2(float a, float b, float s, unsigned &h, unsigned &m) {
    asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
        "v_fma_mixhi_f16 %0, %3, %4, 0\n\t"
        "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h), "=&v"(m) : "v"(a), "v"(b), "v"(s));
}
__device__ __forceinline__ void h2_split8(const float (&x)[8], float s, h16x8 &h, h16x8 &m) {
    u32x4 hp, mp;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned hu, mu;
        h2_split2(x[2 * e], x[2 * e + 1], s, hu, mu);
        hp[e] = hu;
        mp[e] = mu;
    }
    h = __builtin_bit_cast(h16x8, hp);
    m = __builtin_bit_cast(h16x8, mp);
}

}  // namespace toad
