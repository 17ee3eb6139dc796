// gemm_narrow.inc — part of the extractor's translation unit conv.hip (included inside namespace toad): what the extractor's narrow-N GEMMs
// (Cout <= 128: stem, layer1, layer2's 1x1-in / 3x3; models/resnet_custom.py:19-108) share - the convolution geometry, the gather modes
// and the weight-plane format. The kernels that consume them are in gemm_stream.inc.
// ------------------------------------------------------------------------------------------
// Weight planes (split_planes_narrow_h2_kernel): two fp16 planes per weight row with that row's own power-of-two scale (binv = 1 / t_row),
// laid out [column tile][k-stage][plane][pos 0..TN-1][phys chunk 0..3][8 halves], pos = 32 b + li for column NB li + b (a lane of the
// consuming wave owns NB consecutive output columns), 16-byte chunks XOR-swizzled with (pos >> 2) & 3: a stage is a linear copy into LDS
// and its fragments are conflict-free ds_read_b128. Activations carry ONE power-of-two scale per tensor (a_gmax[0] = max |A|, emitted by the
// kernel that produced A): the rows of an implicit convolution tile are gathered from arbitrary pixels, so there is no per-block scale to
// take. fp16 has 5 exponent bits; elements more than 2^17 below the tensor's maximum keep an absolute error <= 2^-39 of it - nothing a
// 1e-4 feature tolerance can see (tests/test_resnet_extractor.py holds the whole network to the reference's goldens).
// Implicit convolution: row m = output pixel (b, oy, ox) of an NHWC activation X[B, H, W, C] (C % 32 == 0), K = kh * kw * C in (ky, kx, c)
// order, so a 32-deep k-stage lies inside ONE tap; the stem runs as a 4x4 convolution over a 12-channel space-to-depth image.
// ------------------------------------------------------------------------------------------
struct ConvGeom { int H, W, C, Ho, Wo, kw, stride, pad; };    // plain ints only (pointers in by-value structs become FLAT)
enum { GATHER_NONE = 0, GATHER_CONV = 1, GATHER_STEM = 2, GATHER_STEM_POOL = 3 };     // how the A operand of the narrow kernel is addressed (3: the stem with the 3x3/2 max-pool in its epilogue, gemm_stream.inc)

template <int NB>
__global__ __launch_bounds__(256) void split_planes_narrow_h2_kernel(const float *__restrict__ src, int64_t sn, unsigned short *__restrict__ Bp,
                                                                      float *__restrict__ binv, int N, int K, int tiles_n, int taps, int C, int nkp) {
    constexpr int TN = NB * 32;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);              // one wave per weight row (rows >= N are zero padding)
    if (n >= tiles_n * TN) return;
    const int nchunks = K / 8;
    const bool real = n < N;
    const float *row = src + (int64_t)(real ? n : 0) * sn;
    float mx = 0.f;
    if (real)
        for (int q = lane; q < nchunks; q += 64) {
            const f32x4 a = ld4(row + q * 8), b = ld4(row + q * 8 + 4);
            mx = __builtin_fmaxf(mx, __builtin_fmaxf(h2_absmax4(a), h2_absmax4(b)));
        }
    mx = h2_wave_max(mx);
    const int kexp = h2_exp_from_amax(mx);
    const float s = h2_pow2(kexp);
    if (lane == 0) binv[n] = h2_pow2(-kexp);
    const int tile = n / TN, cc = n % TN;
    const int pos = 32 * (cc % NB) + cc / NB;                        // column NB * li + b  ->  pos = 32 b + li
    // nkp >= nk stages are written per column tile; the ones past K are zero planes (the streamed kernel walks stages in pairs)
    for (int q = lane; q < nkp * 4; q += 64) {
        float x[8];
        const int stage = q >> 2, chunk = q & 3, phys = chunk ^ ((pos >> 2) & 3);
        // taps > 1 (the streamed implicit convolution, gemm_stream.inc): k-stages run channel-chunk outer, tap inner, so stage
        // (cc, tap) = (stage / taps, stage % taps) takes the weights W[n][tap * C + cc * 32 ...] of the (ky, kx, c) filter row
        const int k0 = taps > 1 ? (stage % taps) * C + (stage / taps) * BK + chunk * 8 : q * 8;
        if (real && q < nchunks) {
            const f32x4 a = ld4(row + k0), b = ld4(row + k0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[4 + e] = b[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = 0.f;
        }
        h16x8 h, m;
        h2_split8(x, s, h, m);
        unsigned short *dst = Bp + ((int64_t)(tile * nkp + stage) * 2) * (TN * BK) + pos * BK + phys * 8;
        *reinterpret_cast<h16x8 *>(dst) = h;
        *reinterpret_cast<h16x8 *>(dst + TN * BK) = m;
    }
}

