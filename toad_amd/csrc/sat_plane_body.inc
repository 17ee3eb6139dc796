// sat_plane_body.inc - the body of sat_plane_kernel<DOWN> and of sat_plane_list_kernel<DOWN> (tissue_seg.hip, where it is described), included in each
// and not a device function: sat_plane_kernel's code layout is a measured matter (see there), and its instructions are to stay what they were. In scope
// where it is included: DOWN, region, pitch, Hi, Wi, vmin, plane, ppitch, nchunks, and bid - the workgroup's index inside the region.
    constexpr int RB = strip_rows(DOWN), RW = RB / 4;              // rows per workgroup, per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned chunk = bid % nchunks, rb = bid / nchunks;
    const unsigned x = chunk * 256u + (unsigned)lane * 4u, off = 3u * x;
    const int64_t y0 = (int64_t)rb * RB + wave * RW;               // first row of this wave (may lie below Hi: then it reads and writes nothing)
    const unsigned char *src = region + y0 * pitch + off;
    unsigned w[RW][3];
    int rows = RW, npx = 4;                                        // rows of this wave and pixels of this lane that are consumed
    if (chunk * 256u + 256u <= (unsigned)Wi && y0 + RW <= Hi) {    // wave-uniform: all 768 bytes of all RW rows are consumed
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) w[r][k] = *reinterpret_cast<const u32_a1 *>(src + r * pitch + 4 * k);
    } else {
        rows = (int)max((int64_t)0, min((int64_t)RW, (int64_t)Hi - y0));
        npx = x < (unsigned)Wi ? min(4, Wi - (int)x) : 0;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            w[r][0] = w[r][1] = w[r][2] = 0;
            if (r < rows) {                                        // load_px4(src + r * pitch, npx, w[r]), written out: see above
                const unsigned char *p = src + r * pitch;
                if (npx == 4) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) w[r][k] = *reinterpret_cast<const u32_a1 *>(p + 4 * k);
                } else {
#pragma unroll
                    for (int k = 0; k < 9; ++k)
                        if (k < 3 * npx) w[r][k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
                }
            }
        }
    }
    if constexpr (DOWN == 1) {
        unsigned char *dst = plane + y0 * ppitch + x;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            unsigned o = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) o |= sat_byte(sg_byte(w[r], 3 * p), sg_byte(w[r], 3 * p + 1), sg_byte(w[r], 3 * p + 2), vmin) << (8 * p);
            if (r < rows) {
                unsigned char *d = dst + r * ppitch;
                if (npx == 4) {
                    *reinterpret_cast<u32_a1 *>(d) = o;
                } else {
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        if (p < npx) d[p] = (unsigned char)(o >> (8 * p));
                }
            }
        }
    } else if constexpr (DOWN == 2) {
        unsigned char *dst = plane + (y0 >> 1) * ppitch + (x >> 1);
#pragma unroll
        for (int q = 0; q < RW / 2; ++q) {
            unsigned o = 0;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                int s[3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    s[c] = (sg_byte(w[2 * q], 6 * p + c) + sg_byte(w[2 * q], 6 * p + 3 + c) + sg_byte(w[2 * q + 1], 6 * p + c) +
                            sg_byte(w[2 * q + 1], 6 * p + 3 + c) + 2) >> 2;
                o |= sat_byte(s[0], s[1], s[2], vmin) << (8 * p);
            }
            if (2 * q < rows) {                                    // rows is even: Hi and y0 are
                unsigned char *d = dst + q * ppitch;
                if (npx == 4) *reinterpret_cast<u16_a1 *>(d) = (unsigned short)o;
                else if (npx == 2) d[0] = (unsigned char)o;
            }
        }
    } else {
        constexpr int LANES = DOWN / 4, SH = DOWN == 4 ? 4 : DOWN == 8 ? 6 : DOWN == 16 ? 8 : 10;      // lanes per box, log2(DOWN^2)
        unsigned b[12];                                            // the 12 column sums over the wave's rows, each at most 8 * 255
        column_sums<RW>(w, b);
        int s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = lanes_allreduce_sum<LANES>((int)(b[c] + b[c + 3] + b[c + 6] + b[c + 9]));
        if constexpr (DOWN == 4) {
            if (rows > 0 && npx == 4)
                plane[(y0 >> 2) * ppitch + (x >> 2)] = (unsigned char)sat_byte((s[0] + 8) >> 4, (s[1] + 8) >> 4, (s[2] + 8) >> 4, vmin);
        } else {
            constexpr int NB = RB / DOWN, WPB = 4 / NB, CPR = 64 / LANES;      // box rows per workgroup, waves per box row, boxes per chunk
            __shared__ int part[3][4][64];
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c][wave][lane] = s[c];
            __syncthreads();
            if (tid < NB * CPR) {
                const int band = tid / CPR, bx = tid - band * CPR;
                int m[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int t = 0;
#pragma unroll
                    for (int k = 0; k < WPB; ++k) t += part[c][band * WPB + k][bx * LANES];
                    m[c] = (t + (1 << (SH - 1))) >> SH;
                }
                const int64_t oy = (int64_t)rb * NB + band;
                const unsigned ox = chunk * CPR + bx;
                if (oy * DOWN < Hi && ox * DOWN < (unsigned)Wi) plane[oy * ppitch + ox] = (unsigned char)sat_byte(m[0], m[1], m[2], vmin);
            }
        }
    }
