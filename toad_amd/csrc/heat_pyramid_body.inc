// heat_pyramid_body.inc - the body of heat_pyramid_kernel<RB,MASK> and of heat_pyramid_list_kernel<RB,MASK> (heatmap.hip, where it is described), included
// in each: as a device function of its own it compiled the older kernel to other instructions, and those are to stay what they were. In scope where it
// is included: RB, MASK, the window's HeatPyrArgs p, lut, bid - the workgroup's index inside the window - and level_Ho, level_Wo, level_out and
// level_pitch, which give p.Ho[k], p.Wo[k], p.out[k] and p.pitch[k] for the k that a thread of the tail holds in a register: the list kernel's p is a
// local, and an index that is no constant would send it to scratch.
    constexpr int RW = RB / 4, NG = RW / 4;                          // rows per wave, 4-row blocks per lane
    __shared__ unsigned lut_s[256];
    __shared__ int part[3][3][4][32];                                // [level - 8, 16, 32][channel][wave][box of the chunk]
    const HeatPxArgs &a = p.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    lut_s[tid] = (unsigned)lut[3 * tid] | ((unsigned)lut[3 * tid + 1] << 8) | ((unsigned)lut[3 * tid + 2] << 16);
    __syncthreads();
    const unsigned chunk = bid % a.nchunks, rb = bid / a.nchunks;
    const unsigned x = chunk * 256u + (unsigned)lane * 4u, off = 3u * x;
    const int64_t y0 = (int64_t)rb * RB + wave * RW;               // first row of this wave (may lie below Hr: then it reads nothing)
    const unsigned char *src = a.region + y0 * a.pitch + off;
    unsigned w[RW][3];
    if (chunk * 256u + 256u <= (unsigned)a.Wi && y0 + RW <= a.Hi) {  // wave-uniform: all 768 bytes of all RW rows exist
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) w[r][k] = *reinterpret_cast<const u32_a1 *>(src + r * a.pitch + 4 * k);
    } else {
        const int rows = (int)max((int64_t)0, min((int64_t)RW, (int64_t)a.Hi - y0));
        const int npx = x < (unsigned)a.Wi ? min(4, a.Wi - (int)x) : 0;
#pragma unroll
        for (int r = 0; r < RW; ++r) load_px4(src + r * a.pitch, r < rows ? npx : 0, w[r]);
    }

    if (p.levels & 7u) {                                             // levels 1, 2, 4: in the lane, block by block
        const bool live = x < (unsigned)a.Wi;
        const unsigned sx = x + (unsigned)a.wx;                    // the block's corner in the table's image: multiples of 4
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int64_t yg = y0 + 4 * g, sy0 = yg + a.wy;
            if (yg >= a.Hi) break;
            const int gy = (int)(sy0 >> a.shift), gx = (int)(sx >> a.shift);
            const int own = live ? min(a.cells[(int64_t)gy * a.Gx + gx], 255) : -1;
            int v[2][2] = {{0, 0}, {0, 0}}, fxb = 0, fyb = 0;
            if (p.smooth) {                                          // cell >= 8: 2 sx - cell and 2 sy0 - cell are multiples of 8
                const int cell = 1 << a.shift, c2 = 2 * cell;
                const int px = (int)(2u * sx) - cell;                // wx + Wr < 2^30, so 2 sx fits on every live lane
                const int64_t py = 2 * sy0 - cell;
                const int bx = px >> (a.shift + 1), by = (int)(py >> (a.shift + 1));
                fxb = px & (c2 - 1); fyb = (int)(py & (c2 - 1));
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int yy = by + r, xx = bx + c;
                        const bool in = live && yy >= 0 && yy < a.Gy && xx >= 0 && xx < a.Gx;
                        const int t = in ? a.cells[(int64_t)yy * a.Gx + xx] : -1;
                        v[r][c] = t >= 0 ? min(t, 255) : max(own, 0);
                    }
            }
            unsigned tis[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            int thr = -1;                                            // without a mask every byte is above it
            if constexpr (MASK) {                                    // mask_down is a multiple of D >= 2: one byte a block, or (levels 1 and 2) two rows of two
                thr = a.mask_thresh;
                const unsigned mx = sx >> a.mshift;
                const int64_t my = sy0 >> a.mshift;
                const int have = live && mx < (unsigned)a.Wm ? a.Wm - (int)mx : 0;
                const unsigned char *mp = a.mask + my * a.mask_pitch + mx;
                if (a.mshift >= 2) {
                    const unsigned t = load_mask<1>(mp, my < a.Hm ? min(have, 1) : 0) * 0x01010101u;
#pragma unroll
                    for (int r = 0; r < 4; ++r) tis[r] = t;
                } else {
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const unsigned t = load_mask<2>(mp + r * a.mask_pitch, my + r < a.Hm ? min(have, 2) : 0);
                        tis[2 * r] = tis[2 * r + 1] = (t & 0xFFu) * 0x0101u | (t >> 8) * 0x01010000u;
                    }
                }
            }
            unsigned w4[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) w4[r][k] = w[4 * g + r][k];
            const bool tent = p.smooth != 0;
            if (p.levels & 1u) heat_pyr_fine<1>(p, lut_s, w4, x, yg, own, tent, v, fxb, fyb, tis, thr);
            if (p.levels & 2u) heat_pyr_fine<2>(p, lut_s, w4, x, yg, own, tent, v, fxb, fyb, tis, thr);
            if (p.levels & 4u) heat_pyr_fine<4>(p, lut_s, w4, x, yg, own, tent, v, fxb, fyb, tis, thr);
        }
    }

    if (!(p.levels & 0x38u)) return;                                 // uniform over the workgroup: nobody waits at the barrier below
    unsigned b[12];                                                // the 12 column sums over the wave's rows, each at most 8 * 255
    column_sums<RW>(w, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s2 = lanes_allreduce_sum<2>((int)(b[c] + b[c + 3] + b[c + 6] + b[c + 9]));
        const int s4 = s2 + dpp_mov<0x4E>(s2), s8 = s4 + dpp_mov<0x141>(s4);
        if ((lane & 1) == 0) part[0][c][wave][lane >> 1] = s2;
        if ((lane & 3) == 0) part[1][c][wave][lane >> 2] = s4;
        if ((lane & 7) == 0) part[2][c][wave][lane >> 3] = s8;
    }
    __syncthreads();
    int k, t;
    if (tid < 128) { k = 3; t = tid; }
    else if (tid < 160) { k = 4; t = tid - 128; }
    else if (tid >= 192 && tid < 200) { k = 5; t = tid - 192; }
    else return;
    if (level_Ho(k) == 0) return;
    const int down = 1 << k, band = t >> (8 - k), bx = t & ((256 >> k) - 1), wpb = down / RW;      // 256 / down boxes a chunk, RB / down box rows
    if (band >= (RB >> k)) return;
    const int64_t oy = (int64_t)rb * (RB >> k) + band;
    const unsigned ox = chunk * (256u >> k) + (unsigned)bx;
    if (oy >= level_Ho(k) || ox >= (unsigned)level_Wo(k)) return;
    int m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < wpb) s += part[k - 3][c][band * wpb + j][bx];
        m[c] = (s + (1 << (2 * k - 1))) >> (2 * k);
    }
    const int64_t py0 = oy * down + a.wy;                          // the box's corner in the table's image
    const int px0 = (int)(ox * down) + a.wx;
    const int own = min(a.cells[(py0 >> a.shift) * a.Gx + (px0 >> a.shift)], 255);
    int idx = max(own, 0);
    if (p.smooth && a.shift != k) {                                  // cell == down: the tent is the own value
        const int cell = 1 << a.shift, c2 = 2 * cell;
        const int px = 2 * px0 + down - cell;                      // wx + Wr < 2^30, so 2 x fits
        const int64_t py = 2 * py0 + down - cell;
        const int gx0 = px >> (a.shift + 1), fx = px & (c2 - 1);
        const int gy0 = (int)(py >> (a.shift + 1)), fy = (int)(py & (c2 - 1));
        int H[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            int v[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int yy = gy0 + r, xx = gx0 + c;
                const bool in = yy >= 0 && yy < a.Gy && xx >= 0 && xx < a.Gx;
                const int tv = in ? a.cells[(int64_t)yy * a.Gx + xx] : -1;
                v[c] = tv >= 0 ? min(tv, 255) : idx;
            }
            H[r] = c2 * v[0] + fx * (v[1] - v[0]);
        }
        idx = (c2 * H[0] + fy * (H[1] - H[0]) + 2 * cell * cell) >> (2 * a.shift + 2);
    }
    bool tissue = true;
    if (MASK) {
        const int64_t my = py0 >> a.mshift;
        const int mx = px0 >> a.mshift;
        tissue = my < a.Hm && mx < a.Wm && (int)a.mask[my * a.mask_pitch + mx] > a.mask_thresh;
    }
    const int al = own >= 0 && tissue ? a.alpha : 0;               // alpha' = 0 leaves m: (256 m + 128) >> 8
    const unsigned col = lut_s[idx];
    unsigned char *d = level_out(k) + oy * level_pitch(k) + 3u * ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (unsigned char)((al * (int)((col >> (8 * c)) & 255u) + (256 - al) * m[c] + 128) >> 8);
