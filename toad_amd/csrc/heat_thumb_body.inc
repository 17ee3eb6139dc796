// heat_thumb_body.inc - the body of heat_thumb_kernel<DOWN,WINDOW> and of heat_thumb_list_kernel<DOWN> (heatmap.hip, where it is described), included
// in each: as a device function of its own it compiled the older kernel to other instructions, and those are to stay what they were. In scope where it
// is included: DOWN, WINDOW, the window's HeatPxArgs a, smooth, lut, and bid - the workgroup's index inside the window.
    constexpr int RB = strip_rows(DOWN), RW = RB / 4;              // rows per workgroup, per wave
    constexpr int LANES = DOWN / 4, SH = DOWN == 8 ? 6 : DOWN == 16 ? 8 : 10;      // lanes per box, log2(DOWN^2)
    constexpr int NB = RB / DOWN, WPB = 4 / NB, CPR = 64 / LANES;  // box rows per workgroup, waves per box row, boxes per chunk
    __shared__ int part[3][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned chunk = bid % a.nchunks, rb = bid / a.nchunks;
    const unsigned x = chunk * 256u + (unsigned)lane * 4u, off = 3u * x;
    const int64_t y0 = (int64_t)rb * RB + wave * RW;               // first row of this wave (may lie below Hi: then it reads nothing)
    const unsigned char *src = a.region + y0 * a.pitch + off;
    unsigned w[RW][3];
    if (chunk * 256u + 256u <= (unsigned)a.Wi && y0 + RW <= a.Hi) {  // wave-uniform: all 768 bytes of all RW rows are consumed
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) w[r][k] = *reinterpret_cast<const u32_a1 *>(src + r * a.pitch + 4 * k);
    } else {
        const int rows = (int)max((int64_t)0, min((int64_t)RW, (int64_t)a.Hi - y0));
        const int npx = x < (unsigned)a.Wi ? 4 : 0;                // Wi is a multiple of 8
#pragma unroll
        for (int r = 0; r < RW; ++r) load_px4(src + r * a.pitch, r < rows ? npx : 0, w[r]);
    }
    unsigned b[12];                                                // the 12 column sums over the wave's rows, each at most 8 * 255
    column_sums<RW>(w, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) part[c][wave][lane] = lanes_allreduce_sum<LANES>((int)(b[c] + b[c + 3] + b[c + 6] + b[c + 9]));
    __syncthreads();
    if (tid >= NB * CPR) return;
    const int band = tid / CPR, bx = tid - band * CPR;
    const int64_t oy = (int64_t)rb * NB + band;
    const unsigned ox = chunk * CPR + bx;
    if (oy * DOWN >= a.Hi || ox * DOWN >= (unsigned)a.Wi) return;
    int m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < WPB; ++k) t += part[c][band * WPB + k][bx * LANES];
        m[c] = (t + (1 << (SH - 1))) >> SH;
    }
    const int64_t py0 = oy * DOWN + (WINDOW ? a.wy : 0);           // the box's corner in the table's image
    const int px0 = (int)(ox * DOWN) + (WINDOW ? a.wx : 0);
    const int own = min(a.cells[(py0 >> a.shift) * a.Gx + (px0 >> a.shift)], 255);
    int idx = max(own, 0);
    if (smooth) {
        const int cell = 1 << a.shift, c2 = 2 * cell;
        const int px = 2 * px0 + DOWN - cell;                      // wx + Wr < 2^30, so 2 x fits
        const int64_t py = 2 * py0 + DOWN - cell;
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
                const int t = in ? a.cells[(int64_t)yy * a.Gx + xx] : -1;
                v[c] = t >= 0 ? min(t, 255) : idx;
            }
            H[r] = c2 * v[0] + fx * (v[1] - v[0]);
        }
        idx = (c2 * H[0] + fy * (H[1] - H[0]) + 2 * cell * cell) >> (2 * a.shift + 2);
    }
    bool tissue = true;
    if (a.mask) {
        const int64_t my = py0 >> a.mshift;
        const int mx = px0 >> a.mshift;
        tissue = my < a.Hm && mx < a.Wm && (int)a.mask[my * a.mask_pitch + mx] > a.mask_thresh;
    }
    const int al = own >= 0 && tissue ? a.alpha : 0;               // alpha' = 0 leaves m: (256 m + 128) >> 8
    unsigned char *d = a.out + oy * a.out_pitch + 3u * ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (unsigned char)((al * (int)lut[3 * idx + c] + (256 - al) * m[c] + 128) >> 8);
