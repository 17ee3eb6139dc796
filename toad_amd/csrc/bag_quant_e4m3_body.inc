// bag_quant_e4m3_body.inc - the loop of bag_quant_e4m3_kernel<IN> and of bags_quant_e4m3_list_kernel<IN> (bag_e4m3.hip, where it is described), included in
// each (an included file and not a device function, so the single-bag kernel compiles to the code it had before the list form existed). In scope: IN; x and
// codes (the bag's first element), n, head, nvec, scale; gid and stride (this lane's first index and the lanes that share the bag).
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
