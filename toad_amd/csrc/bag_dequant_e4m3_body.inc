// bag_dequant_e4m3_body.inc - the loop of bag_dequant_e4m3_kernel<OUT> and of bags_dequant_e4m3_list_kernel<OUT> (bag_e4m3.hip, where it is described), included
// in each (an included file and not a device function, so the single-bag kernel compiles to the code it had before the list form existed). In scope: OUT;
// codes and out (the bag's first element), n, head, nvec, scale2; gid and stride (this lane's first index and the lanes that share the bag).
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
