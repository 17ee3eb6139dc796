// stem_u8.h — the uint8 front end of the extractor: what conv.hip needs from gemm_f32.hip (where stem_halo.inc is compiled) and the
// one check of the normalisation constants both translation units share. Included after common.h.
#pragma once
#include <math.h>

#include "common.h"

namespace toad {

struct StemNorm { float a[3], b[3]; };      // the constants as a kernel argument (scalar registers)

// norm = host float[6]: a_c = 1 / (255 std_c) for c = R, G, B, then b_c = -mean_c / std_c (include/toad_hip.h). A std of 0 arrives as an infinite a_c.
static inline int check_norm_u8(const float *norm, const char *what) {
    for (int i = 0; i < 6; ++i)
        if (!isfinite(norm[i])) { set_error("%s: norm[%d] is not finite (a_c = 1 / (255 std_c) with std_c != 0, b_c = -mean_c / std_c)", what, i); return TOAD_EINVAL; }
    return TOAD_OK;
}

// The stem + ReLU + 3x3/2 max-pool straight from uint8 NHWC tiles [B, H, 256, 3] (stem_halo.inc, uint8 form): ext_stem_nchw_pool's shapes,
// workspace and output; X8 must be 2-byte aligned. norm as above, read at call time (the six floats travel as kernel arguments).
int ext_stem_nhwc_u8_pool(const unsigned char *X8, const float *norm, const float *Wf, const float *bias, float *Yp, float *y_gmax, int B, int H, int W,
                          void *ws, size_t ws_bytes, hipStream_t st, const char *what);

}  // namespace toad
