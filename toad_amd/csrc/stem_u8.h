// stem_u8.h — the uint8 front end of the extractor (conv.hip): the normalisation constants and the region descriptor as the stem kernels
// (stem_halo.inc), the tile converters and the entry points take them, each with its one host-side check. Included after common.h.
#pragma once
#include <math.h>
#include <stdio.h>

#include "common.h"

namespace toad {

struct StemNorm { float a[3], b[3]; };      // the constants as a kernel argument (scalar registers)

// norm = host float[6]: a_c = 1 / (255 std_c) for c = R, G, B, then b_c = -mean_c / std_c (include/toad_hip.h). A std of 0 arrives as an infinite a_c.
static inline int check_norm_u8(const float *norm, const char *what) {
    for (int i = 0; i < 6; ++i)
        if (!isfinite(norm[i])) { set_error("%s: norm[%d] is not finite (a_c = 1 / (255 std_c) with std_c != 0, b_c = -mean_c / std_c)", what, i); return TOAD_EINVAL; }
    return TOAD_OK;
}

// Tiles read by origin from one decoded image (include/toad_hip.h, "tiles by origin"): region = uint8 [Hr, Wr, 3] on the device with a row pitch in bytes,
// origins = DEVICE int32 [B][2], (x, y) of each tile's top-left pixel. What the host can see of it is checked here, by every entry point, before any
// device work; that every origin keeps its tile inside the region is the caller's duty (the Python layer checks it on the host).
// Tiles read from a LIST of regions (include/toad_hip.h, "a LIST of regions"): list = the caller's HOST array of n descriptors, and origins = DEVICE int32
// [B][3], (x, y, k) of each tile in the coordinates of region k; region, pitch, Hr, Wr are not used (region = the list's address, so that "no source" stays
// one test). The kernels get the descriptors by value, 16 bytes each.
// checked: an entry that has run the list's checks (check_regions_u8) sets it on its copy, so that the launchers it calls do not walk the list again.
struct RegionSrc { const unsigned char *region; int64_t pitch; int Hr, Wr; const int *origins; const ToadTileRegion *list = nullptr; int n = 0; bool checked = false; };
constexpr int STEM_REGIONS_MAX = TOAD_TILE_REGIONS_MAX;
struct StemRegionDesc { const unsigned char *base; int pitch; int pad; };   // one region of a list as a kernel sees it
static inline RegionSrc region_list_src(const ToadTileRegion *regions, int n, const int *tiles) {
    return RegionSrc{reinterpret_cast<const unsigned char *>(regions), 0, 0, 0, tiles, regions, n};
}
static inline void fill_region_descs(const RegionSrc &rg, StemRegionDesc (&r)[STEM_REGIONS_MAX]) {
    for (int k = 0; k < STEM_REGIONS_MAX; ++k) r[k] = k < rg.n ? StemRegionDesc{rg.list[k].region, (int)rg.list[k].pitch, 0} : StemRegionDesc{nullptr, 0, 0};
}

static inline int check_shrink_u8(int shrink, const char *what) {
    if (shrink != 1 && shrink != 2) { set_error("%s: shrink must be 1 or 2 (the box filter in front of the tile; larger factors are not built), got %d", what, shrink); return TOAD_ESHAPE; }
    return TOAD_OK;
}
static inline int check_region_extent_u8(const RegionSrc &rg, int H, int W, const char *what, int shrink);
// The list's checks, in the order the header states: n, shrink, region by region what check_region_u8 checks of one region (the first failing region
// wins; its message is prefixed "region k:"), the triples' alignment. The null pointers come first, with the caller's.
static inline int check_regions_u8(const RegionSrc &rg, int H, int W, const char *what, int shrink) {
    if (rg.checked) return TOAD_OK;
    if (!rg.list || !rg.origins) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (rg.n < 1 || rg.n > TOAD_TILE_REGIONS_MAX) { set_error("%s: n = %d regions: one call takes 1 .. %d (TOAD_TILE_REGIONS_MAX)", what, rg.n, TOAD_TILE_REGIONS_MAX); return TOAD_ESHAPE; }
    if (int rc = check_shrink_u8(shrink, what)) return rc;
    for (int k = 0; k < rg.n; ++k) {
        char who[160];
        snprintf(who, sizeof who, "%s: region %d", what, k);
        if (!rg.list[k].region) { set_error("%s: null pointer", who); return TOAD_EINVAL; }
        if (int rc = check_region_extent_u8(RegionSrc{rg.list[k].region, rg.list[k].pitch, rg.list[k].Hr, rg.list[k].Wr, rg.origins}, H, W, who, shrink)) return rc;
    }
    if ((reinterpret_cast<uintptr_t>(rg.origins) & 3u) != 0) { set_error("%s: tiles (int32 [B][3]) must be 4-byte aligned", what); return TOAD_EALIGN; }
    return TOAD_OK;
}
// shrink (the *_box entries; 1 or 2): tile b is the (shrink H, shrink W) FOOTPRINT at its origin, box-filtered to the H x W network tile. The footprint is what has
// to fit the region and what the 32-bit offsets span.
static inline int check_region_u8(const RegionSrc &rg, int H, int W, const char *what, int shrink = 1) {
    if (rg.list) return check_regions_u8(rg, H, W, what, shrink);
    if (!rg.region || !rg.origins) { set_error("%s: null pointer", what); return TOAD_EINVAL; }
    if (int rc = check_shrink_u8(shrink, what)) return rc;
    if (int rc = check_region_extent_u8(rg, H, W, what, shrink)) return rc;
    if ((reinterpret_cast<uintptr_t>(rg.origins) & 3u) != 0) { set_error("%s: origins (int32 [B][2]) must be 4-byte aligned", what); return TOAD_EALIGN; }
    return TOAD_OK;
}
// what the host can see of ONE region and the tile shape: the shape, the pitch, the footprint's fit and the span of the 32-bit offsets
static inline int check_region_extent_u8(const RegionSrc &rg, int H, int W, const char *what, int shrink) {
    if (rg.Hr <= 0 || rg.Wr <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape", what); return TOAD_ESHAPE; }
    if (rg.pitch < 3 * (int64_t)rg.Wr) { set_error("%s: pitch %lld is less than a row of the region (3 Wr = %lld bytes)", what, (long long)rg.pitch, 3ll * rg.Wr); return TOAD_ESHAPE; }
    const int64_t fh = (int64_t)shrink * H, fw = (int64_t)shrink * W;
    if (fh > rg.Hr || fw > rg.Wr) {
        if (shrink == 1) set_error("%s: a %d x %d tile does not fit a %d x %d region", what, H, W, rg.Hr, rg.Wr);
        else set_error("%s: the %lld x %lld footprint of a %d x %d tile (shrink %d) does not fit a %d x %d region", what, (long long)fh, (long long)fw, H, W, shrink, rg.Hr, rg.Wr);
        return TOAD_ESHAPE;
    }
    if (fh * rg.pitch >= (1ll << 31)) {
        if (shrink == 1) set_error("%s: pitch too large: H * pitch must stay below 2^31 (32-bit offsets inside a tile)", what);
        else set_error("%s: pitch too large: %d H * pitch must stay below 2^31 (32-bit offsets inside a footprint)", what, shrink);
        return TOAD_ESHAPE;
    }
    return TOAD_OK;
}

}  // namespace toad
