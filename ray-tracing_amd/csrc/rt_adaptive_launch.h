/* rt_adaptive_launch.h — what rt_post.hip and rt_context.hip need of rt_adaptive.hip: the calls that enqueue its kernels on a stream, and — without
 * HIP, so that a host test reaches them (tests/adaptive_math_driver.cpp) — the tile geometry and the check of a caller's tile list.
 * The entry points of include/rt_adaptive.h themselves live in rt_post.hip; the launch over a tile list (adaptive_launch) is rt_context.hip's. */
#ifndef RT_ADAPTIVE_LAUNCH_H
#define RT_ADAPTIVE_LAUNCH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_adaptive.h"
#include "rt_adaptive_math.h"

namespace rt_ad {

/* The parameter errors of include/rt_adaptive.h: RT_OK and *job filled in, or the status and *why = what is wrong */
inline int check_params(const RtAdaptiveParams* p, rt_ad_job* job, const char** why)
{
    *why = "";
    if (!p) { *why = "null parameters"; return RT_ERR_INVALID_ARG; }
    if (p->struct_size != sizeof(RtAdaptiveParams)) { *why = "RtAdaptiveParams.struct_size is not this library's (32)"; return RT_ERR_ABI_MISMATCH; }
    if (!(p->threshold >= 0.0f) || !rt_dn_finite(p->threshold)) { *why = "threshold must be finite and >= 0"; return RT_ERR_INVALID_ARG; }
    if (!(p->darkFloor > 0.0f) || !rt_dn_finite(p->darkFloor)) { *why = "darkFloor must be finite and > 0"; return RT_ERR_INVALID_ARG; }
    if (p->minFrames < 0) { *why = "minFrames must be >= 0"; return RT_ERR_INVALID_ARG; }
    if (p->maxFrames < 0) { *why = "maxFrames must be >= 0 (0 = no cap)"; return RT_ERR_INVALID_ARG; }
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) { *why = "reserved must be 0"; return RT_ERR_INVALID_ARG; }
    job->threshold = p->threshold;
    job->darkFloor = p->darkFloor;
    job->minFrames = p->minFrames;
    job->maxFrames = p->maxFrames;
    return RT_OK;
}

inline int tiles_x(int W) { return (W + 7) / 8; }
inline int tiles_y(int rows) { return (rows + 7) / 8; }
inline long long tiles_total(int W, int rows) { return (long long)tiles_x(W) * tiles_y(rows); }

/* A caller's list for a W x rows image: strictly increasing, every entry < tiles_total.  0 and *pixels = the pixels inside the image
 * that the listed tiles cover; otherwise 1 + the index of the first entry that breaks the rule. */
inline long long check_tiles(const uint32_t* tiles, int n, int W, int rows, uint32_t* pixels)
{
    const long long total = tiles_total(W, rows);
    const int tx_n = tiles_x(W);
    uint32_t pix = 0;
    for (int i = 0; i < n; i++) {
        if ((long long)tiles[i] >= total || (i > 0 && tiles[i] <= tiles[i - 1])) return (long long)i + 1;
        pix += rt_ad_tile_pixels((int)(tiles[i] % (uint32_t)tx_n), (int)(tiles[i] / (uint32_t)tx_n), W, rows);
    }
    if (pixels) *pixels = pix;
    return 0;
}

} // namespace rt_ad

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rt_ad {

/* Selection of a W x rows image: the tile errors, then — one workgroup — the ordered list and dCounts = {tiles_active, pixels_active, 0, 0} */
hipError_t enqueue_select(hipStream_t st, const rt_ad_job& job, int W, int rows, const void* dSum, const void* dMoments, float* dTileError, uint32_t* dTiles,
                          uint32_t* dCounts);

/* RCC:18-23 for the nFrames (> 1) staged frames of a fused launch over a list, in frame order, for the listed tiles' pixels alone */
hipError_t enqueue_accumulate_tiles(hipStream_t st, const uint32_t* dTiles, int nTiles, int W, int rows, const void* dStaging, int nFrames, size_t stride,
                                    void* dAccumulated, void* dFrameRender);

} // namespace rt_ad
#endif

#endif /* RT_ADAPTIVE_LAUNCH_H */
