/*
 * rt_adaptive_math.h — the per-pixel arithmetic of include/rt_adaptive.h (which states it op by op; this is that text as code).
 * HIP-free: it includes rt_variance_math.h (and through it rt_math.h) alone and every function is RT_HD, so the selection kernel of
 * rt_adaptive.hip and the host driver tests/adaptive_math_driver.cpp evaluate the same operations.  One fp32 rounding per operation,
 * no contraction (FPFLAGS).
 */
#ifndef RT_ADAPTIVE_MATH_H
#define RT_ADAPTIVE_MATH_H

#include "rt_variance_math.h"

/* what the kernels need of RtAdaptiveParams, validated by the host */
struct rt_ad_job {
    float threshold, darkFloor;
    int minFrames, maxFrames;
};

/* "The error of a pixel", rules 1 ... 5: S the accumulated pixel, M its moments.  +inf, or finite and >= +0. */
RT_HD float rt_ad_error(rt_dn4 S, rt_dn4 M, float darkFloor, int minFrames, int maxFrames)
{
    if (!rt_vr_finite4(S)) return 0.0f;
    if (maxFrames > 0 && S.w >= (float)maxFrames) return 0.0f;
    if (S.w < (float)minFrames) return RT_INF;
    if (!(M.w >= 2.0f) || !rt_dn_finite(M.x) || !rt_dn_finite(M.y) || !rt_dn_finite(M.w)) return RT_INF;
    const float mu = rt_div(M.x, M.w);
    const float d = rt_max(M.y - mu * M.x, 0.0f);
    const float var = rt_div(d, M.w * (M.w - 1.0f));
    const float err = rt_div(rt_sqrt(var), rt_abs(mu) + darkFloor);
    return err != err ? RT_INF : err;
}

/* the maximum of two pixel errors (neither is a NaN) */
RT_HD float rt_ad_max(float a, float b) { return a > b ? a : b; }

RT_HD bool rt_ad_active(float tileErr, float threshold) { return tileErr > threshold; }

/* pixels of tile (tx, ty) inside a W x rows image */
RT_HD uint32_t rt_ad_tile_pixels(int tx, int ty, int W, int rows)
{
    const int w = W - 8 * tx < 8 ? W - 8 * tx : 8;
    const int h = rows - 8 * ty < 8 ? rows - 8 * ty : 8;
    return (uint32_t)(w * h);
}

#endif /* RT_ADAPTIVE_MATH_H */
