/*
 * rt_motion_math.h — the per-pixel arithmetic of rt_reproject_buffers_moving and the table of rt_motion_from_scene (include/rt_motion.h
 * states both op by op; this is that text as code, on top of rt_reproject_math.h).  HIP-free, every function RT_HD: the kernel of
 * rt_reproject.hip, rt_context.hip and the host driver tests/motion_math_driver.cpp evaluate the same operations.  One fp32 rounding per
 * operation, no contraction (FPFLAGS).
 *
 * The moved pixel is the static one with (pm, nm) in the place of (a.pos, a.normal): steps 2 ... 5 of rt_reproject.h read the record's
 * position and normal nowhere else, so rt_rp_pixel is called with the two quarters rewritten and does the rest — rt_rp_locate's
 * finiteness test is then the one on pm and nm.
 */
#ifndef RT_MOTION_MATH_H
#define RT_MOTION_MATH_H

#include "rt_reproject_math.h"

struct rt_mo_entry { rt_rp4 r0, r1, r2; }; /* one RtObjectMotion: three aligned 16-byte loads, row r = (m[4r], m[4r+1], m[4r+2], m[4r+3]) */

RT_HD float rt_mo_point(rt_rp4 r, float x, float y, float z) { return ((r.x * x + r.y * y) + r.z * z) + r.w; }
RT_HD float rt_mo_vector(rt_rp4 r, float x, float y, float z) { return (r.x * x + r.y * y) + r.z * z; }

/* Rule 1' for a pixel whose object has an entry.  False: step 1's own finiteness test fails (no history). */
RT_HD bool rt_mo_apply(const rt_mo_entry& e, rt_rp4* a0, rt_rp4* a1)
{
    const rt_rp4 n = *a0, p = *a1;
    if (!(rt_rp_finite(n.y) && rt_rp_finite(n.z) && rt_rp_finite(n.w) && rt_rp_finite(p.x) && rt_rp_finite(p.y) && rt_rp_finite(p.z))) return false;
    *a0 = rt_rp_make4(n.x, rt_mo_vector(e.r0, n.y, n.z, n.w), rt_mo_vector(e.r1, n.y, n.z, n.w), rt_mo_vector(e.r2, n.y, n.z, n.w));
    *a1 = rt_rp_make4(rt_mo_point(e.r0, p.x, p.y, p.z), rt_mo_point(e.r1, p.x, p.y, p.z), rt_mo_point(e.r2, p.x, p.y, p.z), p.w);
    return true;
}

/* The whole pixel.  `src` as rt_rp_pixel's; `table.entry(k)` yields entry k and is only called for 0 <= k < nObjects. */
template <class Src, class Table>
RT_HD rt_rp4 rt_mo_pixel(const rt_rp_job& j, rt_rp4 a0, rt_rp4 a1, int32_t object, const Src& src, const Table& table, int32_t nObjects)
{
    if (object >= 0 && object < nObjects && !rt_mo_apply(table.entry(object), &a0, &a1)) return rt_rp_none();
    return rt_rp_pixel(j, a0, a1, object, src);
}

/* rt_motion_from_scene.  Column-major 4 x 4 inputs (element (r, c) at [4c + r]): m[4r + c] = (prevLocalToWorld x curWorldToLocal)(r, c). */
RT_HD void rt_mo_model_entry(const float* prevLocalToWorld, const float* curWorldToLocal, float* m)
{
    const float *A = prevLocalToWorld, *B = curWorldToLocal;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) m[4 * r + c] = ((A[r] * B[4 * c] + A[4 + r] * B[4 * c + 1]) + A[8 + r] * B[4 * c + 2]) + A[12 + r] * B[4 * c + 3];
}

RT_HD void rt_mo_sphere_entry(const float* prevCentre, const float* curCentre, float* m)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[4 * r + c] = r == c ? 1.0f : 0.0f;
        m[4 * r + 3] = prevCentre[r] - curCentre[r];
    }
}

#endif /* RT_MOTION_MATH_H */
