/*
 * rt_reproject_math.h — the per-pixel arithmetic of rt_reproject and rt_resolve (include/rt_reproject.h states it op by op; this is
 * that text as code).  HIP-free: it includes rt_math.h alone and every function is RT_HD, so the kernels of rt_reproject.hip and the
 * host driver tests/reproject_math_driver.cpp evaluate the same operations.  One fp32 rounding per operation, no contraction (FPFLAGS).
 *
 * An RtPixelAov record is read as 16-byte quarters: quarter 0 = (dst, normal), quarter 1 = (pos, hit); `object` is the last word of
 * quarter 2.  A pixel of an image is one 16-byte quantity (r, g, b, a).
 */
#ifndef RT_REPROJECT_MATH_H
#define RT_REPROJECT_MATH_H

#include "../../include/rt_math.h"

struct rt_rp4 { float x, y, z, w; };                  /* one aligned 16-byte load */
struct rt_rp_sums { float w, n, c0, c1, c2; };        /* sum_w, sum_n, sum_c[0..2] */

/* the call's parameters as the kernel takes them */
struct rt_rp_job {
    float R[3], U[3], F[3], O[3];   /* columns 0 ... 3 of prevCamLocalToWorld, three rows each */
    float pw, ph, fd;               /* prevViewParams */
    float maxPlaneDistance, minNormalDot, maxHistory;
    int glass;                      /* bit 0 of flags */
    int W, H;
};

RT_HD rt_rp4 rt_rp_make4(float x, float y, float z, float w) { rt_rp4 r = {x, y, z, w}; return r; }
RT_HD bool rt_rp_finite(float x) { return (rt_f2u(x) & 0x7f800000u) != 0x7f800000u; }
RT_HD rt_rp4 rt_rp_none() { return rt_rp_make4(0.0f, 0.0f, 0.0f, 0.0f); }

/* Rules 0 ... 3: does pixel p have a place in the previous image, and where.  a0, a1: quarters 0 and 1 of its record. */
RT_HD bool rt_rp_locate(const rt_rp_job& j, rt_rp4 a0, rt_rp4 a1, int32_t object, float* fx, float* fy)
{
    if (j.W == 1 || j.H == 1) return false;
    if (object < 0) return false;
    if ((rt_f2u(a1.w) & 3u) == 2u && !j.glass) return false;
    if (!(rt_rp_finite(a0.y) && rt_rp_finite(a0.z) && rt_rp_finite(a0.w) && rt_rp_finite(a1.x) && rt_rp_finite(a1.y) && rt_rp_finite(a1.z))) return false;
    const rt_f3 d = rt_v3(a1.x - j.O[0], a1.y - j.O[1], a1.z - j.O[2]);
    const float lx = rt_dot(rt_v3(j.R[0], j.R[1], j.R[2]), d);
    const float ly = rt_dot(rt_v3(j.U[0], j.U[1], j.U[2]), d);
    const float lz = rt_dot(rt_v3(j.F[0], j.F[1], j.F[2]), d);
    if (!(lz > 0.0f)) return false;
    const float u = rt_div(lx * j.fd, lz * j.pw) + 0.5f;
    const float v = rt_div(ly * j.fd, lz * j.ph) + 0.5f;
    const float x = u * (float)(j.W - 1);
    const float y = v * (float)(j.H - 1);
    if (!(rt_rp_finite(x) && rt_rp_finite(y) && x > -1.0f && x < (float)j.W && y > -1.0f && y < (float)j.H)) return false;
    *fx = x;
    *fy = y;
    return true;
}

/* Rule 4, one tap inside the image: P = the previous sum at q, b0, b1 = quarters 0 and 1 of the previous record at q */
RT_HD void rt_rp_tap(rt_rp_sums* s, const rt_rp_job& j, float w, rt_rp4 a0, rt_rp4 a1, int32_t object, rt_rp4 P, rt_rp4 b0, rt_rp4 b1, int32_t objectQ)
{
    if (objectQ != object) return;
    const rt_f3 n = rt_v3(a0.y, a0.z, a0.w);
    if (!(rt_dot(n, rt_v3(b0.y, b0.z, b0.w)) >= j.minNormalDot)) return;
    const rt_f3 d = rt_v3(b1.x - a1.x, b1.y - a1.y, b1.z - a1.z);
    if (!(rt_abs(rt_dot(n, d)) <= j.maxPlaneDistance)) return;
    if (!(rt_rp_finite(P.x) && rt_rp_finite(P.y) && rt_rp_finite(P.z) && rt_rp_finite(P.w))) return;
    if (!(P.w > 0.0f)) return;
    s->w += w;
    s->c0 += w * rt_div(P.x, P.w);
    s->c1 += w * rt_div(P.y, P.w);
    s->c2 += w * rt_div(P.z, P.w);
    s->n += w * P.w;
}

/* Rule 5 */
RT_HD rt_rp4 rt_rp_result(const rt_rp_job& j, rt_rp_sums s)
{
    if (!(s.w > 0.0f)) return rt_rp_none();
    const float x = rt_div(s.n, s.w);
    const float n = x < j.maxHistory ? x : j.maxHistory;
    return rt_rp_make4(rt_div(s.c0, s.w) * n, rt_div(s.c1, s.w) * n, rt_div(s.c2, s.w) * n, n);
}

/* The whole pixel.  `src` yields the previous image and records: src.colour(i), src.q0(i), src.q1(i), src.object(i) for the linear
 * pixel index i = y * W + x. */
template <class Src>
RT_HD rt_rp4 rt_rp_pixel(const rt_rp_job& j, rt_rp4 a0, rt_rp4 a1, int32_t object, const Src& src)
{
    float fx, fy;
    if (!rt_rp_locate(j, a0, a1, object, &fx, &fy)) return rt_rp_none();
    const float xf = rt_floor(fx), yf = rt_floor(fy);
    const float tx = fx - xf, ty = fy - yf;
    const int x0 = (int)xf, y0 = (int)yf; /* in [-1, W - 1] and [-1, H - 1]: rt_rp_locate */
    rt_rp_sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int jj = 0; jj < 2; jj++) {
        for (int ii = 0; ii < 2; ii++) {
            const int qx = x0 + ii, qy = y0 + jj;
            if (qx < 0 || qx >= j.W || qy < 0 || qy >= j.H) continue;
            const float w = (ii ? tx : 1.0f - tx) * (jj ? ty : 1.0f - ty);
            const size_t i = (size_t)qy * (size_t)j.W + (size_t)qx;
            rt_rp_tap(&s, j, w, a0, a1, object, src.colour(i), src.q0(i), src.q1(i), src.object(i));
        }
    }
    return rt_rp_result(j, s);
}

/* Resolve */
RT_HD rt_rp4 rt_rp_resolve(rt_rp4 s)
{
    if (!(s.w > 0.0f)) return rt_rp_make4(0.0f, 0.0f, 0.0f, s.w);
    return rt_rp_make4(rt_div(s.x, s.w), rt_div(s.y, s.w), rt_div(s.z, s.w), s.w);
}

#endif /* RT_REPROJECT_MATH_H */
