/*
 * rt_denoise_math.h — the per-pixel and per-tap arithmetic of rt_denoise (include/rt_denoise.h states it op by op; this is that
 * text as code).  HIP-free: it includes rt_math.h alone and every function is RT_HD, so the kernels of rt_denoise.hip and the host
 * driver tests/denoise_math_driver.cpp evaluate the same operations.  One fp32 rounding per operation, no contraction (FPFLAGS).
 *
 * A pixel travels as 16-byte quantities:
 *   colour  (c.r, c.g, c.b, alpha)              scaled, demodulated; alpha rides along untouched
 *   guide0  (n.x, n.y, n.z, bits of object)     guide1  (pos.x, pos.y, pos.z, bits of the demodulation mask)
 * and an RtPixelAov record is read as its four 16-byte quarters: (dst, n) (pos, hit) (albedo, object) (emission, triangle).
 */
#ifndef RT_DENOISE_MATH_H
#define RT_DENOISE_MATH_H

#include "../../include/rt_math.h"

struct rt_dn4 { float x, y, z, w; };                 /* one aligned 16-byte load */
struct rt_dn_sums { float w, c0, c1, c2; };          /* sum_w, sum_c[0..2] */

#define RT_DN_ALBEDO_MIN 0.00390625f /* 1/256: a channel is demodulated only above this */

RT_HD rt_dn4 rt_dn_make4(float x, float y, float z, float w) { rt_dn4 r = {x, y, z, w}; return r; }
RT_HD bool rt_dn_finite(float x) { return (rt_f2u(x) & 0x7f800000u) != 0x7f800000u; }
RT_HD bool rt_dn_finite3(rt_dn4 c) { return rt_dn_finite(c.x) && rt_dn_finite(c.y) && rt_dn_finite(c.z); }

/* a_x = 1 / (sigma_x * sigma_x): host only, IEEE product and divide */
inline float rt_dn_inv_sq(float sigma) { const float s2 = sigma * sigma; return 1.0f / s2; }
/* aC_i = aC * 4^i */
inline float rt_dn_colour_scale(float aC, int pass) { return aC * (float)(1u << (2 * pass)); }

/* h[d + 2], d = -2 ... 2 */
RT_HD float rt_dn_h(int d)
{
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

/* Prepare: the input pixel and quarters 0, 1, 2 of its record -> colour, guide0, guide1 */
RT_HD void rt_dn_prepare(rt_dn4 in, rt_dn4 q0, rt_dn4 q1, rt_dn4 q2, float scale, int demodulate, rt_dn4* colour, rt_dn4* g0, rt_dn4* g1)
{
    rt_dn4 c = rt_dn_make4(in.x * scale, in.y * scale, in.z * scale, in.w);
    uint32_t mask = 0u;
    const int32_t object = (int32_t)rt_f2u(q2.w);
    if (demodulate && object >= 0 && (rt_f2u(q1.w) & 3u) == 1u && rt_dn_finite3(c)) {
        if (q2.x > RT_DN_ALBEDO_MIN) { c.x = rt_div(c.x, q2.x); mask |= 1u; }
        if (q2.y > RT_DN_ALBEDO_MIN) { c.y = rt_div(c.y, q2.y); mask |= 2u; }
        if (q2.z > RT_DN_ALBEDO_MIN) { c.z = rt_div(c.z, q2.z); mask |= 4u; }
    }
    *colour = c;
    *g0 = rt_dn_make4(q0.y, q0.z, q0.w, q2.w);
    *g1 = rt_dn_make4(q1.x, q1.y, q1.z, rt_u2f(mask));
}

/* is p filtered in a pass: a hit whose current colour is finite */
RT_HD bool rt_dn_centre_filtered(rt_dn4 cp, rt_dn4 g0p) { return (int32_t)rt_f2u(g0p.w) >= 0 && rt_dn_finite3(cp); }

/* One tap q of centre p with stencil weight k = h[dy + 2] * h[dx + 2].  `inside`: q lies in the image (when it does not, the caller
 * passes any pixel's values: they are not used).  A skipped tap adds +0 to every sum, which leaves its bits as they are (no sum is
 * ever -0), so the 25 taps run without a branch. */
RT_HD void rt_dn_tap(rt_dn_sums* s, float k, bool inside, rt_dn4 cp, rt_dn4 g0p, rt_dn4 g1p, rt_dn4 cq, rt_dn4 g0q, rt_dn4 g1q,
                     float aN, float aP, float aCi)
{
    const bool use = inside && rt_f2u(g0q.w) == rt_f2u(g0p.w) && rt_dn_finite3(cq);
    const rt_f3 dn = rt_v3(g0p.x - g0q.x, g0p.y - g0q.y, g0p.z - g0q.z);
    const rt_f3 d = rt_v3(g1q.x - g1p.x, g1q.y - g1p.y, g1q.z - g1p.z);
    const float t = rt_dot(rt_v3(g0p.x, g0p.y, g0p.z), d);
    const rt_f3 dc = rt_v3(cp.x - cq.x, cp.y - cq.y, cp.z - cq.z);
    float e = (rt_dot(dn, dn) * aN + (t * t) * aP) + rt_dot(dc, dc) * aCi;
    e = use ? e : 0.0f;
    const float w = k * rt_exp(-e);
    s->w += use ? w : 0.0f;
    s->c0 += use ? w * cq.x : 0.0f;
    s->c1 += use ? w * cq.y : 0.0f;
    s->c2 += use ? w * cq.z : 0.0f;
}

/* c'(p) of a filtered centre */
RT_HD rt_dn4 rt_dn_resolve(rt_dn_sums s, rt_dn4 cp) { return rt_dn_make4(rt_div(s.c0, s.w), rt_div(s.c1, s.w), rt_div(s.c2, s.w), cp.w); }

/* Finish: multiply the demodulated channels back (q2: quarter 2 of the record, the albedo) */
RT_HD rt_dn4 rt_dn_finish(rt_dn4 c, rt_dn4 g1p, rt_dn4 q2)
{
    const uint32_t mask = rt_f2u(g1p.w);
    return rt_dn_make4((mask & 1u) ? c.x * q2.x : c.x, (mask & 2u) ? c.y * q2.y : c.y, (mask & 4u) ? c.z * q2.z : c.z, c.w);
}

#endif /* RT_DENOISE_MATH_H */
