/*
 * rt_variance_math.h — the per-pixel and per-tap arithmetic of include/rt_variance.h (which states it op by op; this is that text as
 * code).  HIP-free: it includes rt_denoise_math.h (and through it rt_math.h) alone and every function is RT_HD, so the kernels of
 * rt_variance.hip and the host driver tests/variance_math_driver.cpp evaluate the same operations.  One fp32 rounding per operation,
 * no contraction (FPFLAGS).
 *
 * A pixel travels as rt_denoise_math.h's three 16-byte quantities, with one change: the colour's fourth word is var, not alpha.
 *   colour  (c.r, c.g, c.b, var)     guide0  (n.x, n.y, n.z, bits of object)     guide1  (pos.x, pos.y, pos.z, bits of the mask)
 * A pass may hand rt_vr_tap a guide1 whose fourth word holds l = lum(colour) instead of the mask: a tap never reads the mask.
 */
#ifndef RT_VARIANCE_MATH_H
#define RT_VARIANCE_MATH_H

#include "rt_denoise_math.h"

struct rt_vr_sums { float w, c0, c1, c2, v; };       /* sum_w, sum_c[0..2], sum_v */
struct rt_vr_gauss { float k, g; };                  /* sum_k, sum_g */

#define RT_VR_INVL_EPS 0.0001220703125f /* 0x1p-13f */

RT_HD float rt_vr_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
RT_HD float rt_vr_lum4(rt_dn4 c) { return rt_vr_lum(c.x, c.y, c.z); }
RT_HD bool rt_vr_finite4(rt_dn4 c) { return rt_dn_finite3(c) && rt_dn_finite(c.w); }

/* Update: now, snap, M -> the new M; *changed says whether M is to be written at all.  (The caller then stores snap := now.) */
RT_HD rt_dn4 rt_vr_update(rt_dn4 now, rt_dn4 snap, rt_dn4 M, bool* changed)
{
    *changed = false;
    const float dn = now.w - snap.w;
    if (!(dn > 0.0f) || !rt_vr_finite4(now) || !rt_vr_finite4(snap)) return M;
    const float L = rt_vr_lum(rt_div(now.x - snap.x, dn), rt_div(now.y - snap.y, dn), rt_div(now.z - snap.z, dn));
    const float Q = L * L;
    if (!rt_dn_finite(Q)) return M;
    *changed = true;
    return rt_dn_make4(M.x + L, M.y + Q, 0.0f, M.w + 1.0f);
}

/* Prepare, steps 1 ... 4: raw = in * scale, c = the demodulated colour, mask = its demodulation mask */
RT_HD float rt_vr_variance(rt_dn4 M, rt_dn4 raw, rt_dn4 c, uint32_t mask, float unknownVariance)
{
    float var = unknownVariance;
    if (M.w >= 2.0f && rt_dn_finite(M.x) && rt_dn_finite(M.y) && rt_dn_finite(M.w)) {
        const float mu = rt_div(M.x, M.w);
        const float d = rt_max(M.y - mu * M.x, 0.0f);
        var = rt_div(d, M.w * (M.w - 1.0f));
    }
    if (mask != 0u) {
        const float lIn = rt_vr_lum4(raw);
        if (rt_dn_finite(lIn) && lIn > 0.0f) {
            const float k = rt_div(rt_vr_lum4(c), lIn);
            var = var * (k * k);
        }
    }
    return rt_dn_finite(var) ? var : unknownVariance;
}

/* Prepare: the input pixel, its moments and quarters 0, 1, 2 of its record -> colour (with var), guide0, guide1 */
RT_HD void rt_vr_prepare(rt_dn4 in, rt_dn4 M, rt_dn4 q0, rt_dn4 q1, rt_dn4 q2, float scale, int demodulate, float unknownVariance, rt_dn4* colour,
                         rt_dn4* g0, rt_dn4* g1)
{
    const rt_dn4 raw = rt_dn_make4(in.x * scale, in.y * scale, in.z * scale, in.w);
    rt_dn4 c;
    rt_dn_prepare(in, q0, q1, q2, scale, demodulate, &c, g0, g1);
    c.w = rt_vr_variance(M, raw, c, rt_f2u(g1->w), unknownVariance);
    *colour = c;
}

/* hg[d + 1], d = -1 ... 1 */
RT_HD float rt_vr_hg(int d) { return d == 0 ? 0.5f : 0.25f; }

RT_HD bool rt_vr_used(bool inside, rt_dn4 g0p, rt_dn4 cq, rt_dn4 g0q) { return inside && rt_f2u(g0q.w) == rt_f2u(g0p.w) && rt_dn_finite3(cq); }

/* One prefilter tap with weight k = hg[dy + 1] * hg[dx + 1]; a skipped tap adds +0, which leaves the sums' bits as they are */
RT_HD void rt_vr_gauss_tap(rt_vr_gauss* s, float k, bool inside, rt_dn4 g0p, rt_dn4 cq, rt_dn4 g0q)
{
    const bool use = rt_vr_used(inside, g0p, cq, g0q);
    s->k += use ? k : 0.0f;
    s->g += use ? k * cq.w : 0.0f;
}

RT_HD float rt_vr_inv_l(rt_vr_gauss s, float sigmaLuminance) { return rt_div(1.0f, sigmaLuminance * rt_sqrt(rt_div(s.g, s.k)) + RT_VR_INVL_EPS); }

/* One tap q of centre p with stencil weight k = h[dy + 2] * h[dx + 2]; lp, lq: lum of the two colours */
RT_HD void rt_vr_tap(rt_vr_sums* s, float k, bool inside, float lp, rt_dn4 g0p, rt_dn4 g1p, rt_dn4 cq, float lq, rt_dn4 g0q, rt_dn4 g1q, float aN, float aP,
                     float invL)
{
    const bool use = rt_vr_used(inside, g0p, cq, g0q);
    const rt_f3 dn = rt_v3(g0p.x - g0q.x, g0p.y - g0q.y, g0p.z - g0q.z);
    const rt_f3 d = rt_v3(g1q.x - g1p.x, g1q.y - g1p.y, g1q.z - g1p.z);
    const float t = rt_dot(rt_v3(g0p.x, g0p.y, g0p.z), d);
    float e = (rt_dot(dn, dn) * aN + (t * t) * aP) + rt_abs(lp - lq) * invL;
    e = use ? e : 0.0f;
    const float w = k * rt_exp(-e);
    s->w += use ? w : 0.0f;
    s->c0 += use ? w * cq.x : 0.0f;
    s->c1 += use ? w * cq.y : 0.0f;
    s->c2 += use ? w * cq.z : 0.0f;
    s->v += use ? (w * w) * cq.w : 0.0f;
}

/* (c', var') of a filtered centre */
RT_HD rt_dn4 rt_vr_resolve(rt_vr_sums s) { return rt_dn_make4(rt_div(s.c0, s.w), rt_div(s.c1, s.w), rt_div(s.c2, s.w), rt_div(s.v, s.w * s.w)); }

/* Finish: multiply the demodulated channels back (mask: the centre's; q2: quarter 2 of its record), alpha from the input image */
RT_HD rt_dn4 rt_vr_finish(rt_dn4 c, uint32_t mask, rt_dn4 q2, float alpha)
{
    return rt_dn_make4((mask & 1u) ? c.x * q2.x : c.x, (mask & 2u) ? c.y * q2.y : c.y, (mask & 4u) ? c.z * q2.z : c.z, alpha);
}

#endif /* RT_VARIANCE_MATH_H */
