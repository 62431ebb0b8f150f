/*
 * rt_sky.h — when the SUN TERM of GetEnvironmentLight (RC:167-183) can never be seen in a launch (internal; plain C++, no HIP).
 *
 *     sky(dir) = lerp(ground, lerp(1, zenith, T1), T) + pow(max(0, dot(dir, toSun)), s) * I * colour * gate
 *     T = smoothstep(-0.01, 0, dir.y), gate = T >= 1, s = 1000 / sunFocus
 *
 * A scene without a sun object has toSun = (0, -1, 0) (RCM:176): the sun stands below the ground plane, and the gate lets the term
 * through only above it.  sky_sun_unseen decides once per launch, from the launch's uniforms alone, that the sum has the bits of its
 * first addend for EVERY direction a frame kernel can hold; the kernels then skip the second (environment_light_frame, rt_kernels.h).
 * With toSun = (+-0, ty, +-0), -1 <= ty <= 0:
 *   - dir.x * (+-0) and dir.z * (+-0) are +-0, or NaN for an infinite or NaN component; dot is dir.y * ty, a zero, or NaN, and
 *     rt_max(0, NaN) = 0.
 *   - gate = 1 needs dir.y >= -RT_SKY_GATE_EDGE (-8.6287e-07, 0xb567a000: the smallest argument whose smoothstep reaches 1 in
 *     binary32; tests/sky_sun_driver.cpp finds it by bisection and checks that the gate is monotone around it).
 *       dir.y >= 0:  dot <= 0 (or NaN), so max gives +-0; log(+-0) = -inf, s * -inf = -inf for 0 < s < inf, exp(-inf) = +0; +0 * I * c
 *                    is +-0 for finite I and c, and x + (+-0) = x for x != -0.  The first addend is never a zero: at T = 1 it is
 *                    0.35 + (g - 0.35) with g in [0.08, 1].
 *       the sliver -RT_SKY_GATE_EDGE <= dir.y < 0:  dot <= |ty| * RT_SKY_Y0, Y0 = 2^-20 the edge rounded up to a power of two.  The
 *                    predicate asks pow(|ty| Y0, s) |I| max|c| <= 2^-31 (in double, with a factor 2 for the error of the fp32 log,
 *                    exp and the three roundings of the products).  The first addend is >= 0.08, where half an ulp is 2^-28: a
 *                    term an eighth of that cannot move the sum, whatever its sign.
 *   - gate = 0: the term is (pow * I * c) * 0 = +-0 as long as pow * I * c is finite.  dir is rt_normalize's result in every frame
 *     kernel (raygen and the shade block): |dir.y| <= about 1.5 (a squared length in the subnormals loses bits), or the squared length
 *     underflowed to 0 and every component is inf or NaN — then the dot product is NaN and the power 0.  pow(1.5, s) <= 2^38 for
 *     s <= RT_SKY_S_MAX, and |I|, |c| <= 2^20 each keep the product below 2^78.  dir.y = NaN has T = 0 (saturate(NaN) = 0): this case.
 * The side passes (radiance, NEE, AOV, query) take caller-made directions of any length — dir = (0, -1e30, 0) gives inf * 0 = NaN
 * in the full function — so their launches never carry the flag and their kernels do not test it (fill_args, rt_context.hip).
 * A launch that fails any clause runs the full function, as every launch did before.
 */
#ifndef RT_SKY_H
#define RT_SKY_H

#include <stdint.h>

#include <cmath>

#include "../../include/rt_abi.h"
#include "../../include/rt_math.h"

/* KArgs::useSky: bit 0 = RtParams::useSky != 0, bit 1 = the launch's sun term is never seen (frame and cost launches only) */
#define RT_USESKY_ON 1
#define RT_USESKY_SUN_UNSEEN 2

#define RT_SKY_GATE_EDGE_BITS 0xb567a000u  /* the largest |y|, y < 0, with smoothstep(-0.01, 0, y) >= 1 */
#define RT_SKY_Y0 9.5367431640625e-07f     /* 2^-20 >= 8.6287e-07 */
#define RT_SKY_S_MIN 0.125f                /* s * -inf = -inf needs s > 0; below 1/8 the sun is no disc any more */
#define RT_SKY_S_MAX 64.0f                 /* pow(1.5, s) stays far from overflow */
#define RT_SKY_SCALE_MAX 1048576.0f        /* 2^20: |sunIntensity| and every |sunColour| */
#define RT_SKY_TERM_MAX 4.656612873077393e-10 /* 2^-31: an eighth of half an ulp of 0.08 */

static inline bool sky_sun_unseen(const RtParams& p)
{
    if (!p.useSky) return false;
    if ((rt_f2u(p.dirToSun[0]) << 1) != 0u || (rt_f2u(p.dirToSun[2]) << 1) != 0u) return false; /* +-0 only */
    const float ty = p.dirToSun[1];
    if (!(ty >= -1.0f && ty <= 0.0f)) return false; /* (a NaN fails) */
    const float s = rt_div(1000 * 1, p.sunFocus);   /* environment_light's own expression */
    if (!(s >= RT_SKY_S_MIN && s <= RT_SKY_S_MAX)) return false;
    const float in = rt_abs(p.sunIntensity);
    if (!(in <= RT_SKY_SCALE_MAX)) return false;
    float cmax = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float c = rt_abs(p.sunColour[k]);
        if (!(c <= RT_SKY_SCALE_MAX)) return false;
        if (c > cmax) cmax = c;
    }
    const double peak = std::pow((double)rt_abs(ty) * (double)RT_SKY_Y0, (double)s) * (double)in * (double)cmax;
    return 2.0 * peak <= RT_SKY_TERM_MAX;
}

#endif
