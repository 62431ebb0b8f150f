/* rt_math_device.h — the kernels' instruction sequences for the transcendental functions of include/rt_math.h: the SAME bits in fewer vector
 * issue slots.  include/rt_math.h stays the one definition of the arithmetic (the host, the oracle and the compiled reference text build it,
 * and its text is pinned by their manifest); what is here restates log, exp, the sine / cosine pair and smoothstep for the device with two
 * kinds of change, each marked where it is made:
 *   (1) where a product a*b is exact in binary32, fmaf(a, b, c) rounds a*b + c once, as the separate multiply and add do.  The multiplier
 *       ranges are enumerated against double-precision products on the host by tests/math_fusion_driver.cpp;
 *   (2) tests of an argument's class in fewer compares and selects.
 * Everything else — constants, polynomials, the order of every operation — is rt_math.h's, through its own helpers (rt_div_narrow,
 * rt_sin_kernel, rt_saturate, RT_WAVE_ALL).  tools/ubench/exact_math.hip compares each function here with rt_math.h's over all 2^32 arguments
 * on the device (0 mismatches, profiles/r17_issue_cost.txt); tests/test_gpu_math_paths.py compares them with the host's bits in the suite.
 * A kernel calls either these or rt_math.h's for a function, never both: a second inlined rt_log spills in every trace kernel.
 * Not taken over, because they cost a BVH kernel scratch (same file): the signs of sine and cosine as sign-bit logic, the second Cody-Waite
 * step fused behind a narrower wave bound, and log's three class tests as one range test. */
#ifndef RT_MATH_DEVICE_H
#define RT_MATH_DEVICE_H

#include "../../include/rt_math.h"

#define RTD __device__ __forceinline__

RTD float rtd_smoothstep(float a, float inv_range, float x)
{
    float t = rt_saturate((x - a) * inv_range);
    return t * t * __builtin_fmaf(-2.0f, t, 3.0f); /* (1) 2 t is exact: t in [0, 1] */
}
RTD float rtd_smoothstep_edges(float a, float b, float x) { return rtd_smoothstep(a, 1.0f / (b - a), x); }

RTD float rtd_log(float x)
{
    const float ln2_hi = 6.9313812256e-01f; /* 0x3f317180 */
    const float ln2_lo = 9.0580006145e-06f; /* 0x3717f7d1 */
    const float Lg1 = 0.66666662693f, Lg2 = 0.40000972152f;
    const float Lg3 = 0.28498786688f, Lg4 = 0.24279078841f;
    uint32_t ix = rt_f2u(x);
    int k = 0;
    /* (2) no test for x == 1: its f = +0 and k = 0 give +0 through the arithmetic below, every term being +0 */
    if (ix < 0x00800000u || (ix >> 31)) {
        if ((ix << 1) == 0) return -RT_INF;
        if (ix >> 31) return rt_u2f(0x7fc00000u);
        k -= 25;
        x *= 33554432.0f;
        ix = rt_f2u(x);
    } else if (ix >= 0x7f800000u) {
        return x;
    }
    ix += 0x3f800000u - 0x3f3504f3u;
    k += (int)(ix >> 23) - 0x7f;
    ix = (ix & 0x007fffffu) + 0x3f3504f3u;
    x = rt_u2f(ix);
    float f = x - 1.0f;
    float s = rt_div_narrow(f, 2.0f + f);
    float z = s * s;
    float w = z * z;
    float t1 = w * (Lg2 + w * Lg4);
    float t2 = z * (Lg1 + w * Lg3);
    float R = t2 + t1;
    float hfsq = 0.5f * f * f;
    float dk = (float)k;
    return __builtin_fmaf(dk, ln2_hi, s * (hfsq + R) + dk * ln2_lo - hfsq + f); /* (1) k ln2_hi is exact: 17 significant bits x |k| <= 149 */
}

RTD float rtd_exp_ordinary(float x)
{
    const float ln2hi = 6.9314575195e-1f, ln2lo = 1.4286067653e-6f, invln2 = 1.4426950216e+0f;
    const float P1 = 1.6666625440e-1f, P2 = -2.7667332906e-3f;
    const int sign = (int)(rt_f2u(x) >> 31);
    const bool under = rt_f2u(x) >= 0xc2cff1b5u; /* (2) the sign and the magnitude in one unsigned compare */
    if (under) x = 0.0f;
    const uint32_t hx = rt_f2u(x) & 0x7fffffffu; /* (of the stand-in, where it stands in: 0) */
    const bool big = hx > 0x3f851592u, mid = hx > 0x3eb17218u, tiny = !(hx > 0x39000000u);
    const int kb = (int)(invln2 * x + (sign ? -0.5f : 0.5f));
    const int k = big ? kb : (mid ? 1 - sign - sign : 0);
    const float fk = (float)k;
    const float hi = __builtin_fmaf(-fk, ln2hi, x); /* (1) k ln2hi is exact: 15 significant bits x |k| <= 126 */
    const float lo = fk * ln2lo;
    const float xr = hi - lo;
    const float xx = xr * xr;
    const float c = xr - xx * (P1 + xx * P2);
    const float y = 1.0f + (rt_div_narrow(xr * c, 2.0f - c) - lo + hi);
    const float r = y * rt_u2f((uint32_t)(k + 127) << 23);
    return under ? 0.0f : (tiny ? 1.0f + x : r);
}
RTD float rtd_exp(float x)
{
    const float ln2hi = 6.9314575195e-1f;  /* 0x3f317200 */
    const float ln2lo = 1.4286067653e-6f;  /* 0x35bfbe8e */
    const float invln2 = 1.4426950216e+0f;
    const float P1 = 1.6666625440e-1f, P2 = -2.7667332906e-3f;
    uint32_t hx = rt_f2u(x);
    int sign = (int)(hx >> 31);
    hx &= 0x7fffffffu;
    /* (2) the wave-uniform branch's set — the result is normal, or -inf <= x <= -103.97... underflows to 0 — with one range test for its second half */
    if (RT_WAVE_ALL(hx < 0x42aeac50u || rt_f2u(x) - 0xc2cff1b5u <= 0xff800000u - 0xc2cff1b5u)) return rtd_exp_ordinary(x);
    if (hx >= 0x42aeac50u) {
        if (hx > 0x7f800000u) return x;
        if (hx >= 0x42b17218u && !sign) return RT_INF;
        if (sign && hx >= 0x42cff1b5u) return 0.0f;
    }
    float hi, lo;
    int k;
    if (hx > 0x3eb17218u) {
        if (hx > 0x3f851592u)
            k = (int)(invln2 * x + (sign ? -0.5f : 0.5f));
        else
            k = 1 - sign - sign;
        float fk = (float)k;
        hi = __builtin_fmaf(-fk, ln2hi, x); /* (1) exact product: |k| <= 150 here */
        lo = fk * ln2lo;
        x = hi - lo;
    } else if (hx > 0x39000000u) {
        k = 0;
        hi = x;
        lo = 0.0f;
    } else {
        return 1.0f + x;
    }
    float xx = x * x;
    float c = x - xx * (P1 + xx * P2);
    float y = 1.0f + (rt_div_narrow(x * c, 2.0f - c) - lo + hi);
    if (k == 0) return y;
    if (k > 127) { y *= 1.7014118346e38f; k -= 127; }
    if (k < -126) {
        y *= rt_u2f((uint32_t)(k + 24 + 127) << 23);
        return y * 5.9604644775e-8f;
    }
    return y * rt_u2f((uint32_t)(k + 127) << 23);
}
RTD float rtd_pow(float x, float y) { return rtd_exp(y * rtd_log(x)); }

RTD int rtd_reduce_pio2(float x, float* r)
{
    const float TWO_OVER_PI = 0.636619772f;
    const float P1 = 1.5703125f;
    const float P2 = 4.837512969970703125e-4f;
    const float P3 = 7.54978995489188216e-8f;
    float q = x * TWO_OVER_PI;
    int n = (int)(q + (q < 0.0f ? -0.5f : 0.5f));
    float fn = (float)n;
    float t = __builtin_fmaf(-fn, P1, x); /* (1) n P1 is exact: 8 significant bits x |n| < 2^16.  (n P2 is exact for |n| < 2^13 only; the callers admit |x| < 3e4.) */
    t = t - fn * P2;
    t = t - fn * P3;
    *r = t;
    return n;
}
RTD float rtd_cos_kernel(float r)
{
    float z = r * r;
    float p = (2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f;
    return __builtin_fmaf(-0.5f, z, 1.0f) + z * z * p; /* (1) z / 2 is exact, or so small that 1 - z / 2 is 1 either way */
}
RTD float rtd_sin(float x)
{
    if (RT_WAVE_ALL(rt_abs(x) < 3.0e4f)) { /* wave-uniform branch */
        float r;
        int n = rtd_reduce_pio2(x, &r);
        float s = (n & 1) ? rtd_cos_kernel(r) : rt_sin_kernel(r);
        return (n & 2) ? -s : s;
    }
    if (!(rt_abs(x) < 3.0e4f)) return (x != x || rt_abs(x) == RT_INF) ? rt_u2f(0x7fc00000u) : 0.0f;
    float r;
    int n = rtd_reduce_pio2(x, &r);
    float s = (n & 1) ? rtd_cos_kernel(r) : rt_sin_kernel(r);
    return (n & 2) ? -s : s;
}
RTD float rtd_cos(float x)
{
    if (RT_WAVE_ALL(rt_abs(x) < 3.0e4f)) { /* wave-uniform branch */
        float r;
        int n = rtd_reduce_pio2(x, &r);
        float c = (n & 1) ? rt_sin_kernel(r) : rtd_cos_kernel(r);
        return ((n + 1) & 2) ? -c : c;
    }
    if (!(rt_abs(x) < 3.0e4f)) return (x != x || rt_abs(x) == RT_INF) ? rt_u2f(0x7fc00000u) : 1.0f;
    float r;
    int n = rtd_reduce_pio2(x, &r);
    float c = (n & 1) ? rt_sin_kernel(r) : rtd_cos_kernel(r);
    return ((n + 1) & 2) ? -c : c;
}
RTD void rtd_sincos(float x, float* s_out, float* c_out)
{
    if (RT_WAVE_ALL(rt_abs(x) < 3.0e4f)) { /* wave-uniform branch */
        float r;
        int n = rtd_reduce_pio2(x, &r);
        float sk = rt_sin_kernel(r), ck = rtd_cos_kernel(r);
        float s = (n & 1) ? ck : sk;
        float c = (n & 1) ? sk : ck;
        *s_out = (n & 2) ? -s : s;
        *c_out = ((n + 1) & 2) ? -c : c;
        return;
    }
    if (!(rt_abs(x) < 3.0e4f)) {
        *s_out = rtd_sin(x);
        *c_out = rtd_cos(x);
        return;
    }
    float r;
    int n = rtd_reduce_pio2(x, &r);
    float sk = rt_sin_kernel(r), ck = rtd_cos_kernel(r);
    float s = (n & 1) ? ck : sk;
    float c = (n & 1) ? sk : ck;
    *s_out = (n & 2) ? -s : s;
    *c_out = ((n + 1) & 2) ? -c : c;
}

#undef RTD
#endif /* RT_MATH_DEVICE_H */
