/* sky_sun_driver.cpp — host proof of ray-tracing_amd/csrc/rt_sky.h (tests/test_sky_sun.py builds and runs it, plain and under
 * the address and undefined-behaviour sanitizers).  GetEnvironmentLight (RC:167-183) is restated here with include/rt_math.h's functions —
 * the bits the kernels' sequences have (tests/test_gpu_math_paths.py) — once whole and once without the sun's addend, and the two are
 * compared bit for bit for every parameter set of a table the predicate accepts, over the directions a frame kernel can hold.
 * One line per row: `name key=value ...`, integers only. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../ray-tracing_amd/csrc/rt_sky.h"

static float gate_t(float y) { return rt_smoothstep_edges(-0.01f, 0.0f, y); }
static bool gate(float y) { return gate_t(y) >= 1.0f; }

static rt_f3 sky_blend(float y)
{
    float skyGradientT = rt_pow(rt_smoothstep_edges(0.0f, 0.4f, y), 0.35f);
    float groundToSkyT = rt_smoothstep_edges(-0.01f, 0.0f, y);
    rt_f3 skyGradient = rt_lerp3(rt_v3(1, 1, 1), rt_v3(0.08f, 0.37f, 0.73f), skyGradientT);
    return rt_lerp3(rt_v3(0.35f, 0.3f, 0.35f), skyGradient, groundToSkyT);
}
/* the statements of environment_light (rt_kernels.h), in their order */
static rt_f3 sky_full(const RtParams& a, rt_f3 dir)
{
    float skyGradientT = rt_pow(rt_smoothstep_edges(0.0f, 0.4f, dir.y), 0.35f);
    float groundToSkyT = rt_smoothstep_edges(-0.01f, 0.0f, dir.y);
    rt_f3 skyGradient = rt_lerp3(rt_v3(1, 1, 1), rt_v3(0.08f, 0.37f, 0.73f), skyGradientT);
    float s = rt_div(1000 * 1, a.sunFocus);
    rt_f3 toSun = rt_v3(a.dirToSun[0], a.dirToSun[1], a.dirToSun[2]);
    float sun = rt_pow(rt_max(0.0f, rt_dot(dir, toSun)), s) * a.sunIntensity;
    float gt = (groundToSkyT >= 1.0f) ? 1.0f : 0.0f;
    return rt_lerp3(rt_v3(0.35f, 0.3f, 0.35f), skyGradient, groundToSkyT)
           + sun * rt_v3(a.sunColour[0], a.sunColour[1], a.sunColour[2]) * gt;
}
static bool same_bits(rt_f3 a, rt_f3 b) { return rt_f2u(a.x) == rt_f2u(b.x) && rt_f2u(a.y) == rt_f2u(b.y) && rt_f2u(a.z) == rt_f2u(b.z); }

static RtParams make(float tx, float ty, float tz, float focus, float intensity, float cr, float cg, float cb, int useSky = 1)
{
    RtParams p;
    memset(&p, 0, sizeof(p));
    p.useSky = useSky;
    p.dirToSun[0] = tx; p.dirToSun[1] = ty; p.dirToSun[2] = tz;
    p.sunFocus = focus;
    p.sunIntensity = intensity;
    p.sunColour[0] = cr; p.sunColour[1] = cg; p.sunColour[2] = cb;
    return p;
}

static const float INF = std::numeric_limits<float>::infinity();
static const float QNAN = std::numeric_limits<float>::quiet_NaN();

/* the (x, z) a direction is crossed with; from `firstNonFinite` on, one of the two is inf or NaN */
static const float kPairs[][2] = {
    {0.0f, 0.0f}, {-0.0f, -0.0f}, {0.0f, -0.0f}, {-0.0f, 0.0f}, {0.6f, -0.3f}, {-1.0f, 1.0f}, {1.5f, 1.5f}, {1e-30f, -1e-30f}, {1e-45f, 0.0f},
    {INF, 0.0f}, {0.0f, -INF}, {QNAN, 0.0f}, {0.0f, QNAN}, {-INF, QNAN}, {INF, INF},
};
static const int kNPairs = (int)(sizeof(kPairs) / sizeof(kPairs[0])), kFirstNonFinite = 9;

struct Tally { long long evals = 0, differ = 0; };

static void compare_y(const RtParams& p, float y, int firstPair, Tally& t)
{
    const rt_f3 blend = sky_blend(y);
    for (int k = firstPair; k < kNPairs; k++) {
        const rt_f3 full = sky_full(p, rt_v3(kPairs[k][0], y, kPairs[k][1]));
        t.evals++;
        if (!same_bits(full, blend)) t.differ++;
    }
}

/* every direction class a frame kernel can hold (rt_normalize's results): `coarse` widens the two strides eightfold */
static Tally sweep(const RtParams& p, uint32_t edgeBits, int coarse)
{
    Tally t;
    /* every float within 20,000 ulps of the gate's edge */
    for (uint32_t b = edgeBits - 20000u; b <= edgeBits + 20000u; b++) compare_y(p, rt_u2f(b), 0, t);
    /* the rest of the gate-1 negative range, -0 ... the edge */
    const uint32_t s1 = 4099u * (uint32_t)coarse, s2 = 9973u * (uint32_t)coarse;
    for (uint32_t b = 0x80000000u; b <= edgeBits; b += s1) compare_y(p, rt_u2f(b), 0, t);
    /* |y| <= 2, both signs */
    for (uint32_t b = 0u; b <= 0x40000000u; b += s2) {
        compare_y(p, rt_u2f(b), 0, t);
        compare_y(p, rt_u2f(b | 0x80000000u), 0, t);
    }
    /* special values */
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1.5f, -1.5f, 2.0f, -2.0f, 0.4f, -0.01f, 1e-45f, -1e-45f, 1.17549435e-38f, -1.17549435e-38f,
                             rt_u2f(edgeBits), rt_u2f(edgeBits + 1u), rt_u2f(edgeBits - 1u), -RT_SKY_Y0, INF, QNAN, -QNAN};
    for (float y : special) compare_y(p, y, 0, t);
    /* y = -inf is what a squared length of 0 leaves: then x and z are inf or NaN as well (v * rsqrt(0)) */
    compare_y(p, -INF, kFirstNonFinite, t);
    return t;
}

int main()
{
    /* ---- the gate's edge: the largest |y|, y < 0, with gate(y); gate(-0) holds, gate(-0.01) does not */
    uint32_t lo = 0x80000000u, hi = rt_f2u(-0.01f);
    const int endsOk = gate(rt_u2f(lo)) && !gate(rt_u2f(hi));
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (gate(rt_u2f(mid))) lo = mid; else hi = mid;
    }
    const uint32_t edge = lo;
    long long notMonotone = 0;
    for (uint32_t b = edge - 20000u; b <= edge + 20000u; b++) {
        if (gate(rt_u2f(b)) != (b <= edge)) notMonotone++;
        if (b > edge - 20000u && gate_t(rt_u2f(b)) > gate_t(rt_u2f(b - 1u))) notMonotone++; /* t falls as |y| grows */
    }
    const float y0 = RT_SKY_Y0, edgeMag = rt_abs(rt_u2f(edge));
    const int y0Covers = y0 >= edgeMag && 0.5f * y0 < edgeMag;
    const int y0PowerOfTwo = (rt_f2u(y0) & 0x007fffffu) == 0u;
    printf("gate ends_ok=%d edge_bits=%lld header_bits=%lld not_monotone=%lld y0_covers=%d y0_power_of_two=%d\n", endsOk, (long long)edge,
           (long long)RT_SKY_GATE_EDGE_BITS, notMonotone, y0Covers, y0PowerOfTwo);

    /* ---- accepted parameter sets: full == shortened, bit for bit */
    const float B = RT_SKY_SCALE_MAX;
    struct Row { const char* name; RtParams p; int coarse; };
    const std::vector<Row> accepted = {
        {"default", make(0, -1, 0, 500, 10, 1, 1, 1), 1},                     /* RCM:173-176 without a sun object */
        {"near_the_bound", make(0, -1, 0, 560, 10, 1, 1, 1), 1},              /* s = 1.786: 2 x 2^-35.7 x 10 = 2^-31.4, the largest term the predicate lets pass */
        {"y_half", make(0, -0.5f, 0, 500, 10, 1, 0.9f, 0.6f), 8},
        {"y_neg_zero", make(0, -0.0f, 0, 500, 10, 1, 0.9f, 0.6f), 8},
        {"y_pos_zero", make(0, 0.0f, 0, 500, 10, 1, 0.9f, 0.6f), 8},
        {"xz_neg_zero", make(-0.0f, -1, -0.0f, 500, 10, 1, 0.9f, 0.6f), 8},
        {"focus_low_end", make(0, -1, 0, 15.625f, 10, 1, 0.9f, 0.6f), 8},      /* s = 64 */
        {"focus_high_end", make(0, -0.0f, 0, 8000, 10, 1, 0.9f, 0.6f), 8},     /* s = 1/8: only a sun whose dot product is always a zero passes */
        {"focus_high_end_dark", make(0, -1, 0, 8000, 0, 1, 0.9f, 0.6f), 8},    /* ... or one without light */
        {"scale_bounds", make(0, -1, 0, 100, B, -B, B, B), 8},                 /* s = 10: 2^-200 x 2^40 */
        {"negative_light", make(0, -1, 0, 250, -B, 1, -0.5f, 0.25f), 8},       /* s = 4: 2^-80 x 2^20 */
    };
    for (const Row& r : accepted) {
        const int ok = sky_sun_unseen(r.p) ? 1 : 0;
        const Tally t = sweep(r.p, edge, r.coarse);
        printf("accept_%s accepted=%d evals=%lld differ=%lld\n", r.name, ok, t.evals, t.differ);
    }

    /* ---- refused parameter sets, one row each */
    const std::vector<Row> refused = {
        {"tilted_sun", make(1e-30f, -1, 0, 500, 10, 1, 0.9f, 0.6f), 0},
        {"sun_above", make(0, 1, 0, 500, 10, 1, 0.9f, 0.6f), 0},
        {"long_sun", make(0, -1.5f, 0, 500, 10, 1, 0.9f, 0.6f), 0},
        {"nan_sun", make(0, QNAN, 0, 500, 10, 1, 0.9f, 0.6f), 0},
        {"focus_zero", make(0, -1, 0, 0, 10, 1, 0.9f, 0.6f), 0},
        {"focus_huge", make(0, -1, 0, 1e30f, 10, 1, 0.9f, 0.6f), 0},
        {"focus_negative", make(0, -1, 0, -500, 10, 1, 0.9f, 0.6f), 0},
        {"focus_nan", make(0, -1, 0, QNAN, 10, 1, 0.9f, 0.6f), 0},
        {"intensity_inf", make(0, -1, 0, 500, INF, 1, 0.9f, 0.6f), 0},
        {"intensity_nan", make(0, -1, 0, 500, QNAN, 1, 0.9f, 0.6f), 0},
        {"colour_huge", make(0, -1, 0, 500, 10, 1, 1e30f, 0.6f), 0},
        {"colour_nan", make(0, -1, 0, 500, 10, 1, 0.9f, QNAN), 0},
        {"visible_in_the_sliver", make(0, -1, 0, 2000, 1000, 1, 1, 1), 0},     /* s = 1/2: sqrt(2^-20) x 1000 is no rounding error */
        {"sky_off", make(0, -1, 0, 500, 10, 1, 0.9f, 0.6f, 0), 0},
    };
    for (const Row& r : refused) printf("refuse_%s accepted=%d\n", r.name, sky_sun_unseen(r.p) ? 1 : 0);

    /* ---- why the side passes never carry the flag: a caller-made direction of any length.  (0, -1e30, 0) under the default sun is
     * pow(1e30, 2) = inf, inf * 0 = NaN in the whole function and the plain blend without the sun */
    {
        const RtParams p = accepted[0].p;
        Tally t;
        const rt_f3 d = rt_v3(0.0f, -1e30f, 0.0f);
        const rt_f3 full = sky_full(p, d), blend = sky_blend(d.y);
        t.evals = 1;
        t.differ = same_bits(full, blend) ? 0 : 1;
        printf("unnormalised_direction evals=%lld differ=%lld full_is_nan=%d\n", t.evals, t.differ, full.x != full.x ? 1 : 0);
    }
    return 0;
}
