// Host proof of the exact-product fusions of the kernels' math sequences (ray-tracing_amd/csrc/rt_math_device.h): where a*b is exact in binary32,
// fmaf(a, b, c) has the bits of a*b + c, because both round the same real number once.  For every multiplier a function can produce
// the product is compared with the double-precision product (24 x 24 bits fit a double: that one is exact), which decides exactness;
// then the fused and the unfused forms are compared bit for bit, std::fma against multiply-then-add, over addends the function meets.
// One line per fusion: name, multipliers, inexact products, addends tried, differing results.  Built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float fromBits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t rngState = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rngState = rngState * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rngState >> 32); }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) * (1.0f / 16777216.0f); }

static bool exactProduct(float a, float b)
{
    volatile float p = a * b;
    return (double)p == (double)a * (double)b;
}

struct Tally { long mult = 0, inexact = 0, addends = 0, differ = 0; };
static void report(const char* name, const Tally& t) { std::printf("%s multipliers=%ld inexact=%ld addends=%ld differ=%ld\n", name, t.mult, t.inexact, t.addends, t.differ); }

// c - m*k against fma(-m, k, c)  (sub = true), or c + m*k against fma(m, k, c)
static void tryAddend(Tally& t, float m, float k, float c, bool sub)
{
    volatile float prod = m * k;
    volatile float plain = sub ? c - prod : c + prod;
    const float fused = sub ? std::fma(-m, k, c) : std::fma(m, k, c);
    t.addends++;
    if (bits(plain) != bits(fused) && !(plain != plain && fused != fused)) t.differ++;
}

int main()
{
    const float P1 = 1.5703125f, P2 = 4.837512969970703125e-4f, TWO_OVER_PI = 0.636619772f;
    const float expLn2hi = 6.9314575195e-1f, logLn2hi = 6.9313812256e-01f;

    // rt_reduce_pio2, first step: t = x - n P1.  rt_sin / rt_cos / rt_sincos reduce |x| < 3e4: |n| <= 19099.
    {
        Tally t;
        for (int n = -19100; n <= 19100; n++) {
            t.mult++;
            if (!exactProduct((float)n, P1)) t.inexact++;
            for (int j = 0; j < 64; j++) { // arguments that round to this n, and a few that do not
                const float x = ((float)n + uniform(-0.6f, 0.6f)) / TWO_OVER_PI;
                tryAddend(t, (float)n, P1, x, true);
            }
            const float edge[] = {0.0f, -0.0f, (float)n * P1, -(float)n * P1, 3.0e4f, -3.0e4f, 6.2831855f, fromBits(1u), fromBits(0x00800000u)};
            for (float x : edge) tryAddend(t, (float)n, P1, x, true);
        }
        report("reduce_P1", t);
    }
    // ... second step, t - n P2: exact for |n| < 2^13 (the header's note), NOT for every n the callers admit: that step stays unfused
    {
        Tally small, all;
        for (int n = -19100; n <= 19100; n++) {
            Tally& t = (n > -8192 && n < 8192) ? small : all;
            t.mult++;
            if (!exactProduct((float)n, P2)) t.inexact++;
        }
        report("reduce_P2_below_8192", small);
        report("reduce_P2_above", all);
    }
    // rt_cos_kernel: 1 - z/2 with z = r r >= 0.  z/2 is exact unless z is subnormal with an odd last bit (or 2^-126 .. 2^-125 odd): then both forms give 1.
    // rt_smoothstep: 3 - 2 t with t in [0, 1].  Every exponent, 4096 random mantissas and the ends of each binade.
    {
        Tally tc, tiny, ts;
        static const uint32_t ends[6] = {0u, 1u, 2u, 0x7fffffu, 0x7ffffeu, 0x400000u};
        for (uint32_t e = 0; e <= 127; e++)
            for (int j = 0; j < 4102; j++) {
                const uint32_t man = j < 4096 ? rnd() & 0x7fffffu : ends[j - 4096];
                const float z = fromBits((e << 23) | man);
                Tally& t = e >= 2 ? tc : tiny; // below 2^-125 halving can drop a bit: only the results have to agree there
                t.mult++;
                if (!exactProduct(0.5f, z)) t.inexact++;
                tryAddend(t, 0.5f, z, 1.0f, true);
                if (z <= 1.0f) {
                    ts.mult++;
                    if (!exactProduct(2.0f, z)) ts.inexact++;
                    tryAddend(ts, 2.0f, z, 3.0f, true);
                }
            }
        for (float t : {0.0f, -0.0f, 1.0f}) { ts.mult++; if (!exactProduct(2.0f, t)) ts.inexact++; tryAddend(ts, 2.0f, t, 3.0f, true); }
        report("cos_half_z", tc);
        report("cos_half_z_below_2^-125", tiny);
        report("smoothstep_2t", ts);
    }
    // rt_exp, both forms: hi = x - k ln2hi.  k = (int)(x / ln 2 +- 0.5) for -103.98 < x < 88.73: -150 ... 128 (swept one wider)
    {
        Tally t;
        for (int k = -151; k <= 129; k++) {
            t.mult++;
            if (!exactProduct((float)k, expLn2hi)) t.inexact++;
            for (int j = 0; j < 4096; j++) tryAddend(t, (float)k, expLn2hi, ((float)k + uniform(-0.6f, 0.6f)) * 0.6931471806f, true);
            for (float x : {0.0f, -0.0f, (float)k * expLn2hi, 88.72f, -103.97f}) tryAddend(t, (float)k, expLn2hi, x, true);
        }
        report("exp_k_ln2hi", t);
    }
    // rt_log: ... + k ln2_hi.  k = exponent of x (with the subnormals' -25): -149 ... 128 (swept one wider); the addend is
    // s (hfsq + R) + k ln2_lo - hfsq + f, of magnitude below 0.5
    {
        Tally t;
        for (int k = -150; k <= 129; k++) {
            t.mult++;
            if (!exactProduct((float)k, logLn2hi)) t.inexact++;
            for (int j = 0; j < 4096; j++) tryAddend(t, (float)k, logLn2hi, uniform(-0.5f, 0.5f), false);
            for (float c : {0.0f, -0.0f, -(float)k * logLn2hi, fromBits(1u), fromBits(0x80000001u)}) tryAddend(t, (float)k, logLn2hi, c, false);
        }
        report("log_k_ln2hi", t);
    }
    return 0;
}
