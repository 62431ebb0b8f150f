/* rt_denoise.hip — the kernels of include/rt_denoise.h: an edge-avoiding a-trous filter guided by the AOV records.
 *
 *   rt_dn_prepare_kernel   reads the input pixel and three quarters of its 64-byte record once; writes the scaled, demodulated colour
 *                          (16 B) and the packed guide (32 B: normal + object, position + demodulation mask).  A tap of a pass then
 *                          costs three aligned 16-byte loads instead of a walk over 64-byte records.
 *   rt_dn_pass_kernel      one pixel per lane; a 256-thread group stages a tile of ONE sub-lattice of the image plus its two-record
 *                          halo into LDS and serves all 25 taps from there (below).  The last pass multiplies the albedo back and
 *                          so writes the caller's image: no extra pass over it.
 *
 * The other form of a pass — every tap a global load, the reuse left to L1 / L2 — measured 1.3 ... 1.6 x slower at every spacing
 * (profiles/r07_denoise.txt) and is kept as tools/experiments/r07_denoise_plain_form.diff.
 *
 * The arithmetic is rt_denoise_math.h's, shared with the host driver of tests/test_denoise.py. */
#include <hip/hip_runtime.h>

#include "rt_denoise_launch.h"
#include "rt_denoise_math.h"

namespace rt_dn {

__device__ __forceinline__ rt_dn4 ld4(const float4* p) { const float4 v = *p; return rt_dn_make4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void st4(float4* p, rt_dn4 v) { *p = make_float4(v.x, v.y, v.z, v.w); }

/* guide == nullptr: iterations == 0, the scaled copy straight into the caller's image (the host passes demodulate = 0) */
__global__ __launch_bounds__(256) void rt_dn_prepare_kernel(const float4* __restrict__ in, const float4* __restrict__ aov, float4* __restrict__ colour,
                                                            float4* __restrict__ guide, size_t n, float scale, int demodulate)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rt_dn4 c, g0, g1;
    rt_dn_prepare(ld4(in + i), ld4(aov + 4 * i), ld4(aov + 4 * i + 1), ld4(aov + 4 * i + 2), scale, demodulate, &c, &g0, &g1);
    st4(colour + i, c);
    if (guide) {
        st4(guide + 2 * i, g0);
        st4(guide + 2 * i + 1, g1);
    }
}

/* A pass, LDS-tiled.  A 256-thread group owns 32 x 8 centres of ONE sub-lattice of the image — the pixels with equal
 * (x mod s, y mod s) — so that a tap `s` pixels away is the neighbouring record of the tile and the halo stays two records wide at every
 * spacing: 36 x 12 records x 48 B = 20,736 B of LDS, filled once (three 16-byte loads per record), then all 25 taps are LDS reads.
 * A record outside the image is staged with an object no centre can have (the sign bit alone: filtered centres have object >= 0), which
 * skips it exactly as `inside = false` does in rt_dn_tap.  For s > 1 the fill loads and the stores of a wave are s pixels apart. */
static constexpr int kLdsW = 32, kLdsH = 8, kLdsRowLen = kLdsW + 4, kLdsRecords = kLdsRowLen * (kLdsH + 4);

template <bool LAST>
__global__ __launch_bounds__(256) void rt_dn_pass_kernel(const float4* __restrict__ cin, const float4* __restrict__ guide, const float4* __restrict__ aov,
                                                               float4* __restrict__ cout, int W, int H, int tilesU, int tilesV, int s, int nOx, float aN, float aP, float aCi)
{
    __shared__ float4 sC[kLdsRecords], sG0[kLdsRecords], sG1[kLdsRecords];
    unsigned b = blockIdx.x;
    const int tu = (int)(b % (unsigned)tilesU); b /= (unsigned)tilesU;
    const int tv = (int)(b % (unsigned)tilesV); b /= (unsigned)tilesV;
    const int ox = (int)(b % (unsigned)nOx), oy = (int)(b / (unsigned)nOx); /* nOx = min(s, W) sub-lattices across, min(s, H) up: none is empty */
    const int u0 = tu * kLdsW, v0 = tv * kLdsH; /* the tile's first centre, in lattice coordinates */
    if ((long long)u0 * s + ox >= W || (long long)v0 * s + oy >= H) return; /* this sub-lattice is narrower or lower than the widest: whole group */
    for (int r = (int)threadIdx.x; r < kLdsRecords; r += 256) {
        const long long x = (long long)(u0 - 2 + r % kLdsRowLen) * s + ox, y = (long long)(v0 - 2 + r / kLdsRowLen) * s + oy;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x80000000u)), g1 = c;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t j = (size_t)y * W + (size_t)x;
            c = cin[j];
            g0 = guide[2 * j];
            g1 = guide[2 * j + 1];
        }
        sC[r] = c;
        sG0[r] = g0;
        sG1[r] = g1;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
    const long long xl = (long long)(u0 + tx) * s + ox, yl = (long long)(v0 + ty) * s + oy;
    if (xl >= W || yl >= H) return;
    const size_t i = (size_t)yl * W + (size_t)xl;
    const int rc = (ty + 2) * kLdsRowLen + tx + 2;
    const float4 c4 = sC[rc], a4 = sG0[rc], b4 = sG1[rc];
    const rt_dn4 cp = rt_dn_make4(c4.x, c4.y, c4.z, c4.w), g0p = rt_dn_make4(a4.x, a4.y, a4.z, a4.w), g1p = rt_dn_make4(b4.x, b4.y, b4.z, b4.w);
    rt_dn4 out = cp;
    if (rt_dn_centre_filtered(cp, g0p)) {
        rt_dn_sums sums = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int r = rc + dy * kLdsRowLen + dx;
                const float4 qc = sC[r], q0 = sG0[r], q1 = sG1[r];
                rt_dn_tap(&sums, rt_dn_h(dy) * rt_dn_h(dx), true, cp, g0p, g1p, rt_dn_make4(qc.x, qc.y, qc.z, qc.w), rt_dn_make4(q0.x, q0.y, q0.z, q0.w),
                          rt_dn_make4(q1.x, q1.y, q1.z, q1.w), aN, aP, aCi);
            }
        }
        out = rt_dn_resolve(sums, cp);
    }
    if (LAST) out = rt_dn_finish(out, g1p, ld4(aov + 4 * i + 2));
    st4(cout + i, out);
}

hipError_t enqueue(hipStream_t st, const Job& job, const void* dIn, const void* dAov, void* dOut, void* scratch)
{
    const size_t n = (size_t)job.W * job.H;
    if (n == 0) return hipSuccess;
    const float4* in = (const float4*)dIn;
    const float4* aov = (const float4*)dAov;
    float4* colour[2] = {(float4*)scratch, (float4*)scratch + n};
    float4* guide = (float4*)scratch + 2 * n;
    const unsigned blocks1d = (unsigned)((n + 255) / 256);
    if (job.iterations == 0) {
        hipLaunchKernelGGL(rt_dn_prepare_kernel, dim3(blocks1d), dim3(256), 0, st, in, aov, (float4*)dOut, (float4*)nullptr, n, job.scale, 0);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(rt_dn_prepare_kernel, dim3(blocks1d), dim3(256), 0, st, in, aov, colour[0], guide, n, job.scale, job.demodulate);
    for (int i = 0; i < job.iterations; i++) {
        const bool last = i == job.iterations - 1;
        const float4* src = colour[i & 1];
        float4* dst = last ? (float4*)dOut : colour[(i + 1) & 1];
        const float aCi = rt_dn_colour_scale(job.aC, i);
        const int sp = 1 << i;
        const int tilesU = ((job.W + sp - 1) / sp + kLdsW - 1) / kLdsW, tilesV = ((job.H + sp - 1) / sp + kLdsH - 1) / kLdsH; /* of the widest, highest sub-lattice */
        const int nOx = sp < job.W ? sp : job.W, nOy = sp < job.H ? sp : job.H;
        const dim3 grid((unsigned)((size_t)tilesU * tilesV * nOx * nOy)); /* <= W * H + the partial tiles: fits for the 2^30 pixels the entry points admit */
        if (last)
            hipLaunchKernelGGL(rt_dn_pass_kernel<true>, grid, dim3(256), 0, st, src, (const float4*)guide, aov, dst, job.W, job.H, tilesU, tilesV, sp, nOx, job.aN, job.aP, aCi);
        else
            hipLaunchKernelGGL(rt_dn_pass_kernel<false>, grid, dim3(256), 0, st, src, (const float4*)guide, aov, dst, job.W, job.H, tilesU, tilesV, sp, nOx, job.aN, job.aP, aCi);
    }
    return hipGetLastError();
}

} // namespace rt_dn
