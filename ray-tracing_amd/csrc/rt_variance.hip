/* rt_variance.hip — the kernels of include/rt_variance.h: the luminance moments' update and the variance-guided a-trous filter.
 *
 *   rt_vr_update_kernel    one pixel per lane: 48 B read (sum, snapshot, moments), 32 B written (snapshot, moments); bound by memory.
 *   rt_vr_copy_kernel      iterations == 0: the scaled copy.
 *   rt_vr_prepare_kernel   rt_dn_prepare_kernel plus one 16-byte load of the moments: writes the colour WITH ITS VARIANCE in the fourth
 *                          word (16 B) and the packed guide (32 B), so a tap of a pass stays three aligned 16-byte reads.
 *   rt_vr_pass_kernel      rt_dn_pass_kernel's tile — 32 x 8 centres of ONE sub-lattice plus a two-record halo, 36 x 12 records x 48 B =
 *                          20,736 B of LDS at every spacing — restated here rather than shared, because the fill differs: a tap needs
 *                          l(q) = lum(c(q)), and a tap never reads the demodulation mask, so the fill computes l once per record and
 *                          stages it in the mask's word.  That is 5 flops per record (1.7 records per lane) instead of 5 per tap (25 taps
 *                          per lane); the centre's own mask is one 4-byte global load in the last pass.  The 3 x 3 variance prefilter reads
 *                          the lattice taps (dx, dy) in {-1, 0, 1}^2 of the same tile — a subset of the 25 — before the tap loop, since
 *                          every tap's weight needs its result.
 *
 * The arithmetic is rt_variance_math.h's, shared with the host driver of tests/test_variance.py. */
#include <hip/hip_runtime.h>

#include "rt_variance_launch.h"
#include "rt_variance_math.h"

namespace rt_vr {

__device__ __forceinline__ rt_dn4 ld4(const float4* p) { const float4 v = *p; return rt_dn_make4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void st4(float4* p, rt_dn4 v) { *p = make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ rt_dn4 as4(float4 v) { return rt_dn_make4(v.x, v.y, v.z, v.w); }

__global__ __launch_bounds__(256) void rt_vr_update_kernel(const float4* __restrict__ sum, float4* __restrict__ snapshot, float4* __restrict__ moments, size_t n, int rebase)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rt_dn4 now = ld4(sum + i);
    if (!rebase) {
        bool changed;
        const rt_dn4 M = rt_vr_update(now, ld4(snapshot + i), ld4(moments + i), &changed);
        if (changed) st4(moments + i, M);
    }
    st4(snapshot + i, now);
}

__global__ __launch_bounds__(256) void rt_vr_copy_kernel(const float4* __restrict__ in, float4* __restrict__ out, size_t n, float scale)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rt_dn4 v = ld4(in + i);
    st4(out + i, rt_dn_make4(v.x * scale, v.y * scale, v.z * scale, v.w));
}

__global__ __launch_bounds__(256) void rt_vr_prepare_kernel(const float4* __restrict__ in, const float4* __restrict__ moments, const float4* __restrict__ aov,
                                                            float4* __restrict__ colour, float4* __restrict__ guide, size_t n, float scale, int demodulate,
                                                            float unknownVariance)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rt_dn4 c, g0, g1;
    rt_vr_prepare(ld4(in + i), ld4(moments + i), ld4(aov + 4 * i), ld4(aov + 4 * i + 1), ld4(aov + 4 * i + 2), scale, demodulate, unknownVariance, &c, &g0, &g1);
    st4(colour + i, c);
    st4(guide + 2 * i, g0);
    st4(guide + 2 * i + 1, g1);
}

/* A pass, LDS-tiled exactly as rt_dn_pass_kernel (rt_denoise.hip explains the sub-lattice tile): a record outside the image is staged
 * with an object no centre can have, which skips it as `inside = false` does.  sG1[r].w holds l, not the mask. */
static constexpr int kLdsW = 32, kLdsH = 8, kLdsRowLen = kLdsW + 4, kLdsRecords = kLdsRowLen * (kLdsH + 4);

template <bool LAST>
__global__ __launch_bounds__(256) void rt_vr_pass_kernel(const float4* __restrict__ cin, const float4* __restrict__ guide, const float4* __restrict__ aov,
                                                         const float4* __restrict__ in, float4* __restrict__ cout, int W, int H, int tilesU, int tilesV, int s, int nOx,
                                                         float aN, float aP, float sigmaLuminance)
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
        g1.w = rt_vr_lum(c.x, c.y, c.z);
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
    const rt_dn4 cp = as4(sC[rc]), g0p = as4(sG0[rc]), g1p = as4(sG1[rc]);
    rt_dn4 out = cp;
    if (rt_dn_centre_filtered(cp, g0p)) {
        rt_vr_gauss gs = {0.0f, 0.0f};
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int r = rc + dy * kLdsRowLen + dx;
                rt_vr_gauss_tap(&gs, rt_vr_hg(dy) * rt_vr_hg(dx), true, g0p, as4(sC[r]), as4(sG0[r]));
            }
        }
        const float invL = rt_vr_inv_l(gs, sigmaLuminance);
        rt_vr_sums sums = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int r = rc + dy * kLdsRowLen + dx;
                const rt_dn4 cq = as4(sC[r]), g1q = as4(sG1[r]);
                rt_vr_tap(&sums, rt_dn_h(dy) * rt_dn_h(dx), true, g1p.w, g0p, g1p, cq, g1q.w, as4(sG0[r]), g1q, aN, aP, invL);
            }
        }
        out = rt_vr_resolve(sums);
    }
    if (LAST) {
        const uint32_t mask = reinterpret_cast<const uint32_t*>(guide + 2 * i + 1)[3];
        out = rt_vr_finish(out, mask, ld4(aov + 4 * i + 2), reinterpret_cast<const float*>(in + i)[3]);
    }
    st4(cout + i, out);
}

static dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

hipError_t enqueue_update(hipStream_t st, const void* dSum, void* dSnapshot, void* dMoments, size_t nPix, int rebase)
{
    if (nPix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_vr_update_kernel, grid_for(nPix), dim3(256), 0, st, (const float4*)dSum, (float4*)dSnapshot, (float4*)dMoments, nPix, rebase);
    return hipGetLastError();
}

hipError_t enqueue(hipStream_t st, const Job& job, const void* dIn, const void* dMoments, const void* dAov, void* dOut, void* scratch)
{
    const size_t n = (size_t)job.W * job.H;
    if (n == 0) return hipSuccess;
    const float4* in = (const float4*)dIn;
    const float4* aov = (const float4*)dAov;
    if (job.iterations == 0) {
        hipLaunchKernelGGL(rt_vr_copy_kernel, grid_for(n), dim3(256), 0, st, in, (float4*)dOut, n, job.scale);
        return hipGetLastError();
    }
    float4* colour[2] = {(float4*)scratch, (float4*)scratch + n};
    float4* guide = (float4*)scratch + 2 * n;
    hipLaunchKernelGGL(rt_vr_prepare_kernel, grid_for(n), dim3(256), 0, st, in, (const float4*)dMoments, aov, colour[0], guide, n, job.scale, job.demodulate,
                       job.unknownVariance);
    for (int i = 0; i < job.iterations; i++) {
        const bool last = i == job.iterations - 1;
        const float4* src = colour[i & 1];
        float4* dst = last ? (float4*)dOut : colour[(i + 1) & 1];
        const int sp = 1 << i;
        const int tilesU = ((job.W + sp - 1) / sp + kLdsW - 1) / kLdsW, tilesV = ((job.H + sp - 1) / sp + kLdsH - 1) / kLdsH; /* of the widest, highest sub-lattice */
        const int nOx = sp < job.W ? sp : job.W, nOy = sp < job.H ? sp : job.H;
        const dim3 grid((unsigned)((size_t)tilesU * tilesV * nOx * nOy)); /* <= W * H + the partial tiles: fits for the 2^30 pixels the entry points admit */
        if (last)
            hipLaunchKernelGGL(rt_vr_pass_kernel<true>, grid, dim3(256), 0, st, src, (const float4*)guide, aov, in, dst, job.W, job.H, tilesU, tilesV, sp, nOx, job.aN, job.aP,
                               job.sigmaLuminance);
        else
            hipLaunchKernelGGL(rt_vr_pass_kernel<false>, grid, dim3(256), 0, st, src, (const float4*)guide, aov, in, dst, job.W, job.H, tilesU, tilesV, sp, nOx, job.aN, job.aP,
                               job.sigmaLuminance);
    }
    return hipGetLastError();
}

} // namespace rt_vr
