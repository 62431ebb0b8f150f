/* rt_adaptive.hip — the kernels of include/rt_adaptive.h: which 8 x 8 tiles are not yet converged, and the frame-ordered additions of a
 * fused launch over a tile list.
 *
 *   rt_ad_tile_error_kernel        one wave per tile, lane l = pixel (8 tx + (l & 7), 8 ty + (l >> 3)): two 16-byte loads (the sum, the
 *                                  moments), rt_ad_error, the maximum over the wave by six __shfl_xor steps (no LDS; a lane outside the
 *                                  image holds +0, the least value an error takes), lane 0 writes the tile's error.  32 B read per
 *                                  pixel: bound by memory.
 *   rt_ad_list_kernel              ONE workgroup of 1,024 lanes, in the shape of rt_order_kernel: walks the tile errors 1,024 at a time
 *                                  in index order, ranks the active ones by a ballot per wave and the 16 waves' counts through LDS, and
 *                                  writes tile i at position (active tiles before i) — the list is in increasing t by construction, no
 *                                  atomic append.  32,400 tiles (1920 x 1080) are 32 rounds.  Also the two counts.
 *   rt_accumulate_tiles_kernel     rt_accumulate_kernel's loop body behind the list: one wave per listed tile, one lane per pixel.  Only
 *                                  the listed pixels of the staging slab are read — no other was written by the launch.
 *
 * The arithmetic is rt_adaptive_math.h's, shared with the host driver of tests/test_adaptive.py. */
#include <hip/hip_runtime.h>

#include "rt_adaptive_launch.h"

namespace rt_ad {

static constexpr int kWavesPerBlock = 4; /* the per-tile kernels: 256 lanes = 4 tiles per workgroup */

__device__ __forceinline__ rt_dn4 ld4(const float4* p) { const float4 v = *p; return rt_dn_make4(v.x, v.y, v.z, v.w); }

__global__ __launch_bounds__(64 * kWavesPerBlock) void rt_ad_tile_error_kernel(const float4* __restrict__ sum, const float4* __restrict__ moments,
                                                                               float* __restrict__ tileError, int W, int rows, int tilesX, long long nTiles,
                                                                               rt_ad_job job)
{
    const long long t = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); /* wave-uniform */
    if (t >= nTiles) return;
    const int lane = threadIdx.x & 63;
    const int ty = (int)(t / tilesX), tx = (int)(t - (long long)ty * tilesX);
    const int x = 8 * tx + (lane & 7), row = 8 * ty + (lane >> 3);
    float err = 0.0f;
    if (x < W && row < rows) {
        const size_t i = (size_t)row * W + x;
        err = rt_ad_error(ld4(sum + i), ld4(moments + i), job.darkFloor, job.minFrames, job.maxFrames);
    }
    for (int m = 32; m >= 1; m >>= 1) err = rt_ad_max(err, __shfl_xor(err, m, 64));
    if (lane == 0) tileError[t] = err;
}

__global__ __launch_bounds__(1024) void rt_ad_list_kernel(const float* __restrict__ tileError, uint32_t* __restrict__ tiles, uint32_t* __restrict__ counts, int W,
                                                          int rows, int tilesX, long long nTiles, float threshold)
{
    __shared__ uint32_t waveCount[16];
    __shared__ uint32_t wavePixels[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t run = 0;    /* active tiles before this round: the same in every lane */
    uint32_t pixels = 0; /* this lane's share of pixels_active */
    for (long long base = 0; base < nTiles; base += 1024) {
        const long long i = base + t;
        const bool active = i < nTiles && rt_ad_active(tileError[i], threshold);
        const unsigned long long ballot = __ballot(active);
        if (lane == 0) waveCount[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < 16; w++) {
            const uint32_t c = waveCount[w];
            before += w < wave ? c : 0u;
            all += c;
        }
        if (active) {
            /* position < (tiles up to and including i) <= nTiles: inside the array */
            tiles[run + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint32_t)i;
            const int ty = (int)(i / tilesX), tx = (int)(i - (long long)ty * tilesX);
            pixels += rt_ad_tile_pixels(tx, ty, W, rows);
        }
        run += all;
        __syncthreads(); /* every lane has read this round's counts before the next round writes them */
    }
    for (int m = 32; m >= 1; m >>= 1) pixels += __shfl_xor(pixels, m, 64);
    if (lane == 0) wavePixels[wave] = pixels;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < 16; w++) sum += wavePixels[w];
        counts[0] = run;
        counts[1] = sum;
        counts[2] = 0u;
        counts[3] = 0u;
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void rt_accumulate_tiles_kernel(const uint32_t* __restrict__ tiles, int nTiles, int W, int rows, int tilesX,
                                                                                  const float4* __restrict__ staging, int nFrames, size_t stride,
                                                                                  float4* __restrict__ accumulated, float4* __restrict__ frameRender)
{
    const int q = (int)blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6); /* wave-uniform */
    if (q >= nTiles) return;
    const int lane = threadIdx.x & 63;
    const uint32_t t = tiles[q];
    const int ty = (int)(t / (uint32_t)tilesX), tx = (int)(t - (uint32_t)ty * (uint32_t)tilesX);
    const int x = 8 * tx + (lane & 7), row = 8 * ty + (lane >> 3);
    if (x >= W || row >= rows) return;
    const size_t i = (size_t)row * W + x;
    float4 acc = accumulated[i];
    float4 c = make_float4(0.f, 0.f, 0.f, 1.f);
    for (int f = 0; f < nFrames; f++) {
        c = staging[(size_t)f * stride + i];
        acc.x += c.x;
        acc.y += c.y;
        acc.z += c.z;
        acc.w += 1.0f;
    }
    accumulated[i] = acc;
    frameRender[i] = c;
}

hipError_t enqueue_select(hipStream_t st, const rt_ad_job& job, int W, int rows, const void* dSum, const void* dMoments, float* dTileError, uint32_t* dTiles,
                          uint32_t* dCounts)
{
    const long long nTiles = tiles_total(W, rows);
    const int tilesX = tiles_x(W);
    if (nTiles > 0) {
        const unsigned blocks = (unsigned)((nTiles + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(rt_ad_tile_error_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, st, (const float4*)dSum, (const float4*)dMoments, dTileError, W, rows,
                           tilesX, nTiles, job);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(rt_ad_list_kernel, dim3(1), dim3(1024), 0, st, (const float*)dTileError, dTiles, dCounts, W, rows, tilesX > 0 ? tilesX : 1, nTiles,
                       job.threshold);
    return hipGetLastError();
}

hipError_t enqueue_accumulate_tiles(hipStream_t st, const uint32_t* dTiles, int nTiles, int W, int rows, const void* dStaging, int nFrames, size_t stride,
                                    void* dAccumulated, void* dFrameRender)
{
    if (nTiles <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((nTiles + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(rt_accumulate_tiles_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, st, dTiles, nTiles, W, rows, tiles_x(W), (const float4*)dStaging,
                       nFrames, stride, (float4*)dAccumulated, (float4*)dFrameRender);
    return hipGetLastError();
}

} // namespace rt_ad
