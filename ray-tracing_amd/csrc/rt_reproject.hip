/* rt_reproject.hip — the kernels of include/rt_reproject.h.
 *
 *   rt_rp_reproject_kernel  one lane per output pixel, lanes along a row.  A lane reads half of its own record (quarters 0 and 1: normal,
 *                           position, hit class) and the record's object word, projects the position into the previous camera and reads
 *                           up to four taps there: one 16-byte load of the previous sum and, of the tap's 64-byte record, the two aligned
 *                           16-byte quarters that hold normal and position plus the object word — albedo, emission and triangle are never
 *                           touched.  One 16-byte store.  The taps of neighbouring lanes are neighbouring pixels under any camera move
 *                           that is not a large roll, so what a wave reads stays a few rows of the previous image and L2 serves the 4 x
 *                           reuse; there is nothing to stage in LDS, because where a group's taps lie is only known after the projection.
 *   rt_mo_reproject_kernel  the same with the table of include/rt_motion.h: a lane whose object word indexes the table reads that entry (three
 *                           16-byte loads; a wave's lanes see a handful of objects, so the entries come from cache) and carries on with the
 *                           moved position and normal.  A kernel of its own: rt_rp_reproject_kernel stays the code it was.
 *   rt_rp_commit_kernel     copies the reprojected image over the accumulator unless the AOV pass's watchdog word is set.
 *   rt_rp_resolve_kernel    the per-pixel divide.
 *
 * All four move 16 bytes per lane and access and do a few dozen flops per pixel: they are bound by memory, 256-thread groups with no
 * LDS and a register count far below the occupancy limit keep every CU's wave slots full, which is all a streaming kernel can use.
 *
 * The arithmetic is rt_reproject_math.h's and rt_motion_math.h's, shared with the host drivers of tests/test_reproject.py and
 * tests/test_motion.py. */
#include <hip/hip_runtime.h>

#include "rt_reproject_launch.h"

namespace rt_rp {

__device__ __forceinline__ rt_rp4 ld4(const float4* p) { const float4 v = *p; return rt_rp_make4(v.x, v.y, v.z, v.w); }

/* the previous view as rt_rp_pixel reads it */
struct PrevView {
    const float4* rgba;
    const float4* aov;
    __device__ __forceinline__ rt_rp4 colour(size_t i) const { return ld4(rgba + i); }
    __device__ __forceinline__ rt_rp4 q0(size_t i) const { return ld4(aov + 4 * i); }
    __device__ __forceinline__ rt_rp4 q1(size_t i) const { return ld4(aov + 4 * i + 1); }
    __device__ __forceinline__ int32_t object(size_t i) const { return reinterpret_cast<const int32_t*>(aov + 4 * i + 2)[3]; }
};

__global__ __launch_bounds__(256) void rt_rp_reproject_kernel(const rt_rp_job job, const float4* __restrict__ prevRgba, const float4* __restrict__ prevAov,
                                                              const float4* __restrict__ curAov, float4* __restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PrevView prev = {prevRgba, prevAov};
    const int32_t object = reinterpret_cast<const int32_t*>(curAov + 4 * i + 2)[3];
    const rt_rp4 r = rt_rp_pixel(job, ld4(curAov + 4 * i), ld4(curAov + 4 * i + 1), object, prev);
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

/* the table as rt_mo_pixel reads it */
struct MotionTable {
    const float4* m;
    __device__ __forceinline__ rt_mo_entry entry(int32_t k) const
    {
        const float4* e = m + 3 * (size_t)k;
        const rt_mo_entry r = {ld4(e), ld4(e + 1), ld4(e + 2)};
        return r;
    }
};

__global__ __launch_bounds__(256) void rt_mo_reproject_kernel(const rt_rp_job job, const float4* __restrict__ prevRgba, const float4* __restrict__ prevAov,
                                                              const float4* __restrict__ curAov, const float4* __restrict__ motion, int32_t nObjects,
                                                              float4* __restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PrevView prev = {prevRgba, prevAov};
    const MotionTable table = {motion};
    const int32_t object = reinterpret_cast<const int32_t*>(curAov + 4 * i + 2)[3];
    const rt_rp4 r = rt_mo_pixel(job, ld4(curAov + 4 * i), ld4(curAov + 4 * i + 1), object, prev, table, nObjects); /* entry(k) only for 0 <= k < nObjects */
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

__global__ __launch_bounds__(256) void rt_rp_commit_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n, const unsigned long long* __restrict__ skipIfSet)
{
    if (*skipIfSet != 0ull) return; /* the same word for every lane of the grid */
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

/* (no __restrict__: in place is allowed; a lane reads and writes its own pixel only) */
__global__ __launch_bounds__(256) void rt_rp_resolve_kernel(const float4* sum, float4* out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rt_rp4 r = rt_rp_resolve(ld4(sum + i));
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

static dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); } /* <= 2^22 groups for the 2^30 pixels the entry points admit */

hipError_t enqueue(hipStream_t st, const rt_rp_job& job, const void* dPrevRgba, const void* dPrevAov, const void* dCurAov, void* dOut)
{
    const size_t n = (size_t)job.W * job.H;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_rp_reproject_kernel, grid_for(n), dim3(256), 0, st, job, (const float4*)dPrevRgba, (const float4*)dPrevAov, (const float4*)dCurAov, (float4*)dOut, n);
    return hipGetLastError();
}

hipError_t enqueue_moving(hipStream_t st, const rt_rp_job& job, const void* dPrevRgba, const void* dPrevAov, const void* dCurAov, const void* dMotion, int nObjects,
                          void* dOut)
{
    const size_t n = (size_t)job.W * job.H;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_mo_reproject_kernel, grid_for(n), dim3(256), 0, st, job, (const float4*)dPrevRgba, (const float4*)dPrevAov, (const float4*)dCurAov,
                       (const float4*)dMotion, (int32_t)nObjects, (float4*)dOut, n);
    return hipGetLastError();
}

hipError_t enqueue_commit(hipStream_t st, const void* src, void* dst, size_t nPix, const unsigned long long* skipIfSet)
{
    if (nPix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_rp_commit_kernel, grid_for(nPix), dim3(256), 0, st, (const float4*)src, (float4*)dst, nPix, skipIfSet);
    return hipGetLastError();
}

hipError_t enqueue_resolve(hipStream_t st, const void* dSum, void* dOut, size_t nPix)
{
    if (nPix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_rp_resolve_kernel, grid_for(nPix), dim3(256), 0, st, (const float4*)dSum, (float4*)dOut, nPix);
    return hipGetLastError();
}

} // namespace rt_rp
