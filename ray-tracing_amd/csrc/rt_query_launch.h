/* rt_query_launch.h — the host arithmetic of include/rt_query.h's four calls, without HIP, so that a host test reaches it
 * (tests/query_launch_driver.cpp): the argument and size checks, the overlap test, and the blocks and the grid of a pass.  The kernel
 * is rt_kernels.h's rt_query_kernel; the entry points live in rt_context.hip, with the context. */
#ifndef RT_QUERY_LAUNCH_H
#define RT_QUERY_LAUNCH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_query.h"

namespace rt_qr {

enum { RAYS_PER_BLOCK = 64 }; /* one ray per lane, one wave per workgroup */

/* n * perRay in size_t: false when the product does not fit (n >= 0) */
inline bool byte_size(long long n, size_t perRay, size_t* bytes)
{
    *bytes = 0;
    if (n < 0) return false;
    if (perRay != 0 && (unsigned long long)n > (unsigned long long)SIZE_MAX / perRay) return false;
    *bytes = (size_t)n * perRay;
    return true;
}

/* do [a, a + na) and [b, b + nb) share a byte?  Ranges that touch do not; an empty range shares nothing.  Written on the distance
 * between the starts, so that a range which ends at the top of the address space does not wrap. */
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    if (na == 0 || nb == 0) return false;
    return ua <= ub ? (ub - ua < na) : (ua - ub < nb);
}

/* The errors every form shares, in the order include/rt_query.h lists them (the context and the scene are the caller's): RT_OK and the
 * three byte counts, or RT_ERR_INVALID_ARG and *why.  outPerRay: sizeof(RtRayHit) or sizeof(uint32_t). */
inline int check_batch(const void* rays, int n, const void* out, size_t outPerRay, size_t* rayBytes, size_t* outBytes, const char** why)
{
    *why = "";
    *rayBytes = *outBytes = 0;
    if (n < 0) { *why = "n < 0"; return RT_ERR_INVALID_ARG; }
    if (n > RT_QUERY_MAX_RAYS) { *why = "more than RT_QUERY_MAX_RAYS (2^26) rays in one call"; return RT_ERR_INVALID_ARG; }
    if (n > 0 && !rays) { *why = "the rays are null"; return RT_ERR_INVALID_ARG; }
    if (n > 0 && !out) { *why = "the output is null"; return RT_ERR_INVALID_ARG; }
    if (!byte_size(n, sizeof(RtRay), rayBytes) || !byte_size(n, outPerRay, outBytes)) { *why = "the byte size of the batch does not fit size_t"; return RT_ERR_INVALID_ARG; }
    if (ranges_overlap(rays, *rayBytes, out, *outBytes)) { *why = "the output overlaps the rays"; return RT_ERR_INVALID_ARG; }
    return RT_OK;
}

/* blocks of 64 consecutive rays: the last one may be ragged */
inline long long blocks(long long n) { return n <= 0 ? 0 : (n + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK; }

/* single-wave workgroups of the launch: every wave the device keeps resident (RT_GRID, when set, in its place), at most one per block;
 * the blocks are strided over them.  0 = nothing to launch. */
inline long long grid(long long nBlocks, long long residentWaves, int gridOverride)
{
    if (nBlocks <= 0) return 0;
    long long g = gridOverride > 0 ? (long long)gridOverride : residentWaves;
    if (g < 1) g = 1;
    return g < nBlocks ? g : nBlocks;
}

} // namespace rt_qr

#endif /* RT_QUERY_LAUNCH_H */
