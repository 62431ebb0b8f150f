/* rt_radiance_launch.h — the host arithmetic of include/rt_radiance.h's two calls, without HIP, so that a host test reaches it
 * (tests/radiance_launch_driver.cpp): the argument and size checks, the blocks, the grid and the order in which the waves of a launch
 * come by their blocks.  Byte sizes, the overlap predicate and the shared checks are rt_query_launch.h's (an RtPathRay is as large as
 * an RtRay); what differs is the record (16 bytes) and the hand-out of blocks.  The kernel is rt_kernels.h's rt_radiance_kernel; the
 * entry points live in rt_context.hip, with the context. */
#ifndef RT_RADIANCE_LAUNCH_H
#define RT_RADIANCE_LAUNCH_H

#include "../../include/rt_radiance.h"
#include "rt_query_launch.h"

namespace rt_rd {

enum { RAYS_PER_BLOCK = rt_qr::RAYS_PER_BLOCK }; /* a wave's pool of rays: 64 consecutive ones */

static_assert(sizeof(RtPathRay) == sizeof(RtRay), "rt_qr::check_batch sizes the rays as RtRay");

/* The errors both forms share, in the order include/rt_radiance.h lists them (the context, the scene and the parameters are the
 * caller's): RT_OK and the two byte counts, or RT_ERR_INVALID_ARG and *why. */
inline int check_batch(const void* rays, int n, const void* out, size_t* rayBytes, size_t* outBytes, const char** why)
{
    return rt_qr::check_batch(rays, n, out, sizeof(RtRadiance), rayBytes, outBytes, why);
}

inline long long blocks(long long n) { return rt_qr::blocks(n); }

/* single-wave workgroups of the launch: every wave the device keeps resident (RT_GRID, when set, in its place), at most one per block */
inline long long grid(long long nBlocks, long long residentWaves, int gridOverride) { return rt_qr::grid(nBlocks, residentWaves, gridOverride); }

/* Which block a wave works on.  Wave w of a grid of g starts on block w; every further block comes from a counter that starts at 0 for
 * the launch and is shared by its waves: ticket t (the value an atomic increment returned) is block g + t, and a block index >= nBlocks
 * means there is no work left.  So every block is handed out exactly once whatever the order in which the waves draw their tickets, and
 * a wave whose paths are long draws fewer of them. */
inline long long first_block(long long wave) { return wave; }
inline long long ticket_block(long long grid, unsigned long long ticket) { return grid + (long long)ticket; }

} // namespace rt_rd

#endif /* RT_RADIANCE_LAUNCH_H */
