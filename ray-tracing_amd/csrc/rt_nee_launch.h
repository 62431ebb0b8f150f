/* rt_nee_launch.h — the host arithmetic of include/rt_nee.h's two ray calls, without HIP, so that a host test reaches it
 * (tests/light_table_driver.cpp): the bytes of the device copy of the light table and the pick rule — the one function body the kernel
 * (rt_kernels.h, nee_sample) and the host test both run.  The rays, the records, their checks and the way the waves of a launch come
 * by their blocks are rt_radiance_launch.h's (rt_rd::), which the calls use as they are and this namespace only names again (the
 * host test checks them under rt_nee::); what this header adds is the table.  The
 * kernel is rt_kernels.h's rt_radiance_nee_kernel; the entry points live in rt_context.hip, with the context. */
#ifndef RT_NEE_LAUNCH_H
#define RT_NEE_LAUNCH_H

#include "../../include/rt_nee.h"
#include "rt_radiance_launch.h"

namespace rt_nee {

/* the blocks, the grid and the batch checks of the two calls are the radiance pass's own, under this pass's name for its host test */
using rt_rd::RAYS_PER_BLOCK;
using rt_rd::check_batch;
using rt_rd::blocks;
using rt_rd::grid;

enum { PICK_STEPS = 23 }; /* 2^22 entries: 22 halvings find the entry, one to spare */

static_assert((1ll << (PICK_STEPS - 1)) >= RT_NEE_MAX_LIGHTS, "the bounded search must reach every entry");

/* The pick rule of include/rt_nee.h: the smallest i with u < cdf[i], the last entry when there is none (u == 1, a NaN).  At most
 * PICK_STEPS halvings; mid lies in [lo, hi] within [0, n - 1] at every step and the result is clamped, so no index leaves the table
 * whatever the cdf holds.  n >= 1. */
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int pick(const float* cdf, const int n, const float u)
{
    int lo = 0, hi = n - 1;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int step = 0; step < PICK_STEPS && lo < hi; step++) {
        const int mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo < n - 1 ? lo : n - 1;
}

/* the table's device copy goes up in pieces of at most this many bytes, so that the pinned staging ring never holds more */
enum : size_t { UPLOAD_CHUNK_BYTES = (size_t)4 << 20 };

/* The device copy of a table of nEntries entries over nObjects objects, one allocation: the entries (80 bytes each, 16-byte aligned),
 * then the cdf, then the per-object flags.  RT_OK, or RT_ERR_SCENE past the cap / RT_ERR_INVALID_ARG for a negative count. */
struct TableBytes {
    size_t entries = 0, cdf = 0, flags = 0, total = 0; /* cdf and flags: byte offsets; total: bytes (never 0) */
};
inline int table_bytes(long long nEntries, long long nObjects, TableBytes* tb, const char** why)
{
    *why = "";
    *tb = TableBytes();
    if (nEntries < 0 || nObjects < 0) { *why = "negative count"; return RT_ERR_INVALID_ARG; }
    if (nEntries > RT_NEE_MAX_LIGHTS) { *why = "more emitters than RT_NEE_MAX_LIGHTS (2^22)"; return RT_ERR_SCENE; }
    tb->entries = 0;
    tb->cdf = (size_t)nEntries * sizeof(RtLightEntry);
    tb->flags = tb->cdf + (((size_t)nEntries * sizeof(float) + 15) & ~(size_t)15);
    tb->total = tb->flags + (((size_t)nObjects * sizeof(uint32_t) + 15) & ~(size_t)15);
    if (tb->total == 0) tb->total = 16;
    return RT_OK;
}

} // namespace rt_nee

#endif /* RT_NEE_LAUNCH_H */
