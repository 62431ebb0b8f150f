/* rt_reproject_launch.h — what rt_post.hip needs of rt_reproject.hip: the calls that enqueue its kernels on a stream.  The entry
 * points of include/rt_reproject.h and include/rt_motion.h themselves live in rt_post.hip, over the context (rt_context.h). */
#ifndef RT_REPROJECT_LAUNCH_H
#define RT_REPROJECT_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "rt_motion_math.h"

namespace rt_rp {

/* d_prev_rgba, d_prev_aov, d_cur_aov -> d_out (job.W x job.H), on `st` */
hipError_t enqueue(hipStream_t st, const rt_rp_job& job, const void* dPrevRgba, const void* dPrevAov, const void* dCurAov, void* dOut);

/* the same with the table of include/rt_motion.h: dMotion holds nObjects entries of 48 bytes (not read when nObjects == 0) */
hipError_t enqueue_moving(hipStream_t st, const rt_rp_job& job, const void* dPrevRgba, const void* dPrevAov, const void* dCurAov, const void* dMotion, int nObjects,
                          void* dOut);

/* dst[i] = src[i] for nPix pixels, unless *skipIfSet != 0 (a watchdog word of the pass that made the inputs): then nothing is written */
hipError_t enqueue_commit(hipStream_t st, const void* src, void* dst, size_t nPix, const unsigned long long* skipIfSet);

/* the per-pixel divide, sum -> out (in place allowed) */
hipError_t enqueue_resolve(hipStream_t st, const void* dSum, void* dOut, size_t nPix);

} // namespace rt_rp

#endif /* RT_REPROJECT_LAUNCH_H */
