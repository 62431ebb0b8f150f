/* rt_variance_launch.h — what rt_post.hip needs of rt_variance.hip: the sizes of the filter's scratch and the calls that enqueue
 * its kernels on a stream.  The entry points of include/rt_variance.h themselves live in rt_post.hip, over the context (rt_context.h). */
#ifndef RT_VARIANCE_LAUNCH_H
#define RT_VARIANCE_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rt_vr {

struct Job {
    int W = 0, H = 0;
    int iterations = 0;
    int demodulate = 0;
    float scale = 1.0f;
    float unknownVariance = 0;
    float sigmaLuminance = 0;
    float aN = 0, aP = 0; /* 1 / sigma^2 each (rt_denoise_math.h, rt_dn_inv_sq) */
};

/* bytes of scratch for a W x H image: two colour images (16 B per pixel each), then the packed guide image (32 B per pixel) — the
 * layout of rt_dn::scratch_bytes, so the two filters share one allocation */
inline size_t scratch_bytes(size_t nPix) { return nPix * 64; }

/* Update (rebase == 0) or snap := sum alone (rebase != 0), nPix pixels, on `st` */
hipError_t enqueue_update(hipStream_t st, const void* dSum, void* dSnapshot, void* dMoments, size_t nPix, int rebase);

/* Prepare + `iterations` passes, in -> out, all on `st`.  `scratch`: scratch_bytes(W * H) bytes, 16-byte aligned. */
hipError_t enqueue(hipStream_t st, const Job& job, const void* dIn, const void* dMoments, const void* dAov, void* dOut, void* scratch);

} // namespace rt_vr

#endif /* RT_VARIANCE_LAUNCH_H */
