/* rt_denoise_launch.h — what rt_post.hip needs of rt_denoise.hip: the sizes of the filter's scratch and the call that enqueues
 * its kernels on a stream.  The entry points of include/rt_denoise.h themselves live in rt_post.hip, over the context (rt_context.h). */
#ifndef RT_DENOISE_LAUNCH_H
#define RT_DENOISE_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rt_dn {

struct Job {
    int W = 0, H = 0;
    int iterations = 0;
    int demodulate = 0;
    float scale = 1.0f;
    float aN = 0, aP = 0, aC = 0; /* 1 / sigma^2 each (rt_denoise_math.h, rt_dn_inv_sq) */
};

/* bytes of scratch for a W x H image: two colour images (16 B per pixel each), then the packed guide image (32 B per pixel) */
inline size_t scratch_bytes(size_t nPix) { return nPix * 64; }

/* Prepare + `iterations` passes, in -> out, all on `st`.  `scratch`: scratch_bytes(W * H) bytes, 16-byte aligned. */
hipError_t enqueue(hipStream_t st, const Job& job, const void* dIn, const void* dAov, void* dOut, void* scratch);

} // namespace rt_dn

#endif /* RT_DENOISE_LAUNCH_H */
