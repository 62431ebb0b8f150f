/*
 * rt_radiance.h — path-traced radiance for batches of caller-made rays against the uploaded scene (exported by libraytrace_hip.so,
 * plain C).
 *
 * rt_query.h answers "what does this ray hit"; these two calls answer "what light arrives along this ray": the integrator the frame is
 * rendered with — Trace, RayCommon.hlsl "RC":479-542: the bounce loop with glass, the specular and diffuse lobes, emission, the sky and
 * Russian roulette — started from a ray and a generator state the caller makes, with the result written to an array of the caller's
 * instead of an image.  That is an irradiance probe, a light-map texel, a cube-map face, an equirectangular, fisheye or orthographic
 * view, or the radiance at a few hundred sensor positions, without restating the shader on top of closest-hit records.
 *
 * Kept apart from rt_abi.h and rt_query.h, whose texts are pinned: this header includes rt_query.h (for RT_QUERY_MAX_RAYS and RtRay,
 * whose layout RtPathRay shares) and adds two types and two calls.
 *
 * ---- The radiance (a contract: every output bit is defined) ---------------------------------------------------------------------------
 * Record i is what the reference's Trace returns for ray i:  rgb = Trace(CreateRay(origin, dir, 1, 0), rng), and rng = the generator's
 * state when Trace returned, i.e. after the path's last draw — feed it back in to chain further samples of the same sequence.  The
 * direction is used as given: it is NOT normalised (as in rt_query.h).  The scene is the one as of the last rt_upload_scene /
 * rt_update_models / rt_update_spheres.  Of the last rt_set_params the pass uses maxBounceCount, useSky, sunFocus, sunIntensity,
 * sunColour and dirToSun, and nothing else: frame, seed, rays per pixel, defocus, diverge, camera and accumulate play no part.  With
 * maxBounceCount < 0 the loop of Trace does not run: rgb = 0 and rng comes back as given.
 *
 * For a camera ray of a frame and the generator state behind its two RandomPointInCircle draws (RC:565-576), rgb holds the bits that ray
 * contributes to its pixel.
 *
 * A record depends on its own ray only: not on n, not on the ray's place in the batch, not on the other rays.
 *
 * ---- Order, memory, state -------------------------------------------------------------------------------------------------------------
 * One path per lane.  A wave takes blocks of 64 consecutive rays, and a lane whose path has ended takes the next ray of the wave's
 * block (the refill of the frame's kernel), so a wave does not idle on its longest path; the CALLER'S ORDER still decides how coherent
 * the rays of a wave are.  The library does not reorder.
 *
 * The calls need rt_upload_scene and rt_set_params — not rt_resize — and ignore the context's image size and strip partition.
 *
 * They change nothing a caller can see: render targets, accumulation, frame counter, RtCounters (segments included), the phase profile,
 * the context's watchdog word, the adaptive tile list and the moments image are as before the call.
 *
 * rt_radiance_trace reads and writes host memory and is synchronous.
 * rt_radiance_trace_buffers reads and writes device memory of the context's device (e.g. a torch tensor's data_ptr()) and only enqueues:
 * the pass runs on the stream the context renders on (rt_set_stream is respected), behind every frame already requested — frames
 * rt_render_frame holds back are launched first — and behind every update already made, and is complete after rt_synchronize.
 *
 * Watchdog.  The pass has a watchdog word of its own, reported as rt_query.h states for its passes: RT_ERR_HIP when the traversal
 * watchdog fired in this pass — the records are then not valid, while the context's own images are not condemned by it.  The host form
 * reports that when it returns.  For the buffer form the report comes from the next rt_synchronize, or from the next rt_radiance_* call
 * if that comes first (which then does not run its own pass); either reports it once.
 *
 * Errors: RT_ERR_INVALID_ARG for a null context, n < 0, n > RT_QUERY_MAX_RAYS (2^26), a null pointer with n > 0, an output that overlaps
 * the input, and — buffer form — pointers that are not 16-byte aligned device memory of the context's device holding n * 32 (rays) and
 * n * 16 (records) bytes; RT_ERR_STATE before rt_upload_scene or before rt_set_params; RT_ERR_HIP as above.  n == 0 is RT_OK and
 * launches nothing (the pointers may then be null).
 *
 * Not in this header:  rt_multi_* forwarding (every context of rt_multi_context holds the whole scene: ask any one);  sorting or
 * regrouping of the rays by the library;  several samples per ray in one call (pass more rays, or chain rng);  per-bounce data.
 */
#ifndef RT_RADIANCE_H
#define RT_RADIANCE_H

#include "rt_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtPathRay {  /* 32 bytes, layout-compatible with RtRay: read as two 16-byte loads                            */
    float    origin[3];     /* world space                                                                                  */
    float    unused;        /* RtRay.tmax's place; ignored                                                                  */
    float    dir[3];        /* world space, used as given: NOT normalised by the library                                    */
    uint32_t rng;           /* the rngState handed to Trace (RtRay.reserved's place)                                        */
} RtPathRay;

typedef struct RtRadiance { /* 16 bytes, written as one 16-byte store                                                       */
    float    rgb[3];        /* Trace(CreateRay(origin, dir, 1, 0), rng), RC:479-542                                         */
    uint32_t rng;           /* the generator's state when Trace returned                                                    */
} RtRadiance;

int rt_radiance_trace(RtContext* ctx, const RtPathRay* rays, int n, RtRadiance* out);
int rt_radiance_trace_buffers(RtContext* ctx, const void* d_rays, int n, void* d_out);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtPathRay) == 32, "RtPathRay must be 32 bytes");
static_assert(sizeof(RtRadiance) == 16, "RtRadiance must be 16 bytes");
#endif

#endif /* RT_RADIANCE_H */
