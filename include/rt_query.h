/*
 * rt_query.h — closest-hit and occlusion queries for batches of caller-made rays against the uploaded scene (exported by
 * libraytrace_hip.so, plain C).
 *
 * Everything else this library answers is image-shaped and bound to the camera.  These four calls answer the question a ray-tracing
 * library is asked first — "what does THIS ray hit" and "is THIS segment blocked" — for picking off the pixel grid, line of sight,
 * ambient occlusion and light baking driven from torch, collision probes, or depth from a second viewpoint.  They run the device
 * functions that render the frame (CalculateRayCollision, RayCommon.hlsl "RC":335-374, with the sphere buffer hooked at RC:341), so a
 * record holds the bit patterns the tracer itself computes for that ray.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes rt_aov.h (for RT_AOV_HIT_*, and through it rt_abi.h) and adds
 * two types and four calls.
 *
 * ---- The closest hit (a contract: every output bit is defined) -------------------------------------------------------------------------
 * Record i is what CalculateRayCollision returns for (rays[i].origin, rays[i].dir) with the scene as of the last rt_upload_scene /
 * rt_update_models / rt_update_spheres.  For the fields they share these are the bits rt_debug_intersect reports for that ray and the
 * bits RtPixelAov holds for a pixel whose camera ray it is; `object` and `triangle` are as in rt_aov.h.  The direction is used as given:
 * it is NOT normalised, so dst is in units of |dir| (pos = origin + dir * dst), as in the reference.  tmax and reserved play no part.
 * Rays with zero, infinite or NaN components are legal: the record is whatever the reference's arithmetic yields for them.
 *
 * ---- Occlusion ------------------------------------------------------------------------------------------------------------------------
 * occluded[i] = 1 iff the closest-hit record of ray i has object >= 0 and dst < tmax; otherwise 0.  The comparison is strict and an
 * ordinary fp32 one: a NaN tmax gives 0, tmax = +inf means "any hit", tmax <= 0 gives 0.  Glass occludes like anything else.
 *
 * Early exit.  The occlusion pass may end a ray's walk at the first ACCEPTED hit with dst < tmax.  Up to that hit the walk is the
 * closest-hit walk, step for step: the same boxes culled against the same closest distance so far, the same tests in the same order.
 * The closest-hit walk accepts that hit too (an accepted hit replaces the closest so far), and every later acceptance only lowers the
 * distance; so the final closest dst is at most this one, hence < tmax, and object >= 0: the answer is 1 either way.  A walk that never
 * accepts such a hit runs to its end and is the closest-hit walk.  So the answers coincide exactly, for every ray.  The walk's closest
 * distance is NOT seeded with tmax: that would cull boxes the closest-hit walk enters and is not needed for the argument.
 *
 * ---- Order, memory, state -------------------------------------------------------------------------------------------------------------
 * One ray per lane; a wave takes 64 consecutive rays, so the CALLER'S ORDER decides how coherent a wave's rays are (camera rays in 8 x 8
 * tile order traverse faster than in row order; rays sorted by origin cell and direction octant faster than shuffled ones).  The library
 * does not reorder.
 *
 * The calls need rt_upload_scene only — not rt_resize, not rt_set_params — and ignore the context's image size and strip partition: a
 * context that owns part of an image answers every ray.
 *
 * They change nothing a caller can see: render targets, accumulation, frame counter, RtCounters, the context's watchdog word, the
 * adaptive tile list and errors and the moments image are as before the call.
 *
 * rt_query_closest / rt_query_occluded read and write host memory and are synchronous.
 * rt_query_closest_buffers / rt_query_occluded_buffers read and write device memory of the context's device (e.g. a torch tensor's
 * data_ptr()) and only enqueue: the pass runs on the stream the context renders on (rt_set_stream is respected), behind every frame
 * already requested — frames rt_render_frame holds back are launched first — and behind every update already made, and is complete
 * after rt_synchronize.
 *
 * Watchdog.  The pass has a watchdog word of its own, reported as rt_aov.h states for the AOV pass: RT_ERR_HIP when the traversal
 * watchdog fired in this pass — the records or answers are then not valid, while the context's own images are not condemned by it.  The
 * host forms report that when they return.  For the buffer forms the report comes from the next rt_synchronize, or from the next
 * rt_query_* call if that comes first (which then does not run its own pass); either reports it once.
 *
 * Errors: RT_ERR_INVALID_ARG for a null context, n < 0, n > RT_QUERY_MAX_RAYS (2^26), a null pointer with n > 0, an output that overlaps
 * the input, and — buffer forms — pointers that are not 16-byte aligned device memory of the context's device holding n * 32 (rays),
 * n * 48 (hits) or n * 4 (answers) bytes; RT_ERR_STATE before rt_upload_scene; RT_ERR_HIP as above.  n == 0 is RT_OK and launches
 * nothing (the pointers may then be null).
 *
 * Not in this header:  rt_multi_* forwarding (every context of rt_multi_context holds the whole scene: ask any one);  a tmin (offset the
 * origin);  sorting of the rays by the library;  any-hit filters by material.
 */
#ifndef RT_QUERY_H
#define RT_QUERY_H

#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_QUERY_MAX_RAYS (1 << 26) /* rays per call */

typedef struct RtRay {      /* 32 bytes, read as two 16-byte loads                                                          */
    float    origin[3];     /* world space                                                                                  */
    float    tmax;          /* occlusion calls only; the closest-hit calls ignore it                                        */
    float    dir[3];        /* world space, used as given: NOT normalised by the library (dst is in units of |dir|)         */
    uint32_t reserved;      /* ignored on the device (not checked per ray)                                                  */
} RtRay;

typedef struct RtRayHit {   /* 48 bytes, written as three 16-byte stores                                                    */
    float    dst;           /* HitInfo.dst of CalculateRayCollision (RC:335-374): +inf on a miss                            */
    float    normal[3];     /* HitInfo.normal; 0 on a miss (as RtPixelAov.normal)                                           */
    float    pos[3];        /* HitInfo.pos = origin + dir * dst; 0 on a miss                                                */
    uint32_t hit;           /* RtPixelAov.hit: bits 0-1 RT_AOV_HIT_MISS / _OPAQUE / _GLASS, bit 8 RT_AOV_HIT_BACKFACE       */
    int32_t  object;        /* -1 miss; [0, nSpheres) sphere index; nSpheres + model index                                  */
    int32_t  triangle;      /* model hit: absolute index into the uploaded triangle array; otherwise -1                     */
    uint32_t reserved[2];   /* written as 0                                                                                 */
} RtRayHit;

int rt_query_closest(RtContext* ctx, const RtRay* rays, int n, RtRayHit* hits);
int rt_query_closest_buffers(RtContext* ctx, const void* d_rays, int n, void* d_hits);
int rt_query_occluded(RtContext* ctx, const RtRay* rays, int n, uint32_t* occluded);            /* one uint32 (0 / 1) per ray */
int rt_query_occluded_buffers(RtContext* ctx, const void* d_rays, int n, void* d_occluded);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtRay) == 32, "RtRay must be 32 bytes");
static_assert(sizeof(RtRayHit) == 48, "RtRayHit must be 48 bytes");
#endif

#endif /* RT_QUERY_H */
