/*
 * rt_aov.h — first-hit feature buffers ("AOVs") of a frame's camera rays (exported by libraytrace_hip.so, plain C).
 *
 * A progressive path tracer's caller sees noise for the first hundreds of frames; what it does about that — a denoiser,
 * temporal reprojection, object picking and outlines, depth compositing — starts from what each pixel's camera ray hit
 * first.  rt_render_aov answers that for every pixel of a frame: depth, world normal, world position, base colour,
 * emission, object and triangle.  It is the sibling of rt_cost.h's rt_render_cost: not what the first segment cost but
 * what it found, from the same device functions that render the frame (CalculateRayCollision, RayCommon.hlsl "RC":335-374).
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes it and adds one type and two calls.
 */
#ifndef RT_AOV_H
#define RT_AOV_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_AOV_HIT_MISS 0u        /* bits 0-1 of RtPixelAov.hit (== RtPixelCost.firstHit) */
#define RT_AOV_HIT_OPAQUE 1u
#define RT_AOV_HIT_GLASS 2u
#define RT_AOV_HIT_CLASS_MASK 3u
#define RT_AOV_HIT_BACKFACE 0x100u /* bit 8 of RtPixelAov.hit: HitInfo.isBackface */

typedef struct RtPixelAov {   /* 64 bytes, one per pixel                                                              */
    float    dst;             /* HitInfo.dst of the segment (RC:335-374), as rt_debug_intersect reports it: +inf on a  */
                              /*   miss                                                                                */
    float    normal[3];       /* HitInfo.normal — the world normal the tracer shades with, NOT flipped for back faces  */
                              /*   beyond what RaySphere / RayTriangle themselves do; 0 on a miss                      */
    float    pos[3];          /* HitInfo.pos = origin + dir * dst; 0 on a miss                                         */
    uint32_t hit;             /* bits 0-1: 0 miss, 1 opaque, 2 glass (material.flag); bit 8: HitInfo.isBackface        */
    float    albedo[3];       /* hit:  GetMaterialColour(material, pos, normal, isSpecular = false) (RC:440-466; the   */
                              /*       checker flag's pattern included)                                                */
                              /* miss: GetEnvironmentLight(rayDir) if RtParams.useSky, else 0 (RC:167-183)             */
    int32_t  object;          /* -1 miss; [0, nSpheres) sphere index; nSpheres + model index                           */
    float    emission[3];     /* hit: emissionColour.rgb * emissionStrength (RC:530, one fp32 multiply each); miss: 0  */
    int32_t  triangle;        /* model hit: absolute index into the uploaded triangle array; otherwise -1              */
} RtPixelAov;

/* Both calls describe CAMERA RAY 0 OF FRAME `frame` (>= 1; the value of RC's Frame uniform) of every pixel: uv as
 * RayCompute.compute:15, pixelIndex and rng = pixelIndex + Frame * 719393 + renderSeed (RC:550-556), then the first
 * pass of the ray loop RC:565-576 — the defocus draw, the diverge draw, normalize — exactly as the trace kernel does it.
 * So the record describes the very ray whose first segment rt_render_frame traces and rt_render_cost counts, with the
 * current scene and RtParams (numRaysPerPixel and maxBounceCount play no part).  Every value is the bit pattern the
 * tracer itself computes for that segment.
 *
 * Rows: rt_local_rows rows of width W, row 0 at the bottom, in the order rt_read_frame uses; uv.y comes from the
 * GLOBAL row, so the contexts of a strip partition together yield the rows of the whole image.
 * bytes = rows * W * 64, exactly.
 *
 * Changes nothing a caller can see: render targets, accumulation, frame counter, RtCounters and the context's watchdog
 * word are as before the call.  Frames rt_render_frame holds back are launched first.
 *
 * rt_render_aov writes host memory and is synchronous.
 *
 * rt_render_aov_to_device writes device memory (on the context's device; e.g. a torch tensor's data_ptr()) and only
 * enqueues: the pass runs on the stream the context renders on (rt_set_stream is respected), ordered after every frame
 * already requested, and is complete after rt_synchronize.
 *
 * Errors: RT_ERR_INVALID_ARG for a null context, a null pointer, frame < 1 or a size other than rows * W * 64, and for
 * a d_out that is not 16-byte aligned device memory of the context's device holding `bytes` bytes;
 * RT_ERR_STATE before rt_resize, rt_upload_scene or rt_set_params; RT_ERR_HIP when the traversal watchdog fired in this
 * pass — the records are then not valid, while the context's own images are not condemned by it (the pass has a watchdog
 * word of its own).  rt_render_aov reports that when it returns.  For rt_render_aov_to_device the report comes from the
 * next rt_synchronize, or from the next rt_render_aov / rt_render_aov_to_device call if that comes first (which then
 * does not run its own pass); either reports it once. */
int rt_render_aov(RtContext* ctx, int frame, RtPixelAov* out, size_t bytes);
int rt_render_aov_to_device(RtContext* ctx, int frame, void* d_out, size_t bytes);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtPixelAov) == 64, "RtPixelAov must be 64 bytes");
#endif

#endif /* RT_AOV_H */
