/*
 * rt_cost.h — per-pixel traversal cost of a frame (exported by libraytrace_hip.so, plain C).
 *
 * The reference declares the pieces of a BVH heatmap and never wires them up: the uniforms visMode / debugVisScale /
 * debugParams (RayCommon.hlsl "RC":24-26) and a per-ray `stats` int2 that counts triangle tests and box tests
 * (RC:254,271,339).  rt_render_cost renders a frame's paths with the same device code as a frame rendered with stats on
 * (rt_enable_stats) and reports, for every pixel, the work its rays did.  Summed over the image the fields equal the
 * RtCounters delta of that frame; per pixel they equal the reference's own counting of the same rays.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes it and adds one type and one call.
 */
#ifndef RT_COST_H
#define RT_COST_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtPixelCost {      /* 32 bytes, one per pixel                                              */
    uint32_t segments;            /* CalculateRayCollision calls (RC:487) over all NumRaysPerPixel paths  */
    uint32_t innerSteps;          /* inner nodes popped = box-test pairs (RC:262-282; stats[1] / 2)       */
    uint32_t leafSteps;           /* leaves popped (RC:248-261)                                           */
    uint32_t triTests;            /* RayTriangle calls (RC:253-254; stats[0])                             */
    uint32_t primaryInnerSteps;   /* the same three, counted only in the FIRST segment of each camera     */
    uint32_t primaryLeafSteps;    /*   ray (bounce 0), summed over the pixel's camera rays                */
    uint32_t primaryTriTests;
    uint32_t firstHit;            /* camera ray 0's first segment: 0 miss, 1 opaque hit, 2 glass hit      */
} RtPixelCost;

/* Traces frame `frame` (>= 1; the value of RC's Frame uniform, so the seed is RC:552's) with the current scene and
 * RtParams, and writes one RtPixelCost per pixel of the context's rows: rt_local_rows rows of width W, row 0 at the
 * bottom, in the order rt_read_frame uses.  bytes = rows * W * 32.
 * Changes no state: render targets, accumulation, frame counter, RtCounters and the watchdog word are as before the
 * call.  Synchronous (frames rt_render_frame holds back are launched first).  Values wrap modulo 2^32.
 * Errors: RT_ERR_INVALID_ARG for a null context, frame < 1 or a size other than rows * W * 32; RT_ERR_STATE before
 * rt_resize, rt_upload_scene or rt_set_params; RT_ERR_HIP when a kernel watchdog fired during this launch (the output
 * is then not valid; the context's own images are not condemned by it). */
int rt_render_cost(RtContext* ctx, int frame, RtPixelCost* out, size_t bytes);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtPixelCost) == 32, "RtPixelCost must be 32 bytes");
#endif

#endif /* RT_COST_H */
