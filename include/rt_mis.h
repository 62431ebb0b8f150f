/*
 * rt_mis.h — radiance with direct light sampling COMBINED with the cosine lobe by the balance heuristic (multiple importance
 * sampling, MIS) for batches of caller-made rays (exported by libraytrace_hip.so, plain C).
 *
 * rt_nee.h samples one emitter at every diffuse vertex and leaves out the emission the next bounce would have found.  Its weight is the
 * ratio of two densities, and next to an emitter that ratio has no bound: a vertex 4 cm from a light returns, rarely, a value thousands
 * of times the light's own radiance.  rt_nee.h says that the blended lobes have no usable density, and that holds for the blended lobes
 * only: a sample is taken at a DIFFUSE VERTEX alone, where the continuation is normalize(normal + RandomDirection) — an exact cosine
 * lobe with density cos / PI.  So both strategies have a density exactly where the sample is taken; this header weights each by the
 * balance heuristic, and every contribution is at most T * Le.
 *
 * ONE call, which takes a call descriptor (RtMisBatch).  It launches the frames rt_render_frame holds back before it reads anything
 * (include/rt_held_back.h: in that header's words it is a `flushes` call): the pass runs behind them, on the render stream.
 *
 * This header includes rt_nee.h and follows rt_nee.h and rt_radiance.h word for word in: the records (RtPathRay in, RtRadiance out), the
 * ray layout, the rng chaining, the limits (n <= 2^26) and the alignment rules (16 bytes, device form); "changes nothing a caller can
 * see" and "a record depends on its own ray only"; the stream and ordering rules — memory == RT_MIS_HOST is the host form (host
 * pointers, synchronous), memory == RT_MIS_DEVICE the buffer form (device pointers, enqueued on the stream the context renders on,
 * rays and out must not overlap); the error codes (RT_ERR_STATE before rt_upload_scene / rt_set_params included; n == 0 with null
 * pointers is RT_OK); and the watchdog report — the pass has a watchdog word of its own, and "the next rt_radiance_* call" reads "the
 * next rt_mis_trace call" here: a device-form pass whose walks were cut short is reported once, by the next rt_mis_trace or by
 * rt_synchronize, and fails that pass, not the context (passes of rt_radiance.h and rt_nee.h report their own words only).
 * The descriptor: struct_size must be sizeof(RtMisBatch), reserved 0, memory RT_MIS_HOST or RT_MIS_DEVICE, ctx not null;
 * otherwise RT_ERR_INVALID_ARG and nothing is written.  The text of an error is rt_last_error(ctx)'s, or the global message when the
 * descriptor or its ctx is null.
 *
 * ---- The estimator (a contract: every output bit is defined) --------------------------------------------------------------------------
 * Record i is Trace (RayCommon.hlsl "RC":479-542) of ray i with the amendments below.  Arithmetic as in rt_nee.h: fp32 with the
 * primitives of rt_math.h, one rounding per operation, no contraction, in the order written; a * b * c means (a * b) * c; dot() and
 * normalize() are rt_dot and rt_normalize; x / y is rt_div(x, y); PI2 = 2 * 3.1415926f and PI = 3.1415926f.
 *
 * The light table is amendment 1 of rt_nee.h, unchanged (rt_debug_light_table builds it without a device).  More than
 * RT_NEE_MAX_LIGHTS entries: RT_ERR_SCENE from this call only.
 *
 * The reverse map.  entry(object, triangle) is the index of the table entry with that object and that triangle (-1 for a sphere), or
 * NONE (RT_MIS_NO_ENTRY) where the table has no such entry: a non-emitter, an excluded sphere, a zero-area triangle.  An instanced
 * mesh has one entry per model, so the object tells them apart.  rt_debug_light_map builds the map without a device.
 *
 * Where a sample is taken.  At a diffuse vertex, as rt_nee.h defines it (a hit on a non-glass object with smoothness * (isSpecularBounce
 * ? 1 : 0) == 0.0f), when the table is not empty AND the path could still continue behind this vertex: bounce < maxBounceCount, with
 * bounce = the index of the vertex counted from 0 (the loop variable i of RC:485).  At the last vertex nothing is drawn and nothing is
 * sampled.  (rt_nee.h samples there as well and so carries one bounce more of emitter light than Trace; this pass does not.  Its
 * expectation is Trace's at every maxBounceCount, not only in the limit.)
 *
 * The light sample follows amendment 2 of rt_nee.h unchanged in: its place (behind rayColour *= GetMaterialColour, before the roulette
 * draw); the draws u0, u1, u2; the pick; x, omega and every "nothing is added" rule (d2 > r2, cn > 0, cl > 0); the one closest-hit walk
 * from x along omega and the identity test with the closest hit.  Only the scalar differs.  With cn (and q, or cl, d2, S) as there:
 *     pb = cn / PI                                      [the cosine lobe's density of omega]
 *     SPHERE:    pl = prob / (PI2 * q)                  [the cone's density: 1 / (2 pi (1 - cos theta_max)), times the pick's]
 *     TRIANGLE:  pl = (prob * d2) / (cl * S)            [the area density 1 / S as a solid-angle density, times the pick's]
 *     g = pb / (pl + pb);  a g that is not within [0, 1] — a NaN, from 0 / 0 or inf / inf — is 0.
 *     incomingLight += (T * Le) * g.
 * The vertex also remembers the lobe's density of the continuation direction actually taken: with rdir_next the direction of RC:527
 * (here diffuseDir), cn' = dot(n, rdir_next) and pbPrev = cn' / PI.
 *
 * The emission of the next hit.  When the previous vertex of the path took a sample (drew u0, u1, u2), let e = entry(hit object, hit
 * triangle) at the emission add of RC:530-531.  If e is NONE, or the hit is a sphere hit from inside (isBackface), emission is added in
 * full as in Trace.  Otherwise emitted * rayColour is added times wb (each component one product more).  wb = 1 unless cn' > 0 and
 * the light sampler could have produced this direction from the previous x — x is the segment's origin, rdir its direction:
 *     SPHERE entry (c, r2):   w = c - x;  d2 = dot(w, w);  unless d2 > r2, wb = 1.  s2 = r2 / d2;  cmax = rt_sqrt(1 - s2);
 *                             q = s2 / (1 + cmax);  pl' = prob / (PI2 * q)
 *     TRIANGLE entry (ng, S): v = hit.pos - x;  d2 = dot(v, v);  cl = dot(ng, -rdir);  unless cl > 0, wb = 1.
 *                             pl' = (prob * d2) / (cl * S)
 *     wb = pbPrev / (pbPrev + pl');  a wb that is not within [0, 1] (a NaN) is 1.
 * (The two NaN rules are each other's complement: a direction whose light density cannot be computed is left to the lobe.)
 * In every other case — the first hit of the caller's ray, behind a specular or glass vertex, behind a vertex that took no sample —
 * emission is added as in the reference.
 *
 * Identities, part of the contract.  Each of these gives the bits of rt_radiance_trace, the generator state included: an empty table;
 * a path without a diffuse vertex; maxBounceCount <= 0.
 *
 * The bound.  g and wb lie in [0, 1] and are never NaN.  With every material colour component at most 1, T <= 1 in every component
 * behind the roulette (RC:535-538 divides by the largest component).  A vertex adds at most one weighted emission and one light sample,
 * each at most T * Le, and a path has at most maxBounceCount + 1 vertices, so for every record, componentwise,
 *     rgb <= 2 * (maxBounceCount + 1) * max(Le over the scene) + the sky's bound
 * (the sky's bound: the largest value GetEnvironmentLight can return; 0 without UseSky).
 *
 * ---- The other calls -------------------------------------------------------------------------------------------------------------------
 * rt_debug_light_map: host only, no device — the reverse map of the table rt_debug_light_table builds from the same arrays.
 * objects[o] (o in RtRayHit.object's numbering, spheres first): a sphere's entry, or for a model the index into `triangles` of the
 * word of its first triangle; RT_MIS_NO_ENTRY where the object has no entry.  triangles[objects[o] + (k - triOffset)] = the entry of
 * triangle k of model o, or RT_MIS_NO_ENTRY; a model with an entry has one word for each triangle of its range [triOffset, end).  On RT_OK the caller frees it with rt_debug_light_map_free.  Errors as
 * rt_debug_light_table.
 *
 * Not in this header: the sun and the sky as targets; the power heuristic; rt_multi_* forwarding.
 */
#ifndef RT_MIS_H
#define RT_MIS_H

#include "rt_nee.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MIS_HOST 0u
#define RT_MIS_DEVICE 1u
#define RT_MIS_NO_ENTRY 0xffffffffu

typedef struct RtMisBatch {
    uint32_t    struct_size;   /* = sizeof(RtMisBatch): handshake, RT_ERR_INVALID_ARG otherwise                              */
    uint32_t    memory;        /* RT_MIS_HOST (0): synchronous, host pointers;  RT_MIS_DEVICE (1): enqueue only              */
    RtContext*  ctx;
    const void* rays;          /* n RtPathRay                                                                                */
    void*       out;           /* n RtRadiance                                                                               */
    int32_t     n;
    int32_t     reserved;      /* 0, RT_ERR_INVALID_ARG otherwise                                                            */
} RtMisBatch;

typedef struct RtLightMapDump {
    int32_t   n_objects, n_triangle_words, n_entries, reserved;
    uint32_t* objects;   /* n_objects                                                                                        */
    uint32_t* triangles; /* n_triangle_words                                                                                 */
} RtLightMapDump;

int rt_mis_trace(const RtMisBatch* batch);
int rt_debug_light_map(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles, const RtSphere* spheres, int n_spheres,
                       RtLightMapDump* out);
void rt_debug_light_map_free(RtLightMapDump* d);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtMisBatch) == 40, "RtMisBatch must be 40 bytes");
#endif

#endif /* RT_MIS_H */
