/*
 * rt_nee.h — radiance with direct light sampling (next-event estimation, NEE) for batches of caller-made rays (exported by
 * libraytrace_hip.so, plain C).
 *
 * rt_radiance.h finds light only by hitting it: Trace adds emissionCol * emissionStrength when a bounce lands on an emitter
 * (RayCommon.hlsl "RC":530-531).  A diffuse vertex finds a small emitter with a probability of a few per cent, and everything else about
 * such a path is noise.  The two calls of this header run the same integrator with one change: at every diffuse vertex one emitter of the
 * scene is sampled directly and tested with one closest-hit walk, and the emission a later bounce would have found by luck is left out in
 * exchange.  Apart from the cut at maxBounceCount (below), the expectation of rgb over the generator is Trace's for every ray; the
 * variance is not.
 *
 * This header includes rt_radiance.h and follows it word for word in: the records (RtPathRay in, RtRadiance out), the ray layout, the rng
 * chaining, the limits and the alignment rules; the error codes (RT_ERR_STATE before rt_upload_scene / rt_set_params included); "changes
 * nothing a caller can see" and "a record depends on its own ray only"; the stream and ordering rules of the host and the buffer form; and
 * the watchdog report — the pass has a watchdog word of its own, and "the next rt_radiance_* call" reads "the next rt_nee_trace*
 * call" here (a pass of rt_radiance_trace_buffers and a pass of this header report their own words only).  The calls are named rt_nee_*:
 * the prefix rt_radiance_ stays with rt_radiance.h's two calls alone.
 *
 * ---- The estimator (a contract: every output bit is defined) --------------------------------------------------------------------------
 * Record i is Trace (RC:479-542) of ray i with the three amendments below.  All arithmetic is fp32 with the primitives of rt_math.h, one
 * rounding per operation, no contraction, in the order written; a * b * c means (a * b) * c; dot() and normalize() are rt_dot and
 * rt_normalize; x / y is rt_div(x, y); PI2 = 2 * 3.1415926f and PI = 3.1415926f (RandomValueNormalDistribution's literal, RC:141-147).
 *
 * Amendment 1 — the light table (built on the host, from the scene as of the last rt_upload_scene / rt_update_models /
 * rt_update_spheres; rt_debug_light_table builds the same table without a device).
 *   Le of an object = emissionCol.rgb * emissionStrength (three fp32 products).  An object is an EMITTER iff its material's flag is not
 *   RT_MATERIAL_GLASS (the glass branch never adds emission), Le is finite in all three components, and a component of Le is > 0.  A
 *   checkered material is an emitter by the same rule and no other.
 *   Entries, in this order: the sphere emitters with radius > 0 (and finite), by sphere index, one entry each; then the model emitters by
 *   model index, one entry per triangle of non-zero area, by triangle index.  A model's triangles are [triOffset, end), end = the
 *   smallest triOffset of any model of the scene that is larger than this one's, or n_triangles: the meshes lie one behind the other
 *   (CreateAllMeshData, RCM:206-236), and an instanced mesh gives one set of entries per model.
 *   World corners of a triangle: P = mul(localToWorld, float4(p, 1)), each row m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * 1
 *   summed left to right (rt_mul_point).  When the 3 x 3 linear part of localToWorld has a negative determinant (evaluated in double,
 *   cofactors along the first row), B and C are swapped, so that the geometric normal points to the side the local-space front-face test
 *   (RC:206, determinant >= 1E-8) accepts.  Then e1 = B - A and e2 = C - A in fp32, and — in double, from the fp32 corners —
 *   E1 = B - A, E2 = C - A, X = cross(E1, E2) (each component a * b - c * d), L = sqrt(X.x * X.x + X.y * X.y + X.z * X.z),
 *   ng = (float)(X / L) per component, S = (float)(0.5 * L).  The triangle is an entry iff S is finite and > 0 and ng is finite.
 *   Weight (double): a sphere's is (4 * pi * ((double)r * r)) * max(Le); a triangle's is (double)S * max(Le); max(Le) the largest
 *   component.  With T = the weights summed in entry order, cdf[i] = (float)((w[0] + ... + w[i]) / T) — the running sum, in entry
 *   order — with the last entry forced to 1.0f, and prob[i] = (float)(w[i] / T).
 *   Pick rule for u in [0, 1]: the smallest i with u < cdf[i]; u == 1 picks the last entry.  (The kernel finds it by a binary search of
 *   at most 23 steps with the index clamped to the table.)
 *   More than RT_NEE_MAX_LIGHTS entries: RT_ERR_SCENE from the calls of this header (the scene itself stays usable by every other call).
 *
 * Amendment 2 — the sample at a diffuse vertex.  A hit on a non-glass object is a DIFFUSE VERTEX iff smoothness * (isSpecularBounce ? 1 :
 * 0) == 0.0f: the direction of RC:527 is then diffuseDir, the cosine lobe about the shading normal n.  At such a vertex, when the table
 * is not empty, behind  rayColour *= GetMaterialColour(...)  (RC:532) and BEFORE the roulette draw of RC:537:
 *   u0 = RandomValue, u1 = RandomValue, u2 = RandomValue (in this order, from the path's generator);  i = pick(u0);
 *   x = the continuation origin hit.pos + hit.normal * 0.001f (RC:524: the origin of the next segment), T = rayColour as just updated.
 *   SPHERE entry (centre c, r2 = radius * radius, the product rt_upload_scene stores):
 *     w = c - x;  d2 = dot(w, w);  unless d2 > r2 nothing is added (and no walk runs).
 *     s2 = r2 / d2;  cmax = rt_sqrt(1 - s2);  q = s2 / (1 + cmax)      [q = 1 - cos(theta_max) = sin^2 / (1 + cos)]
 *     ct = 1 - u1 * q;  st = rt_sqrt(rt_max(0, 1 - ct * ct));  rt_sincos(PI2 * u2, &sn, &cs)
 *     z = normalize(w);  the basis (branch-free; Duff et al. 2017):  sg = copysign(1, z.z) [the sign BIT of z.z];  a = -rt_rcp(sg + z.z);
 *     b = z.x * z.y * a;  b1 = (1 + sg * z.x * z.x * a,  sg * b,  -sg * z.x);  b2 = (b,  sg + z.y * z.y * a,  -z.y)
 *     omega = b1 * (st * cs) + b2 * (st * sn) + z * ct      (per component, summed left to right; not normalised again)
 *     cn = dot(n, omega);  unless cn > 0 nothing is added (no walk).
 *     One closest-hit walk (CalculateRayCollision, RC:335-374 — the walk rt_query_closest runs, no early exit, no tmax) from x along
 *     omega.  Unless the closest hit's object is this sphere nothing is added.
 *     g = (cn * 2 * q) / prob[i];  incomingLight += (T * Le) * g.
 *   TRIANGLE entry (world corner A, e1, e2, ng, S, absolute triangle index k of model m):
 *     the fold map: if u1 + u2 > 1 then (v1, v2) = (1 - u1, 1 - u2) else (u1, u2);  y = A + e1 * v1 + e2 * v2 (left to right)
 *     v = y - x;  d2 = dot(v, v);  omega = normalize(v);  cl = dot(ng, -omega);  cn = dot(n, omega)
 *     unless cl > 0 and cn > 0 nothing is added (no walk).
 *     The same walk from x along omega.  Unless the closest hit's object is model m AND its triangle is k nothing is added.
 *     g = (cn * cl * S) / (PI * d2 * prob[i]);  incomingLight += (T * Le) * g.
 *   Le is the entry's: the object's Le as above.  Identity with the closest hit is the visibility test: there is no tmax and no second
 *   epsilon, and back-face culling of opaque models (RC:355) makes it exact from behind.
 *
 * Amendment 3 — no double counting.  When the previous vertex of the path was a diffuse vertex at which amendment 2 applied (the table
 * was not empty), the emission of RC:530-531 is NOT added for a hit object that has an entry in the table — except a sphere hit from
 * inside (isBackface), which keeps it, because the cone could not sample it.  In every other case emission is added as in the reference:
 * on the first hit of the caller's ray, behind a specular or glass vertex, and for objects without an entry.
 *
 * Two identities follow and are part of the contract: with an empty table the records are rt_radiance_trace's bit for bit, rng included;
 * and a path that meets no diffuse vertex has the same bits too.
 *
 * The expectation, and where it is not Trace's.  With B = maxBounceCount, Trace collects the emission of hits 0 .. B.  Here a sample at
 * vertex k stands for the emission hit k + 1 would have found, and samples are taken at vertices 0 .. B: behind diffuse vertices the
 * estimator carries emitter light of hits 1 .. B + 1, ONE BOUNCE MORE than Trace at the same B.  Its expectation is Trace's plus the
 * expected emission of hit B + 1 where vertex B is a diffuse vertex and that hit is an object of the table (a sphere from inside
 * excepted).  With maxBounceCount = 0 Trace returns the emission a ray sees directly and this pass returns the directly lit surface as
 * well.  The difference falls with the paths that live to bounce B (Russian roulette) and is 0 in the limit of B; it is part of the
 * contract, not an error bound.
 *
 * ---- The other calls -------------------------------------------------------------------------------------------------------------------
 * rt_nee_light_count: the table as the next pass would use it (rebuilt here if an update made it stale): its sphere and its triangle
 * entries.  Either pointer may be null.  RT_ERR_STATE before rt_upload_scene, RT_ERR_SCENE past the cap.
 * rt_debug_light_table: host only, no device — the table of these arrays (nodes are not needed: see the triangle ranges above).  On RT_OK
 * the caller frees it with rt_debug_light_table_free.  RT_ERR_INVALID_ARG for a null output, a negative count, a null array with a
 * positive count or a triOffset outside [0, n_triangles]; RT_ERR_SCENE past the cap; RT_ERR_OOM.
 *
 * Not in this header: the sun and the sky as NEE targets (they stay with the miss branch); multiple importance sampling (the blended
 * lobes of RC:511-512 and RC:527 have no usable density); rt_multi_* forwarding; an image-shaped frame call.
 */
#ifndef RT_NEE_H
#define RT_NEE_H

#include "rt_radiance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_NEE_MAX_LIGHTS (1 << 22)

typedef struct RtLightEntry { /* 80 bytes: what the kernel reads of an entry, as five 16-byte loads                               */
    float    a[3];          /* sphere: the centre;  triangle: world corner A                                                    */
    float    size;          /* sphere: radius * radius;  triangle: the area S                                                   */
    float    e1[3];         /* triangle: B - A (B and C swapped under a mirroring transform);  sphere: 0                        */
    float    prob;          /* the entry's selection probability                                                                */
    float    e2[3];         /* triangle: C - A;  sphere: 0                                                                      */
    int32_t  object;        /* RtRayHit.object's numbering: spheres first, then the models                                      */
    float    ng[3];         /* triangle: the world-space geometric normal;  sphere: 0                                           */
    int32_t  triangle;      /* triangle: its index in the uploaded triangle array;  sphere: -1                                  */
    float    emission[3];   /* Le                                                                                               */
    float    reserved;      /* 0                                                                                                */
} RtLightEntry;

typedef struct RtLightTableDump {
    int32_t       n_entries, n_sphere_entries, n_triangle_entries, reserved;
    RtLightEntry* entries;  /* n_entries                                                                                        */
    float*        cdf;      /* n_entries, non-decreasing, the last one 1.0f                                                     */
} RtLightTableDump;

int rt_nee_trace(RtContext* ctx, const RtPathRay* rays, int n, RtRadiance* out);
int rt_nee_trace_buffers(RtContext* ctx, const void* d_rays, int n, void* d_out);
int rt_nee_light_count(RtContext* ctx, int* n_sphere_emitters, int* n_triangle_emitters);
int rt_debug_light_table(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles, const RtSphere* spheres, int n_spheres,
                         RtLightTableDump* out);
void rt_debug_light_table_free(RtLightTableDump* d);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtLightEntry) == 80, "RtLightEntry must be 80 bytes");
#endif

#endif /* RT_NEE_H */
