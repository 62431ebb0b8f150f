/*
 * rt_motion.h — reprojection that knows where a surface point WAS: records made from the unjittered pixel centre, and a per-object rigid
 * motion between the two views (exported by libraytrace_hip.so, plain C).
 *
 * rt_reproject.h carries the accumulated image across a camera move and has two limits.  Its records are those of camera ray 0 of a
 * frame, which carries that frame's jitter and defocus draw, so the history is resampled at jittered places; and only the camera may
 * move: a pixel on a model that rt_update_models moved restarts.  Both are one gap — "where was this surface point" had one answer,
 * "where it is now" — and this header closes it:
 *
 *   A. rt_render_aov_centre / rt_render_aov_centre_to_device: the RtPixelAov records of the ray through the pixel centre;
 *   B. RtObjectMotion, rt_motion_from_scene, rt_reproject_buffers_moving, rt_reproject_accumulated_moving: the reprojection of
 *      rt_reproject.h with a table that maps a CURRENT world position on object k to where that point lay in the PREVIOUS view's world.
 *
 * The pipeline of a moving camera and moving models:  keep the records the last rt_reproject_accumulated_moving wrote to d_cur_aov_out
 * (the first time: rt_render_aov_centre_to_device) and the scene arrays of that view;  rt_update_models / rt_update_spheres with the new
 * arrays and rt_set_params with the new camera;  rt_motion_from_scene(old arrays, new arrays);  upload the table;
 * rt_reproject_accumulated_moving(..., RT_AOV_CENTRE, ...);  rt_render_frames;  rt_resolve_to_device;  rt_denoise_buffers.
 *
 * Kept apart from rt_abi.h, rt_aov.h and rt_reproject.h, whose text is pinned: this header includes rt_reproject.h and adds one type and
 * five calls.  No existing call computes anything else than before.
 *
 * ---- A. The centre ray (a contract: every output bit is defined) -----------------------------------------------------------
 * For pixel id of a W x H image, with the context's current RtParams:
 *     uv         = id.xy / (Resolution - 1.0)                                                     (RayCompute.compute:15)
 *     focusPoint = mul(CamLocalToWorldMatrix, float4((uv - 0.5) * ViewParams.xy, ViewParams.z, 1))  (RayCommon.hlsl:555-556)
 *     rayOrigin  = camOrigin = mul(CamLocalToWorldMatrix, float4(0, 0, 0, 1))
 *     dir        = rt_normalize(focusPoint - camOrigin)
 * in the arithmetic rt_render_aov uses for the same lines.  There is no random draw: the record does not depend on `frame`, renderSeed,
 * defocusStrength or divergeStrength.  Everything after the ray is rt_render_aov's: the same intersection, hit point, normal, material
 * colour, sky, and triangle index, so the two calls give the same record for the same ray.  An image one pixel wide or high has
 * uv = 0 / 0 and yields the records of NaN rays, as rt_render_aov does.
 *
 * ---- B. The arithmetic of the reprojection ---------------------------------------------------------------------------------
 * rt_reproject.h's, with its conventions (binary32, one rounding per operation written, no contraction, rt_div, dot summed left to
 * right, "finite", "no history"), and these changes.  m = the 12 floats of entry k of the table, rows r = 0, 1, 2 at m[4r .. 4r+3].
 *
 *   1'. After step 1 (which tests a.object, the glass rule and the finiteness of a.pos and a.normal as before), for k = a.object:
 *       when 0 <= k < n_objects,
 *           pm[r] = ((m[4r] * a.pos.x + m[4r+1] * a.pos.y) + m[4r+2] * a.pos.z) + m[4r+3]
 *           nm[r] = (m[4r] * a.normal.x + m[4r+1] * a.normal.y) + m[4r+2] * a.normal.z                  (r = 0, 1, 2)
 *       nm is not renormalised.  Otherwise (k >= n_objects; an empty table) pm = a.pos and nm = a.normal exactly, bit for bit: such
 *       objects are static, and the call then computes what rt_reproject_buffers computes.  No history when a component of pm or nm
 *       is not finite (an entry that holds a NaN or an infinity therefore makes its object restart).
 *       An identity entry (1 0 0 0 / 0 1 0 0 / 0 0 1 0) gives pm == a.pos and nm == a.normal as VALUES: a component -0 becomes +0
 *       (-0 + +0), which can change nothing but the sign of a zero further on.
 *   2'. Step 2 with d = pm - O'.
 *   4'. Step 4's tap tests:  b(q).object != a.object skips, unchanged;
 *           dot(nm, b(q).normal) >= minNormalDot is false skips;
 *           |dot(nm, b(q).pos - pm)| <= maxPlaneDistance is false skips   (the tap's hit point off the tangent plane the centre HAD).
 *   Steps 3 and 5, the glass rule, the W == 1 / H == 1 rule, the tap order, the weights, the renormalisation over the taps that pass, the
 *   maxHistory cap and the form of the output are unchanged.  (csrc/rt_motion_math.h is this text as code, on top of
 *   csrc/rt_reproject_math.h, shared by the kernel and a host test.)
 *
 * rt_motion_from_scene builds the table, with the object numbering of RtPixelAov.object: spheres first, then models.
 *   Sphere i:  rows (1 0 0 tx) (0 1 0 ty) (0 0 1 tz) with t = prev.centre - cur.centre, one subtraction per component: a sphere has no
 *              orientation, its rotation is the identity.
 *   Model j:   the top three rows of prev.localToWorld x cur.worldToLocal.  With the column-major matrices of rt_abi.h (element (r, c)
 *              at [4c + r]) and A = prev.localToWorld, B = cur.worldToLocal:
 *                  m[4r + c] = ((A[r] * B[4c] + A[4 + r] * B[4c + 1]) + A[8 + r] * B[4c + 2]) + A[12 + r] * B[4c + 3]     in binary32.
 *   With an unchanged scale that product is a rigid map whatever the scale, uniform or not: the scales cancel between the two factors.  A
 *   scale (or a sphere's radius) that changed between the views gets the arithmetic as written; its points then mostly fail the plane
 *   test and restart.  Nothing is done about that.
 */
#ifndef RT_MOTION_H
#define RT_MOTION_H

#include "rt_reproject.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_AOV_CENTRE 0 /* aov_frame of rt_reproject_accumulated_moving: the internal pass is rt_render_aov_centre's */

typedef struct RtObjectMotion { /* 48 bytes */
    float m[12];                /* rows r = 0, 1, 2 of a 3 x 4 affine map, m[4r .. 4r+3]: current world position -> previous world position */
} RtObjectMotion;

/* The records of the pixel centres ("A" above).  The same 64-byte RtPixelAov as rt_render_aov / rt_render_aov_to_device, and the same row
 * order, size rule (bytes = rows * W * 64 exactly), side effects (none: render targets, frame counter, RtCounters and the context's
 * watchdog word stay as they are), stream rules (the device variant only enqueues on the stream the context renders on, behind every
 * frame already requested; d_out 16-byte aligned device memory of the context's device), error codes and watchdog reporting of the
 * pass's own word (the host variant fails when it returns; the device variant is reported once by the next rt_synchronize, rt_resolve or
 * call that runs an AOV pass, as RT_ERR_HIP).  A context that owns part of the image writes its rows, like rt_render_aov. */
int rt_render_aov_centre(RtContext* ctx, RtPixelAov* out, size_t bytes);
int rt_render_aov_centre_to_device(RtContext* ctx, void* d_out, size_t bytes);

/* The table from the scene arrays of the two views.  Pure host code, no device, no context.  `out` receives n_spheres + n_models entries.
 * A pointer may be null only where its count is 0 (`out` only when both counts are 0); RT_ERR_INVALID_ARG otherwise and for a negative
 * count. */
int rt_motion_from_scene(const RtSphere* prev_spheres, const RtSphere* cur_spheres, int n_spheres,
                         const RtModel* prev_models, const RtModel* cur_models, int n_models, RtObjectMotion* out);

/* rt_reproject_buffers with the table: d_motion is n_objects * 48 bytes of 16-byte aligned device memory of the context's device that
 * overlaps d_out_rgba nowhere (NULL is allowed when n_objects == 0, and d_motion is not looked at then).  Everything else as
 * rt_reproject_buffers states it: only enqueues, needs no scene and no rt_resize, changes nothing of the context, RT_ERR_STATE on a
 * partitioned context. */
int rt_reproject_buffers_moving(RtContext* ctx, const RtReprojectParams* p, int width, int height,
                                const void* d_prev_rgba, const void* d_prev_aov, const void* d_cur_aov,
                                const void* d_motion, int n_objects, void* d_out_rgba);

/* rt_reproject_accumulated with the table, in every respect that call's text lists: frames held back are launched first; it only
 * enqueues, on the stream the context renders on; it uses the scratch the context shares with rt_denoise; d_cur_aov_out is optional;
 * when the watchdog fired in the internal AOV pass the device leaves AccumulatedRender exactly as it was, and the failure is reported once
 * by the next rt_synchronize, rt_resolve or call that runs an AOV pass.  It changes AccumulatedRender and nothing else.
 * aov_frame == RT_AOV_CENTRE: the internal pass (and so d_cur_aov_out) is rt_render_aov_centre's — d_prev_aov should then hold centre
 * records too;  aov_frame >= 1: the pass of that frame, as in rt_reproject_accumulated;  negative: RT_ERR_INVALID_ARG.
 * d_motion as above; it overlaps neither AccumulatedRender nor d_cur_aov_out.  The table is read when the enqueued work runs: keep it
 * unchanged until then. */
int rt_reproject_accumulated_moving(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, int aov_frame,
                                    const void* d_motion, int n_objects, void* d_cur_aov_out);

/* Errors, beyond those of the calls these extend (rt_aov.h, rt_reproject.h): RT_ERR_INVALID_ARG for n_objects < 0 or more than 2^24, for
 * a null d_motion with n_objects > 0, and for a d_motion that is misaligned, not n_objects * 48 bytes of device memory of the context's
 * device, or overlapping an output;  RT_ERR_STATE on a partitioned context for the two reproject calls. */

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtObjectMotion) == 48, "RtObjectMotion must be 48 bytes");
#endif

#endif /* RT_MOTION_H */
