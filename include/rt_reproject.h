/*
 * rt_reproject.h — carry an accumulated image across a camera move, guided by the first-hit buffers of rt_aov.h (exported by
 * libraytrace_hip.so, plain C).
 *
 * A progressive path tracer's sum belongs to one view.  When the camera moves, the caller either resets it and starts from one noisy
 * frame, or keeps a sum that shows another view.  Temporal reprojection is the third way: for every pixel of the NEW view, find where
 * the surface point it sees lay in the OLD image, take the old mean from there if the old image saw the same surface, and start the
 * new sum from that mean with the old frame count.  rt_aov.h yields what this needs — per pixel the object, the world normal and the
 * world position of what the camera ray hit first, for the old view and for the new.
 *
 * The alpha channel of AccumulatedRender is the number of frames summed into a pixel (RayCompute.compute:22 adds float4(col, 1)).  After
 * a reprojection that count differs from pixel to pixel, the sum stays a sum, and the frames rendered afterwards add onto it exactly
 * as they always do: no trace kernel knows about this header.  What a per-pixel count needs is a per-pixel divide — rt_resolve, below;
 * rt_display divides by the one global Frame.
 *
 * The pipeline of a moving camera:  rt_render_aov_to_device (the records of the view that is about to be left — or keep the ones the
 * last rt_reproject_accumulated wrote), rt_set_params (the new camera), rt_reproject_accumulated, rt_render_frames,
 * rt_resolve_to_device, rt_denoise_buffers with scale = 1.  No step copies through the host.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes rt_aov.h and adds one type and six calls.
 *
 * ---- The arithmetic (a contract, like everything this library computes: every output bit is defined) -----------------------
 * IEEE binary32, one rounding per operation written below, no contraction; rt_div is include/rt_math.h's; dot(a, b) is
 * a.x*b.x + a.y*b.y + a.z*b.z summed left to right.  "Finite" means: the exponent field is not all ones.  (csrc/rt_reproject_math.h is
 * this text as code, shared by the kernels and a host test.)
 *
 * Reprojection.  For pixel p of a W x H image: a = d_cur_aov[p], the current view's record; P = d_prev_rgba, the previous view's RGBA
 * sum; b = d_prev_aov, the previous view's records; R', U', F', O' = columns 0, 1, 2, 3 (three rows each) of prevCamLocalToWorld;
 * (pw, ph, fd) = prevViewParams.  "No history" means out(p) = (+0, +0, +0, +0), exactly what rt_reset_accumulation writes.
 *
 *   1. No history when a.object < 0 (a miss), when (a.hit & 3) == RT_AOV_HIT_GLASS and bit 0 of flags is clear (what is seen THROUGH
 *      glass moves differently from the glass), or when a component of a.pos or a.normal is not finite.
 *   2. Into the previous camera:  d = a.pos - O' (componentwise);  lx = dot(R', d), ly = dot(U', d), lz = dot(F', d).
 *      No history unless lz > 0 (a NaN fails this).  For a camera matrix whose axes are orthonormal this inverts the mapping of
 *      RayCommon.hlsl:555-556, focusPoint = mul(CamLocalToWorldMatrix, (uv - 0.5) * ViewParams.xy, ViewParams.z): the transpose of the
 *      rotation is its inverse.  Any other matrix gets the arithmetic as written (it is then not the inverse: scale the columns of such
 *      a matrix to unit length first).
 *   3. Onto the previous image:  u = rt_div(lx * fd, lz * pw) + 0.5f;  fx = u * (float)(W - 1);  v = rt_div(ly * fd, lz * ph) + 0.5f;
 *      fy = v * (float)(H - 1)  — the inverse of uv = id / (Resolution - 1) (RayCompute.compute:15).  No history unless fx and fy are
 *      finite, -1 < fx < (float)W and -1 < fy < (float)H.  An image one pixel wide or high carries nothing: its uv is 0 / 0, there is
 *      no mapping to invert (and its records come from NaN rays).  That is a rule of its own, since u * 0 would pass the range test:
 *      W == 1 or H == 1 is "no history" for every pixel, whatever the records say.
 *   4. Taps:  x0 = floor(fx), tx = fx - x0;  y0 = floor(fy), ty = fy - y0.  sum_w = sum_n = sum_c[0..2] = +0.  For j = 0, 1 (outer),
 *      i = 0, 1 (inner):  q = (x0 + i, y0 + j);  w = (i ? tx : 1 - tx) * (j ? ty : 1 - ty).  The tap is skipped (adds nothing) when
 *        q is outside the image;  b(q).object != a.object;
 *        dot(a.normal, b(q).normal) >= minNormalDot is false;
 *        |dot(a.normal, b(q).pos - a.pos)| <= maxPlaneDistance is false   (the tap's hit point off the centre's tangent plane);
 *        any of the four components of P(q) is not finite;  P(q).a > 0 is false.
 *      Otherwise  m[k] = rt_div(P(q)[k], P(q).a) (k = 0, 1, 2);  sum_w += w;  sum_c[k] += w * m[k];  sum_n += w * P(q).a.
 *   5. No history when sum_w > 0 is false.  Otherwise  x = rt_div(sum_n, sum_w),  n = x < maxHistory ? x : maxHistory,
 *      mean[k] = rt_div(sum_c[k], sum_w),  out(p) = (mean[0] * n, mean[1] * n, mean[2] * n, n).
 *
 *   So the carried pixel is the bilinear blend of the previous MEANS of the taps that show the same surface, renormalised over those
 *   taps, with the blended frame count, capped: maxHistory bounds how long a stale value (view-dependent shading, a light that changed)
 *   outweighs new frames.  An object that moved or vanished between the views fails the plane test or the object test and simply
 *   restarts.  Neither the source image nor either record image is written.  Rows: row 0 at the bottom, as everywhere in this library.
 *
 * Resolve.  out[k] = rt_div(sum[k], sum.a) for k = 0, 1, 2 when sum.a > 0, otherwise out[k] = +0;  out.a = sum.a, the history
 * length.  The resolved image is what rt_denoise_buffers takes with scale = 1.
 */
#ifndef RT_REPROJECT_H
#define RT_REPROJECT_H

#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_REPROJECT_FLAG_GLASS 1u /* bit 0 of RtReprojectParams.flags: carry history onto glass first hits too */

typedef struct RtReprojectParams {   /* 100 bytes */
    uint32_t struct_size;            /* = sizeof(RtReprojectParams): handshake, RT_ERR_ABI_MISMATCH otherwise */
    float    prevViewParams[3];      /* the previous view's RtParams.viewParams */
    float    prevCamLocalToWorld[16];/* the previous view's RtParams.camLocalToWorld, column-major */
    float    maxPlaneDistance;       /* >= 0, finite; world units */
    float    minNormalDot;           /* finite */
    float    maxHistory;             /* > 0, finite; frames */
    uint32_t flags;                  /* RT_REPROJECT_FLAG_GLASS; every other bit must be 0 */
    int32_t  reserved;               /* must be 0 */
} RtReprojectParams;

/* Fills *out: struct_size set, maxPlaneDistance 0.1, minNormalDot 0.9, maxHistory 256, flags 0; the previous camera is left all zero
 * for the caller to fill (an all-zero camera carries nothing: lz = 0).  RT_ERR_INVALID_ARG for null. */
int rt_reproject_default_params(RtReprojectParams* out);

/* The pass alone, on caller-owned device memory of the context's device: d_prev_rgba width x height RGBA32F, d_prev_aov and d_cur_aov
 * width x height RtPixelAov, d_out_rgba width x height RGBA32F; each 16-byte aligned, row 0 at the bottom; d_out_rgba overlaps no
 * input (the inputs may overlap each other).  Only enqueues: it runs on the stream the context renders on (rt_set_stream is
 * respected), behind everything already requested, and is complete after rt_synchronize.  Needs no scene and no rt_resize: width and
 * height are the call's own.  Changes nothing of the context.  Like the filter of rt_denoise.h it needs the whole image (a tap may lie
 * in any row), so it returns RT_ERR_STATE on a context with rt_set_partition(..., part_count > 1): gather first. */
int rt_reproject_buffers(RtContext* ctx, const RtReprojectParams* p, int width, int height,
                         const void* d_prev_rgba, const void* d_prev_aov, const void* d_cur_aov, void* d_out_rgba);

/* For a context that owns the whole image, AFTER the caller has set the new camera with rt_set_params: replaces the contents of the
 * context's AccumulatedRender (its own or the bound one) by its reprojection into the current view.  THIS CALL CHANGES
 * AccumulatedRender — that is its purpose.  It changes nothing else: FrameRender, the frame counter, RtCounters and the context's
 * watchdog word are as before.
 *
 * d_prev_aov: the records of the view AccumulatedRender was rendered under (rows * W * 64 bytes of device memory, as
 * rt_render_aov_to_device wrote them before the move).  The current view's records are made by the AOV pass of frame `aov_frame`
 * (>= 1) under the current parameters, exactly as rt_render_aov_to_device produces it, into scratch the library owns; when
 * d_cur_aov_out is not NULL they are also copied there (same size; it overlaps neither d_prev_aov nor AccumulatedRender): they are the
 * d_prev_aov of the next move and the guide of rt_denoise_buffers.  Frames rt_render_frame holds back are launched first.  Only
 * enqueues, on the stream the context renders on; frames requested afterwards add onto the reprojected sum.  Scratch (one colour image
 * and the records, shared with rt_denoise's) lives in the context, grows on demand and is freed by rt_destroy.
 *
 * When the traversal watchdog fired in the internal AOV pass, the records are not valid: AccumulatedRender is then left exactly as it
 * was (the device decides that, without a host round trip), and the failure is reported as rt_render_aov_to_device reports its own: by
 * the next rt_synchronize, rt_resolve, or call that runs an AOV pass, whichever comes first, once, as RT_ERR_HIP. */
int rt_reproject_accumulated(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, int aov_frame, void* d_cur_aov_out);

/* The per-pixel divide ("Resolve" above).  rt_resolve_buffers: width x height RGBA32F in caller-owned device memory of the context's
 * device, 16-byte aligned; in place is allowed (d_rgba_out == d_rgba_sum), any other overlap is refused; only enqueues, like
 * rt_reproject_buffers; needs no scene and no rt_resize.  rt_resolve and rt_resolve_to_device resolve the context's
 * AccumulatedRender (bytes = rows * W * 16; a context that owns part of the image resolves its rows): rt_resolve writes host memory, is
 * synchronous and fails, like every call that hands the context's pixels to the host, when the context's watchdog word is set; it also
 * reports (once, RT_ERR_HIP) the watchdog of a preceding rt_reproject_accumulated's AOV pass that has not been reported yet;
 * rt_resolve_to_device writes device memory that does not overlap AccumulatedRender and only enqueues.  None of the three changes
 * anything of the context. */
int rt_resolve_buffers(RtContext* ctx, int width, int height, const void* d_rgba_sum, void* d_rgba_out);
int rt_resolve(RtContext* ctx, float* rgba, size_t bytes);
int rt_resolve_to_device(RtContext* ctx, void* d_rgba, size_t bytes);

/* Errors: RT_ERR_INVALID_ARG for a null context or pointer (d_cur_aov_out alone may be null), a maxPlaneDistance that is negative or
 * not finite, a minNormalDot that is not finite, a maxHistory that is <= 0 or not finite, a flag bit other than bit 0, reserved != 0,
 * aov_frame < 1, a wrong `bytes`, width or height < 1 or more than 2^30 pixels, and misaligned, overlapping or wrong-device memory;
 * RT_ERR_ABI_MISMATCH for a wrong struct_size; RT_ERR_STATE on a partitioned context (rt_reproject_buffers,
 * rt_reproject_accumulated), before rt_resize, rt_upload_scene or rt_set_params (rt_reproject_accumulated) and before rt_resize
 * (rt_resolve, rt_resolve_to_device). */

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtReprojectParams) == 100, "RtReprojectParams must be 100 bytes");
#endif

#endif /* RT_REPROJECT_H */
